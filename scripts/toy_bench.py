"""Time the toy pipeline (BASELINE config 1: Decoder(2, 128, 3), T = 100) on the GPU: the fused decoder forward, forward + backward,
a toy Trainer.step, one sampling step and a 100-step chain, at B = 1000 and B = 30000; the same decoder math composed from eager torch
ops (oracle/toy_ref.decoder_forward on device tensors — a measurement baseline, not product code) for comparison.

    python scripts/toy_bench.py [--blocks 7] [--iters 20]

Device events around blocks of --iters calls after a warm-up; the median block is reported, one JSON line per measurement."""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "ddpm-torch_amd")]

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from ddpm_torch.toy import DataStreamer, Decoder, GaussianDiffusion, Trainer, get_beta_schedule  # noqa: E402
from oracle import toy_ref  # noqa: E402


def eager_forward(sd, x, t, M, L):
    """oracle/toy_ref.decoder_forward with the sinusoidal embedding built on the device (the oracle builds its frequencies on the host)."""
    half = M // 2
    freqs = torch.exp(-torch.arange(half, dtype=torch.float32, device=x.device) * (math.log(10000) / (half - 1)))
    arg = torch.outer(t.float(), freqs)
    te = F.leaky_relu(F.linear(torch.cat([arg.sin(), arg.cos()], 1), sd["t_proj.0.weight"], sd["t_proj.0.bias"]), 0.02)
    h = F.linear(x, sd["in_fc.weight"])
    for _ in range(L):
        h = toy_ref._temporal(sd, "temp_fc.0.", h, te, M)
    return F.linear(F.layer_norm(h, (M,), sd["out_norm.weight"], sd["out_norm.bias"]), sd["out_fc.weight"], sd["out_fc.bias"])


def timed(fn, blocks, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(blocks):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / iters)
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    D, M, L, T = 2, 128, 3, 100
    torch.manual_seed(0)
    m = Decoder(D, M, L).to(dev)
    m.timesteps = T
    sd = {k: v for k, v in m.state_dict().items()}
    dif = GaussianDiffusion(get_beta_schedule("linear", 1e-3, 0.2, T), "eps", "fixed-large", "mse")
    for B in (1000, 30000):
        x = torch.randn(B, D, device=dev)
        t = torch.randint(T, (B,), device=dev)
        gy = torch.randn(B, D, device=dev)
        flop = B * 2 * (2 * D * M + 2 * L * M * M) + 4 * T * M * M
        rows = {}
        with torch.no_grad():
            rows["forward"] = timed(lambda: m(x, t), args.blocks, args.iters)
            rows["forward_eager_torch"] = timed(lambda: eager_forward(sd, x, t, M, L), args.blocks, args.iters)

        def fb():
            m.zero_grad(set_to_none=True)
            (m(x, t) * gy).sum().backward()

        p = {k: v.detach().clone().requires_grad_(True) for k, v in sd.items()}

        def fb_eager():
            for v in p.values():
                v.grad = None
            (eager_forward(p, x, t, M, L) * gy).sum().backward()

        rows["forward_backward"] = timed(fb, args.blocks, args.iters)
        rows["forward_backward_eager_torch"] = timed(fb_eager, args.blocks, args.iters)
        opt = torch.optim.Adam(m.parameters(), lr=1e-4)
        tr = Trainer(m, opt, dif, epochs=1, trainloader=DataStreamer("gaussian8", B, 1), device=dev)
        xb = next(iter(tr.trainloader)).to(dev)
        rows["trainer_step"] = timed(lambda: tr.step(xb), args.blocks, max(1, args.iters // 4))
        with torch.no_grad():
            tt = torch.full((B,), T - 1, dtype=torch.int64, device=dev)
            rows["sampling_step_eager"] = timed(lambda: dif.p_sample_step(m, x, tt, clip_denoised=False), args.blocks, args.iters)
        rows["sampling_chain_100"] = timed(lambda: dif.p_sample(m, (B, D), device=dev, seed=0), args.blocks, 1)
        for k, ms in rows.items():
            r = {"B": B, "what": k, "ms": round(ms, 4)}
            if k == "forward":
                r["tflops"] = round(flop / ms / 1e9, 2)
                r["share_of_157tf"] = round(flop / ms / 1e9 / 157.3, 3)
            print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
