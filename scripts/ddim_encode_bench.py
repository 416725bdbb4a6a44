"""ms per step of `DDIM.encode` beside the sampling step it inverts, and `ddim.slerp` against its traffic.
BASELINE config 4 (CelebA 64 x 64 UNet, DDIM-50, linear sub-sequence, eta 0, B = 128, bf16): whole chains of `DDIM.encode` and of
`DDIM.p_sample` alternate in one process, 7 pairs after one warm-up pair (which captures both steps), device events around each chain,
medians.  The encode step is the sampling step's network call plus one elementwise launch and no `normal_()`: expect encode <= 1.05 x
sampling (5 % = run-to-run spread on a shared box).  Slerp at P = 64, K = 9, n = 12 288 (64 pairs of 64 x 64 latents, nine columns):
median of 7 timed runs of 20 calls against the bytes it has to move (read a, b twice, write out).

    python scripts/ddim_encode_bench.py [--chains 7] [--batch 128] > profiles/ddim_encode_bench.log
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "ddpm-torch_amd")]
import torch  # noqa: E402

import ddim  # noqa: E402
import ddpm_torch  # noqa: E402
from bench import CELEBA  # noqa: E402

S, T = 50, 1000


def timed(fn, dev):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(dev)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize(dev)
    return a.elapsed_time(b)


def median(v):
    return sorted(v)[len(v) // 2]


def main():
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--chains", type=int, default=7)
    p.add_argument("--batch", type=int, default=128)
    args = p.parse_args()
    dev = torch.device("cuda", 0)
    print(f"device: {torch.cuda.get_device_name(0)}; CelebA 64x64 UNet, bf16, DDIM-{S} (linear, eta 0), B = {args.batch}", flush=True)
    torch.manual_seed(0)
    m = ddpm_torch.UNet(**CELEBA).to(dev).set_compute_dtype("bf16").eval()
    dif = ddim.DDIM(ddpm_torch.get_beta_schedule("linear", 1e-4, 0.02, T), "eps", "fixed-small", "mse", eta=0.0,
                    subsequence=ddim.get_selection_schedule("linear", S, T))
    shape = (args.batch, 3, 64, 64)
    x_0 = torch.rand(shape, device=dev) * 2 - 1
    enc = lambda: dif.encode(m, x_0)                                                       # noqa: E731
    smp = lambda: dif.p_sample(m, shape, device=dev, seed=131071)                          # noqa: E731
    enc(); smp()                                                                           # captures both steps
    kinds = [k[3] for k in dif._sample_graphs]
    assert any(k[-1] == ("encode",) for k in kinds) and any(len(k) == 3 and k[2] is None for k in kinds), f"a step was not captured: {kinds}"
    rows = []
    for c in range(args.chains):
        e, s = timed(enc, dev) / S, timed(smp, dev) / S
        rows.append((e, s))
        print(f"chain pair {c}: encode {e:.3f} ms/step | sampling {s:.3f} ms/step", flush=True)
    e, s = median([r[0] for r in rows]), median([r[1] for r in rows])
    print(f"median of {args.chains}: encode {e:.3f} ms/step, sampling {s:.3f} ms/step, encode / sampling = {e / s:.3f} "
          f"({'within' if e <= 1.05 * s else 'ABOVE'} 1.05)", flush=True)

    P, K, n = 64, 9, 12288
    a, b = torch.randn(P, 3, 64, 64, device=dev), torch.randn(P, 3, 64, 64, device=dev)
    al = torch.linspace(0, 1, K)
    ddim.slerp(a, b, al)
    times = [timed(lambda: [ddim.slerp(a, b, al) for _ in range(20)], dev) / 20 for _ in range(7)]
    t = median(times)
    moved = (4 * P * n + P * K * n) * 4                        # a and b in both passes, out once
    print(f"slerp P = {P}, K = {K}, n = {n}: {t * 1e3:.1f} us per call (two launches, allocation of out and ws included), "
          f"{moved / 1e6:.1f} MB read + written -> {moved / t / 1e9:.2f} TB/s", flush=True)


if __name__ == "__main__":
    main()
