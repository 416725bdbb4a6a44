"""ms per step of the bits/dim evaluation (`GaussianDiffusion.calc_all_bpd`): the graph-replayed fused step against the eager composition
of the entry points that existed before it — `ddpm_q_sample`, forward, `ddpm_vlb_terms` with `pred_x0`, `ddpm_mse_fwd`, two column copies,
`ddpm_add_i64` — and, beside them, the replayed sampling step on the same box (the same forward plus two small kernels).
CIFAR-10 UNet at B = 128 and CelebA-HQ 256 x 256 at B = 8, bf16, T = 1000 tables; the two forms alternate, three pairs, device events.

    python scripts/bpd_bench.py [--steps-cifar 200] [--steps-hq 10] > profiles/bpd_bench.log
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "ddpm-torch_amd")]
import torch  # noqa: E402

import ddpm_torch  # noqa: E402
from bench import CELEBAHQ, CIFAR  # noqa: E402
from ddpm_torch import _hip  # noqa: E402
from ddpm_torch.diffusion import _MEAN_CODE, _VLB_TABLES  # noqa: E402

T = 1000


def timed(fn, steps, dev):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(dev)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize(dev)
    return a.elapsed_time(b) / steps


def run(name, cfg, shape, steps, dev):
    torch.manual_seed(0)
    m = ddpm_torch.UNet(**cfg).to(dev).set_compute_dtype("bf16").eval()
    dif = ddpm_torch.GaussianDiffusion(ddpm_torch.get_beta_schedule("linear", 1e-4, 0.02, T), "eps", "fixed-large", "mse")
    B, n = shape[0], shape[1] * shape[2] * shape[3]
    x_0 = torch.rand(shape, device=dev) * 2 - 1
    with torch.inference_mode(), dif._time_tables(m):
        ent = dif._graph_entry(m, shape, dev, default_rng=True, bpd=(True,))
        smp = dif._graph_entry(m, shape, dev, default_rng=True)
        assert ent is not None and smp is not None, "capture failed"
        for e in dif._engines_of(m):
            e.ensure_fresh()
        ent["x_0"].copy_(x_0)
        # the eager composition of the parent's entry points
        z, x_t = torch.empty_like(x_0), torch.empty_like(x_0)
        pred = torch.empty_like(x_0)
        t = torch.full((B,), T - 1, dtype=torch.int64, device=dev)
        loss, mse = torch.empty(B, device=dev), torch.empty(B, device=dev)
        losses, mses = torch.zeros(B, T, device=dev), torch.zeros(B, T, device=dev)
        tabs = [dif._tab(k, dev) for k in _VLB_TABLES]
        qa, qb = dif._tab("sqrt_alphas_bar", dev), dif._tab("sqrt_one_minus_alphas_bar", dev)
        col = [T - 1]

        def eager():
            z.normal_()
            _hip.call("ddpm_q_sample", x_0.data_ptr(), z.data_ptr(), t.data_ptr(), qa.data_ptr(), qb.data_ptr(), x_t.data_ptr(), B, n, T, _hip.stream())
            out = m(x_t, t).contiguous().float()
            _hip.call("ddpm_vlb_terms", x_0.data_ptr(), x_t.data_ptr(), out.data_ptr(), t.data_ptr(), *[tb.data_ptr() for tb in tabs],
                      loss.data_ptr(), pred.data_ptr(), B, n, _MEAN_CODE["eps"], 1, T, _hip.stream())
            _hip.call("ddpm_mse_fwd", pred.data_ptr(), x_0.data_ptr(), mse.data_ptr(), B, n, _hip.stream())
            losses[:, col[0]] = loss
            mses[:, col[0]] = mse
            _hip.call("ddpm_add_i64", t.data_ptr(), B, -1, _hip.stream())
            col[0] -= 1

        def reset():
            ent["t"].fill_(T - 1)
            smp["t"].fill_(T - 1)
            t.fill_(T - 1)
            col[0] = T - 1

        reset()
        for _ in range(3):
            ent["graph"].replay(); smp["graph"].replay(); eager()
        rows = []
        for pair in range(3):
            reset()
            a = timed(ent["graph"].replay, steps, dev)
            b = timed(eager, steps, dev)
            c = timed(smp["graph"].replay, steps, dev)
            rows.append((a, b, c))
            print(f"{name} B={B} pair {pair}: replayed evaluation step {a:.3f} ms | eager composition {b:.3f} ms | replayed sampling step {c:.3f} ms"
                  f"  ({steps} steps each)", flush=True)
        med = [sorted(r[i] for r in rows)[1] for i in range(3)]
        print(f"{name} B={B} median of 3: replayed {med[0]:.3f} ms/step, eager {med[1]:.3f} ms/step ({med[1] / med[0]:.2f}x), sampling {med[2]:.3f} ms/step; "
              f"{T} steps of a batch = {med[0] * T / 1e3:.2f} s replayed", flush=True)
    del m, ent, smp
    dif.__dict__.pop("_sample_graphs", None)
    torch.cuda.empty_cache()


def main():
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--steps-cifar", type=int, default=200)
    p.add_argument("--steps-hq", type=int, default=10)
    p.add_argument("--skip-hq", action="store_true")
    args = p.parse_args()
    dev = torch.device("cuda", 0)
    print(f"device: {torch.cuda.get_device_name(0)}; bf16, T = {T}, linear schedule, eps / fixed-large, clip_denoised=True", flush=True)
    run("cifar10 32x32", CIFAR, (128, 3, 32, 32), args.steps_cifar, dev)
    if not args.skip_hq:
        run("celebahq 256x256", CELEBAHQ, (8, 3, 256, 256), args.steps_hq, dev)


if __name__ == "__main__":
    main()
