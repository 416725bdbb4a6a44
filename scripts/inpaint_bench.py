"""The masked sampling step against the three launches it replaces, and ms per network call of inpainting chains beside `p_sample`.

(a) The step: `ddpm_p_sample_step_masked` against the composition out of entries the project already had — `ddpm_p_sample_step`, then
`ddpm_q_sample` on the previous level's tables, then `torch.lerp` with the mask — on [B][3][H][W] fp32 state: B = 128 at 32 x 32 and at
64 x 64, B = 2 at 256 x 256.  Blocks of `--launches` updates alternate in one process, 7 pairs after one warm-up pair, device events
around each block, medians — in two forms: every update issued from Python (a time per CALL: the host paces it as much as the device
does), and the block captured once into a hipGraph and replayed, as the update runs inside the captured sampling step (the device
paces it; `--replays` replays per timed block).  The fused step issues one launch instead of three and moves 6 n + hw floats per sample
(x_t, model_out, z, x_known, e in, x_prev out, one mask row) instead of 10 n + hw (the composition writes u and k and reads them again):
it must not be slower at any size; the log records the measured ratios, and a ratio above 1 is a finding to explain there.

(b) The chain: ms per network call of `inpaint(resamples=1)` beside `p_sample` on the config-2 UNet (CIFAR-10, bf16, B = 128; whole
replayed chains of a T = `--steps` schedule: the step's cost does not depend on T), and of a RePaint chain (j = 10, r = 10) beside
`p_sample` on DDIM-50 of config 4 (CelebA 64 x 64, B = 128), after checking that every step was captured.  Recorded only.

    python scripts/inpaint_bench.py [--chains 7] [--launches 200] [--replays 20] [--steps 100] > profiles/inpaint_bench.log
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "ddpm-torch_amd")]
import torch  # noqa: E402

import ddim  # noqa: E402
import ddpm_torch  # noqa: E402
from bench import CELEBA, CIFAR  # noqa: E402
from ddpm_torch import _hip  # noqa: E402
from ddpm_torch._graphs import SegmentedGraph  # noqa: E402
from ddpm_torch.diffusion import _MEAN_CODE, _STEP_TABLES, repaint_schedule  # noqa: E402


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


def step_pair(dif, B, C, H, W, dev):
    """(fused, composed): one masked update each on the same buffers, out of place, a half-image mask."""
    shape, n, hw, T = (B, C, H, W), C * H * W, H * W, dif.timesteps
    x, out, z, xk, e = (torch.randn(shape, device=dev) for _ in range(5))
    mask = torch.zeros(1, hw, device=dev)
    mask.view(H, W)[:, :W // 2] = 1
    t = torch.randint(1, T, (B,), device=dev)
    step = [dif._tab(k, dev).data_ptr() for k in _STEP_TABLES]
    prev = [dif._tab(k, dev).data_ptr() for k in ("sqrt_alphas_bar_prev", "sqrt_one_minus_alphas_bar_prev")]
    dst, u, k = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)
    code = _MEAN_CODE[dif.model_mean_type]
    mb = mask.view(1, 1, H, W)                                          # lerp broadcasts it over batch and channels

    def fused():
        _hip.call("ddpm_p_sample_step_masked", x.data_ptr(), out.data_ptr(), z.data_ptr(), xk.data_ptr(), e.data_ptr(), mask.data_ptr(), t.data_ptr(),
                  *step, 0, *prev, dst.data_ptr(), B, n, hw, 1, n, code, 1, 0, T, _hip.stream())

    def composed():
        _hip.call("ddpm_p_sample_step", x.data_ptr(), out.data_ptr(), z.data_ptr(), t.data_ptr(), *step, u.data_ptr(), 0, B, n, code, 1, T, _hip.stream())
        _hip.call("ddpm_q_sample", xk.data_ptr(), e.data_ptr(), t.data_ptr(), *prev, k.data_ptr(), B, n, T, _hip.stream())
        torch.lerp(u, k, mb, out=dst)

    fused()
    a = dst.clone()
    composed()
    keep = mb.expand(shape) == 1
    assert torch.equal(a[~keep], dst[~keep]) and torch.equal(a[keep], k[keep]), "the two forms disagree on a 0 / 1 mask"
    return fused, composed


def captured_kinds(proc):
    """The ``kind`` of every captured step in the sampler's cache (None: the plain sampling step)."""
    return [k[3][3] if len(k[3]) > 3 else None for k in getattr(proc, "_sample_graphs", {})]


def main():
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--chains", type=int, default=7)
    p.add_argument("--launches", type=int, default=200)
    p.add_argument("--replays", type=int, default=20)
    p.add_argument("--steps", type=int, default=100)
    p.add_argument("--batch", type=int, default=128)
    args = p.parse_args()
    dev = torch.device("cuda", 0)
    print(f"device: {torch.cuda.get_device_name(0)}", flush=True)
    betas = ddpm_torch.get_beta_schedule("linear", 1e-4, 0.02, 1000)
    dif = ddpm_torch.GaussianDiffusion(betas, "eps", "fixed-large", "mse")

    N, R = args.launches, args.replays
    print(f"(a) the step, us per update: blocks of {N} updates, {args.chains} alternating pairs after one warm-up pair, medians; issued = every "
          f"update launched from Python (call time), replayed = the block captured once into a hipGraph, {R} replays per timed block", flush=True)
    for B, C, H, W in ((128, 3, 32, 32), (128, 3, 64, 64), (2, 3, 256, 256)):
        fused, composed = step_pair(dif, B, C, H, W, dev)
        n = C * H * W
        forms = {"issued": (lambda fn: (lambda: [fn() for _ in range(N)]), 1)}
        graphs = {name: SegmentedGraph(dev).capture(lambda cut, fn=fn: [fn() for _ in range(N)]) for name, fn in (("fused", fused), ("composed", composed))}
        assert all(g.launches == 1 for g in graphs.values())
        forms["replayed"] = (lambda fn: (lambda g=graphs["fused" if fn is fused else "composed"]: [g.replay() for _ in range(R)]), R)
        print(f"  B = {B:3d}, {C} x {H} x {W} (fused moves {B * (6 * n + H * W) * 4 / 1e6:.1f} MB per update, composed {B * (10 * n + H * W) * 4 / 1e6:.1f} MB):", flush=True)
        for name, (wrap, reps) in forms.items():
            block = lambda fn: timed(wrap(fn), dev) / (N * reps) * 1e3                      # noqa: E731  us per update
            block(fused); block(composed)
            rows = [(block(fused), block(composed)) for _ in range(args.chains)]
            f, c = median([r_[0] for r_ in rows]), median([r_[1] for r_ in rows])
            print(f"    {name:8s}: fused {f:7.2f} us | composed (3 launches) {c:7.2f} us | fused / composed = {f / c:.3f} "
                  f"({'not slower' if f <= c else 'SLOWER'})", flush=True)

    print(f"(b) the chain, ms per network call: whole replayed chains, {args.chains} alternating pairs after one warm-up pair, medians", flush=True)
    S = args.steps
    torch.manual_seed(0)
    m = ddpm_torch.UNet(**CIFAR).to(dev).set_compute_dtype("bf16").eval()
    short = ddpm_torch.GaussianDiffusion(ddpm_torch.get_beta_schedule("linear", 1e-4, 0.02, S), "eps", "fixed-large", "mse")
    shape = (args.batch, 3, 32, 32)
    x_0 = torch.rand(shape, device=dev) * 2 - 1
    mask = torch.zeros(32, 32)
    mask[:, :16] = 1
    inp = lambda: short.inpaint(m, x_0, mask, seed=131071)                                  # noqa: E731
    smp = lambda: short.p_sample(m, shape, device=dev, seed=131071)                         # noqa: E731
    inp(); smp()
    kinds = captured_kinds(short)
    assert ("inpaint", 0, 1, None) in kinds and None in kinds, f"a step was not captured: {kinds}"
    rows = [(timed(inp, dev) / S, timed(smp, dev) / S) for _ in range(args.chains)]
    i, s = median([r_[0] for r_ in rows]), median([r_[1] for r_ in rows])
    print(f"  config 2 (CIFAR-10 UNet, bf16, B = {args.batch}, T = {S}): inpaint(resamples=1) {i:.3f} ms/call | p_sample {s:.3f} ms/call | ratio {i / s:.3f}",
          flush=True)
    del m
    m = ddpm_torch.UNet(**CELEBA).to(dev).set_compute_dtype("bf16").eval()
    dd = ddim.DDIM(betas, "eps", "fixed-small", "mse", eta=0.0, subsequence=ddim.get_selection_schedule("linear", 50, 1000))
    shape = (args.batch, 3, 64, 64)
    x_0 = torch.rand(shape, device=dev) * 2 - 1
    mask = torch.zeros(64, 64)
    mask[:, :32] = 1
    ops = repaint_schedule(50, 10, 10)
    calls = ops.count("down")
    rep = lambda: dd.inpaint(m, x_0, mask, jump_length=10, resamples=10, seed=131071)       # noqa: E731
    smp = lambda: dd.p_sample(m, shape, device=dev, seed=131071)                            # noqa: E731
    rep(); smp()
    kinds = captured_kinds(dd)
    assert ("inpaint", 10, 1, None) in kinds and None in kinds, f"a step was not captured: {kinds}"
    rows = [(timed(rep, dev) / calls, timed(smp, dev) / 50) for _ in range(args.chains)]
    i, s = median([r_[0] for r_ in rows]), median([r_[1] for r_ in rows])
    print(f"  config 4 (CelebA 64 x 64 UNet, bf16, B = {args.batch}, DDIM-50): RePaint j = 10, r = 10 ({calls} network calls, {ops.count('up')} jumps) "
          f"{i:.3f} ms/call | p_sample {s:.3f} ms/call | ratio {i / s:.3f}", flush=True)


if __name__ == "__main__":
    main()
