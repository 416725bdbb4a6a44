"""What classifier-free guidance costs per sampling step, on one box in one session, at config 2 (CIFAR-10 UNet, bf16, T = 1000):

  * the replayed guided step at B = 128 (one 256-row network call on [x | x] with labels [y | null], then `ddpm_p_sample_step_cfg`)
    against the replayed unguided step of an unconditional model at B = 128 and at B = 256 (the two ways the same 256 network rows could
    be spent without guidance), and the replayed conditional step at scale 1 (B = 128, the embedding MLP instead of the time table):
    device events around blocks of replays, the median of 7 blocks, the forms alternating block by block;
  * `ddpm_p_sample_step_cfg` alone (dup, in place) against `ddpm_p_sample_step` (in place) on the same [128][3072] state, back-to-back
    launches between two device events.

    python scripts/bench_cfg.py [--steps 50] [--blocks 7] [--launches 200] > profiles/bench_cfg.log
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "ddpm-torch_amd")]
import torch  # noqa: E402

import ddpm_torch  # noqa: E402
from bench import CIFAR, median  # noqa: E402
from ddpm_torch import _hip  # noqa: E402
from ddpm_torch.diffusion import _STEP_TABLES  # noqa: E402

T, K, IMAGE = 1000, 10, (3, 32, 32)


def model(dev, num_classes):
    torch.manual_seed(0)
    m = ddpm_torch.UNet(**CIFAR, num_classes=num_classes).to(dev).set_compute_dtype("bf16").eval()
    for p in m.parameters():
        p.requires_grad_(False)
    return m


class Replayed:
    """One captured sampling step of ``dif`` on ``m`` at batch ``B``: ``block(steps)`` refills the state and times ``steps`` replays."""

    def __init__(self, dif, m, B, dev, y=None, scale=1.0):
        self.dif, self.m, self.dev = dif, m, dev
        shape = (B,) + IMAGE
        form = dif._guidance_form(m, y, scale)
        with torch.inference_mode(), dif._time_tables(m):
            self.ent = dif._graph_entry(m, shape, dev, default_rng=True, kind=form)
            if self.ent is None:
                raise RuntimeError("the sampling step could not be captured")
            if y is not None:
                self.ent["y"][:B].copy_(y)

    def block(self, steps):
        ent = self.ent
        with torch.inference_mode(), self.dif._time_tables(self.m):
            for e in self.dif._engines_of(self.m):
                e.ensure_fresh()
            ent["x_t"].normal_()
            if ent.get("x_dup") is not None:
                ent["x_dup"].copy_(ent["x_t"])
            ent["t"].fill_(T - 1)
            torch.cuda.synchronize(self.dev)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(steps):
                ent["graph"].replay()
            b.record()
            torch.cuda.synchronize(self.dev)
        return a.elapsed_time(b) / steps


def launches_ms(fn, count, dev):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(10):
        fn()
    torch.cuda.synchronize(dev)
    a.record()
    for _ in range(count):
        fn()
    b.record()
    torch.cuda.synchronize(dev)
    return a.elapsed_time(b) / count


def main():
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--steps", type=int, default=50)
    p.add_argument("--blocks", type=int, default=7)
    p.add_argument("--launches", type=int, default=200)
    p.add_argument("--scale", type=float, default=2.0)
    args = p.parse_args()
    dev = torch.device("cuda", 0)
    print(f"device: {torch.cuda.get_device_name(0)}; CIFAR-10 UNet, bf16, T = {T}, {K} classes, guidance scale {args.scale}", flush=True)
    dif = ddpm_torch.GaussianDiffusion(ddpm_torch.get_beta_schedule("linear", 1e-4, 0.02, T), "eps", "fixed-large", "mse")
    plain, cond = model(dev, None), model(dev, K)
    y = torch.arange(128, device=dev) % K
    forms = {
        "unguided, unconditional model, B = 128": Replayed(dif, plain, 128, dev),
        "unguided, unconditional model, B = 256": Replayed(dif, plain, 256, dev),
        "conditional at scale 1, B = 128": Replayed(dif, cond, 128, dev, y, 1.0),
        f"guided at scale {args.scale:g}, B = 128 (256 network rows)": Replayed(dif, cond, 128, dev, y, args.scale),
    }
    for f in forms.values():                                                             # warm every shape the timed windows use
        f.block(args.steps)
    times = {k: [] for k in forms}
    for blk in range(args.blocks):                                                       # alternate: every form sees the same box drift
        for name, f in forms.items():
            times[name].append(f.block(args.steps))
            print(f"block {blk} {name}: {times[name][-1]:.3f} ms/step", flush=True)
    for name in forms:
        print(f"{name}: median of {args.blocks} x {args.steps} replays {median(times[name]):.3f} ms/step "
              f"(min {min(times[name]):.3f}, max {max(times[name]):.3f})", flush=True)

    # the step kernels alone
    B, n = 128, IMAGE[0] * IMAGE[1] * IMAGE[2]
    g = lambda *s: torch.randn(*s, device=dev)                                           # noqa: E731
    state, out2, z = g(2 * B, n), g(2 * B, n), g(B, n)
    t = torch.randint(1, T, (B,), device=dev)
    tabs = [dif._tab(k, dev).data_ptr() for k in _STEP_TABLES]
    s = _hip.stream()

    def step_old():
        _hip.call("ddpm_p_sample_step", state.data_ptr(), out2.data_ptr(), z.data_ptr(), t.data_ptr(), *tabs, state.data_ptr(), 0, B, n, 0, 1, T, s)

    def step_cfg():
        _hip.call("ddpm_p_sample_step_cfg", state.data_ptr(), out2.data_ptr(), z.data_ptr(), t.data_ptr(), *tabs, args.scale, state.data_ptr(), 0, B, n, 0, 1, 1, T, s)

    for name, fn in (("ddpm_p_sample_step (4 arrays)", step_old), ("ddpm_p_sample_step_cfg (dup: 6 arrays)", step_cfg)):
        runs = [launches_ms(fn, args.launches, dev) for _ in range(3)]
        print(f"{name}: {median(runs) * 1e3:.1f} us per call (3 x {args.launches} back-to-back calls: " + ", ".join(f"{r * 1e3:.1f}" for r in runs) + ")", flush=True)


if __name__ == "__main__":
    main()
