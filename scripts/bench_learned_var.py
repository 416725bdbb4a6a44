"""What the learned reverse-process variance costs, on one box in one session, at config 2 (CIFAR-10 UNet, B = 128, bf16):

  * ms per training step of the fixed-variance `mse` step (3 output channels) and of the `learned-range` + `hybrid` step (6 output
    channels, one `ddpm_learned_loss` launch in the place of the `ddpm_mse_fwd` / `ddpm_mse_bwd` pair): the median of five 20-step blocks
    after warm-up and settling, the two trainers alternating block by block;
  * per launch, device events over back-to-back launches: `ddpm_learned_loss` (hybrid, with gradient) against `ddpm_mse_fwd` +
    `ddpm_mse_bwd`, and `ddpm_p_sample_step_lv` (var_mode 2, in place) against `ddpm_p_sample_step`, at [128, 3, 32, 32].

    python scripts/bench_learned_var.py [--steps 20] [--blocks 5] [--launches 200] > profiles/bench_learned_var.log
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "ddpm-torch_amd")]
import torch  # noqa: E402

import ddpm_torch  # noqa: E402
from bench import CIFAR, median, settle  # noqa: E402
from ddpm_torch import _hip  # noqa: E402
from ddpm_torch.diffusion import _STEP_TABLES  # noqa: E402

T, SHAPE = 1000, (128, 3, 32, 32)


def trainer(dev, var_type, loss_type):
    learned = var_type in ("learned", "learned-range")
    torch.manual_seed(0)
    m = ddpm_torch.UNet(**dict(CIFAR, out_channels=6 if learned else 3)).to(dev).set_compute_dtype("bf16")
    dif = ddpm_torch.GaussianDiffusion(ddpm_torch.get_beta_schedule("linear", 1e-4, 0.02, T), "eps", var_type, loss_type)
    opt = torch.optim.Adam(m.parameters(), lr=2e-4, betas=(0.9, 0.999))
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lr_lambda=lambda s: min((s + 1) / 5000, 1.0))
    tr = ddpm_torch.Trainer(m, opt, dif, epochs=1, trainloader=None, scheduler=sched, use_ema=True, grad_norm=1.0, shape=SHAPE[1:], device=dev)
    m.train()
    return tr, dif


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
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--blocks", type=int, default=5)
    p.add_argument("--warmup", type=int, default=20)
    p.add_argument("--launches", type=int, default=200)
    args = p.parse_args()
    dev = torch.device("cuda", 0)
    print(f"device: {torch.cuda.get_device_name(0)}; CIFAR-10 UNet, B = {SHAPE[0]}, bf16, T = {T}", flush=True)
    x0 = torch.rand(SHAPE, device=dev) * 2 - 1
    sync = lambda: torch.cuda.synchronize(dev)                                           # noqa: E731
    pairs = {"mse / fixed-large (3 ch)": trainer(dev, "fixed-large", "mse"), "hybrid / learned-range (6 ch)": trainer(dev, "learned-range", "hybrid")}
    done, times = {}, {k: [] for k in pairs}
    for name, (tr, _) in pairs.items():
        for i in range(args.warmup):
            tr.step(x0, global_steps=i + 1)
        done[name] = args.warmup + settle(tr, x0, args.warmup + 1)
        ds = next(iter(tr._direct.values()))
        print(f"{name}: settled after {done[name]} steps on the {ds.last_kind} form", flush=True)
    for blk in range(args.blocks):                                                       # alternate: both see the same box drift
        for name, (tr, _) in pairs.items():
            sync()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for i in range(args.steps):
                tr.step(x0, global_steps=done[name] + i + 1)
            tr.current_stats
            b.record()
            sync()
            done[name] += args.steps
            times[name].append(a.elapsed_time(b) / args.steps)
            print(f"block {blk} {name}: {times[name][-1]:.3f} ms/step", flush=True)
    for name in pairs:
        print(f"{name}: median of {args.blocks} x {args.steps} steps {median(times[name]):.3f} ms/step (min {min(times[name]):.3f}, max {max(times[name]):.3f})", flush=True)

    # per launch
    dif = pairs["hybrid / learned-range (6 ch)"][1]
    fixed = pairs["mse / fixed-large (3 ch)"][1]
    B, n = SHAPE[0], SHAPE[1] * SHAPE[2] * SHAPE[3]
    g = lambda *s: torch.randn(*s, device=dev)                                           # noqa: E731
    x_0, x_t, z, out3, out6, target = g(B, n).clamp(-1, 1), g(B, n), g(B, n), g(B, n), g(B, 2 * n), g(B, n)
    t = torch.randint(0, T, (B,), device=dev)
    gloss = torch.full((B,), 1.0 / B, device=dev)
    loss, g3, g6, xp = torch.empty(B, device=dev), torch.empty(B, n, device=dev), torch.empty(B, 2 * n, device=dev), torch.empty(B, n, device=dev)
    s = _hip.stream()

    def mse_pair():
        _hip.call("ddpm_mse_fwd", out3.data_ptr(), target.data_ptr(), loss.data_ptr(), B, n, s)
        _hip.call("ddpm_mse_bwd", out3.data_ptr(), target.data_ptr(), gloss.data_ptr(), g3.data_ptr(), B, n, s)

    def learned():
        dif.learned_loss(x_0, x_t, out6, target, t, gloss, g6, 1.0, dif.vlb_weight, True, loss=loss)

    tabs = [fixed._tab(k, dev).data_ptr() for k in _STEP_TABLES]

    def step_old():
        _hip.call("ddpm_p_sample_step", x_t.data_ptr(), out3.data_ptr(), z.data_ptr(), t.data_ptr(), *tabs, xp.data_ptr(), 0, B, n, 0, 1, T, s)

    def step_lv():
        dif._step_call(x_t, out6, z, t, xp, None, True)

    for name, fn in (("ddpm_mse_fwd + ddpm_mse_bwd", mse_pair), ("ddpm_learned_loss (hybrid, with gradient)", learned),
                     ("ddpm_p_sample_step", step_old), ("ddpm_p_sample_step_lv (var_mode 2)", step_lv)):
        runs = [launches_ms(fn, args.launches, dev) for _ in range(3)]
        print(f"{name}: {median(runs) * 1e3:.1f} us per call (3 x {args.launches} back-to-back calls: " + ", ".join(f"{r * 1e3:.1f}" for r in runs) + ")", flush=True)


if __name__ == "__main__":
    main()
