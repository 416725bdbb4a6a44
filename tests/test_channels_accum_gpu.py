"""-m gpu: the networks and the step the shipped command lines build besides the 3 -> 3 UNet with one update per call — 1 image channel
(``--dataset mnist``), 4 and 12 (``train.py --block-size 2``: the UNet between PixelUnshuffle(2) and PixelShuffle(2)), and
``--num-accum N`` — on the MI355X through the real C ABI.  tests/test_channels_accum_host.py is the CPU twin on the emulated ABI.

  * the reduced network of launch_replay._reduced(mult=(1, 2)) at (in, out) = (1, 1) on 32 x 32 (B = 16) and (4, 4), (12, 12) on
    16 x 16 (B = 64) — 16384 pixels, where the edge kernels are dispatched: forward, every parameter gradient and the input gradient
    against oracle.unet_ref, fp32 and bf16, dropout 0.1 with the engine's masks injected; the bars of the reduced-UNet test of
    tests/test_odd_geometry_gpu.py (fp32: forward 1e-3, gradients 3e-3; bf16: 6e-2, 5e-2);
  * ``Trainer.step`` with ``num_accum=2`` for six calls at 3 and 12 channels: in fp32 against the float64 oracle trainer and the
    reference's own Trainer (fixture G19) with the host test's bars, in bf16 against the fp32 run with the relation of
    tests/test_training_convergence_gpu.py::test_bf16_mode_trains_like_the_fp32_mode (loss windows within 12 %) at this length;
    parameters and EMA shadow bit-unchanged after a call that is no update;
  * the wrapped 12-channel model: the graph-replayed sampler against the eager loop bit for bit, both against the oracle chain over
    ten steps.
The kernel-level rows of these networks are in tests/test_kernels_gpu.py, their recorded launches in tests/test_step_launches_gpu.py
(W18-W24)."""
import pytest
import torch

import ddpm_torch
from oracle import diffusion_ref as D
from oracle import unet_ref as U
from tests import channels_accum as CA
from tests import launch_replay as LR
from tests.golden.recipes import check, check_state, rnd
from tests.test_unet_gpu import DEV, FP32_BAR, make

pytestmark = pytest.mark.gpu
GEOMETRY = {(1, 1): (16, 32), (4, 4): (64, 16), (12, 12): (64, 16)}          # (in, out) -> (B, side)


def _reduced_cfg(ch, drop):
    return {k: v for k, v in LR._reduced(mult=(1, 2), drop=drop, ch=ch)["model"].items() if k != "block_size"}


# ------------------------------------------------------------------------------------------------------------------ UNet vs oracle
@pytest.mark.parametrize("dtype,fwd_bar,grad_bar,floor", [(torch.float32, FP32_BAR, 3e-3, 0.02), (torch.bfloat16, 6e-2, 5e-2, 0.1)], ids=["fp32", "bf16"])
@pytest.mark.parametrize("ch", list(GEOMETRY), ids=[f"{a}to{b}" for a, b in GEOMETRY])
def test_reduced_unet_with_edge_channels_forward_backward_vs_oracle(ch, dtype, fwd_bar, grad_bar, floor):
    """Per-tensor gradient error relative to the tensor's largest gradient, floored at 2 % (fp32) / 10 % (bf16) of the median tensor
    scale, as tests/test_odd_geometry_gpu.py measures it; the input gradient is one more tensor of that list."""
    B, side = GEOMETRY[ch]
    cfg = _reduced_cfg(ch, 0.1)
    m, sd = make(cfg, dtype=dtype)
    m.train()
    m.engine().debug_keep_tape = True
    x, gy = rnd(B, ch[0], side, side, seed=3), rnd(B, ch[1], side, side, seed=4)
    t = (torch.arange(B) * 47 + 5) % 1000
    xd = x.to(DEV).clone().requires_grad_(True)
    y = m(xd, t.to(DEV))
    (y * gy.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    masks = CA.masks_from_tape(m, 0.1, DEV)
    p = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    xr = x.clone().requires_grad_(True)
    ref = U.unet_forward(p, cfg, xr, t, training=True, masks=masks)
    (ref * gy).sum().backward()
    rel = float((y.detach().cpu() - ref.detach()).abs().max() / ref.detach().abs().max())
    scales = {k: float(v.grad.abs().max()) for k, v in p.items()}
    fl = floor * sorted(scales.values())[len(scales) // 2]
    rows = sorted(((float((q.grad.cpu() - p[k].grad).abs().max()) / max(scales[k], fl), k) for k, q in m.named_parameters()), reverse=True)
    dx = float((xd.grad.cpu() - xr.grad).abs().max()) / max(float(xr.grad.abs().max()), fl)
    print(f"\nreduced UNet {ch[0]}->{ch[1]} {side}x{side} B={B} {dtype}: fwd rel {rel:.3e}; d/dx {dx:.2e}; worst grads "
          + ", ".join(f"{k}={e:.2e}" for e, k in rows[:4]))
    assert bool(torch.isfinite(xd.grad).all())
    assert rel < fwd_bar, rel
    assert rows[0][0] < grad_bar, rows[:4]
    assert dx < grad_bar, dx


# ------------------------------------------------------------------------------------------------------------------ accumulation
def _accum_case(golden, ch):
    """(cfg, initial state dict, images, lr, lr change, fixture part or None): 3 channels = G19's accum2 run, 12 = the same recipe at
    12 channels on 16 x 16 images."""
    g = golden("g19_accum_wrapper.pt")
    r = g["accum2"]
    if ch == 3:
        cfg, xs = r["cfg"], r["xs"]
    else:
        cfg = CA.edge(r["cfg"], ch, ch)
        gen = torch.Generator().manual_seed(190)
        xs = [torch.rand(4, ch, 16, 16, generator=gen) * 2 - 1 for _ in range(6)]
    torch.manual_seed(g["init_seed"])
    sd = U.randomize_state_dict(ddpm_torch.UNet(**cfg).state_dict(), g["rand_seed"])
    return cfg, sd, xs, g["lr"], r["lr_change"], (r if ch == 3 else None)


def _run_accum(cfg, sd, xs, lr, lr_change, dtype):
    """Six ``Trainer.step`` calls with ``num_accum=2`` on the device, the reference's CPU (t, noise) stream injected; returns the model,
    the trainer, the scheduler and the per-call losses.  Parameters and shadow must be bit-unchanged after the odd calls."""
    m = ddpm_torch.UNet(**cfg)
    m.load_state_dict(sd)
    m.to(DEV).set_compute_dtype(dtype)
    lam = lambda s: 1.0 if s < lr_change else 0.5
    dif = ddpm_torch.GaussianDiffusion(ddpm_torch.get_beta_schedule("linear", 1e-4, 0.02, 1000), "eps", "fixed-large", "mse")
    opt = torch.optim.Adam(m.parameters(), lr=lr, betas=(0.9, 0.999))
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lr_lambda=lam)
    tr = ddpm_torch.Trainer(m, opt, dif, epochs=1, trainloader=None, scheduler=sched, num_accum=2, use_ema=True, grad_norm=1.0,
                            shape=tuple(xs[0].shape[1:]), device=torch.device(DEV), ema_decay=0.9999)
    draw = CA.reference_stream()

    def get_input(x):
        t, noise = draw(x)
        return {"x_0": x.to(DEV), "t": t.to(DEV), "noise": noise.to(DEV)}
    tr.get_input = get_input
    m.train()
    losses = []
    for i, x in enumerate(xs):
        before = CA.snapshot(m, tr.ema)
        tr.stats.reset()
        tr.step(x, global_steps=i + 1)
        losses.append(tr.current_stats["loss"])
        now = CA.snapshot(m, tr.ema)
        if (i + 1) % 2:
            CA.assert_bit_equal(now[0], before[0], "param")
            CA.assert_bit_equal(now[1], before[1], "shadow")
        else:
            assert any(not torch.equal(now[0][k], before[0][k]) for k in now[0])
    assert not tr._direct, "num_accum > 1 must take the generic step"
    return m, tr, sched, torch.tensor(losses, dtype=torch.float64)


@pytest.mark.parametrize("ch", [3, 12])
def test_accumulating_steps_fp32_match_the_oracle_trainer_and_the_reference(golden, ch):
    """Bars of the host test: losses rtol 5e-4, check_state 1e-3 with adam_slack = 0.25 lr updates."""
    cfg, sd, xs, lr, lr_change, fixture = _accum_case(golden, ch)
    m, tr, sched, losses = _run_accum(cfg, sd, xs, lr, lr_change, torch.float32)
    oracle = CA.OracleTrainer(sd, cfg, lr, 2, lambda s: 1.0 if s < lr_change else 0.5)
    ref = torch.tensor([oracle.step(x)[0] for x in xs], dtype=torch.float64)
    print(f"\naccumulation fp32 {ch} channels: losses {losses.tolist()} vs oracle {ref.tolist()}")
    updates = len(xs) // 2
    slack = 0.25 * lr * updates
    state = {k: v.cpu() for k, v in m.state_dict().items()}
    shadow = {k: v.cpu() for k, v in tr.ema.shadow.items()}
    assert torch.allclose(losses, ref, rtol=5e-4), (losses, ref)
    assert tr.ema.num_updates == oracle.num_updates == updates - 1
    assert abs(sched.get_last_lr()[0] - oracle.sched.get_last_lr()[0]) < 1e-15
    check_state(state, oracle.state(), 1e-3, "param", adam_slack=slack)
    check_state(shadow, oracle.shadow, 1e-3, "shadow", adam_slack=slack)
    if fixture is not None:
        assert torch.allclose(losses, fixture["losses"], rtol=5e-4), (losses, fixture["losses"])
        assert tr.ema.num_updates == fixture["num_updates"] and abs(sched.get_last_lr()[0] - fixture["last_lr"]) < 1e-15
        check_state(state, fixture["params"], 1e-3, "param", adam_slack=slack)
        check_state(shadow, fixture["shadow"], 1e-3, "shadow", adam_slack=slack)


@pytest.mark.parametrize("ch", [3, 12])
def test_accumulating_steps_bf16_train_like_fp32(golden, ch):
    """The relation of test_bf16_mode_trains_like_the_fp32_mode — the mean loss of a window of calls within 12 % of the fp32 run's —
    at this length: one window of six calls, same initial weights, same (t, noise) stream."""
    cfg, sd, xs, lr, lr_change, _ = _accum_case(golden, ch)
    _, tr16, _, l16 = _run_accum(cfg, sd, xs, lr, lr_change, torch.bfloat16)
    _, tr32, _, l32 = _run_accum(cfg, sd, xs, lr, lr_change, torch.float32)
    gap = float((l16.mean() - l32.mean()).abs() / l32.mean())
    print(f"\naccumulation {ch} channels: loss fp32 {l32.tolist()}\n{' ' * 25}bf16 {l16.tolist()}\nwindow gap {gap:.3%}")
    assert bool(torch.isfinite(l16).all()) and bool(torch.isfinite(l32).all())
    assert gap < 0.12
    assert tr16.ema.num_updates == tr32.ema.num_updates == 2


# ------------------------------------------------------------------------------------------------------------------ ModelWrapper
def test_wrapped_12_channel_sampler_graph_equals_eager_and_matches_oracle(monkeypatch):
    """ModelWrapper(UNet(12 -> 12), PixelUnshuffle(2), PixelShuffle(2)) on 32 x 32 images (the network sees 12 x 16 x 16), ten ancestral
    steps in fp32: the hipGraph-replayed loop equals the eager loop bit for bit (injected noise and a device seed), and both stay within
    FP32_BAR of oracle.diffusion_ref's loop over the wrapped oracle network on the same (x_T, z_1..z_10)."""
    cfg = _reduced_cfg((12, 12), 0.0)
    unet, sd = make(cfg)
    net = ddpm_torch.ModelWrapper(unet, torch.nn.PixelUnshuffle(2), torch.nn.PixelShuffle(2)).eval()
    steps, shape = 10, (4, 3, 32, 32)
    dif = ddpm_torch.GaussianDiffusion(ddpm_torch.get_beta_schedule("linear", 1e-4, 0.02, steps), "eps", "fixed-large", "mse")
    g = torch.Generator("cpu").manual_seed(31)
    x_T = torch.empty(shape).normal_(generator=g)
    zs = [torch.empty(shape).normal_(generator=g) for _ in range(steps)]
    outs = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("DDPM_TORCH_AMD_GRAPH", mode)
        with torch.inference_mode():
            outs[mode] = dif._sample_loop(net, shape, DEV, x_T, None, z_stream=iter(zs))
        outs[mode + "s"] = dif.p_sample(net, shape=shape, device=DEV, seed=77)
    assert getattr(dif, "_sample_graphs", None), "the sampling step was not captured"
    assert torch.equal(outs["1"], outs["0"]), float((outs["1"] - outs["0"]).abs().max())
    assert torch.equal(outs["1s"], outs["0s"]), float((outs["1s"] - outs["0s"]).abs().max())
    T = D.ddpm_tables(D.beta_schedule("linear", 1e-4, 0.02, steps), "fixed-large")
    wrapped = CA.OracleTrainer(sd, cfg, 1e-3, block=2)
    with torch.no_grad():
        ref = D.sample_loop(T, lambda x, t: wrapped.denoise(x, t, params=sd), x_T, zs)
    err = check(outs["1"], ref, FP32_BAR, name="wrapped chain graph")
    check(outs["0"], ref, FP32_BAR, name="wrapped chain eager")
    print(f"\n10-step chain, wrapped 12 -> 12 on 32x32 fp32: rel err {err:.3e} vs oracle; graph == eager")
