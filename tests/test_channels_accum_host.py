"""Host-logic tests (CPU, emulated ABI) of what the shipped command lines build besides the 3 -> 3 network with one update per step:

  * UNets whose edge channel counts are not 3 — 1 (``--dataset mnist``), 4 and 12 (``--block-size 2``), and the counts at which the
    packed widths change (5 and 8 in fp32, 12 -> 24, 48) — forward, every parameter gradient and the input gradient against the oracle;
  * ``Trainer.step`` with ``num_accum`` in {2, 4}: the generic autograd branch, gradients accumulating over the micro-batches, clip /
    Adam / EMA / scheduler on every N-th call, against a float64 oracle trainer (tests/channels_accum.py) and the reference's own
    Trainer (fixture G19);
  * ``ModelWrapper(UNet(12 -> 12), PixelUnshuffle(2), PixelShuffle(2))``: the generic step with the fused update, and the samplers;
  * the 3-channel step: its launch sequence against a committed list of signatures (tests/golden/w1_host_signatures.txt).

What this found: ``_Engine.forward`` staged the image into a buffer of one 16-byte vector of channels (8 in bf16, 4 in fp32) whatever
``in_channels`` was, so a 12-channel network — every ``--block-size 2`` run on an RGB data set — and any fp32 network with 5 to 8
input channels failed on their first forward (DDPM_ERR_SHAPE from ddpm_nchw_to_nhwc).  The engine now stages at in_conv's packed width."""
import hashlib
import os

import pytest
import torch

import ddpm_torch
from ddpm_torch import _hip
from oracle import diffusion_ref as D
from oracle import unet_ref as U
from tests import abi_emulator
from tests import channels_accum as CA
from tests import launch_replay as LR
from tests.golden.recipes import check, check_state, rnd

pytestmark = pytest.mark.skipif(not os.path.exists(_hip.LIB_PATH), reason="libddpm_hip.so not built")
TINY = CA.TINY
CHANNELS = [(1, 1), (4, 4), (5, 5), (8, 8), (12, 12), (12, 24), (48, 48)]
CPU = torch.device("cpu")


@pytest.fixture
def emu(monkeypatch):
    return abi_emulator.install(monkeypatch, _hip)


def make(cfg, seed=5, dtype=torch.float32, rand=17):
    torch.manual_seed(seed)
    m = ddpm_torch.UNet(**cfg)
    sd = U.randomize_state_dict(m.state_dict(), rand)
    m.load_state_dict(sd)
    m.set_compute_dtype(dtype)
    return m, sd


# ------------------------------------------------------------------------------------------------------------------ UNet vs oracle
@pytest.mark.parametrize("cin,cout", CHANNELS, ids=[f"{a}to{b}" for a, b in CHANNELS])
def test_unet_fp32_forward_backward_and_input_gradient_match_the_oracle(emu, cin, cout):
    """The bars of tests/test_host_emulated.py (forward 2e-5; parameter gradients 2e-4 + 2e-5) and of
    tests/test_trainer_host.py::test_input_gradient_flows_through_the_autograd_node (2e-4 + 2e-6)."""
    cfg = CA.edge(TINY, cin, cout)
    m, sd = make(cfg)
    x, t, gy = rnd(2, cin, 16, 16, seed=3), torch.tensor([7, 912]), rnd(2, cout, 16, 16, seed=4)
    m.eval()
    with torch.no_grad():
        check(m(x, t), U.unet_forward(sd, cfg, x, t), 2e-5, name="fwd")
    m.train()
    xd = x.clone().requires_grad_(True)
    y = m(xd, t)
    (y * gy).sum().backward()
    p = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    xr = x.clone().requires_grad_(True)
    ref = U.unet_forward(p, cfg, xr, t, training=True)
    check(y, ref.detach(), 2e-5, name="train fwd")
    (ref * gy).sum().backward()
    for k, prm in m.named_parameters():
        check(prm.grad, p[k].grad, 2e-4, atol=2e-5, name="grad." + k)
    check(xd.grad, xr.grad, 2e-4, atol=2e-6, name="d/dx")
    eng = m.engine()
    assert eng.convs[id(m.in_conv)].Cp == -(-cin // 4) * 4 and eng.convs[id(m.out_conv[2])].Np == -(-cout // 4) * 4


@pytest.mark.parametrize("cin,cout", CHANNELS, ids=[f"{a}to{b}" for a, b in CHANNELS])
def test_unet_bf16_forward_close_and_gradients_finite(emu, cin, cout):
    """The bar of tests/test_host_emulated.py::test_forward_bf16_close (5e-2 of the output's range).  No host test sets a bar for
    bf16 gradients (the -m gpu twin, tests/test_channels_accum_gpu.py, holds them to the oracle): here the backward must run at the
    bf16 paddings (8-wide vectors), give finite gradients of the right shapes, and an input gradient that points the oracle's way."""
    cfg = CA.edge(TINY, cin, cout)
    m, sd = make(cfg, dtype=torch.bfloat16)
    x, t, gy = rnd(2, cin, 8, 8, seed=2), torch.tensor([10, 500]), rnd(2, cout, 8, 8, seed=4)
    m.eval()
    with torch.no_grad():
        check(m(x, t), U.unet_forward(sd, cfg, x, t), 5e-2, name="fwd_bf16")
    m.train()
    xd = x.clone().requires_grad_(True)
    y = m(xd, t)
    (y * gy).sum().backward()
    p = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    xr = x.clone().requires_grad_(True)
    ref = U.unet_forward(p, cfg, xr, t, training=True)
    check(y, ref.detach(), 5e-2, name="train fwd_bf16")
    (ref * gy).sum().backward()
    for k, prm in m.named_parameters():
        assert prm.grad.shape == prm.shape and bool(torch.isfinite(prm.grad).all()), k
    assert xd.grad.shape == x.shape and bool(torch.isfinite(xd.grad).all())
    cos = float(torch.nn.functional.cosine_similarity(xd.grad.flatten(), xr.grad.flatten(), dim=0))
    print(f"bf16 {cin}->{cout}: cos(d/dx, oracle) = {cos:.4f}")
    assert cos > 0.9
    eng = m.engine()
    assert eng.convs[id(m.in_conv)].Cp == -(-cin // 8) * 8 and eng.convs[id(m.out_conv[2])].Np == -(-cout // 8) * 8


# ------------------------------------------------------------------------------------------------------------------ accumulation
LR_STEP = 1e-3


def _lr_lambda(s):
    return 1.0 if s < 1 else 0.5          # changes after the first UPDATE: inside the window for num_accum 2 and 4 (as G9's does)


def _trainer(model, num_accum, shape, lr=LR_STEP, device=CPU):
    dif = ddpm_torch.GaussianDiffusion(ddpm_torch.get_beta_schedule("linear", 1e-4, 0.02, 1000), "eps", "fixed-large", "mse")
    opt = torch.optim.Adam(model.parameters(), lr=lr, betas=(0.9, 0.999))
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lr_lambda=_lr_lambda)
    tr = ddpm_torch.Trainer(model, opt, dif, epochs=1, trainloader=None, scheduler=sched, num_accum=num_accum, use_ema=True, grad_norm=1.0,
                            shape=shape, device=device, ema_decay=0.9999)
    model.train()
    return opt, sched, tr


def _images(n, B, C, hw, seed=21):
    g = torch.Generator().manual_seed(seed)
    return [torch.rand(B, C, hw, hw, generator=g) * 2 - 1 for _ in range(n)]


@pytest.mark.parametrize("drop", [0.0, 0.1], ids=["nodrop", "drop0.1"])
@pytest.mark.parametrize("ch", [3, 1, 12])
@pytest.mark.parametrize("num_accum", [2, 4])
def test_accumulating_steps_match_the_float64_oracle_trainer(emu, num_accum, ch, drop):
    """Eight ``Trainer.step`` calls.  Bars: those of tests/test_trainer_host.py::test_steps_that_move_the_weights_match_the_reference
    (losses rtol 5e-4; check_state 1e-3 with adam_slack = 0.25 lr updates)."""
    cfg = CA.edge(TINY, ch, ch, drop)
    m, sd = make(cfg, seed=11, rand=23)
    opt, sched, tr = _trainer(m, num_accum, (ch, 8, 8))
    assert tr.generator.device.type == "cpu" and tr.generator.initial_seed() == CA.GEN_SEED
    m.engine().debug_keep_tape = True
    oracle = CA.OracleTrainer(sd, cfg, LR_STEP, num_accum, _lr_lambda)
    calls = 8
    losses, ref = [], []
    for i, x in enumerate(_images(calls, 2, ch, 8)):
        before = CA.snapshot(m, tr.ema)
        tr.stats.reset()
        tr.step(x, global_steps=i + 1)
        losses.append(tr.current_stats["loss"])
        lo, updated = oracle.step(x, masks=CA.masks_from_tape(m, drop, CPU))
        ref.append(lo)
        assert updated == ((i + 1) % num_accum == 0)
        now = CA.snapshot(m, tr.ema)
        if not updated:
            CA.assert_bit_equal(now[0], before[0], "param")
            CA.assert_bit_equal(now[1], before[1], "shadow")
            assert all(p.grad is not None for p in m.parameters())             # ... while the gradients accumulate
        else:
            assert any(not torch.equal(now[0][k], before[0][k]) for k in now[0])
            assert all(p.grad is None for p in m.parameters())
    updates = calls // num_accum
    assert not tr._direct, "num_accum > 1 must take the generic step"
    assert "ddpm_mt_adam_ema" in emu.log
    assert torch.allclose(torch.tensor(losses, dtype=torch.float64), torch.tensor(ref, dtype=torch.float64), rtol=5e-4), (losses, ref)
    assert tr.ema.num_updates == oracle.num_updates == updates - 1
    assert int(opt.state[next(iter(m.parameters()))]["step"]) == updates
    assert abs(sched.get_last_lr()[0] - oracle.sched.get_last_lr()[0]) < 1e-15 and sched.get_last_lr()[0] == LR_STEP * 0.5
    slack = 0.25 * LR_STEP * updates
    check_state(m.state_dict(), oracle.state(), 1e-3, "param", adam_slack=slack)
    check_state(tr.ema.shadow, oracle.shadow, 1e-3, "shadow", adam_slack=slack)


def test_two_forwards_before_one_backward_do_not_alias(emu):
    """Two autograd graphs are built, then ``(l1 + l2).backward()``: the engine shares its GroupNorm workspace and the gradient staging
    buffer between calls, the tapes must not."""
    cfg = CA.edge(TINY, 3, 3, 0.1)
    m, sd = make(cfg)
    m.train()
    eng = m.engine()
    eng.debug_keep_tape = True
    xs = [rnd(2, 3, 16, 16, seed=3), rnd(2, 3, 16, 16, seed=8)]
    ts = [torch.tensor([7, 912]), torch.tensor([401, 0])]
    gys = [rnd(2, 3, 16, 16, seed=4), rnd(2, 3, 16, 16, seed=9)]
    xd = [x.clone().requires_grad_(True) for x in xs]
    ys, masks = [], []
    for x, t in zip(xd, ts):
        ys.append(m(x, t))
        masks.append(CA.masks_from_tape(m, 0.1, CPU))
    ((ys[0] * gys[0]).sum() + (ys[1] * gys[1]).sum()).backward()
    p = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    xr = [x.clone().requires_grad_(True) for x in xs]
    refs = [U.unet_forward(p, cfg, x, t, training=True, masks=mk) for x, t, mk in zip(xr, ts, masks)]
    ((refs[0] * gys[0]).sum() + (refs[1] * gys[1]).sum()).backward()
    for i in range(2):
        check(ys[i], refs[i].detach(), 2e-5, name=f"fwd{i}")
        check(xd[i].grad, xr[i].grad, 2e-4, atol=2e-6, name=f"d/dx{i}")
    for k, prm in m.named_parameters():
        check(prm.grad, p[k].grad, 2e-4, atol=2e-5, name="grad." + k)


# ------------------------------------------------------------------------------------------------------------------ G19
def _g19_oracle_and_product(g, part, emu_device=CPU):
    r = g[part]
    cfg, block, num_accum = r["cfg"], r["block"], r["num_accum"]
    torch.manual_seed(g["init_seed"])
    unet = ddpm_torch.UNet(**cfg)
    sd = U.randomize_state_dict(unet.state_dict(), g["rand_seed"])
    unet.load_state_dict(sd)
    net = unet if block == 1 else ddpm_torch.ModelWrapper(unet, torch.nn.PixelUnshuffle(block), torch.nn.PixelShuffle(block))
    return r, sd, unet, net


@pytest.mark.parametrize("part", ["accum2", "wrapped12"])
def test_reference_trainer_fixture_g19(emu, golden, part):
    """The reference's own Trainer — ``num_accum=2`` for six calls on the tiny net; its ModelWrapper with PixelUnshuffle(2) at 12
    channels for three calls — against the emulated run AND the float64 oracle trainer of this file: the test's reference is pinned
    to upstream."""
    g = golden("g19_accum_wrapper.pt")
    r, sd, unet, net = _g19_oracle_and_product(g, part)
    lam = lambda s: 1.0 if s < r["lr_change"] else 0.5
    dif = ddpm_torch.GaussianDiffusion(ddpm_torch.get_beta_schedule("linear", 1e-4, 0.02, 1000), "eps", "fixed-large", "mse")
    opt = torch.optim.Adam(net.parameters(), lr=g["lr"], betas=(0.9, 0.999))
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lr_lambda=lam)
    tr = ddpm_torch.Trainer(net, opt, dif, epochs=1, trainloader=None, scheduler=sched, num_accum=r["num_accum"], use_ema=True, grad_norm=1.0,
                            shape=tuple(r["xs"][0].shape[1:]), device=CPU, ema_decay=0.9999)
    net.train()
    oracle = CA.OracleTrainer(sd, r["cfg"], g["lr"], r["num_accum"], lam, block=r["block"], seed=g["gen_seed"])
    losses, ref = [], []
    for i, x in enumerate(r["xs"]):
        tr.stats.reset()
        tr.step(x, global_steps=i + 1)
        losses.append(tr.current_stats["loss"])
        ref.append(oracle.step(x)[0])
    updates = len(r["xs"]) // r["num_accum"]
    assert not tr._direct and "ddpm_mt_adam_ema" in emu.log
    assert torch.allclose(torch.tensor(ref, dtype=torch.float64), r["losses"], rtol=2e-4), (ref, r["losses"])       # oracle vs upstream (G9's bar)
    assert torch.allclose(torch.tensor(losses, dtype=torch.float64), r["losses"], rtol=5e-4), (losses, r["losses"])
    assert tr.ema.num_updates == oracle.num_updates == r["num_updates"]
    assert abs(sched.get_last_lr()[0] - r["last_lr"]) < 1e-15
    slack = 0.25 * g["lr"] * updates
    check_state(oracle.state(), r["params"], 5e-4, "oracle.param", adam_slack=slack)
    check_state(oracle.shadow, r["shadow"], 5e-4, "oracle.shadow", adam_slack=slack)
    check_state(CA.strip(net.state_dict()), r["params"], 1e-3, "param", adam_slack=slack)
    check_state(CA.strip(tr.ema.shadow), r["shadow"], 1e-3, "shadow", adam_slack=slack)


# ------------------------------------------------------------------------------------------------------------------ ModelWrapper
def _wrapped(dtype=torch.float32, drop=0.0):
    cfg = CA.edge(TINY, 12, 12, drop)
    unet, sd = make(cfg, seed=11, rand=23, dtype=dtype)
    return cfg, sd, unet, ddpm_torch.ModelWrapper(unet, torch.nn.PixelUnshuffle(2), torch.nn.PixelShuffle(2))


def test_wrapped_12_channel_model_takes_the_generic_step_with_the_fused_update(emu):
    cfg, sd, unet, net = _wrapped()
    opt, sched, tr = _trainer(net, 1, (3, 16, 16))
    oracle = CA.OracleTrainer(sd, cfg, LR_STEP, 1, _lr_lambda, block=2)
    losses, ref = [], []
    for i, x in enumerate(_images(4, 2, 3, 16)):
        tr.stats.reset()
        tr.step(x, global_steps=i + 1)
        losses.append(tr.current_stats["loss"])
        ref.append(oracle.step(x)[0])
    assert not tr._direct, "a ModelWrapper is not a UNet: the generic branch"
    assert "ddpm_mt_adam_ema" in emu.log
    assert all(k.startswith("_model.") for k in tr.ema.shadow)
    assert torch.allclose(torch.tensor(losses, dtype=torch.float64), torch.tensor(ref, dtype=torch.float64), rtol=5e-4), (losses, ref)
    slack = 0.25 * LR_STEP * 4
    check_state(CA.strip(net.state_dict()), oracle.state(), 1e-3, "param", adam_slack=slack)
    check_state(CA.strip(tr.ema.shadow), oracle.shadow, 1e-3, "shadow", adam_slack=slack)


def test_wrapped_model_samples_like_the_oracle_chain(emu):
    """``Trainer.sample_fn`` and ``GaussianDiffusion.p_sample`` over the wrapped model (the sampler reaches the engine through
    ``_engines_of`` of the wrapper): the seeded eager loop equals oracle.diffusion_ref.sample_loop over the wrapped oracle network on
    the same CPU noise stream."""
    cfg, sd, unet, net = _wrapped()
    steps, shape = 6, (2, 3, 16, 16)
    dif = ddpm_torch.GaussianDiffusion(ddpm_torch.get_beta_schedule("linear", 1e-4, 0.02, steps), "eps", "fixed-large", "mse")
    assert [e is unet.engine() for e in dif._engines_of(net)] == [True]
    opt = torch.optim.Adam(net.parameters(), lr=1e-3)
    tr = ddpm_torch.Trainer(net, opt, dif, epochs=1, trainloader=None, use_ema=True, shape=shape[1:], device=CPU)
    net.eval()
    g = torch.Generator("cpu").manual_seed(77)
    x_T = torch.empty(shape).normal_(generator=g)
    zs = [torch.empty(shape).normal_(generator=g) for _ in range(steps)]
    T = D.ddpm_tables(D.beta_schedule("linear", 1e-4, 0.02, steps), "fixed-large")
    oracle = CA.OracleTrainer(sd, cfg, 1e-3, block=2)
    with torch.no_grad():
        ref = D.sample_loop(T, lambda x, t: oracle.denoise(x, t, params=sd), x_T, zs)
    out = dif.p_sample(net, shape=shape, device=CPU, seed=77)
    check(out, ref, 5e-4, name="p_sample")                           # the bar of test_sampling_loop_matches_oracle_with_reference_noise_stream
    out2 = tr.sample_fn(sample_size=2, sample_seed=77)
    assert torch.equal(out, out2)                                    # the shadow equals the live weights before any update
    assert out.shape == shape and "ddpm_p_sample_step" in emu.log


# ------------------------------------------------------------------------------------------------------------------ 3-channel launches
def test_three_channel_step_issues_the_committed_launch_sequence(emu, monkeypatch):
    """W1 (cifar10 train step, dropout 0.1) at B = 2 on the emulator: entry name and argument words of EVERY launch, in order, against
    what the step issued before the staging width followed ``in_channels`` (tests/golden/w1_host_signatures.txt: the distinct launches
    in first-seen order, then the length and SHA-256 of the whole sequence).  Pointer offsets and dropout seeds are dropped: they depend
    on the allocator and on the call count."""
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "w1_host_signatures.txt")
    with open(path) as f:
        lines = [ln for ln in f.read().split("\n") if ln]
    want, (_, count, digest) = lines[:-1], lines[-1].split()
    run = LR.WORKLOADS["W1"][1]("cpu", 2, 32)
    seq, inner = [], _hip._invoke

    def rec(name, args):
        seq.append(LR.short(LR.geometry(LR.signature(name, args), offsets=False)))
        return inner(name, args)
    monkeypatch.setattr(_hip, "_invoke", rec)
    run()
    got = list(dict.fromkeys(seq))
    for i, (a, b) in enumerate(zip(got, want)):
        assert a == b, f"distinct launch {i}: {a} != {b}"
    assert len(got) == len(want), (len(got), len(want))
    assert len(seq) == int(count) and hashlib.sha256("\n".join(seq).encode()).hexdigest() == digest
