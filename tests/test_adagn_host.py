"""CPU, C ABI emulated (tests/abi_emulator.py + tests/adagn_emulator.py): the host side of the scale-shift norm —
``UNet(use_scale_shift_norm=True)`` / ``ResidualBlock(use_scale_shift_norm=True)``, the engine's widened time projection ([scale | shift]
columns, no conv1.bias folded in), the launches of a modulated block, the ``train.py --scale-shift-norm`` / ``generate.py`` round trip — and
the argument validation of the two new entry points in the real library.  The float64 reference is tests/adagn_ref.py; the kernels
themselves are held to it in tests/test_adagn_gpu.py.

Bars: the reduced fp32 network is held to what tests/test_host_emulated.py holds the plain reduced network to (forward 2e-5, gradients
2e-4 with atol 2e-5, of the largest reference magnitude); trainer steps and chains to tests/test_learned_var_host.py's and
tests/test_cond_host.py's (losses rtol 5e-4, states 1e-3 with the Adam slack, chains 2e-4)."""
import glob
import importlib
import json
import os
import sys

import pytest
import torch

import ddpm_torch
from ddpm_torch import _hip
from oracle import diffusion_ref as D
from oracle import unet_ref as U
from tests import abi_emulator, adagn_emulator, batch_emulator, cond_emulator, ddim_emulator, learned_var_emulator, mha_emulator
from tests import adagn_ref as R
from tests import channels_accum as CA
from tests import cond_ref
from tests.golden.recipes import check, check_state, rnd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "ddpm-torch_amd")
if PKG not in sys.path:
    sys.path.insert(0, PKG)
import ddim  # noqa: E402

pytestmark = pytest.mark.skipif(not os.path.exists(_hip.LIB_PATH), reason="libddpm_hip.so not built")
CPU = torch.device("cpu")
NEW = ("ddpm_groupnorm_mod_silu_fwd", "ddpm_groupnorm_mod_silu_bwd")
RED = dict(in_channels=3, hid_channels=64, out_channels=3, ch_multipliers=[1, 2], num_res_blocks=1, apply_attn=[True, True], drop_rate=0.0)
OK, SHAPE, DTYPE, ALIGN, LAUNCH, NULL = 0, 1, 2, 3, 4, 5
FAKE = 0x10000                                  # 16-byte aligned, never dereferenced: validation is on the host
BF16, F32 = 1, 0
K = 3


@pytest.fixture
def emu(monkeypatch):
    e = abi_emulator.install(monkeypatch, _hip)
    return adagn_emulator.attach(mha_emulator.attach(cond_emulator.attach(batch_emulator.attach(learned_var_emulator.attach(ddim_emulator.attach(e))))))


def betas_of(T):
    return ddpm_torch.get_beta_schedule("linear", 1e-4, 0.02, T)


def _make(cfg, dtype=torch.float32, seed=11, rand=23, **kw):
    torch.manual_seed(seed)
    m = ddpm_torch.UNet(**cfg, use_scale_shift_norm=True, **kw)
    sd = U.randomize_state_dict(m.state_dict(), rand)
    m.load_state_dict(sd)
    m.set_compute_dtype(dtype)
    return m, sd


def _res_blocks(m):
    return [b for b in m.modules() if type(b).__name__ == "ResidualBlock"]


# ------------------------------------------------------------------------------------------------------------------ the reference
def test_the_reference_block_is_the_oracle_block_where_the_two_coincide():
    """The two blocks differ in where the embedding enters, so the tie is made where it is exact: a zero fc (scale = shift = 0; no time
    bias) makes both the embedding-free block.  A non-zero fc is checked against the equations written out, and the entry points'
    backward restatement against autograd's derivative of the forward one."""
    g = torch.Generator().manual_seed(1)
    cin, cout, E = 32, 64, 16
    sd = {k: torch.randn(s, generator=g, dtype=torch.float64) * 0.2 for k, s, _ in U._res_keys("b.", cin, cout, E)}
    x, t_emb = torch.randn(2, cin, 4, 6, generator=g, dtype=torch.float64), torch.randn(2, E, generator=g, dtype=torch.float64)
    plain = dict(sd, **{"b.fc.weight": torch.zeros(cout, E, dtype=torch.float64), "b.fc.bias": torch.zeros(cout, dtype=torch.float64)})
    mod = dict(sd, **{"b.fc.weight": torch.zeros(2 * cout, E, dtype=torch.float64), "b.fc.bias": torch.zeros(2 * cout, dtype=torch.float64)})
    assert float((R.residual_block(mod, "b.", x, t_emb) - U.residual_block(plain, "b.", x, t_emb)).abs().max()) <= 1e-12
    saved = U.residual_block
    with R.bound():
        assert U.residual_block is R.residual_block
    assert U.residual_block is saved, "the binding is restored on exit"
    # a non-zero fc: h = norm2 * (1 + scale) + shift, checked by hand on the block's pieces
    mod["b.fc.weight"], mod["b.fc.bias"] = torch.randn(2 * cout, E, generator=g, dtype=torch.float64) * 0.3, torch.randn(2 * cout, generator=g, dtype=torch.float64)
    emb = torch.nn.functional.linear(torch.nn.functional.silu(t_emb), mod["b.fc.weight"], mod["b.fc.bias"])
    h = torch.nn.functional.conv2d(torch.nn.functional.silu(U.group_norm(x, sd["b.norm1.weight"], sd["b.norm1.bias"])), sd["b.conv1.weight"], sd["b.conv1.bias"], padding=1)
    h = U.group_norm(h, sd["b.norm2.weight"], sd["b.norm2.bias"]) * (1 + emb[:, :cout, None, None]) + emb[:, cout:, None, None]
    want = torch.nn.functional.conv2d(torch.nn.functional.silu(h), sd["b.conv2.weight"], sd["b.conv2.bias"], padding=1) \
        + torch.nn.functional.conv2d(x, sd["b.skip.weight"], sd["b.skip.bias"])
    assert float((R.residual_block(mod, "b.", x, t_emb) - want).abs().max()) <= 1e-12
    # entry_bwd is the derivative of entry_fwd (given the forward's own statistics), dropout included
    B, HW, C, G = 3, 10, 64, 32
    xs, dy = torch.randn(B * HW, C, generator=g, dtype=torch.float64) + 1.5, torch.randn(B * HW, C, generator=g, dtype=torch.float64)
    gamma, beta = 1 + 0.3 * torch.randn(C, generator=g, dtype=torch.float64), 0.5 * torch.randn(C, generator=g, dtype=torch.float64)
    md = 0.5 * torch.randn(B, 2 * C + 12, generator=g, dtype=torch.float64)
    for silu, p in ((1, 0.0), (1, 0.1), (0, 0.0)):
        leaves = [v.clone().requires_grad_(True) for v in (xs, gamma, beta, md)]
        y, stats = R.entry_fwd(leaves[0], leaves[1], leaves[2], leaves[3], B, HW, C, G, 1e-6, silu, p, 12345)
        (y * dy).sum().backward()
        dx, dg, db, dmod, _ = R.entry_bwd(xs, dy, gamma, beta, stats.detach(), md, B, HW, C, G, silu, p, 12345)
        for got, leaf in ((dx, leaves[0]), (dg, leaves[1]), (db, leaves[2]), (dmod, leaves[3])):
            want = leaf.grad[:, :2 * C] if leaf is leaves[3] else leaf.grad
            assert float((got - want).abs().max()) <= 1e-11 * (float(want.abs().max()) + 1), (silu, p)
        assert float(leaves[3].grad[:, 2 * C:].abs().max()) == 0, "the padding of a mod row is never read"


# ------------------------------------------------------------------------------------------------------------------ the constructor
def test_constructor_rules():
    RB = ddpm_torch.models.unet.ResidualBlock
    assert RB(32, 64, 128).fc.weight.shape == (64, 128) and not RB(32, 64, 128).use_scale_shift_norm
    on = RB(32, 64, 128, use_scale_shift_norm=True)
    assert on.fc.weight.shape == (128, 128) and on.fc.bias.shape == (128,) and on.use_scale_shift_norm
    assert not ddpm_torch.UNet(**RED).use_scale_shift_norm and ddpm_torch.UNet(**RED, use_scale_shift_norm=True).use_scale_shift_norm
    assert all(b.use_scale_shift_norm for b in _res_blocks(ddpm_torch.UNet(**RED, use_scale_shift_norm=True)))
    for bad in (1, 0, "yes", None, 1.0):
        torch.manual_seed(3)
        before = torch.get_rng_state()
        with pytest.raises(TypeError, match="use_scale_shift_norm"):
            ddpm_torch.UNet(**RED, use_scale_shift_norm=bad)
        assert torch.equal(torch.get_rng_state(), before), "a refused model draws nothing"
        with pytest.raises(TypeError, match="use_scale_shift_norm"):
            RB(32, 64, 128, use_scale_shift_norm=bad)


def test_flag_off_changes_no_parameter_and_flag_on_only_the_fc_shapes():
    torch.manual_seed(5)
    base = ddpm_torch.UNet(**RED)
    torch.manual_seed(5)
    off = ddpm_torch.UNet(**RED, use_scale_shift_norm=False)
    torch.manual_seed(5)
    want = U.init_state_dict(RED)
    a, b = base.state_dict(), off.state_dict()
    assert list(a) == list(b) == list(want) == [k for k, _ in off.named_parameters()]
    assert all(a[k].shape == b[k].shape and torch.equal(a[k], b[k]) and torch.equal(b[k], want[k]) for k in a)
    torch.manual_seed(5)
    on = ddpm_torch.UNet(**RED, use_scale_shift_norm=True).state_dict()
    torch.manual_seed(5)
    want_on = R.init_state_dict(RED)
    assert list(on) == list(a) == list(want_on)
    for k in a:
        if k.endswith(("fc.weight", "fc.bias")):
            assert on[k].shape == (2 * a[k].shape[0],) + tuple(a[k].shape[1:]), k
        else:
            assert on[k].shape == a[k].shape, k
        assert torch.equal(on[k], want_on[k]), k
    # a checkpoint of the other kind fails in load_state_dict with its ordinary shape message
    with pytest.raises(RuntimeError, match="size mismatch.*fc.weight"):
        base.load_state_dict(on)
    with pytest.raises(RuntimeError, match="size mismatch.*fc.weight"):
        ddpm_torch.UNet(**RED, use_scale_shift_norm=True).load_state_dict(a)


# ------------------------------------------------------------------------------------------------------------------ the engine
def _logged(emu, monkeypatch):
    """Record (name, args) of every call next to the emulator's name log."""
    calls = []
    real = emu.call

    def call(name, *args):
        calls.append((name, args))
        return real(name, *args)
    monkeypatch.setattr(_hip, "call", call)
    return calls


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_launches_of_a_modulated_block(emu, monkeypatch, dtype):
    calls = _logged(emu, monkeypatch)
    m, _ = _make(RED, dtype)
    m.train()
    x, t = rnd(3, 3, 8, 8, seed=1), torch.tensor([3, 500, 977])
    (m(x, t) * rnd(3, 3, 8, 8, seed=2)).sum().backward()
    nres = len(_res_blocks(m))
    names = [n for n, _ in calls]
    assert nres == 8 and names.count(NEW[0]) == nres and names.count(NEW[1]) == nres
    # per ResidualBlock one modulated and one plain norm each way (the other plain ones: 7 attention norms and out_conv's)
    assert names.count("ddpm_groupnorm_silu_fwd") == nres + 7 + 1 and names.count("ddpm_groupnorm_silu_bwd") == nres + 7 + 1
    eng = m.engine()
    assert eng.tb_total == sum(2 * b.out_channels for b in _res_blocks(m))
    # conv1 (the convolution in front of a modulated norm) carries its bias and no row bias
    fwd_at = [i for i, n in enumerate(names) if n == NEW[0]]
    for i in fwd_at:
        conv = next(calls[j] for j in range(i - 1, -1, -1) if calls[j][0] == "ddpm_conv2d_nhwc" and calls[j][1][17] == 3)    # the last 3x3 before it
        bias, rowbias = conv[1][5], conv[1][6]
        assert bias != 0 and rowbias == 0
        a = calls[i][1]
        assert a[18] == eng.tb_total and a[17] != 0                                          # mod_ld, mod
    assert not any(c[1][6] for c in calls if c[0] == "ddpm_conv2d_nhwc"), "no convolution of a scale-shift network adds a row bias"
    # the backward writes [dscale | dshift] straight into the block's columns of one [B][tb_total] buffer
    bw = [c[1] for c in calls if c[0] == NEW[1]]
    assert all(a[28] == eng.tb_total and a[26] == eng.tb_total for a in bw)
    offs = sorted((a[27] - min(q[27] for q in bw)) // 4 for a in bw)
    assert offs == sorted(eng.tb_off.values())
    # the flag-off network issues none of the new calls
    calls.clear()
    torch.manual_seed(11)
    off = ddpm_torch.UNet(**RED).set_compute_dtype(dtype)
    off.train()
    (off(x, t) * rnd(3, 3, 8, 8, seed=2)).sum().backward()
    assert not any(n in NEW for n, _ in calls) and sum(1 for n, a in calls if n == "ddpm_conv2d_nhwc" and a[6]) == nres


@pytest.mark.parametrize("drop", [0.0, 0.1])
def test_fp32_forward_and_every_gradient_against_float64(emu, drop):
    cfg = dict(RED, drop_rate=drop)
    m, sd = _make(cfg)
    m.train()
    m.engine().debug_keep_tape = True
    x, t, gy = rnd(3, 3, 8, 8, seed=3), torch.tensor([7, 912, 0]), rnd(3, 3, 8, 8, seed=4)
    y = m(x, t)
    (y * gy).sum().backward()
    masks = CA.masks_from_tape(m, drop, CPU)
    assert (len(masks) == 8) == (drop > 0)
    p = {k: v.double().clone().requires_grad_(True) for k, v in sd.items()}
    ref = R.unet_forward(p, cfg, x.double(), t, training=True, masks=masks)
    check(y, ref.detach(), 2e-5, name="train fwd")
    (ref * gy.double()).sum().backward()
    for k, prm in m.named_parameters():
        check(prm.grad, p[k].grad, 2e-4, atol=2e-5, name="grad." + k)
    for k in ("middle.0.fc.weight", "middle.0.fc.bias", "middle.0.conv1.bias", "middle.0.norm2.weight", "middle.0.norm2.bias"):
        assert float(p[k].grad.abs().max()) > 0, k
    assert dict(m.named_parameters())["middle.0.fc.weight"].grad.shape == (256, 256)
    m.eval()
    with torch.no_grad():
        check(m(x, t), R.unet_forward({k: v.double() for k, v in sd.items()}, cfg, x.double(), t), 2e-5, name="eval fwd")


def test_bf16_mode_follows_the_reference_and_folds_the_conv1_bias_gradient_into_the_weight_gradient(emu):
    m, sd = _make(RED, torch.bfloat16)
    m.train()
    x, t, gy = rnd(3, 3, 8, 8, seed=3), torch.tensor([7, 912, 0]), rnd(3, 3, 8, 8, seed=4)
    y = m(x, t)
    (y * gy).sum().backward()
    with torch.no_grad():
        ref = R.unet_forward({k: v.double() for k, v in sd.items()}, RED, x.double(), t)
    check(y, ref, 5e-2, name="fwd_bf16")
    assert all(torch.isfinite(p.grad).all() and float(p.grad.abs().max()) > 0 for p in m.parameters())


def _trainer(m, dif, lr, num_accum=1, **kw):
    opt = torch.optim.Adam(m.parameters(), lr=lr, betas=(0.9, 0.999))
    return ddpm_torch.Trainer(m, opt, dif, epochs=1, trainloader=None, scheduler=None, num_accum=num_accum, use_ema=True, grad_norm=1.0,
                              shape=(3, 8, 8), device=CPU, ema_decay=0.9999, **kw)


@pytest.mark.parametrize("path", ["plan", False], ids=["plan", "eager"])
def test_three_trainer_steps_match_the_float64_oracle_trainer(emu, monkeypatch, path):
    from ddpm_torch.utils import train as train_mod
    monkeypatch.setattr(train_mod, "_TRAIN_GRAPH", path)
    lr = 1e-3
    m, sd = _make(CA.TINY)
    tr = _trainer(m, ddpm_torch.GaussianDiffusion(betas_of(1000), "eps", "fixed-large", "mse"), lr)
    m.train()
    oracle = CA.OracleTrainer(sd, CA.TINY, lr)
    g = torch.Generator().manual_seed(21)
    losses, ref = [], []
    with R.bound():
        for i in range(3):
            x = torch.rand(2, 3, 8, 8, generator=g) * 2 - 1
            tr.stats.reset()
            tr.step(x, global_steps=i + 1)
            losses.append(tr.current_stats["loss"])
            ref.append(oracle.step(x)[0])
    assert tr._direct and emu.log.count(NEW[1]) == 3 * 8
    if path == "plan":
        ds = next(iter(tr._direct.values()))
        assert ds.plan is not None and ds.last_kind == "plan" and NEW[0] in {n for seg in ds.plan.segments for n, _ in seg}
    assert torch.allclose(torch.tensor(losses, dtype=torch.float64), torch.tensor(ref, dtype=torch.float64), rtol=5e-4), (losses, ref)
    slack = 0.25 * lr * 3
    check_state(m.state_dict(), oracle.state(), 1e-3, "param", adam_slack=slack)
    check_state(tr.ema.shadow, oracle.shadow, 1e-3, "shadow", adam_slack=slack)


def test_generic_step_with_accumulation(emu):
    m, sd = _make(CA.TINY)
    tr = _trainer(m, ddpm_torch.GaussianDiffusion(betas_of(1000), "eps", "fixed-large", "mse"), 1e-3, num_accum=2)
    m.train()
    oracle = CA.OracleTrainer(sd, CA.TINY, 1e-3, num_accum=2)
    g = torch.Generator().manual_seed(5)
    with R.bound():
        for i in range(2):
            x = torch.rand(2, 3, 8, 8, generator=g) * 2 - 1
            tr.stats.reset()
            tr.step(x, global_steps=i + 1)
            lo, _ = oracle.step(x)
            assert abs(tr.current_stats["loss"] - lo) <= 5e-4 * abs(lo)
    assert not tr._direct and NEW[1] in emu.log
    check_state(m.state_dict(), oracle.state(), 1e-3, "param", adam_slack=0.25e-3)


def test_the_adm_combination_trains(emu):
    """Scale-shift norm + heads + class conditioning + a learned-range 2C output: three hybrid Trainer.steps."""
    cfg = dict(RED, out_channels=6)
    m, sd = _make(cfg, num_head_channels=32, num_classes=K)
    tr = _trainer(m, ddpm_torch.GaussianDiffusion(betas_of(1000), "eps", "learned-range", "hybrid"), 1e-3, label_drop=0.25)
    m.train()
    g = torch.Generator().manual_seed(21)
    losses = []
    for i in range(3):
        tr.stats.reset()
        tr.step((torch.rand(3, 3, 8, 8, generator=g) * 2 - 1, torch.randint(0, K, (3,), generator=g)), global_steps=i + 1)
        losses.append(tr.current_stats["loss"])
    assert all(l == l and abs(l) < 1e6 for l in losses), losses
    assert emu.log.count("ddpm_class_embed_bwd") == 3 and emu.log.count(NEW[1]) == 24
    now = m.state_dict()
    assert all(torch.isfinite(v).all() for v in now.values()) and any(not torch.equal(now[k], sd[k]) for k in sd)


# ------------------------------------------------------------------------------------------------------------------ sampling
def test_p_sample_guided_p_sample_and_ddim(emu):
    T, shape = 4, (2, 3, 8, 8)
    x_T, zs = rnd(*shape, seed=7), rnd(T, *shape, seed=8)
    # the unconditional chain: the sampler's [T][tb_total] time table and its gather work unchanged on the widened projection
    m, sd = _make(CA.TINY)
    m.eval()
    sd64 = {k: v.double() for k, v in sd.items()}
    dif = ddpm_torch.GaussianDiffusion(betas_of(T), "eps", "fixed-large", "mse")
    with torch.no_grad():                                         # (as p_sample runs it: the forward keeps no tape and reads the table)
        got = dif._sample_loop(m, shape, CPU, x_T, None, z_stream=iter(zs))
    assert emu.log.count("ddpm_gather_rows_f32") == T and emu.log.count(NEW[0]) == 8 * T and m.engine().tt.shape == (T, m.engine().tb_total)
    net64 = lambda x, t: R.unet_forward(sd64, CA.TINY, x, t)                                  # noqa: E731
    check(got, D.sample_loop(D.ddpm_tables(betas_of(T), "fixed-large"), net64, x_T.double(), zs.double()), 2e-4, name="chain")
    # DDIM-4 on a 40-step schedule
    S = 4
    sub = ddim.get_selection_schedule("linear", size=S, timesteps=40)
    dd = ddim.DDIM(betas_of(40), "eps", "fixed-small", "mse", eta=0.0, subsequence=sub)
    got = dd.p_sample(m, shape, device=CPU, noise=x_T)
    want = D.sample_loop(D.ddim_tables(betas_of(40), "fixed-small", 0.0, sub), net64, x_T.double(), torch.zeros(S, *shape, dtype=torch.float64), timestep_map=sub)
    check(got, want, 2e-4, name="DDIM-4")
    # the guided chain of a class-conditional model
    mc, sdc = _make(CA.TINY, num_classes=K)
    mc.eval()
    sdc64 = {k: v.double() for k, v in sdc.items()}
    y = torch.tensor([2, 0])
    emu.log.clear()
    got = dif._sample_loop(mc, shape, CPU, x_T, None, z_stream=iter(zs), y=y, guidance_scale=2.0)
    assert emu.log.count("ddpm_p_sample_step_cfg") == T and "ddpm_gather_rows_f32" not in emu.log

    def netc(x, t, yy):
        with R.bound():
            return cond_ref.unet_forward(sdc64, CA.TINY, x, t, yy)
    check(got, cond_ref.guided_chain(D.ddpm_tables(betas_of(T), "fixed-large"), "eps", netc, x_T.double(), zs.double(), y, K, 2.0), 2e-4, name="guided chain")


# ------------------------------------------------------------------------------------------------------------------ command lines
TINY_CFG = {
    "dataset": "cifar10",
    "diffusion": {"timesteps": 8, "beta_start": 1e-4, "beta_end": 0.02, "beta_schedule": "linear", "model_mean_type": "eps"},
    "model": {"in_channels": 3, "hid_channels": 32, "ch_multipliers": [1, 2], "num_res_blocks": 1, "apply_attn": [False, True], "drop_rate": 0.1},
    "train": {"lr": 2e-4, "batch_size": 4, "grad_norm": 1.0, "epochs": 1, "warmup": 10, "use_ema": True, "ema_decay": 0.9999},
}


def test_train_then_generate_round_trip_with_the_checkpoint_deciding(emu, tmp_path, monkeypatch):
    cfg = tmp_path / "tiny.json"
    cfg.write_text(json.dumps(TINY_CFG))
    monkeypatch.setenv("DDPM_TORCH_AMD_SYNTHETIC_DATA", "8")
    monkeypatch.chdir(tmp_path)
    train = importlib.import_module("train")
    common = ["--train-device", "cpu", "--dry-run", "--num-samples", "2", "--num-workers", "0", "--compute", "fp32"]
    tr = train.main(["--config-path", str(cfg), "--scale-shift-norm", "--chkpt-dir", str(tmp_path / "chk"), "--image-dir", str(tmp_path / "img")] + common)
    assert tr.model.use_scale_shift_norm and NEW[0] in emu.log and NEW[1] in emu.log
    chk = tmp_path / "chk" / "tiny" / "tiny_1.pt"
    assert chk.exists() and (tmp_path / "img" / "train" / "tiny" / "1.jpg").exists()
    rec = json.load(open(glob.glob(str(tmp_path / "chk" / "tiny" / "exp_*.info"))[0]))
    assert rec["model"]["use_scale_shift_norm"] is True
    assert torch.load(chk, weights_only=False)["model"]["middle.0.fc.weight"].shape == (128, 128)
    # the config's model section wins over the flag; without either the network is the plain one
    named = tmp_path / "named.json"
    named.write_text(json.dumps(dict(TINY_CFG, model=dict(TINY_CFG["model"], use_scale_shift_norm=False))))
    tr2 = train.main(["--config-path", str(named), "--scale-shift-norm", "--chkpt-dir", str(tmp_path / "chk2"), "--image-dir", str(tmp_path / "img2")] + common)
    assert not tr2.model.use_scale_shift_norm
    emu.log.clear()
    tr3 = train.main(["--config-path", str(cfg), "--chkpt-dir", str(tmp_path / "chk3"), "--image-dir", str(tmp_path / "img3")] + common)
    assert not tr3.model.use_scale_shift_norm and NEW[0] not in emu.log
    # generate.py: the checkpoint decides (fc.weight has 2 Cout rows), whatever the configuration's model section says
    gen = importlib.import_module("generate")
    from PIL import Image
    gcfg = tmp_path / "tiny_gen.json"                              # generate.py reads the variance and loss types from the configuration
    gcfg.write_text(json.dumps(dict(TINY_CFG, diffusion=dict(TINY_CFG["diffusion"], model_var_type="fixed-large", loss_type="mse"))))
    for ck, want in ((chk, True), (tmp_path / "chk3" / "tiny" / "tiny_1.pt", False)):
        emu.log.clear()
        out = gen.main(["--config-path", str(gcfg), "--device", "cpu", "--chkpt-path", str(ck), "--total-size", "2", "--batch-size", "2",
                        "--save-dir", str(tmp_path / f"g{int(want)}"), "--compute", "fp32", "--seed", "7"])
        files = glob.glob(os.path.join(out, "*.png"))
        assert len(files) == 2 and Image.open(files[0]).size == (32, 32)
        assert (NEW[0] in emu.log) == want


# ------------------------------------------------------------------------------------------------------------------ the real library
def test_the_two_entry_points_are_declared_bound_and_known_to_the_plan_executor():
    lib = _hip.lib()
    header = open(os.path.join(ROOT, "include", "ddpm_hip.h")).read()
    for name, nargs in zip(NEW, (21, 31)):
        assert f"int {name}(" in header and len(_hip.PROTOTYPES[name]) == nargs
        assert lib.ddpm_plan_entry_arity(name.encode()) == nargs
    for text in ("mod_ld >= 2C", "scale s in columns [0, C), shift h in [C, 2C)", "OVERWRITTEN", "bit for bit"):
        assert text in header, text
    # the parameter lists are the plain pair's with (mod, mod_ld) [+ (dmod, dmod_ld)] in front of (dtype, stream)
    P, L = _hip.P, _hip.L
    f, b = list(_hip.PROTOTYPES[NEW[0]]), list(_hip.PROTOTYPES[NEW[1]])
    assert f[:-4] + f[-2:] == list(_hip.PROTOTYPES["ddpm_groupnorm_silu_fwd"]) and f[-4:-2] == [P, L]
    assert b[:-6] + b[-2:] == list(_hip.PROTOTYPES["ddpm_groupnorm_silu_bwd"]) and b[-6:-2] == [P, L, P, L]


def fwd(x=FAKE, x_ld=128, y=FAKE, y_ld=128, gamma=FAKE, beta=FAKE, stats=FAKE, ws=FAKE, B=2, HW=64, C=128, G=32, mod=FAKE, mod_ld=256, dtype=BF16):
    return _hip.lib().ddpm_groupnorm_mod_silu_fwd(x, x_ld, y, y_ld, gamma, beta, stats, ws, B, HW, C, G, 1e-6, 1, 0.0, 0, 0, mod, mod_ld, dtype, 0)


def bwd(x=FAKE, x_ld=128, dy=FAKE, dy_ld=128, dx=FAKE, dx_ld=128, gamma=FAKE, beta=FAKE, stats=FAKE, ws=FAKE, B=2, HW=64, C=128, G=32,
        add=0, add_ld=0, mod=FAKE, mod_ld=256, dmod=FAKE, dmod_ld=256, dtype=BF16):
    return _hip.lib().ddpm_groupnorm_mod_silu_bwd(x, x_ld, dy, dy_ld, dx, dx_ld, gamma, beta, stats, 0, 0, ws, B, HW, C, G, 1, 0.0, 0, 0, 0, 0, 0,
                                                  add, add_ld, mod, mod_ld, dmod, dmod_ld, dtype, 0)


def test_argument_validation_returns_status_codes_without_a_gpu():
    """Every call here is REFUSED on the host: an accepted one would launch on these fake addresses wherever a GPU is present."""
    for name in ("x", "y", "gamma", "beta", "ws", "mod"):
        assert fwd(**{name: 0}) == NULL, name
    for name in ("x", "dy", "dx", "gamma", "beta", "stats", "ws", "mod", "dmod"):
        assert bwd(**{name: 0}) == NULL, name
    for f in (fwd, bwd):
        assert f(mod_ld=255) == SHAPE and f(mod_ld=0) == SHAPE and f(mod_ld=-256) == SHAPE
        assert f(dtype=7) == DTYPE
        assert f(C=100, mod_ld=200) == SHAPE                                              # 100 channels in 32 groups
        assert f(G=0) == SHAPE and f(B=0) == SHAPE and f(HW=0) == SHAPE and f(G=128) == SHAPE
        assert f(x=FAKE + 2) == ALIGN and f(x_ld=128 + 4) == ALIGN
        assert f(C=4096, x_ld=4096, mod_ld=8192) == SHAPE                                 # past the kernels' channel limit
    assert bwd(dmod_ld=255) == SHAPE and bwd(dmod_ld=0) == SHAPE
    assert fwd(y=FAKE + 8) == ALIGN and fwd(y_ld=128 + 4) == ALIGN
    assert bwd(dy_ld=128 + 4) == ALIGN and bwd(dx_ld=128 + 4) == ALIGN and bwd(dy=FAKE + 2) == ALIGN
    assert bwd(add=FAKE + 2, add_ld=128) == ALIGN and bwd(add=FAKE, add_ld=128 + 4) == ALIGN
    # the plain entry points refuse the same arguments with the same codes
    lib = _hip.lib()
    assert lib.ddpm_groupnorm_silu_fwd(0, 128, FAKE, 128, FAKE, FAKE, FAKE, FAKE, 2, 64, 128, 32, 1e-6, 1, 0.0, 0, 0, BF16, 0) == NULL
    assert lib.ddpm_groupnorm_silu_fwd(FAKE, 128, FAKE, 128, FAKE, FAKE, FAKE, FAKE, 2, 64, 100, 32, 1e-6, 1, 0.0, 0, 0, BF16, 0) == SHAPE
    with pytest.raises(RuntimeError, match="bad shape"):
        _hip.call(NEW[0], FAKE, 128, FAKE, 128, FAKE, FAKE, FAKE, FAKE, 2, 64, 128, 32, 1e-6, 1, 0.0, 0, 0, FAKE, 255, BF16, 0)
