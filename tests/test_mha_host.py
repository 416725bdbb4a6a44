"""CPU, C ABI emulated (tests/abi_emulator.py + tests/mha_emulator.py): the host side of multi-head attention — ``UNet(num_heads=)`` /
``UNet(num_head_channels=)``, ``AttentionBlock(num_heads=)``, the engine's per-mode dispatch (``ddpm_attention_mh_*`` in the bf16 mode, the
materialised products per head in the fp32 mode), the ``train.py --num-heads`` / ``generate.py`` round trip — and the argument validation of
the two new entry points in the real library.  The float64 reference is tests/mha_ref.py; the kernels themselves are held to it in
tests/test_mha_gpu.py.

Bars: the reduced fp32 network is held to what tests/test_host_emulated.py holds the single-head reduced network to (forward 2e-5,
gradients 2e-4 with atol 2e-5, of the largest reference magnitude); the bf16 mode to that file's bf16 bar (5e-2)."""
import glob
import importlib
import json
import os
import sys

import pytest
import torch
import torch.nn.functional as F

import ddpm_torch
from ddpm_torch import _hip
from oracle import unet_ref as U
from tests import abi_emulator, batch_emulator, cond_emulator, ddim_emulator, learned_var_emulator, mha_emulator
from tests import mha_ref as R
from tests.golden.recipes import check, rnd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "ddpm-torch_amd")
if PKG not in sys.path:
    sys.path.insert(0, PKG)

pytestmark = pytest.mark.skipif(not os.path.exists(_hip.LIB_PATH), reason="libddpm_hip.so not built")
CPU = torch.device("cpu")
NEW = ("ddpm_attention_mh_fwd", "ddpm_attention_mh_bwd")
# the reduced network: attention on both levels and in the middle; num_head_channels=32 gives 2 heads over 64 and 4 over 128 channels
RED = dict(in_channels=3, hid_channels=64, out_channels=3, ch_multipliers=[1, 2], num_res_blocks=1, apply_attn=[True, True], drop_rate=0.0)
OK, SHAPE, DTYPE, ALIGN, LAUNCH, NULL = 0, 1, 2, 3, 4, 5
FAKE = 0x10000                                  # 16-byte aligned, never dereferenced: validation is on the host
BF16, F32 = 1, 0


@pytest.fixture
def emu(monkeypatch):
    e = abi_emulator.install(monkeypatch, _hip)
    return mha_emulator.attach(cond_emulator.attach(batch_emulator.attach(learned_var_emulator.attach(ddim_emulator.attach(e)))))


def betas_of(T):
    return ddpm_torch.get_beta_schedule("linear", 1e-4, 0.02, T)


def _make(cfg, dtype=torch.float32, seed=11, rand=23, **kw):
    torch.manual_seed(seed)
    m = ddpm_torch.UNet(**cfg, **kw)
    sd = U.randomize_state_dict(m.state_dict(), rand)
    m.load_state_dict(sd)
    m.set_compute_dtype(dtype)
    return m, sd


def _blocks(m):
    return [b for b in m.modules() if type(b).__name__ == "AttentionBlock"]


# ------------------------------------------------------------------------------------------------------------------ the reference
def test_the_reference_is_the_oracle_at_one_head_and_sdpa_at_several():
    g = torch.Generator().manual_seed(1)
    q, k, v = (torch.randn(2, 64, 3, 5, generator=g, dtype=torch.float64) for _ in range(3))
    assert torch.equal(R.attention_core_mh(q, k, v, 1), U.attention_core(q, k, v))
    saved = U.attention_core
    with R.bound(num_heads=1):
        assert U.attention_core is not saved and torch.equal(U.attention_core(q, k, v), saved(q, k, v))
    assert U.attention_core is saved, "the binding is restored on exit"
    for heads in (2, 4):
        d = 64 // heads
        split = lambda z: z.reshape(2, heads, d, 15).transpose(2, 3)                       # noqa: E731  [B][H][L][d]
        want = F.scaled_dot_product_attention(split(q), split(k), split(v)).transpose(2, 3).reshape(2, 64, 3, 5)
        got = R.attention_core_mh(q, k, v, heads)
        assert float((got - want).abs().max()) <= 1e-12
        assert float((got - U.attention_core(q, k, v)).abs().max()) > 1e-3, "several heads are not the single head"
        # the entry points' restatement is the same function on the packed layout
        packed = torch.cat([z.reshape(2, 64, 15).transpose(1, 2) for z in (q, k, v)], dim=-1).reshape(30, 192)
        o, lse = R.entry_fwd(packed, 2, 15, 64, heads, d ** -0.5)
        assert float((o.reshape(2, 15, 64).transpose(1, 2).reshape(2, 64, 3, 5) - want).abs().max()) <= 1e-12 and lse.shape == (2, heads, 15)
        # ... and its backward is autograd's
        leaf = packed.clone().requires_grad_(True)
        d_o = torch.randn(30, 64, generator=g, dtype=torch.float64)
        (R.entry_fwd(leaf, 2, 15, 64, heads, d ** -0.5)[0] * d_o).sum().backward()
        D, grad = R.entry_bwd(packed, o, d_o, lse, 2, 15, 64, heads, d ** -0.5)
        assert float((grad - leaf.grad).abs().max()) <= 1e-12 * float(leaf.grad.abs().max()) + 1e-13 and D.shape == (2, heads, 15)


# ------------------------------------------------------------------------------------------------------------------ the constructor
def test_constructor_rules():
    assert [b.num_heads for b in _blocks(ddpm_torch.UNet(**RED))] == [1] * 7
    assert [b.num_heads for b in _blocks(ddpm_torch.UNet(**RED, num_heads=4))] == [4] * 7
    by_width = ddpm_torch.UNet(**RED, num_head_channels=32)
    assert [(b.in_channels, b.num_heads) for b in _blocks(by_width)] == [(64, 2), (128, 4), (128, 4), (64, 2), (64, 2), (128, 4), (128, 4)]
    assert by_width.num_head_channels == 32 and by_width.num_heads == 1
    assert ddpm_torch.models.unet.AttentionBlock(96, num_heads=3).num_heads == 3 and ddpm_torch.models.unet.AttentionBlock(96).num_heads == 1
    with pytest.raises(ValueError, match="not both"):
        ddpm_torch.UNet(**RED, num_heads=2, num_head_channels=32)
    with pytest.raises(ValueError, match="level_0"):
        ddpm_torch.UNet(**RED, num_head_channels=128)              # 64 % 128
    with pytest.raises(ValueError, match="level_1"):
        ddpm_torch.UNet(**dict(RED, hid_channels=96, apply_attn=[False, True]), num_head_channels=128)     # 96 is not attended; 192 % 128
    with pytest.raises(ValueError, match="level_0"):
        ddpm_torch.UNet(**dict(RED, hid_channels=96), num_heads=64)                                       # 96 % 64
    for name in ("num_heads", "num_head_channels"):
        for bad in (0, -2, 2.5, True):
            with pytest.raises(ValueError, match=name):
                ddpm_torch.UNet(**RED, **{name: bad})
    with pytest.raises(ValueError, match="num_heads"):
        ddpm_torch.models.unet.AttentionBlock(64, num_heads=3)


def test_level_named_in_the_error_is_the_first_that_fails():
    # 96 -> 192 channels: 64-channel heads divide level 1 (and the middle) but not level 0
    with pytest.raises(ValueError, match="level_0"):
        ddpm_torch.UNet(**dict(RED, hid_channels=96), num_head_channels=64)
    assert [b.num_heads for b in _blocks(ddpm_torch.UNet(**dict(RED, hid_channels=96, apply_attn=[False, True]), num_head_channels=64))] == [3] * 4


def test_the_head_count_changes_no_parameter():
    models = {}
    for heads in (1, 2, 4):
        torch.manual_seed(5)
        models[heads] = ddpm_torch.UNet(**RED, num_heads=heads)
    torch.manual_seed(5)
    models["width"] = ddpm_torch.UNet(**RED, num_head_channels=32)
    torch.manual_seed(5)
    want = U.init_state_dict(RED)
    for key, m in models.items():
        sd = m.state_dict()
        assert list(sd) == list(want) == [k for k, _ in m.named_parameters()], key
        assert all(sd[k].shape == want[k].shape and torch.equal(sd[k], want[k]) for k in want), key
    models[1].load_state_dict(models[4].state_dict())                  # strict: no new key either way


# ------------------------------------------------------------------------------------------------------------------ the engine
def _attention_names(log):
    return [n for n in log if n.startswith("ddpm_attention") or n.startswith("ddpm_softmax")]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_the_default_head_count_issues_the_launches_it_issued(emu, dtype):
    m, _ = _make(RED, dtype)
    m.train()
    x, t = rnd(3, 3, 8, 8, seed=1), torch.tensor([3, 500, 977])
    (m(x, t) * rnd(3, 3, 8, 8, seed=2)).sum().backward()
    names = _attention_names(emu.log)
    assert not any(n.startswith("ddpm_attention_mh") for n in emu.log)
    if dtype == torch.bfloat16:                                          # 64 and 16 tokens: the on-chip pair, seven blocks
        assert names == ["ddpm_attention_fwd_lse"] * 7 + ["ddpm_attention_bwd"] * 7
    else:
        assert names == ["ddpm_softmax_fwd"] * 7 + ["ddpm_softmax_bwd"] * 7
    # ... and the head-counted network differs from it in the attention core's launches alone
    one = [n for n in emu.log if n not in names and n != "ddpm_gemm"]
    emu.log.clear()
    m2, _ = _make(RED, dtype, num_heads=2)
    m2.train()
    (m2(x, t) * rnd(3, 3, 8, 8, seed=2)).sum().backward()
    assert [n for n in emu.log if n not in _attention_names(emu.log) and n != "ddpm_gemm"] == one


def test_fp32_forward_and_every_gradient_against_float64(emu):
    """num_head_channels=32 -> 2 and 4 heads; the materialised products per head, one softmax launch per block over H * B * L rows."""
    m, sd = _make(RED, num_head_channels=32)
    m.train()
    x, t, gy = rnd(3, 3, 8, 8, seed=3), torch.tensor([7, 912, 0]), rnd(3, 3, 8, 8, seed=4)
    y = m(x, t)
    (y * gy).sum().backward()
    assert not any(n.startswith("ddpm_attention") for n in emu.log), "the fp32 mode has no attention kernel: gemm + softmax per head"
    assert emu.log.count("ddpm_softmax_fwd") == 7 and emu.log.count("ddpm_softmax_bwd") == 7
    p = {k: v.double().clone().requires_grad_(True) for k, v in sd.items()}
    ref = R.unet_forward(p, RED, x.double(), t, num_head_channels=32, training=True)
    check(y, ref.detach(), 2e-5, name="train fwd")
    (ref * gy.double()).sum().backward()
    for k, prm in m.named_parameters():
        check(prm.grad, p[k].grad, 2e-4, atol=2e-5, name="grad." + k)
    # the same weights under one head are a different function: the reference above is not satisfied by ignoring the heads
    with torch.no_grad():
        single = U.unet_forward({k: v.double() for k, v in sd.items()}, RED, x.double(), t)
    assert float((single - ref.detach()).abs().max()) > 1e-2 * float(ref.detach().abs().max())
    m.eval()
    with torch.no_grad():
        check(m(x, t), R.unet_forward({k: v.double() for k, v in sd.items()}, RED, x.double(), t, num_head_channels=32), 2e-5, name="eval fwd")


def test_bf16_takes_the_head_indexed_kernels_with_per_head_statistics(emu):
    m, sd = _make(RED, torch.bfloat16, num_head_channels=32)
    m.train()
    m.engine().debug_keep_tape = True
    x, t, gy = rnd(3, 3, 8, 8, seed=3), torch.tensor([7, 912, 0]), rnd(3, 3, 8, 8, seed=4)
    y = m(x, t)
    (y * gy).sum().backward()
    assert _attention_names(emu.log) == ["ddpm_attention_mh_fwd"] * 7 + ["ddpm_attention_mh_bwd"] * 7
    lses = [(r[1].num_heads, tuple(r[9].shape)) for r in m.engine().last_tape if r[0] == "attn"]
    assert lses == [(2, (3, 2, 64))] + [(4, (3, 4, 16))] * 4 + [(2, (3, 2, 64))] * 2       # [B][H][L]
    sd64 = {k: v.double() for k, v in sd.items()}
    with torch.no_grad():
        ref = R.unet_forward(sd64, RED, x.double(), t, num_head_channels=32)
    check(y, ref, 5e-2, name="fwd_bf16")
    assert all(torch.isfinite(p.grad).all() and float(p.grad.abs().max()) > 0 for p in m.parameters())
    # inference saves nothing: lse = NULL
    m.eval()
    emu.log.clear()
    with torch.no_grad():
        check(m(x, t), ref, 5e-2, name="eval fwd_bf16")
    assert _attention_names(emu.log) == ["ddpm_attention_mh_fwd"] * 7


def test_a_head_width_the_kernels_do_not_serve_takes_the_materialised_path_in_bf16(emu):
    cfg = dict(RED, hid_channels=96, apply_attn=[False, True])           # 192 channels in 4 heads of 48: no multiple of 32
    m, sd = _make(cfg, torch.bfloat16, num_heads=4)
    m.eval()
    x, t = rnd(2, 3, 8, 8, seed=3), torch.tensor([7, 912])
    with torch.no_grad():
        y = m(x, t)
        ref = R.unet_forward({k: v.double() for k, v in sd.items()}, cfg, x.double(), t, num_heads=4)
    assert not any(n.startswith("ddpm_attention") for n in emu.log) and emu.log.count("ddpm_softmax_fwd") == 4
    check(y, ref, 5e-2, name="fwd_bf16 d=48")
    with pytest.raises(NotImplementedError, match="token count that is a multiple of 4"):      # that path's restriction and message stay
        _make(RED, num_heads=2)[0].eval()(rnd(1, 3, 6, 6, seed=1), torch.tensor([5]))
    with pytest.raises(NotImplementedError, match="head width must be a multiple of 4"):      # 192 channels in 64 heads of 3
        _make(cfg, num_heads=64)[0].eval()(x, t)


def test_the_adm_combination_trains_and_samples(emu):
    """Heads + class conditioning + a learned-range 2C output: three hybrid Trainer.steps, then sampling with labels.  (A learned
    variance samples at guidance scale 1 only — diffusion.py refuses any other — so the guided chain runs on a fixed-variance twin.)"""
    K = 3
    cfg = dict(RED, out_channels=6)
    m, sd = _make(cfg, num_head_channels=32, num_classes=K)
    dif = ddpm_torch.GaussianDiffusion(betas_of(1000), "eps", "learned-range", "hybrid")
    opt = torch.optim.Adam(m.parameters(), lr=1e-3, betas=(0.9, 0.999))
    tr = ddpm_torch.Trainer(m, opt, dif, epochs=1, trainloader=None, scheduler=None, num_accum=1, use_ema=True, grad_norm=1.0, shape=(3, 8, 8),
                            device=CPU, ema_decay=0.9999, label_drop=0.25)
    m.train()
    g = torch.Generator().manual_seed(21)
    losses = []
    for i in range(3):
        tr.stats.reset()
        tr.step((torch.rand(3, 3, 8, 8, generator=g) * 2 - 1, torch.randint(0, K, (3,), generator=g)), global_steps=i + 1)
        losses.append(tr.current_stats["loss"])
    assert all(l == l and abs(l) < 1e6 for l in losses), losses
    assert emu.log.count("ddpm_class_embed_bwd") == 3 and emu.log.count("ddpm_softmax_bwd") == 21 and "ddpm_attention_bwd" not in emu.log
    now = m.state_dict()
    assert all(torch.isfinite(v).all() for v in now.values()) and any(not torch.equal(now[k], sd[k]) for k in sd)
    m.eval()
    y = torch.tensor([2, 0])
    small = ddpm_torch.GaussianDiffusion(betas_of(3), "eps", "learned-range", "hybrid")
    emu.log.clear()
    out = small.p_sample(m, (2, 3, 8, 8), device=CPU, y=y, guidance_scale=1.0)
    assert out.shape == (2, 3, 8, 8) and torch.isfinite(out).all() and emu.log.count("ddpm_p_sample_step_lv") == 3
    twin, _ = _make(RED, num_head_channels=32, num_classes=K)
    twin.eval()
    emu.log.clear()
    out = ddpm_torch.GaussianDiffusion(betas_of(3), "eps", "fixed-large", "mse").p_sample(twin, (2, 3, 8, 8), device=CPU, y=y, guidance_scale=2.0)
    assert out.shape == (2, 3, 8, 8) and torch.isfinite(out).all() and emu.log.count("ddpm_p_sample_step_cfg") == 3


# ------------------------------------------------------------------------------------------------------------------ command lines
TINY_CFG = {
    "dataset": "cifar10",
    "diffusion": {"timesteps": 8, "beta_start": 1e-4, "beta_end": 0.02, "beta_schedule": "linear", "model_mean_type": "eps"},
    "model": {"in_channels": 3, "hid_channels": 32, "ch_multipliers": [1, 2], "num_res_blocks": 1, "apply_attn": [False, True], "drop_rate": 0.1},
    "train": {"lr": 2e-4, "batch_size": 4, "grad_norm": 1.0, "epochs": 1, "warmup": 10, "use_ema": True, "ema_decay": 0.9999},
}


def test_train_then_generate_round_trip_with_heads(emu, tmp_path, monkeypatch):
    cfg = tmp_path / "tiny.json"
    cfg.write_text(json.dumps(TINY_CFG))
    monkeypatch.setenv("DDPM_TORCH_AMD_SYNTHETIC_DATA", "8")
    monkeypatch.chdir(tmp_path)
    train = importlib.import_module("train")
    tr = train.main(["--config-path", str(cfg), "--train-device", "cpu", "--dry-run", "--num-samples", "2", "--num-workers", "0", "--compute", "fp32",
                     "--num-heads", "2", "--chkpt-dir", str(tmp_path / "chk"), "--image-dir", str(tmp_path / "img")])
    assert [b.num_heads for b in _blocks(tr.model)] == [2] * 4
    chk = tmp_path / "chk" / "tiny" / "tiny_1.pt"
    assert chk.exists() and (tmp_path / "img" / "train" / "tiny" / "1.jpg").exists()
    rec = json.load(open(glob.glob(str(tmp_path / "chk" / "tiny" / "exp_*.info"))[0]))
    assert rec["model"]["num_heads"] == 2 and "num_head_channels" not in rec["model"]
    # the config's model section wins over the flags
    named = tmp_path / "named.json"
    named.write_text(json.dumps(dict(TINY_CFG, model=dict(TINY_CFG["model"], num_head_channels=32))))
    tr2 = train.main(["--config-path", str(named), "--train-device", "cpu", "--dry-run", "--num-samples", "2", "--num-workers", "0", "--compute", "fp32",
                      "--num-heads", "4", "--chkpt-dir", str(tmp_path / "chk2"), "--image-dir", str(tmp_path / "img2")])
    assert [b.num_heads for b in _blocks(tr2.model)] == [2] * 4               # 64 channels / 32
    gen = importlib.import_module("generate")
    from PIL import Image
    base = dict(TINY_CFG, diffusion=dict(TINY_CFG["diffusion"], model_var_type="fixed-large", loss_type="mse"))
    gcfg = tmp_path / "tiny_gen.json"                              # generate.py reads the variance and loss types from the configuration
    gcfg.write_text(json.dumps(dict(base, model=dict(base["model"], num_heads=2))))
    plain = tmp_path / "tiny_plain.json"
    plain.write_text(json.dumps(base))
    seen = []
    real = ddpm_torch.UNet

    class Spy(real):                                               # the networks generate.py builds
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            seen.append(self)
    monkeypatch.setattr(ddpm_torch, "UNet", Spy)
    for conf, extra, want in ((gcfg, [], 2), (plain, ["--num-heads", "2"], 2), (plain, [], 1), (gcfg, ["--num-heads", "4"], 2)):
        emu.log.clear()
        out = gen.main(["--config-path", str(conf), "--device", "cpu", "--chkpt-path", str(chk), "--total-size", "2", "--batch-size", "2",
                        "--save-dir", str(tmp_path / f"g{len(seen)}"), "--compute", "fp32", "--seed", "7"] + extra)
        files = glob.glob(os.path.join(out, "*.png"))
        assert len(files) == 2 and Image.open(files[0]).size == (32, 32)
        assert [b.num_heads for b in _blocks(seen[-1])] == [want] * 4
    bpd = importlib.import_module("eval_bpd")
    args = bpd.parse_args(["--num-head-channels", "32"])
    assert args.num_head_channels == 32 and args.num_heads == 1


# ------------------------------------------------------------------------------------------------------------------ the real library
def test_the_two_entry_points_are_declared_bound_and_known_to_the_plan_executor():
    lib = _hip.lib()
    header = open(os.path.join(ROOT, "include", "ddpm_hip.h")).read()
    for name, nargs in zip(NEW, (12, 17)):
        assert f"int {name}(" in header and len(_hip.PROTOTYPES[name]) == nargs
        assert lib.ddpm_plan_entry_arity(name.encode()) == nargs
    # the parameter lists are the streaming pair's with `heads` after C
    for mh, one in zip(NEW, ("ddpm_attention_stream_fwd", "ddpm_attention_stream_bwd")):
        p = list(_hip.PROTOTYPES[mh])
        at = len(p) - 4                                           # ..., C, heads, scale, dtype, stream
        assert p[:at] + p[at + 1:] == list(_hip.PROTOTYPES[one]) and p[at] == p[at - 1]


def fwd(qkv=FAKE, ld=3 * 128, out=FAKE, out_ld=128, lse=0, B=2, L=100, C=128, heads=2, dtype=BF16):
    return _hip.lib().ddpm_attention_mh_fwd(qkv, ld, out, out_ld, lse, B, L, C, heads, 0.125, dtype, 0)


def bwd(qkv=FAKE, ld=3 * 128, o=FAKE, o_ld=128, d_o=FAKE, do_ld=128, lse=FAKE, dvec=FAKE, dqkv=FAKE, dqkv_ld=3 * 128, B=2, L=100, C=128, heads=2,
        dtype=BF16):
    return _hip.lib().ddpm_attention_mh_bwd(qkv, ld, o, o_ld, d_o, do_ld, lse, dvec, dqkv, dqkv_ld, B, L, C, heads, 0.125, dtype, 0)


def test_argument_validation_returns_status_codes_without_a_gpu():
    """Every call here is REFUSED on the host: an accepted one would launch on these fake addresses wherever a GPU is present (so the
    forward's optional lse is not among the NULLs)."""
    assert fwd(qkv=0) == NULL and fwd(out=0) == NULL
    for name in ("qkv", "o", "d_o", "lse", "dvec", "dqkv"):
        assert bwd(**{name: 0}) == NULL, name
    for f in (fwd, bwd):
        assert f(heads=0) == SHAPE and f(heads=-1) == SHAPE
        assert f(heads=3) == SHAPE                                                  # C % heads
        assert f(dtype=F32) == DTYPE
        assert f(B=32768, heads=2) == SHAPE                                         # B * heads = 65536: past blockIdx.y
        assert f(ld=3 * 128 + 4) == ALIGN                                           # a pitch that is no 16-byte multiple
        assert f(ld=3 * 128 - 8) == SHAPE                                           # C > ld / 3
        assert f(L=0) == SHAPE and f(B=0) == SHAPE
        assert f(qkv=FAKE + 2) == ALIGN
    assert fwd(C=96, ld=3 * 96, out_ld=96) == SHAPE                                 # d = 48
    assert bwd(C=96, ld=3 * 96, o_ld=96, do_ld=96, dqkv_ld=3 * 96) == SHAPE
    assert fwd(C=1088, ld=3 * 1088, out_ld=1088) == SHAPE                           # d = 544
    assert bwd(C=1088, ld=3 * 1088, o_ld=1088, do_ld=1088, dqkv_ld=3 * 1088) == SHAPE
    assert fwd(out_ld=128 + 4) == ALIGN and fwd(out_ld=64) == SHAPE and fwd(out=FAKE + 8) == ALIGN
    for name in ("o_ld", "do_ld"):
        assert bwd(**{name: 128 + 4}) == ALIGN and bwd(**{name: 64}) == SHAPE, name
    assert bwd(dqkv_ld=3 * 128 + 4) == ALIGN and bwd(dqkv_ld=3 * 128 - 8) == ALIGN     # as the streaming pair reports a short gradient pitch
    with pytest.raises(RuntimeError):
        _hip.call("ddpm_attention_mh_fwd", FAKE, 3 * 128, FAKE, 128, 0, 2, 100, 128, 3, 0.125, BF16, 0)
