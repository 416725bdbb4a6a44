"""-m gpu: multi-head attention — the head-indexed streaming kernels (ddpm_attention_mh_fwd / ddpm_attention_mh_bwd,
csrc/attention_stream.hip) at the kernel level, and ``UNet(num_head_channels=)`` through the engine in both compute modes.

Kernel level (helpers of tests/test_attention_stream_gpu.py: pitched operands with NaN guard rows and NaN pitch padding, sentinel-filled
outputs):
* bit identity: every head's O, lse, D and dq | dk | dv equal what ddpm_attention_stream_fwd / _bwd produce on that head's three slices
  copied into a packed [B][L][3d] buffer of their own — the per-head arithmetic is the same code in the same order, so no tolerance;
* accuracy: tests/mha_ref.py in float64 on the bf16-rounded inputs, the bars of this kernel family (1.2e-2 forward, 2e-2 backward; max abs
  error over the reference's max abs) applied PER HEAD, with head h's inputs scaled by 2^h so that a quiet head cannot hide behind a loud one;
* head isolation: head 1's slices set to NaN change no bit of any other head;
* the backward twice is bit-identical, the forward with lse = NULL gives the same O, nothing outside [B][L][C] / [B][H][L] is written.

Model level: the reduced UNet of tests/test_mha_host.py (2 and 4 heads of 32 channels) at 8 x 8 and at 24 x 20 (480 tokens), against
tests/mha_ref.py in float64.  Measures and bars are those the single-head reduced-model tests use (tests/test_unet_gpu.py
test_backward_with_dropout_vs_oracle: forward 1e-3 / 1.5e-1 of the reference's largest value in the fp32 / bf16 mode, gradients 3 x that
per tensor with the floor at 2 % / 10 % of the median tensor scale; tests/test_cond_gpu.py: trainer losses rtol 5e-4, states 1e-3 with the
Adam slack; replayed chains equal to eager ones bit for bit; tests/test_ddim_inverse_gpu.py: 1e-3 fp32, 1.48e-2 bf16 on the latent), and
each test first holds the SINGLE-head network with the same seeds to the same bar."""
import functools
import math
import os
import sys

import pytest
import torch

import ddpm_torch
from ddpm_torch import _hip
from oracle import unet_ref as U
from tests import cond_ref
from tests import ddim_inverse_ref as DR
from tests import mha_ref as R
from tests import test_attention_stream_gpu as S
from tests.golden.recipes import check_state

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ddpm-torch_amd")
if PKG not in sys.path:
    sys.path.insert(0, PKG)
import ddim  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = S.GUARD

# (B, L, C, heads): the smallest shapes that reach each mechanism
CASES = [(2, 1, 64, 2),          # d = 32 in the 64 bucket, one token
         (2, 7, 128, 2),
         (3, 33, 192, 3),        # d = 64, an odd head count
         (2, 65, 256, 4),        # one past the 64-token tile
         (2, 129, 256, 2),       # d = 128, one past the 128-row block
         (1, 257, 384, 4),       # d = 96: a non-power-of-two width in the 128 bucket
         (1, 65, 512, 2),        # d = 256: the MT = 1 backward
         (1, 40, 1024, 2),       # d = 512: two-unit operands, the z-split dK / dV; ld = 3 * 1024 + 16
         (2, 300, 256, 8),
         (2, 256, 256, 4)]       # the CIFAR-10 geometry, d = 64


def _bits16(buf, R_, W, what):
    """The [R][W] payload of a sentinel-filled bf16 output as int16 bit patterns (finite or not); nothing else may have been written."""
    rest = buf.clone()
    rest[GUARD:GUARD + R_, :W] = S.SENT_BF16
    assert bool((rest == S.SENT_BF16).all()), f"{what}: bytes outside [B][L][C] were written"
    return buf[GUARD:GUARD + R_, :W].contiguous()


def _bits32(buf, n, what):
    assert bool((buf[:GUARD] == S.SENT_F32).all()) and bool((buf[GUARD + n:] == S.SENT_F32).all()), f"{what}: guard rows were written"
    return buf[GUARD:GUARD + n].contiguous().view(torch.int32)


def _f64(bits):
    return (bits.view(torch.bfloat16) if bits.dtype == torch.int16 else bits.view(torch.float32)).double()


def run_entry(qkv, d_o, B, L, C, heads, mh=True):
    """Forward (with lse, and with lse = NULL: same O) and the backward twice (bit-identical) on the forward's own O and lse, as the engine
    calls them.  ``mh`` False: the streaming pair (heads must be 1).  Returns the raw bit patterns: O [R][C], lse / D [B][H][L], G [R][3C]."""
    ld, old, gld = 3 * C + 16, C + 8, 3 * C + 24
    scale, R_, n = 1.0 / math.sqrt(C // heads), B * L, B * heads * L
    hs = (heads,) if mh else ()
    fwd, bwd = ("ddpm_attention_mh_fwd", "ddpm_attention_mh_bwd") if mh else ("ddpm_attention_stream_fwd", "ddpm_attention_stream_bwd")
    st = _hip.stream()
    qb, qp = S._operand(qkv, ld)
    ob, op = S._out_bf16(R_, old)
    lb, lp = S._out_f32(n)
    _hip.call(fwd, qp, ld, op, old, lp, B, L, C, *hs, scale, 1, st)
    ob2, op2 = S._out_bf16(R_, old)
    _hip.call(fwd, qp, ld, op2, old, 0, B, L, C, *hs, scale, 1, st)
    torch.cuda.synchronize()
    o = _bits16(ob, R_, C, "O")
    lse = _bits32(lb, n, "lse")
    assert torch.equal(ob, ob2), "O differs between lse and lse = NULL"
    o_in, oip = S._operand(o.view(torch.bfloat16), old)
    db, dp = S._operand(d_o, old)
    outs = []
    for _ in range(2):
        vb, vp = S._out_f32(n)
        gb, gp = S._out_bf16(R_, gld)
        _hip.call(bwd, qp, ld, oip, old, dp, old, lp, vp, gp, gld, B, L, C, *hs, scale, 1, st)
        outs.append((vb, gb))
    torch.cuda.synchronize()
    (vb, gb), (vb2, gb2) = outs
    D, G = _bits32(vb, n, "D"), _bits16(gb, R_, 3 * C, "dqkv")
    assert torch.equal(vb.view(torch.int32), vb2.view(torch.int32)) and torch.equal(gb, gb2), "the backward is not bit-identical when repeated"
    del qb, o_in, db
    return dict(O=o, lse=lse.reshape(B, heads, L), D=D.reshape(B, heads, L), G=G)


def _inputs(B, L, C, heads):
    """Head h's q, k, v and d_o are 2^h times a draw of one common amplitude.  The amplitude is 1.2 * 2^(-(H - 1) / 2) — the 1.2 of
    tests/test_attention_stream_gpu.py centred over the heads — so the scaled logits' standard deviation runs from 1.44 / 2^(H - 1) to
    1.44 * 2^(H - 1): at eight heads from a uniform softmax to a one-hot one with |logit| of a few hundred, the range that file's planted
    cases cover.  (Starting at 1.2 instead would put head 7's logits near 1e5, where one fp32 ulp of lse — 0.008 — is by itself a
    1 % error of every rebuilt probability: a property of the fp32 statistic, not of the head indexing.)"""
    d = C // heads
    gen = torch.Generator().manual_seed(21)
    qkv = torch.randn(B * L, 3, heads, d, generator=gen) * (1.2 * 2.0 ** (-(heads - 1) / 2))
    d_o = torch.randn(B * L, heads, d, generator=torch.Generator().manual_seed(22))
    w = (2.0 ** torch.arange(heads)).reshape(1, heads, 1)
    return (qkv * w[:, None]).reshape(B * L, 3 * C).to(torch.bfloat16), (d_o * w).reshape(B * L, C).to(torch.bfloat16)


def _head(x, h, d, thirds):
    """Columns of head h in a [R][thirds * C] tensor -> [R][thirds * d]"""
    C = x.shape[1] // thirds
    return torch.cat([x[:, i * C + h * d:i * C + (h + 1) * d] for i in range(thirds)], dim=1).contiguous()


def _rel(got, ref):
    return float((got - ref).abs().max()) / (float(ref.abs().max()) or 1.0)


@pytest.mark.parametrize("B,L,C,heads", CASES)
def test_heads_against_the_streaming_pair_and_float64(B, L, C, heads):
    d, scale = C // heads, 1.0 / math.sqrt(C // heads)
    qkv, d_o = _inputs(B, L, C, heads)
    got = run_entry(qkv, d_o, B, L, C, heads)
    # ---- accuracy, per head, against float64 on the bf16-rounded inputs (the backward from the kernel's own o and lse)
    o64, lse64, g64 = _f64(got["O"]), _f64(got["lse"]), _f64(got["G"])
    x = qkv.to(DEV).double()
    o_ref, lse_ref = R.entry_fwd(x, B, L, C, heads, scale)
    D_ref, g_ref = R.entry_bwd(x, o64, d_o.to(DEV).double(), lse64, B, L, C, heads, scale)
    assert torch.isfinite(o64).all() and torch.isfinite(lse64).all() and torch.isfinite(g64).all() and torch.isfinite(_f64(got["D"])).all()
    for h in range(heads):
        errs = {"O": _rel(_head(o64, h, d, 1), _head(o_ref, h, d, 1)), "lse": _rel(lse64[:, h], lse_ref[:, h]),
                "D": _rel(_f64(got["D"])[:, h], D_ref[:, h]), "dqkv": _rel(_head(g64, h, d, 3), _head(g_ref, h, d, 3))}
        print(f"mh B{B} L{L} C{C} H{heads} head {h}: " + "  ".join(f"{k} {v:.3e}" for k, v in errs.items()))
        assert errs["O"] <= S.TOL_FWD and errs["lse"] <= S.TOL_FWD, (h, errs)
        assert errs["D"] <= S.TOL_BWD and errs["dqkv"] <= S.TOL_BWD, (h, errs)
        gh = _head(g64, h, d, 3)
        assert float(gh[:, 2 * d:].abs().max()) > 0 and (L == 1 or (float(gh[:, :d].abs().max()) > 0 and float(gh[:, d:2 * d].abs().max()) > 0))
    # ---- bit identity with the single-head streaming kernels on each head's own packed buffer
    for h in range(heads):
        one = run_entry(_head(qkv, h, d, 3), _head(d_o, h, d, 1), B, L, d, 1, mh=False)
        assert torch.equal(one["O"], _head(got["O"], h, d, 1)), f"head {h}: O"
        assert torch.equal(one["lse"][:, 0], got["lse"][:, h]), f"head {h}: lse"
        assert torch.equal(one["D"][:, 0], got["D"][:, h]), f"head {h}: D"
        assert torch.equal(one["G"], _head(got["G"], h, d, 3)), f"head {h}: dq | dk | dv"
    # ---- head isolation: head 1 all NaN (q, k, v and d_o) changes no bit of any other head
    nan_q, nan_do = qkv.clone().reshape(B * L, 3, heads, d), d_o.clone().reshape(B * L, heads, d)
    nan_q[:, :, 1], nan_do[:, 1] = float("nan"), float("nan")
    iso = run_entry(nan_q.reshape(B * L, 3 * C), nan_do.reshape(B * L, C), B, L, C, heads)
    for h in range(heads):
        parts = ((_head(iso["O"], h, d, 1), _head(got["O"], h, d, 1)), (iso["lse"][:, h], got["lse"][:, h]), (iso["D"][:, h], got["D"][:, h]),
                 (_head(iso["G"], h, d, 3), _head(got["G"], h, d, 3)))
        if h == 1:
            assert all(not bool(torch.isfinite(_f64(a)).any()) for a, _ in parts), "head 1 was all NaN: its outputs are not"
        else:
            assert all(torch.equal(a, b) for a, b in parts), f"head {h} changed when head 1 became NaN"


@pytest.mark.parametrize("B,L,C", [(b, l, c) for b, l, c, _ in CASES if c <= 512])
def test_one_head_through_the_new_entry_is_the_streaming_entry(B, L, C):
    qkv, d_o = S._inputs(B, L, C, 1.0)
    a, b = run_entry(qkv, d_o, B, L, C, 1), run_entry(qkv, d_o, B, L, C, 1, mh=False)
    assert all(torch.equal(a[k], b[k]) for k in ("O", "lse", "D", "G"))


# ====================================================================================================== model level
RED = dict(in_channels=3, hid_channels=64, out_channels=3, ch_multipliers=[1, 2], num_res_blocks=1, apply_attn=[True, True], drop_rate=0.0)
HEADS = {"one": {}, "mh": {"num_head_channels": 32}}             # 2 heads over 64 channels, 4 over 128
SIZES = [(8, 8), (24, 20)]                                       # 64 / 16 tokens; 480 / 120 tokens (streaming-only in the bf16 mode)
MODES = [(torch.float32, 1e-3), (torch.bfloat16, 1.5e-1)]
K = 3


def r(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


@functools.lru_cache(maxsize=None)
def weights(conditional=False):
    torch.manual_seed(5)
    m = ddpm_torch.UNet(**RED, **({"num_classes": K} if conditional else {}))
    sd = U.randomize_state_dict(m.state_dict(), 17)
    return sd, {k: v.double() for k, v in sd.items()}


def model_of(kind, dtype, conditional=False):
    m = ddpm_torch.UNet(**RED, **HEADS[kind], **({"num_classes": K} if conditional else {}))
    m.load_state_dict(weights(conditional)[0])
    return m.to(DEV).set_compute_dtype(dtype)


def net64(kind, conditional=False):
    sd64 = weights(conditional)[1]
    if conditional:
        def f(x, t, y):
            with R.bound(**HEADS[kind]):
                return cond_ref.unet_forward(sd64, RED, x, t, y)
        return f
    return lambda x, t: R.unet_forward(sd64, RED, x, t, **HEADS[kind])


@functools.lru_cache(maxsize=None)
def net_reference(kind, H, W):
    """Forward and every parameter's gradient of the float64 network, once per head layout and image size."""
    x, t, gy = r(3, 3, H, W, seed=1), torch.tensor([3, 977, 40]), r(3, 3, H, W, seed=2)
    p = {k: v.clone().requires_grad_(True) for k, v in weights()[1].items()}
    out = R.unet_forward(p, RED, x.double(), t, training=True, **HEADS[kind])
    (out * gy.double()).sum().backward()
    return x, t, gy, out.detach(), {k: v.grad for k, v in p.items()}


@pytest.mark.parametrize("H,W", SIZES)
@pytest.mark.parametrize("dtype,bar", MODES, ids=["fp32", "bf16"])
def test_forward_and_every_gradient_against_float64(dtype, bar, H, W):
    for kind in ("one", "mh"):                                   # the single head first: the bar is the one it is held to
        x, t, gy, out64, grads64 = net_reference(kind, H, W)
        m = model_of(kind, dtype).train()
        m.engine().debug_keep_tape = True
        out = m(x.to(DEV), t.to(DEV))
        (out * gy.to(DEV)).sum().backward()
        rel = float((out.detach().cpu().double() - out64).abs().max() / out64.abs().max())
        scales = {k: float(v.abs().max()) for k, v in grads64.items()}
        floor = (0.02 if dtype == torch.float32 else 0.1) * sorted(scales.values())[len(scales) // 2]
        rows = sorted(((float((q.grad.cpu().double() - grads64[k]).abs().max()) / max(scales[k], floor), k) for k, q in m.named_parameters()), reverse=True)
        print(f"\n  {kind} {H}x{W} {dtype}: forward rel err {rel:.3e}; worst gradients " + ", ".join(f"{k} {e:.2e}" for e, k in rows[:3]))
        assert rel < bar, (kind, rel)
        assert rows[0][0] < 3 * bar, (kind, rows[0])
        recs = [rec for rec in m.engine().last_tape if rec[0] == "attn"]
        if kind == "mh" and dtype == torch.bfloat16:             # the head-indexed kernels: per-head statistics, no L x L tensor
            assert all(rec[7] is None and tuple(rec[9].shape) == (3, rec[1].num_heads, rec[2].H * rec[2].W) for rec in recs)
        elif kind == "mh":                                       # the materialised products per head
            assert all(rec[9] is None and tuple(rec[7].shape)[:2] == (rec[1].num_heads, 3) for rec in recs)
    assert float((net_reference("mh", H, W)[3] - net_reference("one", H, W)[3]).abs().max()) > 1e-2 * float(net_reference("one", H, W)[3].abs().max())


@pytest.mark.parametrize("H,W", SIZES)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_three_trainer_steps_through_the_launch_plan_equal_the_eager_engine(dtype, H, W, monkeypatch):
    """fp32 mode: the equality tests/test_cond_gpu.py demands of its trainer (lr 1e-3; losses rtol 5e-4, states 1e-3 with the Adam slack).
    That test runs in the fp32 mode only, and in the bf16 mode the SINGLE-head network does not meet it (measured on the MI355X at
    24 x 20: one weight 7.84e-4 apart against a slack of 7.5e-4 — the two forms differ by the weight gradients' atomic summation order,
    and Adam moves an element by up to lr per step whatever its gradient).  The bf16 mode therefore takes the measure and bars the project
    holds the single-head reduced network to for this very comparison, tests/test_attention_any_tokens_gpu.py (lr 1e-4): first loss
    1e-5, second 7.5e-3, third 1.2e-1 relative, parameters within 2 lr x steps."""
    from ddpm_torch.utils import train as train_mod
    lr = 1e-3 if dtype == torch.float32 else 1e-4
    g = torch.Generator().manual_seed(21)
    xs = [torch.rand(4, 3, H, W, generator=g) * 2 - 1 for _ in range(3)]
    for kind in ("one", "mh"):
        runs = {}
        for path in ("plan", False):
            monkeypatch.setattr(train_mod, "_TRAIN_GRAPH", path)
            m = model_of(kind, dtype)
            dif = ddpm_torch.GaussianDiffusion(ddpm_torch.get_beta_schedule("linear", 1e-4, 0.02, 1000), "eps", "fixed-large", "mse")
            opt = torch.optim.Adam(m.parameters(), lr=lr, betas=(0.9, 0.999))
            tr = ddpm_torch.Trainer(m, opt, dif, epochs=1, trainloader=None, scheduler=None, use_ema=True, grad_norm=1.0, shape=(3, H, W),
                                    device=torch.device(DEV), ema_decay=0.9999)
            m.train()
            losses = []
            for i, x in enumerate(xs):
                tr.stats.reset()
                tr.step(x, global_steps=i + 1)
                losses.append(tr.current_stats["loss"])
            if path == "plan":
                ds = next(iter(tr._direct.values()))
                assert ds.plan is not None and ds.last_kind == "plan", "the third step was not replayed from the launch plan"
            runs[path] = (losses, {k: v.cpu() for k, v in m.state_dict().items()}, {k: v.cpu() for k, v in tr.ema.shadow.items()})
        (la, pa, sa), (lb, pb, sb) = runs["plan"], runs[False]
        print(f"\n  {kind} {H}x{W} {dtype}: losses plan {la} eager {lb}")
        if dtype == torch.float32:
            assert torch.allclose(torch.tensor(la, dtype=torch.float64), torch.tensor(lb, dtype=torch.float64), rtol=5e-4), (kind, la, lb)
            slack = 0.25 * lr * 3
            check_state(pa, pb, 1e-3, f"{kind} param", adam_slack=slack)
            check_state(sa, sb, 1e-3, f"{kind} shadow", adam_slack=slack)
        else:
            worst = max(float((pa[k] - v).abs().max()) for k, v in pb.items()) / (lr * 3)
            print(f"  parameters differ by at most {worst:.2f} x lr x steps")
            assert abs(la[0] - lb[0]) <= 1e-5 * abs(lb[0]), (kind, la, lb)
            assert abs(la[1] - lb[1]) <= 7.5e-3 * abs(lb[1]) and abs(la[2] - lb[2]) <= 1.2e-1 * abs(lb[2]), (kind, la, lb)
            assert worst <= 2.0, (kind, worst)
        assert any(not torch.equal(pa[k], weights()[0][k]) for k in pa), "the steps moved nothing"


@pytest.mark.parametrize("H,W", SIZES)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_replayed_chains_equal_eager_chains(dtype, H, W, monkeypatch):
    """A 10-step graph-replayed p_sample chain and one guided chain (num_classes = 3, scale 2): bit-equal to the eager loops."""
    dif = ddpm_torch.GaussianDiffusion(ddpm_torch.get_beta_schedule("linear", 1e-4, 0.02, 10), "eps", "fixed-large", "mse")
    shape, y, by_kind = (3, 3, H, W), torch.tensor([2, 0, 1], device=DEV), {}
    for kind in ("one", "mh"):
        m, mc = model_of(kind, dtype).eval(), model_of(kind, dtype, conditional=True).eval()
        outs = {}
        for mode in ("1", "0"):
            monkeypatch.setenv("DDPM_TORCH_AMD_GRAPH", mode)
            outs[mode] = dif.p_sample(m, shape=shape, device=DEV, seed=77)
            outs[mode + "g"] = dif.p_sample(mc, shape=shape, device=DEV, seed=77, y=y, guidance_scale=2.0)
        assert torch.equal(outs["1"], outs["0"]) and torch.equal(outs["1g"], outs["0g"]), kind
        assert bool(torch.isfinite(outs["1"]).all()) and bool(torch.isfinite(outs["1g"]).all()) and not torch.equal(outs["1"], outs["1g"])
        by_kind[kind] = outs["1"]
    assert not torch.equal(by_kind["one"], by_kind["mh"]), "the heads changed nothing"


T_SMALL, S_SMALL = 32, 8
BF16_BAR = 1.48e-2                                               # tests/test_ddim_inverse_gpu.py


def small_process():
    betas = ddpm_torch.get_beta_schedule("linear", 1e-4, 0.02, T_SMALL)
    sub = ddim.get_selection_schedule("linear", size=S_SMALL, timesteps=T_SMALL)
    return ddim.DDIM(betas, "eps", "fixed-small", "mse", eta=0.0, subsequence=sub), betas, sub


@functools.lru_cache(maxsize=None)
def ddim_reference(kind, H, W):
    x_0 = torch.rand(3, 3, H, W, generator=torch.Generator().manual_seed(H * 100 + W)) * 2 - 1
    _, betas, sub = small_process()
    tb = DR.tables(betas, sub)
    with torch.no_grad():
        latent = DR.encode(tb, net64(kind), x_0)
        x_rec = DR.decode(tb, net64(kind), latent)
    return x_0, latent, x_rec


@pytest.mark.parametrize("H,W", SIZES)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_ddim_encode_then_decode(dtype, H, W):
    dif, _, _ = small_process()
    for kind in ("one", "mh"):
        x_0, want_latent, want_rec = ddim_reference(kind, H, W)
        m = model_of(kind, dtype).eval()
        x_rec, latent = dif.reconstruct(m, x_0.to(DEV))
        assert torch.equal(latent, dif.encode(m, x_0.to(DEV)))
        e_enc = float((latent.cpu().double() - want_latent).abs().max() / want_latent.abs().max())
        e_rec = float((x_rec.cpu().double() - want_rec).abs().max() / want_rec.abs().max())
        print(f"\n  {kind} {H}x{W} {dtype}: encode rel err {e_enc:.3e}, reconstruct rel err {e_rec:.3e}; round trip max |x_rec - x_0| "
              f"{float((x_rec.cpu() - x_0).abs().max()):.3e} (float64: {float((want_rec - x_0).abs().max()):.3e})")
        if dtype == torch.float32:
            assert e_enc <= 1e-3 and e_rec <= 1e-3, (kind, e_enc, e_rec)
        else:
            assert e_enc <= BF16_BAR, (kind, e_enc)
