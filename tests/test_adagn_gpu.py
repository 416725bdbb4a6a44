"""-m gpu: the scale-shift norm — the modulated GroupNorm kernels (ddpm_groupnorm_mod_silu_fwd / ddpm_groupnorm_mod_silu_bwd,
csrc/norm.hip) at the kernel level, and ``UNet(use_scale_shift_norm=True)`` through the engine in both compute modes.

Kernel level.  Shapes: ``GN_CASES`` of tests/test_kernels_gpu.py (one per dispatch family: the comment above REG_CASES, read from the
dispatcher of csrc/norm.hip) plus two shapes that reach the register-resident kernels, in both dtypes.  Pitched operands with NaN pitch padding and NaN
guard rows, ``mod_ld = 2C + 12`` / ``dmod_ld = 2C + 4`` with NaN in the padding, sentinel-filled outputs, per-sample distinct
s, h ~ 0.5 N(0, 1).
* bit tie: at mod == 0, y, stats and dx equal the plain entry points' bit for bit (accumulate 0 without and 1 with the ``add`` operand);
* float64 accuracy: per-element bars by the model of ``rep_gn_fwd`` / ``rep_gn_bwd`` in tests/launch_replay.py with gamma, beta replaced by
  the per-sample g_eff, b_eff; dmod, dgamma, dbeta by that model's GEMM-shaped pixel-sum bar (dgamma / dbeta: the terms carry the
  sample's factor 1 + s, and the rounding of each sample's product A (1 + s) is added as u |A (1 + s)|; dscale = gamma A + beta D: the
  two sums' bars weighted by |gamma|, |beta| plus the rounding of the combination).  No new constant.  ONE derived term is added: the
  model's e_t (what bounds the fp32 error of t = g xhat + b, in units of u_acc: |g| (|x| + |mean|) rstd + |b|) assumes exact gamma, beta; here the kernels FORM the affine in fp32 — 1 + s is rounded, g_eff = gamma * fl(1 + s) is rounded, b_eff is one fma of
  beta, fl(1 + s) and h — so t carries in addition 2 |g_eff xhat| + 2 |beta (1 + s)| + |b_eff| (units of u_acc: two roundings on the
  scale path; the rounding of 1 + s carried through beta, and the fma's own rounding bounded by |beta (1 + s)| + |b_eff|).  The forward
  bar takes it times |y'|, the backward inside e_t;
* edge: one sample with s = -1 on every channel (g_eff = 0): y = drop(silu(shift)) per channel, that sample's dx is exactly zero (no
  ``add``, no accumulate), its dshift is still right;
* sample isolation: a NaN row of mod for sample 1 changes no bit of any other sample's y, dx or dmod rows;
* determinism and bounds: the backward twice gives bit-identical dx and dmod; nothing outside [B*HW][C], [B][2C] and stats is written.

Model level: the reduced UNet of tests/test_mha_host.py with the flag on, at 8 x 8 and 24 x 20, against tests/adagn_ref.py in float64.
Measures and bars are those the single-head reduced-model tests use (tests/test_unet_gpu.py test_backward_with_dropout_vs_oracle: forward
1e-3 / 1.5e-1 of the reference's largest value in the fp32 / bf16 mode, gradients 3 x that per tensor with the floor at 2 % / 10 % of the
median tensor scale; tests/test_cond_gpu.py: trainer losses rtol 5e-4, states 1e-3 with the Adam slack, in the fp32 mode — the bf16 mode
takes tests/test_attention_any_tokens_gpu.py's, as tests/test_mha_gpu.py does and explains; replayed chains equal to eager ones bit for
bit; the time table against DDPM_TIME_TABLE=0 within 2e-5 of the sample's range, tests/test_configs_gpu.py), and each test first holds
the flag-off network with the same seeds to the same bar."""
import functools
import math
import os
import sys

import pytest
import torch

import ddpm_torch
from ddpm_torch import _hip
from oracle import diffusion_ref as D
from oracle import unet_ref as U
from tests import adagn_ref as R
from tests import channels_accum as CA
from tests import launch_replay as LR
from tests.golden.recipes import check_state
from tests.test_kernels_gpu import GN_CASES

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ddpm-torch_amd")
if PKG not in sys.path:
    sys.path.insert(0, PKG)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DT = {0: torch.float32, 1: torch.bfloat16}
GUARD = 8                                       # rows of NaN / sentinel before and after every tensor
SENT = {0: 12345.5, 1: 23040.0}                 # what outputs are pre-filled with (finite, exactly representable in fp32 / bf16)
G, EPS, SEED = 32, 1e-6, 0x1234567

# which kernels of csrc/norm.hip a shape reaches (forward | backward), read from gn_fused_plan / gn_lds_plan and the two dispatchers:
#   fp32  (2,16,32) staged 256-thread, 1 vector | same, groups of one channel (the ordered reduction)
#         (2,64,128) staged 256-thread, 2 vectors;  (130,16,256) staged 256-thread at B = 130;  (2,16,768) staged 256, 24 channels / group
#         (3,256,256), (2,256,512) staged 512-thread, 4 vectors;  (3,1024,128), (2,1024,256) staged 512, 8 vectors | gn_lds_bwd8
#         (2,256,384), (2,1024,384) staged 512, 7 vectors, 12 channels / group (12 and 3 vector columns) | gn_lds_bwd8, ordered reduction
#         (1,4096,64) streaming (stats + finalize + apply | reduce + finalize + apply)
#   bf16  the same families except (2,16,32): a 64-byte segment -> streaming; the 8-vector backward is gn_lds_bwd_kernel<.., 8, 512, ..>
#   (128,4,1024) fp32 and (128,4,2048) bf16: 64 vector columns per block -> the register-resident forward and backward
REG_CASES = [(128, 4, 1024), (128, 4, 2048)]
CASES = GN_CASES + REG_CASES
FLAGS = [(1, 0.0), (1, 0.1)]
PLAIN_FLAGS_ON = [(2, 64, 128), (1, 4096, 64)]           # (silu, drop) = (0, 0) on two shapes: a staged one and the streaming one


def _operand(payload, pitch):
    """[R][W] -> device buffer [GUARD + R + GUARD][pitch] of the payload's dtype, NaN everywhere else; (buffer, pointer to row 0)."""
    R_, W = payload.shape
    buf = torch.full((R_ + 2 * GUARD, pitch), float("nan"), dtype=payload.dtype, device=DEV)
    buf[GUARD:GUARD + R_, :W] = payload.to(DEV)
    return buf, buf[GUARD:].data_ptr()


def _output(R_, W, pitch, dt, prior=None):
    buf = torch.full((R_ + 2 * GUARD, pitch), SENT[dt], dtype=DT[dt], device=DEV)
    if prior is not None:
        buf[GUARD:GUARD + R_, :W] = prior.to(DEV)
    return buf, buf[GUARD:].data_ptr()


def _payload(buf, R_, W, dt, what):
    """The [R][W] payload of a sentinel-filled output as raw bits; nothing else may have been written."""
    rest = buf.clone()
    rest[GUARD:GUARD + R_, :W] = SENT[dt]
    assert bool((rest == SENT[dt]).all()), f"{what}: bytes outside the [{R_}][{W}] payload were written"
    return buf[GUARD:GUARD + R_, :W].contiguous().view(torch.int16 if dt else torch.int32)


def _f64(bits):
    return (bits.view(torch.bfloat16) if bits.dtype == torch.int16 else bits.view(torch.float32)).double()


def _r(*shape, seed, scale=1.0, shift=0.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale + shift


# x and dy are drawn as rep_gn_fwd / rep_gn_bwd draw them (x ~ N(1.5, 1), dy ~ N(0.3, 1)): the model's bars are stated for that regime —
# its terms for the group means c1, c2 carry |c1|, |c2| themselves, which a zero-mean dy would cancel to nothing under the summation error
# (measured on the MI355X with dy ~ N(0, 1): the PLAIN kernels, reached through mod == 0, miss this dx bar by up to 1.63 x on dropped
#  elements of (130, 16, 256) and (128, 4, 1024) in fp32, the modulated ones by up to 2.4 x; in the model's regime the worst is 0.64)
X_MEAN, DY_MEAN = 1.5, 0.3


@functools.lru_cache(maxsize=None)
def inputs(B, HW, C, dt):
    x = _r(B * HW, C, seed=1, shift=X_MEAN).to(DT[dt])
    dy = _r(B * HW, C, seed=4, shift=DY_MEAN).to(DT[dt])
    add, prior = _r(B * HW, C, seed=8).to(DT[dt]), _r(B * HW, C, seed=7).to(DT[dt])
    gamma, beta = 1 + 0.3 * _r(C, seed=2), 0.5 * _r(C, seed=3)
    mod = 0.5 * _r(B, 2 * C, seed=5)
    return x, dy, add, prior, gamma, beta, mod


def run(B, HW, C, dt, silu, drop, mod=None, acc=0, use_add=False, twice=False):
    """One forward and one (``twice``: two) backward of the modulated (``mod`` [B][2C]) or the plain (None) pair on the shared inputs, the
    backward on the forward's own statistics.  Returns raw bits: y, dx [B*HW][C], stats [B][G][2], dmod [B][2C]; fp32 dgamma, dbeta."""
    x, dy, add, prior, gamma, beta, _ = inputs(B, HW, C, dt)
    ld, yld, dyld, dxld, adld, mld, dmld = C + 16, C + 32, C + 48, C + 64, C + 80, 2 * C + 12, 2 * C + 4
    rows, st = B * HW, _hip.stream()
    nws = int(_hip.lib().ddpm_gn_workspace_floats(B, HW, C, G, dt))
    assert nws > 0
    ws = torch.full((nws,), float("nan"), device=DEV)                        # scratch: its initial content is not part of the contract
    keep = [_operand(x, ld), _operand(dy, dyld), _operand(add, adld), _operand(gamma[None], C), _operand(beta[None], C)]
    (_, xp), (_, dyp), (_, adp), (_, gp), (_, bp) = keep
    seed = SEED if drop else 0
    tail_f, tail_b, name_f, name_b = (), (), "ddpm_groupnorm_silu_fwd", "ddpm_groupnorm_silu_bwd"
    yb, yp = _output(rows, C, yld, dt)
    sb, sp = _output(B, 2 * G, 2 * G, 0)
    dmb = None
    if mod is not None:
        mb, mp = _operand(mod, mld)
        keep.append((mb, mp))
        tail_f, name_f, name_b = (mp, mld), "ddpm_groupnorm_mod_silu_fwd", "ddpm_groupnorm_mod_silu_bwd"
    _hip.call(name_f, xp, ld, yp, yld, gp, bp, sp, ws.data_ptr(), B, HW, C, G, EPS, silu, drop, seed, 0, *tail_f, dt, st)
    torch.cuda.synchronize()
    out = dict(y=_payload(yb, rows, C, dt, "y"), stats=_payload(sb, B, 2 * G, 0, "stats"))
    stp = sp
    runs = []
    for _ in range(2 if twice else 1):
        dxb, dxp = _output(rows, C, dxld, dt, prior if acc else None)
        dg, db = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
        if mod is not None:
            dmb, dmp = _output(B, 2 * C, dmld, 0)
            tail_b = (mp, mld, dmp, dmld)
        _hip.call(name_b, xp, ld, dyp, dyld, dxp, dxld, gp, bp, stp, dg.data_ptr(), db.data_ptr(), ws.data_ptr(), B, HW, C, G, silu, drop, seed, 0,
                  acc, 0, 0, adp if use_add else 0, adld if use_add else 0, *tail_b, dt, st)
        torch.cuda.synchronize()
        runs.append(dict(dx=_payload(dxb, rows, C, dt, "dx"), dgamma=dg.double(), dbeta=db.double(),
                         dmod=None if dmb is None else _payload(dmb, B, 2 * C, 0, "dmod")))
    if twice:
        assert torch.equal(runs[0]["dx"], runs[1]["dx"]) and torch.equal(runs[0]["dmod"], runs[1]["dmod"]), "the backward is not bit-identical when repeated"
    out.update(runs[0])
    del keep
    return out


def _per_c(v, B, HW, C):
    """[B][G] -> [B][HW][C]"""
    return LR._per_c(v, B, HW, C, G)


def check_against_float64(got, B, HW, C, dt, silu, drop, mod, tag):
    """The bars of rep_gn_fwd / rep_gn_bwd (tests/launch_replay.py) with the per-sample affine; see the module docstring for the one added term."""
    x, dy, _, _, gamma, beta, _ = inputs(B, HW, C, dt)
    seed = SEED if drop else 0
    xs, dys = x.to(DEV).double().reshape(B, HW, C), dy.to(DEV).double().reshape(B, HW, C)
    gm, bt, md = gamma.to(DEV).double(), beta.to(DEV).double(), mod.to(DEV).double()
    s1 = 1 + md[:, :C]
    g_eff, b_eff = (v[:, None, :] for v in R.affine(gm, bt, md, C))
    e_aff = (2 * (bt[None, :] * s1).abs())[:, None, :] + b_eff.abs()                       # + 2 |g_eff xhat| below
    n, u, CN, UA = (C // G) * HW, (LR.U_BF16 if dt else LR.U_F32), LR.C_NORM, LR.U_ACC
    worst = {}

    def cmp(name, val, ref, bar):
        err = (val - ref).abs()
        ok = err <= torch.clamp(bar, min=LR.TINY)
        worst[name] = float((err / torch.clamp(bar, min=LR.TINY)).max())
        assert bool(torch.isfinite(val).all()), f"{tag} {name}: not finite"
        assert bool(ok.all()), f"{tag} {name}: {int((~ok).sum())} of {ok.numel()} elements beyond the bar, worst {worst[name]:.2f} bars"

    # ---- forward
    y_ref, st_ref = R.entry_fwd(xs.reshape(B * HW, C), gm, bt, md, B, HW, C, G, EPS, silu, drop, seed)
    mean, rstd = st_ref[..., 0], st_ref[..., 1]
    mu, rs = _per_c(mean, B, HW, C), _per_c(rstd, B, HW, C)
    xh = (xs - mu) * rs
    t = g_eff * xh + b_eff
    sg = torch.sigmoid(t)
    yv, dyv = (t * sg, sg * (1 + t * (1 - sg))) if silu else (t, torch.ones_like(t))
    keepf = None
    if drop > 0:
        keepf = R.keep_mask(seed, B, HW, C, drop, DEV).reshape(B, HW, C).double() / (1.0 - drop)
        yv, dyv = yv * keepf, dyv * keepf
    bar = CN * (u * yv.abs() + UA * math.sqrt(n) * (g_eff.abs() * (xs.abs() + mu.abs()) * rs + b_eff.abs()) * dyv.abs())
    bar = bar + CN * UA * (2 * (g_eff * xh).abs() + e_aff) * dyv.abs()
    if dt == 0:
        bar = bar + CN * UA * ((LR._sigmoid_err(t) + 3) if silu else 1.0) * yv.abs()
    cmp("y", _f64(got["y"]).reshape(B, HW, C), y_ref.reshape(B, HW, C), bar)
    stats = _f64(got["stats"]).reshape(B, G, 2)
    cmp("mean", stats[..., 0], mean, CN * UA * math.sqrt(n) * (mean.abs() + 1.0 / rstd))
    cmp("rstd", stats[..., 1], rstd, CN * UA * math.sqrt(n) * rstd)
    # ---- backward, on the fp32 statistics the kernel was given (its own)
    dx_ref, dg_ref, db_ref, dmod_ref, mid = R.entry_bwd(xs.reshape(B * HW, C), dys.reshape(B * HW, C), gm, bt, stats, md, B, HW, C, G, silu, drop, seed)
    mu, rs = _per_c(stats[..., 0], B, HW, C), _per_c(stats[..., 1], B, HW, C)
    xh, dz = mid["xhat"], mid["dz"]
    dyk = dys.abs() if keepf is None else dys.abs() * keepf
    e_t = g_eff.abs() * (xs.abs() + mu.abs()) * rs + b_eff.abs() + 2 * (g_eff * xh).abs() + e_aff
    dt_err = dyk * e_t if silu else 0.0 * dyk
    a = dz * g_eff
    grp = lambda v: _per_c(v.reshape(B, HW, G, C // G).mean((1, 3)), B, HW, C)             # noqa: E731
    c1, c2 = grp(a * xh), grp(a)
    inner = rs * (a.abs() + (xh * c1).abs() + c2.abs())
    fp32_part = UA * math.sqrt(n) * (inner + rs * c1.abs() * (xs.abs() + mu.abs()) * rs + rs * g_eff.abs() * dt_err)
    cmp("dx", _f64(got["dx"]).reshape(B, HW, C), dx_ref.reshape(B, HW, C), CN * (u * inner + fp32_part))
    # pixel sums, GEMM-shaped: M = |sum of terms|, S = root of the sum of squared terms, K terms, the per-term error added linearly
    lin_a = dt_err * xh.abs() + dz.abs() * (xs.abs() + mu.abs()) * rs
    lin_d = dt_err

    def sum_bar(terms, lin, dims, K):
        return CN * (LR.U_F32 * terms.sum(dims).abs() + UA * (math.sqrt(K) * (terms * terms).sum(dims).sqrt() + lin.sum(dims)))
    s1b = s1[:, None, :]
    cmp("dgamma", got["dgamma"], dg_ref, sum_bar(dz * xh * s1b, lin_a * s1b.abs(), (0, 1), B * HW) + CN * LR.U_F32 * (mid["A"] * s1).abs().sum(0))
    cmp("dbeta", got["dbeta"], db_ref, sum_bar(dz * s1b, lin_d * s1b.abs(), (0, 1), B * HW) + CN * LR.U_F32 * (mid["D"] * s1).abs().sum(0))
    bar_a, bar_d = sum_bar(dz * xh, lin_a, 1, HW), sum_bar(dz, lin_d, 1, HW)
    dmod = _f64(got["dmod"])
    cmp("dshift", dmod[:, C:], dmod_ref[:, C:], bar_d)
    cmp("dscale", dmod[:, :C], dmod_ref[:, :C], gm.abs() * bar_a + bt.abs() * bar_d + CN * LR.U_F32 * ((gm * mid["A"]).abs() + (bt * mid["D"]).abs()))
    print(f"{tag}: " + "  ".join(f"{k} {v:.2f}" for k, v in worst.items()) + "  (worst error in bars)")


def _cases():
    out = []
    for dt in (0, 1):
        for B, HW, C in CASES:
            if (B, HW, C) in REG_CASES and REG_CASES.index((B, HW, C)) != dt:
                continue                                            # (each of the two reaches the register kernels in one dtype)
            for silu, drop in FLAGS + ([(0, 0.0)] if (B, HW, C) in PLAIN_FLAGS_ON else []):
                out.append(pytest.param(dt, B, HW, C, silu, drop, id=f"{'bf16' if dt else 'fp32'}-{B}x{HW}x{C}-silu{silu}-drop{drop}"))
    return out


@pytest.mark.parametrize("dt,B,HW,C,silu,drop", _cases())
def test_modulated_pair_bit_tie_float64_isolation_determinism(dt, B, HW, C, silu, drop):
    mod = inputs(B, HW, C, dt)[6]
    tag = f"adagn {'bf16' if dt else 'fp32'} B{B} HW{HW} C{C} silu{silu} drop{drop}"
    got = run(B, HW, C, dt, silu, drop, mod=mod, twice=True)
    check_against_float64(got, B, HW, C, dt, silu, drop, mod, tag)
    # ---- bit tie with the plain entry points at mod == 0: both accumulate values, the add operand
    zero = torch.zeros(B, 2 * C)
    for acc, use_add in ((0, False), (1, True)):
        a, b = run(B, HW, C, dt, silu, drop, mod=zero, acc=acc, use_add=use_add), run(B, HW, C, dt, silu, drop, mod=None, acc=acc, use_add=use_add)
        assert torch.equal(a["y"], b["y"]), f"{tag}: y differs from the plain entry at mod == 0"
        assert torch.equal(a["stats"], b["stats"]), f"{tag}: stats differ from the plain entry at mod == 0"
        assert torch.equal(a["dx"], b["dx"]), f"{tag}: dx differs from the plain entry at mod == 0 (accumulate {acc}, add {use_add})"
    assert not torch.equal(got["y"], b["y"]), "the modulation changed nothing"
    # ---- sample isolation: a NaN row of mod for sample 1
    if B >= 2:
        bad = mod.clone()
        bad[1] = float("nan")
        iso = run(B, HW, C, dt, silu, drop, mod=bad)
        others = [i for i in range(B) if i != 1]
        rows = torch.tensor([i * HW + p for i in others for p in range(HW)], device=DEV)
        assert torch.equal(iso["y"][rows], got["y"][rows]) and torch.equal(iso["dx"][rows], got["dx"][rows]), f"{tag}: another sample changed"
        assert torch.equal(iso["dmod"][others], got["dmod"][others]) and torch.equal(iso["stats"], got["stats"]), f"{tag}: another sample changed"
        y1 = _f64(iso["y"])[HW:2 * HW]
        assert not bool(torch.isfinite(y1[y1 != 0]).any()), "sample 1's mod row was NaN: its kept outputs are not"


EDGE_CASES = [(0, 2, 64, 128), (1, 3, 1024, 128), (1, 2, 256, 384), (0, 1, 4096, 64), (1, 2, 16, 32), (0, 128, 4, 1024), (0, 3, 1024, 128)]


@pytest.mark.parametrize("dt,B,HW,C", EDGE_CASES)
@pytest.mark.parametrize("drop", [0.0, 0.1])
def test_scale_minus_one(dt, B, HW, C, drop):
    """The last sample has s = -1 on every channel: g_eff = gamma * (1 - 1) = 0 and b_eff = beta * 0 + h = h exactly, so that sample's
    y is drop(silu(shift)) per channel whatever x is, its dx from the norm is exactly zero, and dshift = sum dz is still right."""
    x, dy, _, _, gamma, beta, mod = inputs(B, HW, C, dt)
    mod = mod.clone()
    e = B - 1
    mod[e, :C] = -1.0
    got = run(B, HW, C, dt, 1, drop, mod=mod)
    h = mod[e, C:].to(DEV)
    want = torch.nn.functional.silu(h.double())[None, :].expand(HW, C)
    seed = SEED if drop else 0
    keep = torch.ones(HW, C, dtype=torch.bool, device=DEV)
    if drop:
        keep = R.keep_mask(seed, B, HW, C, drop, DEV).reshape(B, HW, C)[e]
        want = torch.where(keep, want / (1.0 - drop), torch.zeros_like(want))
    y = _f64(got["y"])[e * HW:(e + 1) * HW]
    u = LR.U_BF16 if dt else LR.U_F32
    # silu(h) in fp32 (the fast sigmoid: _sigmoid_err) then the store: the forward bar of the module docstring with its statistics terms at zero
    bar = LR.C_NORM * (u * want.abs() + LR.U_ACC * (LR._sigmoid_err(h.double())[None, :] + 3) * want.abs())
    assert bool(((y - want).abs() <= torch.clamp(bar, min=LR.TINY)).all()), float(((y - want).abs() / torch.clamp(bar, min=LR.TINY)).max())
    hi = torch.where(keep, y, torch.full_like(y, -math.inf)).max(0).values
    lo = torch.where(keep, y, torch.full_like(y, math.inf)).min(0).values
    assert bool(((hi == lo) | ~keep.any(0)).all()), "every kept pixel of a channel holds the same value"
    assert bool((y[~keep] == 0).all())
    dx = _f64(got["dx"])[e * HW:(e + 1) * HW]
    assert bool((dx == 0).all()), "g_eff = 0: the norm passes no gradient to x"
    sg = torch.sigmoid(h.double())
    dz = dy.to(DEV).double().reshape(B, HW, C)[e] * (sg * (1 + h.double() * (1 - sg)))[None, :]
    if drop:
        dz = torch.where(keep, dz / (1.0 - drop), torch.zeros_like(dz))
    dsh, ref = _f64(got["dmod"])[e, C:], dz.sum(0)
    # the pixel-sum bar of the module docstring: t = h exactly here, so e_t = |b_eff| + |b_eff| = 2 |h| (the model's term and the affine's)
    dyk = dy.to(DEV).double().reshape(B, HW, C)[e].abs() * (keep.double() / (1.0 - drop) if drop else 1.0)
    bar = LR.C_NORM * (LR.U_F32 * ref.abs() + LR.U_ACC * (math.sqrt(HW) * (dz * dz).sum(0).sqrt() + (dyk * 2 * h.abs().double()[None, :]).sum(0)))
    assert bool(((dsh - ref).abs() <= bar).all()), float(((dsh - ref).abs() / bar).max())
    if B > 1:                                                      # the other samples are the ordinary case
        other = _f64(got["dx"])[:HW]
        assert float(other.abs().max()) > 0


# ====================================================================================================== model level
RED = dict(in_channels=3, hid_channels=64, out_channels=3, ch_multipliers=[1, 2], num_res_blocks=1, apply_attn=[True, True], drop_rate=0.0)
KINDS = {"plain": False, "ssn": True}
SIZES = [(8, 8), (24, 20)]
MODES = [(torch.float32, 1e-3), (torch.bfloat16, 1.5e-1)]
K = 3


def r(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


@functools.lru_cache(maxsize=None)
def weights(kind, conditional=False, drop=0.0, out_channels=3):
    torch.manual_seed(5)
    m = ddpm_torch.UNet(**dict(RED, drop_rate=drop, out_channels=out_channels), use_scale_shift_norm=KINDS[kind], **({"num_classes": K} if conditional else {}))
    sd = U.randomize_state_dict(m.state_dict(), 17)
    return sd, {k: v.double() for k, v in sd.items()}


def model_of(kind, dtype, conditional=False, drop=0.0, out_channels=3):
    m = ddpm_torch.UNet(**dict(RED, drop_rate=drop, out_channels=out_channels), use_scale_shift_norm=KINDS[kind], **({"num_classes": K} if conditional else {}))
    m.load_state_dict(weights(kind, conditional, drop, out_channels)[0])
    return m.to(DEV).set_compute_dtype(dtype)


def forward64(kind, sd, cfg, x, t, **kw):
    return R.unet_forward(sd, cfg, x, t, **kw) if KINDS[kind] else U.unet_forward(sd, cfg, x, t, **kw)


@pytest.mark.parametrize("H,W,drop", [(8, 8, 0.0), (24, 20, 0.0), (8, 8, 0.1)])
@pytest.mark.parametrize("dtype,bar", MODES, ids=["fp32", "bf16"])
def test_forward_and_every_gradient_against_float64(dtype, bar, H, W, drop):
    cfg = dict(RED, drop_rate=drop)
    x, t, gy = r(3, 3, H, W, seed=1), torch.tensor([3, 977, 40]), r(3, 3, H, W, seed=2)
    for kind in ("plain", "ssn"):                                # the flag-off network first: the bar is the one it is held to
        m = model_of(kind, dtype, drop=drop).train()
        m.engine().debug_keep_tape = True
        out = m(x.to(DEV), t.to(DEV))
        (out * gy.to(DEV)).sum().backward()
        masks = CA.masks_from_tape(m, drop, DEV)
        p = {k: v.clone().requires_grad_(True) for k, v in weights(kind, False, drop)[1].items()}
        out64 = forward64(kind, p, cfg, x.double(), t, training=True, masks=masks)
        (out64 * gy.double()).sum().backward()
        out64, grads64 = out64.detach(), {k: v.grad for k, v in p.items()}
        rel = float((out.detach().cpu().double() - out64).abs().max() / out64.abs().max())
        scales = {k: float(v.abs().max()) for k, v in grads64.items()}
        floor = (0.02 if dtype == torch.float32 else 0.1) * sorted(scales.values())[len(scales) // 2]
        errs = {k: float((q.grad.cpu().double() - grads64[k]).abs().max()) / max(scales[k], floor) for k, q in m.named_parameters()}
        rows = sorted(((e, k) for k, e in errs.items()), reverse=True)
        print(f"\n  {kind} {H}x{W} drop {drop} {dtype}: forward rel err {rel:.3e}; worst gradients " + ", ".join(f"{k} {e:.2e}" for e, k in rows[:3]))
        assert rel < bar, (kind, rel)
        assert rows[0][0] < 3 * bar, (kind, rows[0])
        if kind == "ssn":
            named = dict(m.named_parameters())
            assert named["middle.0.fc.weight"].grad.shape == (256, 256) and named["middle.0.fc.bias"].grad.shape == (256,)
            for k in ("fc.weight", "fc.bias", "conv1.bias", "norm2.weight", "norm2.bias"):
                for blk in ("middle.0.", "downsamples.level_0.0.0.", "upsamples.level_1.1.0."):
                    assert errs[blk + k] < 3 * bar and scales[blk + k] > 0, (blk + k, errs[blk + k])
                    print(f"    {blk + k}: {errs[blk + k]:.2e}")


@pytest.mark.parametrize("H,W", SIZES)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_three_trainer_steps_plan_equals_eager_and_both_follow_the_oracle_trainer(dtype, H, W, monkeypatch):
    """fp32 mode: tests/test_cond_gpu.py's equality (lr 1e-3; losses rtol 5e-4, states 1e-3 with the Adam slack), plan against eager and
    both against the float64 oracle trainer.  bf16 mode: tests/test_attention_any_tokens_gpu.py's (lr 1e-4: first loss 1e-5, second
    7.5e-3, third 1.2e-1 relative, parameters within 2 lr x steps) between the two forms, as tests/test_mha_gpu.py explains; against the
    oracle the bf16 losses are held to that file's forward bar (1.5e-1)."""
    from ddpm_torch.utils import train as train_mod
    lr = 1e-3 if dtype == torch.float32 else 1e-4
    g = torch.Generator().manual_seed(21)
    xs = [torch.rand(4, 3, H, W, generator=g) * 2 - 1 for _ in range(3)]
    for kind in ("plain", "ssn"):
        runs = {}
        for path in ("plan", False):
            monkeypatch.setattr(train_mod, "_TRAIN_GRAPH", path)
            m = model_of(kind, dtype)
            dif = ddpm_torch.GaussianDiffusion(ddpm_torch.get_beta_schedule("linear", 1e-4, 0.02, 1000), "eps", "fixed-large", "mse")
            opt = torch.optim.Adam(m.parameters(), lr=lr, betas=(0.9, 0.999))
            tr = ddpm_torch.Trainer(m, opt, dif, epochs=1, trainloader=None, scheduler=None, use_ema=True, grad_norm=1.0, shape=(3, H, W),
                                    device=torch.device(DEV), ema_decay=0.9999)
            m.train()
            losses, drawn = [], []
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
        slack = 0.25 * lr * 3
        if dtype == torch.float32:
            assert torch.allclose(torch.tensor(la, dtype=torch.float64), torch.tensor(lb, dtype=torch.float64), rtol=5e-4), (kind, la, lb)
            check_state(pa, pb, 1e-3, f"{kind} param", adam_slack=slack)
            check_state(sa, sb, 1e-3, f"{kind} shadow", adam_slack=slack)
        else:
            worst = max(float((pa[k] - v).abs().max()) for k, v in pb.items()) / (lr * 3)
            print(f"  parameters differ by at most {worst:.2f} x lr x steps")
            assert abs(la[0] - lb[0]) <= 1e-5 * abs(lb[0]), (kind, la, lb)
            assert abs(la[1] - lb[1]) <= 7.5e-3 * abs(lb[1]) and abs(la[2] - lb[2]) <= 1.2e-1 * abs(lb[2]), (kind, la, lb)
            assert worst <= 2.0, (kind, worst)
        assert any(not torch.equal(pa[k], weights(kind)[0][k]) for k in pa), "the steps moved nothing"
        # ---- the float64 oracle trainer on the trainer's own (t, noise) stream: the device generator's draws are replayed on the device
        gen = torch.Generator(DEV).manual_seed(CA.GEN_SEED)
        oracle = CA.OracleTrainer(weights(kind)[0], RED, lr)
        ref = []
        with (R.bound() if KINDS[kind] else _null()):
            for x in xs:
                t = torch.empty((4,), dtype=torch.int64, device=DEV).random_(to=1000, generator=gen)
                noise = torch.empty(4, 3, H, W, device=DEV).normal_(generator=gen)
                ref.append(oracle.step(x, inputs=(t.cpu(), noise.cpu()))[0])
        print(f"  oracle losses {ref}")
        if dtype == torch.float32:
            for got in (la, lb):
                assert torch.allclose(torch.tensor(got, dtype=torch.float64), torch.tensor(ref, dtype=torch.float64), rtol=5e-4), (kind, got, ref)
            check_state(pa, oracle.state(), 1e-3, f"{kind} param vs oracle", adam_slack=slack)
            check_state(pb, oracle.state(), 1e-3, f"{kind} param vs oracle (eager)", adam_slack=slack)
        else:
            assert all(abs(a - b) <= 1.5e-1 * abs(b) for a, b in zip(la, ref)), (kind, la, ref)


class _null:
    def __enter__(self):
        return None

    def __exit__(self, *a):
        return False


@pytest.mark.parametrize("H,W", SIZES)
@pytest.mark.parametrize("dtype,bar", MODES, ids=["fp32", "bf16"])
def test_replayed_chains_equal_eager_chains_and_follow_the_oracle(dtype, bar, H, W, monkeypatch):
    """A 10-step graph-replayed p_sample chain and one guided chain (num_classes = 3, scale 2): bit-equal to the eager loops; the chain with
    the time table against DDPM_TIME_TABLE=0 inside 2e-5 of the sample's range (fp32 mode, where tests/test_configs_gpu.py sets that bar);
    and an injected-noise chain against oracle.diffusion_ref.sample_loop on the float64 network, at the forward bar of the mode."""
    T = 10
    dif = ddpm_torch.GaussianDiffusion(ddpm_torch.get_beta_schedule("linear", 1e-4, 0.02, T), "eps", "fixed-large", "mse")
    shape, y, by_kind = (3, 3, H, W), torch.tensor([2, 0, 1], device=DEV), {}
    x_T, zs = r(*shape, seed=7), r(T, *shape, seed=8)
    tables = D.ddpm_tables(D.beta_schedule("linear", 1e-4, 0.02, T), "fixed-large")
    for kind in ("plain", "ssn"):
        m, mc = model_of(kind, dtype).eval(), model_of(kind, dtype, conditional=True).eval()
        outs = {}
        for mode in ("1", "0"):
            monkeypatch.setenv("DDPM_TORCH_AMD_GRAPH", mode)
            outs[mode] = dif.p_sample(m, shape=shape, device=DEV, seed=77)
            outs[mode + "g"] = dif.p_sample(mc, shape=shape, device=DEV, seed=77, y=y, guidance_scale=2.0)
        assert torch.equal(outs["1"], outs["0"]) and torch.equal(outs["1g"], outs["0g"]), kind
        assert bool(torch.isfinite(outs["1"]).all()) and bool(torch.isfinite(outs["1g"]).all()) and not torch.equal(outs["1"], outs["1g"])
        by_kind[kind] = outs["1"]
        if dtype == torch.float32:
            monkeypatch.setenv("DDPM_TIME_TABLE", "0")
            no_table = dif.p_sample(model_of(kind, dtype).eval(), shape=shape, device=DEV, seed=77)
            monkeypatch.delenv("DDPM_TIME_TABLE")
            gap = float((no_table - outs["0"]).abs().max()) / float(no_table.max() - no_table.min())
            print(f"\n  {kind} {H}x{W}: time table vs DDPM_TIME_TABLE=0: {gap:.3e} of the sample's range")
            assert gap <= 2e-5, (kind, gap)
        sd64 = weights(kind)[1]
        with torch.no_grad():
            got = dif._sample_loop(m, shape, torch.device(DEV), x_T.to(DEV), None, z_stream=iter(zs.to(DEV)))
            want = D.sample_loop(tables, lambda a, b: forward64(kind, sd64, RED, a, b), x_T.double(), zs.double())
        rel = float((got.cpu().double() - want).abs().max() / want.abs().max())
        print(f"  {kind} {H}x{W} {dtype}: injected-noise chain rel err {rel:.3e}")
        assert rel < bar, (kind, rel)
    assert not torch.equal(by_kind["plain"], by_kind["ssn"])


def test_one_learned_range_hybrid_plan_step(monkeypatch):
    """Scale-shift norm + a learned-range 2C output under the hybrid loss through the launch-plan step: equal to the eager form (the fp32 bars of
    the test above)."""
    from ddpm_torch.utils import train as train_mod
    lr, H, W = 1e-3, 8, 8
    g = torch.Generator().manual_seed(21)
    xs = [torch.rand(4, 3, H, W, generator=g) * 2 - 1 for _ in range(3)]
    runs = {}
    for path in ("plan", False):
        monkeypatch.setattr(train_mod, "_TRAIN_GRAPH", path)
        m = model_of("ssn", torch.float32, out_channels=6)
        dif = ddpm_torch.GaussianDiffusion(ddpm_torch.get_beta_schedule("linear", 1e-4, 0.02, 1000), "eps", "learned-range", "hybrid")
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
            assert ds.plan is not None and ds.last_kind == "plan"
            assert "ddpm_groupnorm_mod_silu_bwd" in {n for seg in ds.plan.segments for n, _ in seg}
        runs[path] = (losses, {k: v.cpu() for k, v in m.state_dict().items()})
    (la, pa), (lb, pb) = runs["plan"], runs[False]
    print(f"\n  learned-range hybrid: losses plan {la} eager {lb}")
    assert all(l == l for l in la) and torch.allclose(torch.tensor(la, dtype=torch.float64), torch.tensor(lb, dtype=torch.float64), rtol=5e-4), (la, lb)
    check_state(pa, pb, 1e-3, "param", adam_slack=0.25 * lr * 3)
