"""TEST INFRASTRUCTURE for the scale-shift norm (csrc/norm.hip: ``ddpm_groupnorm_mod_silu_fwd`` / ``ddpm_groupnorm_mod_silu_bwd``):
numpy restatements of the two entry points as include/ddpm_hip.h states them, over the raw host pointers the product passes, for the host
emulator (tests/abi_emulator.py; ``attach`` hangs them on the Emulator instance ``install`` returns).  Float64 arithmetic on the stored
operands, rounded where the entry point stores.  They say nothing about the kernels themselves — tests/test_adagn_gpu.py holds those to
float64."""
import ctypes

import numpy as np

from tests.abi_emulator import F32, Mat, _keep_mask, _np, _thresh, f32


def _seed(seed, seed_dev, drop_p):
    if seed_dev and drop_p > 0:
        seed = (seed + int(_np(seed_dev, 1, ctypes.c_uint64, np.uint64)[0])) & ((1 << 64) - 1)
    return seed


def _affine(gamma, beta, mod, mod_ld, B, C):
    """g_eff, b_eff as [B][1][C] float64; the padding of a mod row (columns past 2C) is never read."""
    m = Mat(mod, B, 2 * C, mod_ld, F32).get().astype(np.float64)
    gm, bt = f32(gamma, C).astype(np.float64), f32(beta, C).astype(np.float64)
    s1 = 1.0 + m[:, :C]
    return (gm[None, :] * s1)[:, None, :], (bt[None, :] * s1 + m[:, C:])[:, None, :], s1, gm, bt


def _keep(seed, B, HW, C, drop_p):
    return _keep_mask(seed, np.arange(B * HW * C, dtype=np.uint64), _thresh(drop_p)).reshape(B, HW, C)


def ddpm_groupnorm_mod_silu_fwd(x, x_ld, y, y_ld, gamma, beta, stats, ws, B, HW, C, G, eps, silu, drop_p, seed, seed_dev, mod, mod_ld, dt, st):
    assert x and y and gamma and beta and ws and mod and mod_ld >= 2 * C and C % G == 0
    seed = _seed(seed, seed_dev, drop_p)
    xin = Mat(x, B * HW, C, x_ld, dt).get().astype(np.float64).reshape(B, HW, G, C // G)
    mean = xin.mean((1, 3), keepdims=True)
    var = ((xin - mean) ** 2).mean((1, 3), keepdims=True)
    rstd = 1.0 / np.sqrt(var + eps)
    g_eff, b_eff, _, _, _ = _affine(gamma, beta, mod, mod_ld, B, C)
    t = ((xin - mean) * rstd).reshape(B, HW, C) * g_eff + b_eff
    out = t / (1.0 + np.exp(-t)) if silu else t
    if drop_p > 0:
        out = np.where(_keep(seed, B, HW, C, drop_p), out / (1.0 - drop_p), 0.0)        # a select: a dropped element is 0 whatever its value
    Mat(y, B * HW, C, y_ld, dt).set(out.reshape(B * HW, C).astype(np.float32))
    if stats:
        s = f32(stats, B * G * 2).reshape(B, G, 2)
        s[..., 0] = mean.reshape(B, G).astype(np.float32); s[..., 1] = rstd.reshape(B, G).astype(np.float32)


def ddpm_groupnorm_mod_silu_bwd(x, x_ld, dy, dy_ld, dx, dx_ld, gamma, beta, stats, dgamma, dbeta, ws, B, HW, C, G, silu, drop_p, seed, seed_dev,
                                acc, dx_colsum, colsum_ld, add, add_ld, mod, mod_ld, dmod, dmod_ld, dt, st):
    assert x and dy and dx and gamma and beta and stats and ws and mod and dmod and mod_ld >= 2 * C and dmod_ld >= 2 * C
    seed = _seed(seed, seed_dev, drop_p)
    # the contract's formula on the statistics the caller passes (the kernel recomputes neither), in float64
    stv = f32(stats, B * G * 2).astype(np.float64).reshape(B, G, 2)
    mean, rstd = stv[:, None, :, :1], stv[:, None, :, 1:]
    grouped = lambda v: v.reshape(B, HW, G, C // G)                                          # noqa: E731
    xh = ((grouped(Mat(x, B * HW, C, x_ld, dt).get().astype(np.float64)) - mean) * rstd).reshape(B, HW, C)
    g_eff, b_eff, s1, gm, bt = _affine(gamma, beta, mod, mod_ld, B, C)
    tt = g_eff * xh + b_eff
    dz = Mat(dy, B * HW, C, dy_ld, dt).get().astype(np.float64).reshape(B, HW, C)
    if silu:
        sg = 1.0 / (1.0 + np.exp(-tt))
        dz = dz * sg * (1.0 + tt * (1.0 - sg))
    if drop_p > 0:
        dz = np.where(_keep(seed, B, HW, C, drop_p), dz / (1.0 - drop_p), 0.0)
    a = dz * g_eff
    c1, c2 = grouped(a * xh).mean((1, 3), keepdims=True), grouped(a).mean((1, 3), keepdims=True)
    val = (rstd * (grouped(a) - grouped(xh) * c1 - c2)).reshape(B * HW, C).astype(np.float32)
    dst = Mat(dx, B * HW, C, dx_ld, dt)
    if add:
        val = val + Mat(add, B * HW, C, add_ld, dt).get()
    dst.set(dst.get() + val if acc else val)
    if dx_colsum:
        cs = Mat(dx_colsum, B, C, colsum_ld, F32)
        cs.set(cs.get() + dst.get().reshape(B, HW, C).sum(1))
    A, D = (dz * xh).sum(1), dz.sum(1)                                                        # [B][C]
    if dgamma:
        f32(dgamma, C)[...] += (A * s1).sum(0).astype(np.float32)
    if dbeta:
        f32(dbeta, C)[...] += (D * s1).sum(0).astype(np.float32)
    Mat(dmod, B, 2 * C, dmod_ld, F32).set(np.concatenate([gm[None, :] * A + bt[None, :] * D, D], 1).astype(np.float32))    # overwritten


def attach(emu):
    """Add the two entry points to an ``abi_emulator.Emulator`` instance (its ``call`` is ``getattr(self, name)``)."""
    emu.ddpm_groupnorm_mod_silu_fwd = ddpm_groupnorm_mod_silu_fwd
    emu.ddpm_groupnorm_mod_silu_bwd = ddpm_groupnorm_mod_silu_bwd
    return emu
