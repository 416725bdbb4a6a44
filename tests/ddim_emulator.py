"""TEST INFRASTRUCTURE for DDIM inversion and latent interpolation (csrc/ddim.hip, ddim.DDIM.encode / ddim.slerp): numpy restatements of
``ddpm_ddim_encode_step`` and ``ddpm_slerp`` as include/ddpm_hip.h states them, over the raw host pointers the product passes, for the
host emulator (tests/abi_emulator.py; ``attach`` hangs them on the Emulator instance ``install`` returns).  fp32 arithmetic like the
kernels'; they say nothing about the kernels themselves — tests/test_ddim_inverse_gpu.py holds those to float64."""
import numpy as np

from tests.abi_emulator import f32, i64

SLERP_CHUNK = 2048                      # csrc/ddim.hip: elements of a pair per workgroup (and per workspace entry)


def ddpm_ddim_encode_step(x, model_out, t, cx, ce, recip, recip_m1, x_next, pred_x0, B, n, S, st):
    assert x and model_out and t and cx and ce and recip and recip_m1 and x_next and B > 0 and n > 0 and S > 0
    tt = i64(t, B)
    ok = (tt >= 0) & (tt < S)
    tc = np.clip(tt, 0, S - 1)
    g = lambda p: f32(p, S)[tc][:, None]                                                   # noqa: E731
    xv, ev = f32(x, B * n).reshape(B, n).copy(), f32(model_out, B * n).reshape(B, n)       # copy: x_next may be x
    nan = np.float32("nan")
    f32(x_next, B * n).reshape(B, n)[...] = np.where(ok[:, None], g(cx) * xv + g(ce) * ev, nan)
    if pred_x0:
        f32(pred_x0, B * n).reshape(B, n)[...] = np.where(ok[:, None], g(recip) * xv - g(recip_m1) * ev, nan)


def slerp_workspace_floats(P, n):
    return -1 if P < 0 or n < 0 else 6 * P * ((n + SLERP_CHUNK - 1) // SLERP_CHUNK)


def ddpm_slerp(a, b, alpha, out, ws, P, K, n, st):
    assert a and b and alpha and out and ws and P > 0 and K > 0 and n > 0
    av, bv, al = f32(a, P * n).reshape(P, n), f32(b, P * n).reshape(P, n), f32(alpha, K).astype(np.float64)
    chunks = (n + SLERP_CHUNK - 1) // SLERP_CHUNK
    part = f32(ws, 6 * P * chunks).reshape(P, chunks, 3, 2)                                # every sum as a (hi, lo) pair of floats
    for c in range(chunks):
        sa = av[:, c * SLERP_CHUNK:(c + 1) * SLERP_CHUNK].astype(np.float64)
        sb = bv[:, c * SLERP_CHUNK:(c + 1) * SLERP_CHUNK].astype(np.float64)
        with np.errstate(all="ignore"):
            for q, sm in enumerate(((sa * sb).sum(1), (sa * sa).sum(1), (sb * sb).sum(1))):
                hi = sm.astype(np.float32)
                part[:, c, q, 0], part[:, c, q, 1] = hi, (sm - hi).astype(np.float32)
    tot = part.astype(np.float64).sum(3).sum(1)
    with np.errstate(all="ignore"):
        cs = np.clip(tot[:, 0] / (np.sqrt(tot[:, 1]) * np.sqrt(tot[:, 2])), -1.0, 1.0)
        linear = ~((1.0 - np.abs(cs)) >= 1e-6)
        th = np.arccos(np.where(linear, 0.0, cs))[:, None]
        w0 = np.where(linear[:, None], 1.0 - al[None], np.sin((1.0 - al[None]) * th) / np.sin(th)).astype(np.float32)
        w1 = np.where(linear[:, None], al[None] + 0.0 * th, np.sin(al[None] * th) / np.sin(th)).astype(np.float32)
        f32(out, P * K * n).reshape(P, K, n)[...] = w0[:, :, None] * av[:, None, :] + w1[:, :, None] * bv[:, None, :]


def attach(emu):
    """Add the two entry points to an ``abi_emulator.Emulator`` instance (its ``call`` is ``getattr(self, name)``)."""
    emu.ddpm_ddim_encode_step = ddpm_ddim_encode_step
    emu.ddpm_slerp = ddpm_slerp
    return emu
