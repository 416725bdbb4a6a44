"""TEST INFRASTRUCTURE for class conditioning and classifier-free guidance (csrc/guidance.hip: ``ddpm_class_embed_fwd``,
``ddpm_class_embed_bwd``, ``ddpm_p_sample_step_cfg``): numpy restatements of the three entry points as include/ddpm_hip.h states them, over
the raw host pointers the product passes, for the host emulator (tests/abi_emulator.py; ``attach`` hangs them on the Emulator instance
``install`` returns).  fp32 arithmetic like the kernels'.  They say nothing about the kernels themselves — tests/test_cond_gpu.py holds
those to float64."""
import numpy as np
import torch
import torch.nn.functional as F

from tests.abi_emulator import f32, i64

NAN = np.float32("nan")


def ddpm_class_embed_fwd(t_emb, table, y, pre, s, B, E, K1, st):
    assert t_emb and table and y and pre and s and B > 0 and E > 0 and K1 > 0
    yy = i64(y, B)
    ok = (yy >= 0) & (yy < K1)
    rows = f32(table, K1 * E).reshape(K1, E)[np.where(ok, yy, 0)]
    p = np.where(ok[:, None], f32(t_emb, B * E).reshape(B, E) + rows, NAN).astype(np.float32)
    f32(pre, B * E)[...] = p.reshape(-1)
    f32(s, B * E)[...] = F.silu(torch.from_numpy(p)).numpy().reshape(-1)


def ddpm_class_embed_bwd(dpre, y, dtable, B, E, K1, st):
    assert dpre and y and dtable and B > 0 and E > 0 and 0 < K1 <= 65535
    yy, d = i64(y, B), f32(dpre, B * E).reshape(B, E)
    out = np.zeros((K1, E), dtype=np.float32)
    for b in range(B):                               # ascending b, fp32 adds: the kernel's order
        if 0 <= yy[b] < K1:
            out[yy[b]] = out[yy[b]] + d[b]
    f32(dtable, K1 * E)[...] = out.reshape(-1)


def ddpm_p_sample_step_cfg(x_t, out2, z, t, recip, recip_m1, c1, c2, logvar, scale, x_prev, pred, B, n, mean_type, clip, dup, T, st):
    assert x_t and out2 and z and t and x_prev and recip and recip_m1 and c1 and c2 and logvar and 0 < B <= 65535 and n > 0 and 0 <= mean_type <= 2
    tt = i64(t, B)
    ok = (tt >= 0) & (tt < T)
    tc = np.clip(tt, 0, T - 1)
    g = lambda p: f32(p, T)[tc][:, None]                                                   # noqa: E731
    xt, zz = f32(x_t, B * n).reshape(B, n).copy(), f32(z, B * n).reshape(B, n).copy()      # (copies: x_prev may be x_t)
    o2 = f32(out2, 2 * B * n).reshape(2 * B, n)
    sc = np.float32(scale)
    o = (sc * o2[:B] + (np.float32(1.0) - sc) * o2[B:]).astype(np.float32)
    if mean_type == 0:
        x0 = g(recip) * xt - g(recip_m1) * o
    elif mean_type == 1:
        x0 = o.copy()
    else:
        x0 = o / g(c1) - g(c2) / g(c1) * xt
    if clip:
        x0 = np.where(np.isnan(x0), x0, np.clip(x0, -1.0, 1.0))
    mean = o if mean_type == 2 else g(c1) * x0 + g(c2) * xt
    mask = (tt > 0).astype(np.float32)[:, None]
    nxt = np.where(ok[:, None], mean + mask * np.exp(np.float32(0.5) * g(logvar)) * zz, NAN).astype(np.float32)
    dst = f32(x_prev, (2 if dup else 1) * B * n).reshape(-1, n)
    dst[:B] = nxt
    if dup:
        dst[B:] = nxt
    if pred:
        f32(pred, B * n).reshape(B, n)[...] = np.where(ok[:, None], x0, NAN)


def attach(emu):
    """Add the three entry points to an ``abi_emulator.Emulator`` instance (its ``call`` is ``getattr(self, name)``)."""
    emu.ddpm_class_embed_fwd = ddpm_class_embed_fwd
    emu.ddpm_class_embed_bwd = ddpm_class_embed_bwd
    emu.ddpm_p_sample_step_cfg = ddpm_p_sample_step_cfg
    return emu
