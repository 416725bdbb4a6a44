"""TEST INFRASTRUCTURE: the float64 reference of the scale-shift norm (``UNet(use_scale_shift_norm=True)``;
``ddpm_groupnorm_mod_silu_fwd`` / ``ddpm_groupnorm_mod_silu_bwd``).  Nothing of it exists upstream (the reference's block adds
``fc(SiLU(t_emb))`` behind ``conv1``), so it is stated here from the equations of the Improved-DDPM / ADM residual block with
``use_scale_shift_norm=True``, on top of the pinned oracle and in its style:

    emb = fc(SiLU(t_emb));  scale, shift = emb.chunk(2, dim=1)                      fc: Linear(E, 2 Cout)
    h = conv1(SiLU(norm1(x)))                                                       conv1.bias only
    h = norm2(h) * (1 + scale[:, :, None, None]) + shift[:, :, None, None]
    out = skip(x) + conv2(dropout(SiLU(h)))

* ``residual_block`` is that block, composed of the oracle's own ``group_norm`` and storage hooks;
* ``bound`` runs the oracle's network (and its trainer, which looks ``unet_forward`` up at call time) with that block in the place of
  ``oracle.unet_ref.residual_block`` — ``_block`` / ``unet_forward`` look the name up in their module at call time, so the oracle's file
  is untouched and the binding is restored on exit;
* ``entry_fwd`` / ``entry_bwd`` restate the two entry points' contracts over [B*HW][C] operands: the backward from the GIVEN statistics,
  the dropout mask by the project's hash as tests/launch_replay.py restates it (``keep_mask``).

Everything follows the dtype of its inputs: float64 inputs give the reference."""
import contextlib

import torch
import torch.nn.functional as F

from oracle import unet_ref as U
from tests import launch_replay as LR


def residual_block(sd, p, x, t_emb, drop_p=0.0, training=False, mask=None):
    """The modulated block; the signature of ``oracle.unet_ref.residual_block``."""
    skip = x
    if p + "skip.weight" in sd:
        skip = U._st("conv", F.conv2d(x, sd[p + "skip.weight"], sd[p + "skip.bias"]))
    cout = sd[p + "conv1.weight"].shape[0]
    emb = F.linear(F.silu(t_emb), sd[p + "fc.weight"], sd[p + "fc.bias"])
    assert emb.shape[1] == 2 * cout, (p, tuple(emb.shape), cout)
    scale, shift = emb.chunk(2, dim=1)
    h = U._st("conv", F.conv2d(U._st("gn", F.silu(U.group_norm(x, sd[p + "norm1.weight"], sd[p + "norm1.bias"]))),
                               sd[p + "conv1.weight"], sd[p + "conv1.bias"], padding=1))
    h = U.group_norm(h, sd[p + "norm2.weight"], sd[p + "norm2.bias"]) * (1 + scale[:, :, None, None]) + shift[:, :, None, None]
    h = U._st("gn", F.silu(h))
    if training and drop_p > 0:
        if mask is not None:
            h = h * mask.to(h.dtype) / (1.0 - drop_p)
        else:
            h = F.dropout(h, drop_p, training=True)
    h = F.conv2d(h, sd[p + "conv2.weight"], sd[p + "conv2.bias"], padding=1)
    return U._st("conv", h + skip)


@contextlib.contextmanager
def bound():
    """``oracle.unet_ref`` with the modulated block bound in the place of ``residual_block`` for the duration of the block."""
    saved = U.residual_block
    U.residual_block = residual_block
    try:
        yield U
    finally:
        U.residual_block = saved


def unet_forward(sd, cfg, x, t, **kw):
    """``oracle.unet_ref.unet_forward`` of the scale-shift network (``cfg``: the reference's keys only; every fc holds 2 Cout rows)."""
    with bound():
        return U.unet_forward(sd, cfg, x, t, **kw)


def init_state_dict(cfg, dtype=torch.float32):
    """``oracle.unet_ref.init_state_dict`` with every ResidualBlock's fc drawn at [2 Cout, E] (same draw order)."""
    saved = U._res_keys

    def keys(prefix, cin, cout, edim):
        return [(k, ((2 * s[0],) + tuple(s[1:]) if k.endswith(("fc.weight", "fc.bias")) else s), i) for k, s, i in saved(prefix, cin, cout, edim)]
    U._res_keys = keys
    try:
        return U.init_state_dict(cfg, dtype)
    finally:
        U._res_keys = saved


def keep_mask(seed, B, HW, C, drop_p, device=None):
    """The project's dropout keep-mask over the linear NHWC index, [B*HW][C] bool."""
    idx = torch.arange(B * HW * C, dtype=torch.int64, device=device)
    return LR.keep_mask(int(seed) & ((1 << 64) - 1), idx, drop_p).reshape(B * HW, C)


def affine(gamma, beta, mod, C):
    """g_eff, b_eff [B][C] of rows ``mod`` = [scale | shift | ...]."""
    s, h = mod[:, :C], mod[:, C:2 * C]
    return gamma[None, :] * (1 + s), beta[None, :] * (1 + s) + h


def _grouped(x, B, HW, G, C):
    return x.reshape(B, HW, G, C // G)


def entry_fwd(x, gamma, beta, mod, B, HW, C, G, eps, silu, drop_p, seed):
    """Contract of ddpm_groupnorm_mod_silu_fwd: y [B*HW][C], stats [B][G][2] = (mean, rstd)."""
    xg = _grouped(x, B, HW, G, C)
    mean = xg.mean((1, 3), keepdim=True)
    var = ((xg - mean) ** 2).mean((1, 3), keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    g_eff, b_eff = affine(gamma, beta, mod, C)
    t = ((xg - mean) * rstd).reshape(B, HW, C) * g_eff[:, None, :] + b_eff[:, None, :]
    y = F.silu(t) if silu else t
    if drop_p > 0:
        y = torch.where(keep_mask(seed, B, HW, C, drop_p, x.device).reshape(B, HW, C), y / (1.0 - drop_p), torch.zeros_like(y))
    return y.reshape(B * HW, C), torch.stack([mean.reshape(B, G), rstd.reshape(B, G)], -1)


def entry_bwd(x, dy, gamma, beta, stats, mod, B, HW, C, G, silu, drop_p, seed):
    """Contract of ddpm_groupnorm_mod_silu_bwd on the GIVEN stats [B][G][2]: returns dx [B*HW][C] (before accumulate / add), dgamma [C],
    dbeta [C], dmod [B][2C] = [dscale | dshift], and the intermediates a bar is built from (xhat, dz, g_eff)."""
    mean, rstd = stats[:, None, :, :1], stats[:, None, :, 1:]
    xh = ((_grouped(x, B, HW, G, C) - mean) * rstd).reshape(B, HW, C)
    g_eff, b_eff = affine(gamma, beta, mod, C)
    t = xh * g_eff[:, None, :] + b_eff[:, None, :]
    dz = dy.reshape(B, HW, C)
    if drop_p > 0:
        dz = torch.where(keep_mask(seed, B, HW, C, drop_p, x.device).reshape(B, HW, C), dz / (1.0 - drop_p), torch.zeros_like(dz))
    if silu:
        sg = torch.sigmoid(t)
        dz = dz * sg * (1 + t * (1 - sg))
    a = dz * g_eff[:, None, :]
    c1 = _grouped(a * xh, B, HW, G, C).mean((1, 3), keepdim=True)
    c2 = _grouped(a, B, HW, G, C).mean((1, 3), keepdim=True)
    dx = (rstd * (_grouped(a, B, HW, G, C) - _grouped(xh, B, HW, G, C) * c1 - c2)).reshape(B * HW, C)
    A, D = (dz * xh).sum(1), dz.sum(1)                                                 # [B][C]
    s1 = 1 + mod[:, :C]
    dmod = torch.cat([gamma[None, :] * A + beta[None, :] * D, D], 1)
    return dx, (A * s1).sum(0), (D * s1).sum(0), dmod, dict(xhat=xh, dz=dz, g_eff=g_eff, A=A, D=D)
