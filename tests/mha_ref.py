"""TEST INFRASTRUCTURE: the float64 reference of multi-head attention (``UNet(num_heads=)`` / ``num_head_channels=``;
``ddpm_attention_mh_fwd`` / ``ddpm_attention_mh_bwd``).  Nothing of it exists upstream (the reference's block is the single head), so it is
stated here on top of the pinned oracle, in its style:

* ``attention_core_mh`` is ``oracle.unet_ref.attention_core`` with every third of the projection split into ``heads`` groups of
  d = C / heads consecutive channels (``qkv.chunk(3, 1)`` first, then the split: the ordering of ADM's ``QKVAttention``), one softmax per
  head at scale 1/sqrt(d);
* ``bound`` runs the oracle's network with that core in the place of ``attention_core`` — ``attention_block`` looks the name up in its
  module at call time, so the oracle's file is untouched and the binding is restored on exit;
* ``entry_fwd`` / ``entry_bwd`` restate the two entry points' contracts over a packed [B][L][3C] buffer, the backward from the GIVEN lse and
  the GIVEN o as tests/test_attention_stream_gpu.py does for one head.

Everything follows the dtype of its inputs: float64 inputs give the reference."""
import contextlib
import math

import torch

from oracle import unet_ref as U


def attention_core_mh(q, k, v, heads):
    """q, k, v: [B, C, H, W].  Head h = channels [h d, (h + 1) d), softmax over the H*W keys, scale 1/sqrt(d)."""
    B, C, H, W = q.shape
    assert C % heads == 0, (C, heads)
    d = C // heads
    qf, kf, vf = (z.reshape(B, heads, d, H * W) for z in (q, k, v))
    logits = torch.einsum("bhcq,bhck->bhqk", qf, kf) / math.sqrt(d)
    p = U._st("attn", torch.softmax(logits, dim=-1))
    out = torch.einsum("bhqk,bhck->bhcq", p, vf)
    return U._st("attn", out.reshape(B, C, H, W))


def heads_of(C, num_heads=1, num_head_channels=None):
    return C // num_head_channels if num_head_channels is not None else num_heads


@contextlib.contextmanager
def bound(num_heads=1, num_head_channels=None):
    """``oracle.unet_ref`` with the multi-head core bound in the place of ``attention_core`` for the duration of the block."""
    saved = U.attention_core
    U.attention_core = lambda q, k, v: attention_core_mh(q, k, v, heads_of(q.shape[1], num_heads, num_head_channels))
    try:
        yield U
    finally:
        U.attention_core = saved


def unet_forward(sd, cfg, x, t, num_heads=1, num_head_channels=None, **kw):
    """``oracle.unet_ref.unet_forward`` of the multi-head network (``cfg``: the reference's keys only)."""
    with bound(num_heads, num_head_channels):
        return U.unet_forward(sd, cfg, x, t, **kw)


def _split(x, B, L, C, heads):
    """packed [B*L][3C] -> q, k, v as [B][heads][L][d]"""
    x = x.reshape(B, L, 3, heads, C // heads)
    return tuple(x[:, :, i].permute(0, 2, 1, 3) for i in range(3))


def entry_fwd(qkv, B, L, C, heads, scale):
    """Contract of ddpm_attention_mh_fwd: O [B*L][C] (head h at channels [h d, (h + 1) d)), lse [B][heads][L]."""
    q, k, v = _split(qkv, B, L, C, heads)
    s = torch.einsum("bhic,bhjc->bhij", q, k) * scale
    lse = torch.logsumexp(s, dim=-1)
    o = torch.einsum("bhij,bhjc->bhic", torch.exp(s - lse[..., None]), v)
    return o.permute(0, 2, 1, 3).reshape(B * L, C), lse


def entry_bwd(qkv, o, d_o, lse, B, L, C, heads, scale):
    """Contract of ddpm_attention_mh_bwd: P rebuilt from q, k and the GIVEN lse [B][heads][L], D from the GIVEN o [B*L][C].
    Returns D [B][heads][L] and dq | dk | dv [B*L][3C] in the head layout of qkv."""
    d = C // heads
    q, k, v = _split(qkv, B, L, C, heads)
    oh, doh = (z.reshape(B, L, heads, d).permute(0, 2, 1, 3) for z in (o, d_o))
    p = torch.exp(torch.einsum("bhic,bhjc->bhij", q, k) * scale - lse.reshape(B, heads, L)[..., None])
    D = (doh * oh).sum(-1)
    ds = p * (torch.einsum("bhic,bhjc->bhij", doh, v) - D[..., None])
    dq = torch.einsum("bhij,bhjc->bhic", ds, k) * scale
    dk = torch.einsum("bhij,bhic->bhjc", ds, q) * scale
    dv = torch.einsum("bhij,bhic->bhjc", p, doh)
    g = torch.stack([z.permute(0, 2, 1, 3) for z in (dq, dk, dv)], dim=2)          # [B][L][3][heads][d]
    return D, g.reshape(B * L, 3 * C)
