"""TEST INFRASTRUCTURE for multi-head attention (csrc/attention_stream.hip: ``ddpm_attention_mh_fwd`` / ``ddpm_attention_mh_bwd``, and
the single-head streaming pair ``ddpm_attention_stream_fwd`` / ``ddpm_attention_stream_bwd`` as their one-head case):
numpy restatements of the entry points as include/ddpm_hip.h states them, over the raw host pointers the product passes, for the host
emulator (tests/abi_emulator.py; ``attach`` hangs them on the Emulator instance ``install`` returns).  Float64 arithmetic on the stored
operands, rounded where the entry point stores.  They say nothing about the kernels themselves — tests/test_mha_gpu.py holds those to
float64."""
import numpy as np

from tests.abi_emulator import Mat, f32


def _heads(m, B, L, heads, d):
    """[B*L][heads*d] -> [B][heads][L][d]"""
    return m.reshape(B, L, heads, d).transpose(0, 2, 1, 3)


def _rows(x, B, L, heads, d):
    """[B][heads][L][d] -> [B*L][heads*d]"""
    return x.transpose(0, 2, 1, 3).reshape(B * L, heads * d)


def _qkv(qkv, ld, B, L, C, heads, dt):
    x = Mat(qkv, B * L, 3 * C, ld, dt).get().astype(np.float64)
    d = C // heads
    return tuple(_heads(x[:, i * C:(i + 1) * C], B, L, heads, d) for i in range(3))


def ddpm_attention_mh_fwd(qkv, ld, out, out_ld, lse, B, L, C, heads, scale, dt, st):
    assert qkv and out and heads >= 1 and C % heads == 0 and (C // heads) % 32 == 0 and C // heads <= 512 and B * heads <= 65535 and dt == 1
    d = C // heads
    q, k, v = _qkv(qkv, ld, B, L, C, heads, dt)
    s = np.einsum("bhic,bhjc->bhij", q, k) * scale
    m = s.max(-1, keepdims=True)
    e = np.exp(s - m)
    if lse:
        f32(lse, B * heads * L)[...] = (m[..., 0] + np.log(e.sum(-1))).reshape(-1)              # [B][heads][L]
    o = np.einsum("bhij,bhjc->bhic", e / e.sum(-1, keepdims=True), v)
    Mat(out, B * L, C, out_ld, dt).set(_rows(o, B, L, heads, d).astype(np.float32))


def ddpm_attention_mh_bwd(qkv, ld, o, o_ld, d_o, do_ld, lse, dvec, dqkv, dqkv_ld, B, L, C, heads, scale, dt, st):
    assert qkv and o and d_o and lse and dvec and dqkv and heads >= 1 and C % heads == 0 and (C // heads) % 32 == 0 and dt == 1
    d = C // heads
    q, k, v = _qkv(qkv, ld, B, L, C, heads, dt)
    O = _heads(Mat(o, B * L, C, o_ld, dt).get().astype(np.float64), B, L, heads, d)
    dO = _heads(Mat(d_o, B * L, C, do_ld, dt).get().astype(np.float64), B, L, heads, d)
    p = np.exp(np.einsum("bhic,bhjc->bhij", q, k) * scale - f32(lse, B * heads * L).reshape(B, heads, L, 1))
    D = (dO * O).sum(-1)
    f32(dvec, B * heads * L)[...] = D.reshape(-1)
    ds = p * (np.einsum("bhic,bhjc->bhij", dO, v) - D[..., None]) * scale
    g = np.concatenate([_rows(np.einsum("bhij,bhjc->bhic", ds, k), B, L, heads, d), _rows(np.einsum("bhij,bhic->bhjc", ds, q), B, L, heads, d),
                        _rows(np.einsum("bhij,bhic->bhjc", p, dO), B, L, heads, d)], -1)
    Mat(dqkv, B * L, 3 * C, dqkv_ld, dt).set(g.astype(np.float32))


def ddpm_attention_stream_fwd(qkv, ld, out, out_ld, lse, B, L, C, scale, dt, st):
    """The single-head streaming forward: the heads = 1 case (the parameter list is the one above without ``heads``)."""
    ddpm_attention_mh_fwd(qkv, ld, out, out_ld, lse, B, L, C, 1, scale, dt, st)


def ddpm_attention_stream_bwd(qkv, ld, o, o_ld, d_o, do_ld, lse, dvec, dqkv, dqkv_ld, B, L, C, scale, dt, st):
    ddpm_attention_mh_bwd(qkv, ld, o, o_ld, d_o, do_ld, lse, dvec, dqkv, dqkv_ld, B, L, C, 1, scale, dt, st)


def attach(emu):
    """Add the entry points to an ``abi_emulator.Emulator`` instance (its ``call`` is ``getattr(self, name)``)."""
    for fn in (ddpm_attention_mh_fwd, ddpm_attention_mh_bwd, ddpm_attention_stream_fwd, ddpm_attention_stream_bwd):
        setattr(emu, fn.__name__, fn)
    return emu
