"""-m gpu: the streaming attention pair (ddpm_attention_stream_fwd / ddpm_attention_stream_bwd, csrc/attention_stream.hip) at the
kernel level, against a float64 torch restatement of its contract computed from the bf16-rounded inputs (the ABI emulator has no entry
for the two names).

Measure and bars are those the L <= 256 pair is held to in tests/test_kernels_gpu.py: max abs error over the reference's max abs, per
output tensor; 1.2e-2 for O and lse, 2e-2 for D and the packed dq | dk | dv.  Operands are allocated with their pitch padding and
guard rows filled with bf16 NaN, outputs with a sentinel: a kernel that reads outside [B][L][C] shows as a non-finite result, one that
writes outside it as a changed sentinel."""
import math

import pytest
import torch

from ddpm_torch import _hip

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL_FWD, TOL_BWD = 1.2e-2, 2e-2
GUARD = 8                                       # rows of NaN / sentinel before and after every tensor
SENT_BF16 = 0x5A5A                              # bit pattern the bf16 outputs are pre-filled with (a finite number)
SENT_F32 = 12345.678

CASES = [(2, 1, 32), (2, 7, 64), (3, 30, 128), (2, 60, 128), (2, 100, 64), (1, 196, 256), (2, 256, 256), (2, 257, 64), (2, 300, 128),
         (1, 520, 512), (1, 1000, 96), (2, 1024, 64), (1, 1024, 256), (1, 4096, 64),
         # one past the streamed tile (32 tokens at C > 128, 64 below) and one past the row block (64 at C > 256, 128 below)
         (2, 33, 256), (2, 65, 128), (2, 129, 128), (1, 65, 512), (2, 40, 288)]


def _operand(payload, pitch):
    """[R][W] bf16 -> device buffer [GUARD + R + GUARD][pitch], NaN everywhere but the payload; returns (buffer, pointer to row 0)."""
    R, W = payload.shape
    buf = torch.full((R + 2 * GUARD, pitch), float("nan"), dtype=torch.bfloat16, device=DEV)
    buf[GUARD:GUARD + R, :W] = payload.to(DEV)
    return buf, buf[GUARD:].data_ptr()


def _out_bf16(R, pitch):
    buf = torch.full((R + 2 * GUARD, pitch), SENT_BF16, dtype=torch.int16, device=DEV)
    return buf, buf[GUARD:].data_ptr()


def _out_f32(R):
    buf = torch.full((R + 2 * GUARD,), SENT_F32, dtype=torch.float32, device=DEV)
    return buf, buf[GUARD:].data_ptr()


def _payload_bf16(buf, R, W, what):
    """The [R][W] result of a sentinel-filled bf16 output; asserts that it is finite and that nothing else was written."""
    got = buf[GUARD:GUARD + R, :W].contiguous().view(torch.bfloat16).double()
    assert torch.isfinite(got).all(), f"{what}: not finite"
    rest = buf.clone()
    rest[GUARD:GUARD + R, :W] = SENT_BF16
    assert bool((rest == SENT_BF16).all()), f"{what}: bytes outside [B][L][C] were written"
    return got


def _payload_f32(buf, R, what):
    got = buf[GUARD:GUARD + R].double()
    assert torch.isfinite(got).all(), f"{what}: not finite"
    assert bool((buf[:GUARD] == SENT_F32).all()) and bool((buf[GUARD + R:] == SENT_F32).all()), f"{what}: guard rows were written"
    return got


def _rel(got, ref):
    return float((got - ref).abs().max()) / (float(ref.abs().max()) or 1.0)


def reference_fwd(qkv, B, L, C, scale):
    """float64 on the bf16-rounded inputs: O [B*L][C], lse [B*L]."""
    x = qkv.to(DEV).double().reshape(B, L, 3 * C)
    q, k, v = x[..., :C], x[..., C:2 * C], x[..., 2 * C:]
    s = torch.einsum("bic,bjc->bij", q, k) * scale
    lse = torch.logsumexp(s, dim=-1)
    o = torch.einsum("bij,bjc->bic", torch.exp(s - lse[..., None]), v)
    return o.reshape(B * L, C), lse.reshape(B * L)


def reference_bwd(qkv, o, d_o, lse, B, L, C, scale):
    """float64 restatement of the backward's contract: P rebuilt from q, k and the GIVEN lse, D from the GIVEN o."""
    x = qkv.to(DEV).double().reshape(B, L, 3 * C)
    q, k, v = x[..., :C], x[..., C:2 * C], x[..., 2 * C:]
    o, d_o, lse = o.double().reshape(B, L, C), d_o.to(DEV).double().reshape(B, L, C), lse.double().reshape(B, L)
    p = torch.exp(torch.einsum("bic,bjc->bij", q, k) * scale - lse[..., None])
    D = (d_o * o).sum(-1)
    ds = p * (torch.einsum("bic,bjc->bij", d_o, v) - D[..., None])
    dq = torch.einsum("bij,bjc->bic", ds, k) * scale
    dk = torch.einsum("bij,bic->bjc", ds, q) * scale
    dv = torch.einsum("bij,bic->bjc", p, d_o)
    return D.reshape(B * L), torch.cat([dq, dk, dv], dim=-1).reshape(B * L, 3 * C)


def run_pair(qkv, d_o, B, L, C, fwd="ddpm_attention_stream_fwd", bwd="ddpm_attention_stream_bwd", tag="", nonzero=True):
    """Both kernels on pitched, NaN-padded operands.  Returns the measured errors against float64 and the raw results."""
    ld, old, gld = 3 * C + 16, C + 8, 3 * C + 24
    scale = 1.0 / math.sqrt(C)
    R = B * L
    st = _hip.stream()
    qb, qp = _operand(qkv, ld)
    ob, op = _out_bf16(R, old)
    lb, lp = _out_f32(R)
    _hip.call(fwd, qp, ld, op, old, lp, B, L, C, scale, 1, st)
    ob2, op2 = _out_bf16(R, old)
    _hip.call(fwd, qp, ld, op2, old, 0, B, L, C, scale, 1, st)
    torch.cuda.synchronize()
    o = _payload_bf16(ob, R, C, tag + " O")
    lse = _payload_f32(lb, R, tag + " lse")
    _payload_bf16(ob2, R, C, tag + " O (lse = NULL)")
    assert torch.equal(ob, ob2), tag + ": O differs between lse and lse = NULL"
    o_ref, lse_ref = reference_fwd(qkv, B, L, C, scale)
    errs = {"O": _rel(o, o_ref), "lse": _rel(lse, lse_ref)}
    # backward on the kernel's own saved o and lse, as the engine calls it: o and d_o NaN-padded operands too
    o_in, oip = _operand(ob[GUARD:GUARD + R, :C].contiguous().view(torch.bfloat16), old)
    db, dp = _operand(d_o, old)
    outs = []
    for _ in range(2):
        vb, vp = _out_f32(R)
        gb, gp = _out_bf16(R, gld)
        _hip.call(bwd, qp, ld, oip, old, dp, old, lp, vp, gp, gld, B, L, C, scale, 1, st)
        outs.append((vb, gb))
    torch.cuda.synchronize()
    (vb, gb), (vb2, gb2) = outs
    D = _payload_f32(vb, R, tag + " D")
    g = _payload_bf16(gb, R, 3 * C, tag + " dqkv")
    assert torch.equal(vb, vb2) and torch.equal(gb, gb2), tag + ": the backward is not bit-identical when repeated"
    D_ref, g_ref = reference_bwd(qkv, o, d_o, lse, B, L, C, scale)
    errs["D"], errs["dqkv"] = _rel(D, D_ref), _rel(g, g_ref)
    for nm, sl in (("dq", g[:, :C]), ("dk", g[:, C:2 * C]), ("dv", g[:, 2 * C:])):
        if nonzero and (L > 1 or nm == "dv"):
            assert float(sl.abs().max()) > 0, (tag, nm)
    del qb, o_in, db
    return errs, o, lse


def _inputs(B, L, C, peak):
    gen = torch.Generator().manual_seed(21)
    qkv = torch.randn(B * L, 3 * C, generator=gen) * 1.2
    qkv[:, :C] *= peak
    d_o = torch.randn(B * L, C, generator=torch.Generator().manual_seed(22))
    return qkv.to(torch.bfloat16), d_o.to(torch.bfloat16)


def _hold(errs, tag):
    print(f"{tag}: " + "  ".join(f"{k} {v:.3e}" for k, v in errs.items()))
    assert errs["O"] <= TOL_FWD and errs["lse"] <= TOL_FWD, (tag, errs)
    assert errs["D"] <= TOL_BWD and errs["dqkv"] <= TOL_BWD, (tag, errs)


@pytest.mark.parametrize("B,L,C", CASES)
def test_streaming_pair_against_float64(B, L, C):
    """Forward (with and without lse, O bit-identical), backward run twice (bit-identical): O, lse, D and dq | dk | dv against float64;
    NaN-filled padding and guard rows around every operand, sentinels around every output."""
    for peak in (1.0, 5.0):
        qkv, d_o = _inputs(B, L, C, peak)
        errs, _, _ = run_pair(qkv, d_o, B, L, C, tag=f"stream B{B} L{L} C{C} x{peak:g}")
        _hold(errs, f"stream B{B} L{L} C{C} x{peak:g}")
        if (B, L, C) == (2, 256, 256):
            old, _, _ = run_pair(qkv, d_o, B, L, C, fwd="ddpm_attention_fwd_lse", bwd="ddpm_attention_bwd", tag="flash")
            print(f"flash  B{B} L{L} C{C} x{peak:g}: " + "  ".join(f"{k} {v:.3e}" for k, v in old.items()))


def _planted(L, C, logits, qv=0.5):
    """qkv [L][3C] whose scaled logits s_ij = logits[j] for every query i: q = the constant qv, k_j = a multiple of the all-ones direction."""
    scale = 1.0 / math.sqrt(C)
    q = torch.full((L, C), qv)
    k = (logits / (scale * qv * C))[:, None].expand(L, C)
    v = torch.randn(L, C, generator=torch.Generator().manual_seed(5))
    return torch.cat([q, k, v], dim=1).to(torch.bfloat16)


def test_identical_keys_give_the_mean_of_v():
    """Every key the same: P is uniform whatever the tiling, O = mean of V (within the bf16 rounding of O) and lse = s + log L."""
    L, C = 300, 128
    scale = 1.0 / math.sqrt(C)
    gen = torch.Generator().manual_seed(3)
    q, key, v = torch.randn(L, C, generator=gen), torch.randn(1, C, generator=gen), torch.randn(L, C, generator=gen)
    qkv = torch.cat([q, key.expand(L, C), v], dim=1).to(torch.bfloat16)
    d_o = torch.randn(L, C, generator=gen).to(torch.bfloat16)
    errs, o, lse = run_pair(qkv, d_o, 1, L, C, tag="identical keys", nonzero=False)
    _hold(errs, "identical keys")
    x = qkv.to(DEV).double()
    mean_v = x[:, 2 * C:].mean(0, keepdim=True).expand(L, C)
    s = (x[:, :C] * x[:1, C:2 * C]).sum(-1) * scale
    # O is stored as bf16: half an ulp (2^-9 relative) of each element, plus the fp32 accumulation of 300 bf16 probabilities
    assert float((o - mean_v).abs().max()) <= 2.0 ** -8 * float(mean_v.abs().max()) + 1e-3 * float(x[:, 2 * C:].abs().max())
    assert float((lse - (s + math.log(L))).abs().max()) <= 1e-4 * float(s.abs().max() + math.log(L))


@pytest.mark.parametrize("kind", ["rising", "falling", "large_negative"])
def test_planted_logits(kind):
    """Logits that rise with the key index across every tile (the running max moves in each tile), the same reversed (the max sits
    in the first tile), and all logits equal to a large negative constant (nothing may depend on exp of an unshifted logit)."""
    L, C = 300, 64
    ramp = torch.linspace(-30.0, 30.0, L)
    logits = {"rising": ramp, "falling": ramp.flip(0), "large_negative": torch.full((L,), -3000.0)}[kind]
    # (the constant -3000 is split evenly between q = 16 and k ~ -23: dq = scale * sum_j dS_ij k_j carries the bf16 rounding of dS times
    #  |k| * scale, and a constant built from q = 0.5, k = -750 would put 94 x that rounding — a property of the operands, which any
    #  kernel that hands dS to the matrix unit as bf16 shares — against a dv of ordinary size in the same packed tensor)
    qkv = _planted(L, C, logits, qv=16.0 if kind == "large_negative" else 0.5)
    d_o = torch.randn(L, C, generator=torch.Generator().manual_seed(6)).to(torch.bfloat16)
    errs, o, lse = run_pair(qkv, d_o, 1, L, C, tag=kind, nonzero=False)
    _hold(errs, kind)
    if kind == "large_negative":
        x = qkv.to(DEV).double()
        s = float((x[0, :C] * x[0, C:2 * C]).sum() / math.sqrt(C))
        assert s < -2000.0
        assert float((lse - (s + math.log(L))).abs().max()) <= 1e-4 * abs(s)
        mean_v = x[:, 2 * C:].mean(0, keepdim=True).expand(L, C)
        assert float((o - mean_v).abs().max()) <= 2.0 ** -8 * float(mean_v.abs().max()) + 1e-3 * float(x[:, 2 * C:].abs().max())
