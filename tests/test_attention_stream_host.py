"""CPU: the streaming attention pair is exported, and its host-side validation returns the contract's status codes before anything is
launched.  Every call here is one that is REJECTED: an accepted call would launch a kernel on these fake addresses wherever a GPU is
present (tests/test_abi_surface.py explains the same rule for the conv entry point)."""
import ctypes
import os

import pytest

from ddpm_torch import _hip

pytestmark = pytest.mark.skipif(not os.path.exists(_hip.LIB_PATH), reason="libddpm_hip.so not built")

OK, SHAPE, DTYPE, ALIGN, LAUNCH, NULL = 0, 1, 2, 3, 4, 5
FAKE = 0x10000                                  # 16-byte aligned, never dereferenced: validation is on the host
BF16, F32 = 1, 0
BUF_OOB = 0x7FFFFFF0


def test_library_exports_the_streaming_pair():
    handle = ctypes.CDLL(_hip.LIB_PATH)
    for name, nargs in (("ddpm_attention_stream_fwd", 11), ("ddpm_attention_stream_bwd", 16)):
        assert hasattr(handle, name), name
        assert len(_hip.PROTOTYPES[name]) == nargs
    # the parameter lists are those of the L <= 256 pair: the dispatch is a change of name
    assert _hip.PROTOTYPES["ddpm_attention_stream_fwd"] == _hip.PROTOTYPES["ddpm_attention_fwd_lse"]
    assert _hip.PROTOTYPES["ddpm_attention_stream_bwd"] == _hip.PROTOTYPES["ddpm_attention_bwd"]
    lib = _hip.lib()
    assert lib.ddpm_plan_entry_arity(b"ddpm_attention_stream_fwd") == 11 and lib.ddpm_plan_entry_arity(b"ddpm_attention_stream_bwd") == 16


def fwd(qkv=FAKE, ld=3 * 64, out=FAKE, out_ld=64, lse=0, B=2, L=100, C=64, dtype=BF16):
    return _hip.lib().ddpm_attention_stream_fwd(qkv, ld, out, out_ld, lse, B, L, C, C ** -0.5, dtype, 0)


def bwd(qkv=FAKE, ld=3 * 64, o=FAKE, o_ld=64, d_o=FAKE, do_ld=64, lse=FAKE, dvec=FAKE, dqkv=FAKE, dqkv_ld=3 * 64, B=2, L=100, C=64, dtype=BF16):
    return _hip.lib().ddpm_attention_stream_bwd(qkv, ld, o, o_ld, d_o, do_ld, lse, dvec, dqkv, dqkv_ld, B, L, C, C ** -0.5, dtype, 0)


def test_forward_validation_returns_status_codes_without_launching():
    assert fwd(qkv=0) == NULL and fwd(out=0) == NULL
    assert fwd(dtype=F32) == DTYPE
    assert fwd(C=48, ld=3 * 48) == SHAPE                  # C % 32
    assert fwd(C=544, ld=3 * 544, out_ld=544) == SHAPE    # C > 512
    assert fwd(ld=3 * 64 - 8) == SHAPE                    # ld < 3C
    assert fwd(ld=3 * 64 + 4) == ALIGN                    # pitch not a 16-byte multiple
    assert fwd(out_ld=64 + 4) == ALIGN
    assert fwd(qkv=FAKE + 2) == ALIGN and fwd(out=FAKE + 8) == ALIGN
    assert fwd(L=0) == SHAPE and fwd(B=0) == SHAPE
    # L * ld * 2 bytes must stay within the buffer descriptors' range: the first L beyond it is refused
    L_over = BUF_OOB // (3 * 64 * 2) + 1
    assert L_over * 3 * 64 * 2 > BUF_OOB and fwd(L=L_over) == SHAPE


def test_backward_validation_returns_status_codes_without_launching():
    for name in ("qkv", "o", "d_o", "lse", "dvec", "dqkv"):
        assert bwd(**{name: 0}) == NULL, name
    assert bwd(dtype=F32) == DTYPE
    assert bwd(C=48, ld=3 * 48, dqkv_ld=3 * 48) == SHAPE
    assert bwd(C=544, ld=3 * 544, o_ld=544, do_ld=544, dqkv_ld=3 * 544) == SHAPE
    assert bwd(ld=3 * 64 - 8) == SHAPE
    assert bwd(ld=3 * 64 + 4) == ALIGN
    for name in ("o_ld", "do_ld"):
        assert bwd(**{name: 64 + 4}) == ALIGN, name
    assert bwd(dqkv_ld=3 * 64 + 4) == ALIGN and bwd(dqkv_ld=3 * 64 - 8) == ALIGN      # as ddpm_attention_bwd reports a short gradient pitch
    for name in ("qkv", "o", "d_o", "dqkv"):
        assert bwd(**{name: FAKE + 2}) == ALIGN, name
    assert bwd(L=0) == SHAPE
    assert bwd(L=BUF_OOB // (3 * 64 * 2) + 1) == SHAPE


def test_the_short_pair_keeps_its_rejections():
    """The existing entry points still refuse what they refused: more than 256 tokens and token counts that are no multiple of 16."""
    f = _hip.lib().ddpm_attention_fwd_lse
    assert f(FAKE, 192, FAKE, 64, 0, 1, 512, 64, 0.125, BF16, 0) == SHAPE
    assert f(FAKE, 192, FAKE, 64, 0, 1, 24, 64, 0.125, BF16, 0) == SHAPE
