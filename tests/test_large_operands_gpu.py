"""-m gpu: the kernels behind a BUF_OOB guard at the top of the range the guard admits, and the refusal one step beyond it.

Every GEMM-shaped kernel addresses its operands through buffer descriptors with 32-bit byte offsets, and its launcher refuses an
operand whose extent exceeds BUF_OOB = 0x7ffffff0 bytes.  The largest operand any other test replays is W13's 1.5 GiB: byte offsets
between 0x60000000 and the limit were never formed on the GPU, and the refusal was tested on made-up pointers only.  Here every row of
launch_replay.LARGE_OPERANDS — a signature whose largest guarded operand ends within one image (or one row) of BUF_OOB, dense (natural
pitch, 16.8 M pixels) or stretched (few pixels, the pitch raised until the last row ends at the limit) — is replayed on fresh random
inputs against the float64 restatement of include/ddpm_hip.h, every output element held to its own error-model bar (err/bar <= 1, the
bars tests/launch_replay.py defines), after the dispatch query has named the kernel the table expects.  The neighbour of every row,
one image or one pitch step larger, must come back DDPM_ERR_SHAPE from the dry dispatch query and from the launching entry (which
returns before any launch; an admitted size is never put through it).  The one exception is written into the table: the
few-input-channel edge conv reads x through 64-bit pointers behind no guard, so its neighbour is admitted and names the same kernel.

The weight-gradient rows multiply dy by 16 on three images (the first, the last, the one whose bytes straddle offset 2^30): a sum over
16.8 M pixels would otherwise hide a lost image within a few bars.  The test asserts on the float64 reference alone that dropping any
one of the three moves at least half of the output elements by more than 8 bars.

Rows run one at a time; a row's arena is released before the next row, its peak device memory is printed and must stay below 48 GiB.
A family skips only when, before its first row, the device reports less free memory than that ceiling.

The family "across" is launch_replay.ACROSS_2_31: the unguarded entries whose indexing is 64-bit (ddpm_add_rows, ddpm_colsum,
ddpm_upsample2x_bwd, ddpm_nchw_to_nhwc; the table quotes the lines) on a bf16 operand of just over 2^31 elements.

Measured on the MI355X (profiles/large_operands.log has one line per row: signature, variant, largest extent in bytes, distance to
BUF_OOB, worst err/bar and where, seconds, peak GiB); worst err/bar, slowest row and highest peak per family:
  conv       15 rows  0.341 (fp32 tile GEMM into NCHW; every bf16 row 0.249 = the store)   1.9 s   34.1 GiB (dense 1x1 with residual)
  wgrad      10 rows  0.159 (_up_, x stretched)   1.7 s (dense 3x3, 16.8 M pixels; 5.2 s in a cold process)   17.8 GiB   3-image sensitivity >= 0.94
  gemm        3 rows  0.249   1.6 s   24.2 GiB          attention  13 rows  0.392 (mh backward dq)   2.8 s   24.2 GiB
  across      5 rows  0.996 (nchw_to_nhwc: the bf16 rounding itself, its bar is u |x|)   2.2 s (6.2 s cold)   28.6 GiB
  W13's record + replay on the same machine: 10.5 s.  No row skipped.  (46 + 5 rows.)
What the rows found when they first ran: no kernel gave a wrong result — all 43 rows of the first table passed on their first run, at extents 112 .. 131 056 bytes
below the limit, and every neighbour was refused with status 1 before a launch.  Two things about the contract came out of writing
them: the few-input-channel edge conv (kernel 12) has no extent guard and needs none (64-bit pointers), so a conv of that form is
admitted at any size; and the specialised conv launchers answer an oversized x with "not covered", the refusal itself comes from
finish_desc of the generic path.  The float64 weight-gradient reference took 32 s on the dense row as one [N x P] x [P x C] matmul per tap
(one output tile); launch_replay.wgrad_fp64 now adds up batched partial products over runs of 1024 pixels (5.2 s).
Read, not run: the GroupNorm entries.  Their LDS-staged forms keep 32-bit byte offsets inside one sample's slice and draw the dropout
index in `unsigned`; the launchers now take those forms only when the slice ends within BUF_OOB and the tensor holds fewer than 2^32
elements (gn_lds_addressable — the 256-thread form used to skip the element-count condition), and refuse any operand of 2^31 elements or
more with status 1 (gn_operand_ok; tests/test_large_operands_host.py tests the refusal).  ddpm_attention_bwd read d_o through a
descriptor behind no extent check: the launcher now refuses L * do_ld * 2 > BUF_OOB, and the table has top-of-range rows with do_ld
stretched.  A dense ddpm_upsample2x_bwd input of more than 2^31 elements is not run (the row stretches dx).
"""
import time

import pytest
import torch

from tests import launch_replay as LR
from tests.test_unet_gpu import DEV

pytestmark = pytest.mark.gpu

PEAK_LIMIT = 48 << 30
FAMILIES = {
    "conv": ("ddpm_conv2d_nhwc",),
    "wgrad": ("ddpm_conv3x3_wgrad_nhwc", "ddpm_conv3x3_wgrad_up_nhwc", "ddpm_conv2d_wgrad_nhwc", "ddpm_conv1x1_wgrad_nhwc"),
    "gemm": ("ddpm_gemm",),
    "attention": ("ddpm_attention_fwd", "ddpm_attention_fwd_lse", "ddpm_attention_bwd", "ddpm_attention_mh_fwd", "ddpm_attention_mh_bwd"),
}
# entries whose dry dispatch query sees the pitches (ddpm_conv3x3_wgrad_variant takes none, the 1x1 weight gradient has no query)
PITCH_AWARE_QUERY = ("ddpm_conv2d_nhwc", "ddpm_conv2d_wgrad_nhwc", "ddpm_gemm")


def test_every_large_operand_row_belongs_to_a_family():
    names = {n for fam in FAMILIES.values() for n in fam}
    assert {r[0][0] for r in LR.LARGE_OPERANDS} == names


def test_every_neighbour_is_refused_before_any_launch():
    """No launch: the dry dispatch query where the entry has one, and the launching entry on the refused size."""
    for sig, _, neighbour, expect, _ in LR.LARGE_OPERANDS:
        assert LR.largest_extent(neighbour)[1] > LR.BUF_OOB, LR.short(neighbour)
        dry = LR.variant_of(neighbour)
        if expect == "refused":
            if sig[0] in PITCH_AWARE_QUERY:
                assert dry == -LR.ERR_SHAPE, (LR.short(neighbour), dry)
            assert LR.refusal_status(neighbour) == LR.ERR_SHAPE, LR.short(neighbour)
        else:
            assert dry == expect, (LR.short(neighbour), dry)


def _rows(family):
    """(seed, signature, variant, amplification, operand, extent) of the family's rows of both tables"""
    for i, (sig, variant, _, _, amp) in enumerate(LR.LARGE_OPERANDS):
        if sig[0] in FAMILIES.get(family, ()):
            yield (i, sig, variant, amp) + LR.largest_extent(sig, amp and amp[1])[:2]
    if family == "across":
        for i, (sig, amp) in enumerate(LR.ACROSS_2_31):
            yield 1000 + i, sig, None, amp, "", 0


@pytest.mark.parametrize("family", list(FAMILIES) + ["across"])
def test_large_operand_rows_match_float64(family):
    """family "across": launch_replay.ACROSS_2_31, the unguarded 64-bit entries on an operand of more than 2^31 elements."""
    bad, lines = [], []
    torch.cuda.empty_cache()
    free = torch.cuda.mem_get_info()[0]
    if free < PEAK_LIMIT:                   # decided once, before the family's first row: no row's result is ever discarded
        pytest.skip(f"{family}: the device reports {free / 2 ** 30:.1f} GiB free, a row may use up to {PEAK_LIMIT >> 30} GiB")
    for i, sig, variant, amp, operand, extent in _rows(family):
        got = LR.variant_of(sig)
        assert variant is None or got == variant, f"{LR.short(sig)}: dispatched to {got}, the table names {variant}"
        torch.cuda.reset_peak_memory_stats()
        t0 = time.perf_counter()
        r = LR.replay(sig, DEV, seed=i, amplify=amp, keep_outputs=False)
        torch.cuda.synchronize()
        secs = time.perf_counter() - t0
        peak = torch.cuda.max_memory_allocated()
        sens = min(r.sensitivity.values()) if r.sensitivity else None
        if family == "across":
            operand, extent = "", r.max_bytes
            assert extent > 1 << 32, f"{LR.short(sig)}: the largest operand has {extent} bytes, not more than 2^32"
        del r.outputs, r.tensors
        torch.cuda.empty_cache()
        lines.append(f"  {LR.short(sig):<140s} v{'-' if variant is None else variant:<3} {operand:<4s} {extent:>10d} B  gap {LR.BUF_OOB - extent:>7d}  "
                     f"{r.where:<8s} err/bar {r.worst:.3f}  {secs:5.1f} s  peak {peak / 2 ** 30:5.1f} GiB"
                     + ("" if sens is None else f"  3-image sensitivity {sens:.2f}"))
        if r.worst > 1.0:
            bad.append(f"{LR.short(sig)}: {r.where} err/bar {r.worst:.3g}")
        if peak >= PEAK_LIMIT:
            bad.append(f"{LR.short(sig)}: peak device memory {peak / 2 ** 30:.1f} GiB")
        if amp is not None:
            assert r.sensitivity, LR.short(sig)
            if sens < 0.5:
                bad.append(f"{LR.short(sig)}: dropping one amplified image moves only {sens:.2f} of the outputs by more than 8 bars: {r.sensitivity}")
    assert lines
    print(f"\n== large operands, {family}: {len(lines)} rows")
    print("\n".join(lines))
    assert not bad, f"{family}: {len(bad)} finding(s):\n" + "\n".join(bad)


@pytest.mark.parametrize("name,size", [("celebahq.json", 256), ("celeba.json", 64)])
def test_engine_plan_is_admitted_at_max_batch_and_refused_beyond(monkeypatch, name, size):
    """No launch: the signatures of a training forward + backward at max_batch and max_batch + 1 are recorded with every C-ABI call
    dropped, and put to the launchers' extent arithmetic and the dry dispatch queries (tests/test_large_operands_host.py has the body;
    here it runs against the library of the GPU machine)."""
    from tests.test_large_operands_host import test_plan_matches_the_signatures_the_engine_emits as check
    check(monkeypatch, name, size)
