"""-m gpu: every launch of the benchmarked steps, and of the fp32 mode and the CLIs' other batch sizes, replayed on the MI355X against a
float64 reference at the geometry the step uses.

The workloads (tests/launch_replay.py WORKLOADS: W1-W4 the benchmarked bf16 steps, W5-W8 the same configurations in the fp32 compute
mode, W9-W13 bf16 steps at the batch sizes train.py --num-accum and generate.py run, up to operands >= 1 GiB, W14-W17 a reduced network
on non-square 16 x 48, 48 x 16 and 24 x 20 images, W18-W24 the reduced network with 1, 4 and 12 image channels — what --dataset mnist
and train.py --block-size 2 build — in both compute modes) are recorded live through
ddpm_torch._hip._invoke — the geometry list is taken from the step every time the test runs, not from a committed snapshot.  Each
distinct signature of a replayed entry is (dropout seeds aside) re-issued once on fresh random inputs (same pitches, pointer offsets
modulo 256, optional operands, modes, splits and workspaces) and every output element is held to its own error-model bar; the float64
references run in torch on the GPU, over every image (in slices of images where one pass would need tens of GB).
Every recorded entry must be either replayed or mapped to the existing test that covers it (launch_replay.COVERED_ELSEWHERE).

The optimizer tail of a training step — ddpm_wgrad_unpack_sumsq, ddpm_mt_adam_ema, ddpm_pack_weight_multi, ddpm_mt_gather_f32 — is
replayed with the rest on the geometry of the tables the step built (W1: the CIFAR trainer's 304 rows), and at the end of this module
on hand-written tables (launch_replay.TAIL), planted sums of squares, bit identities and a three-step chain on the real tables.
Measured on the MI355X, worst |got - ref| / bar per entry over the hand-written rows, the hostile modes and W1 / W14 / W15:
  ddpm_mt_adam_ema       0.125 (shadow; the yardstick — the same update as a plain fp32 torch composition — 0.125: the final store)
  ddpm_adam_ema_step     0.125 (yardstick 0.125)
  ddpm_mt_grad_sumsq     0.044 of d u sum g^2 (d = 24 .. 166)      ddpm_sumsq_accumulate    0.055
  ddpm_wgrad_unpack      bit-exact at scale 1, 0.5, 0.125, 1/3     ddpm_wgrad_unpack_sumsq  gflat bit-exact, norm 0.023 (d = 39 .. 110)
  ddpm_pack_weight_multi bit-exact; the 4 x 4 kernels of the Upsample convs 0.249 (bf16) / 0.304 (fp32) of their rounding bar
  ddpm_mt_gather_f32     bit-exact                                 chained tail: 0.296 (fp32), 0.249 (bf16), both the 4 x 4 kernels
Every planted sum exact, every identity bit for bit, every second launch bit-equal to the first.  W1's update replays in 0.61 s (1216
guarded buffers; its float64 reference already runs in two passes, ADAM_CHUNK), the slowest other replay of W1 in 0.30 s."""
import collections
import time

import pytest
import torch

from ddpm_torch import _hip
from tests import launch_replay as LR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# kernels the benchmark line is made of (include/ddpm_hip_debug.h): 13 conv3x3_pc, 10 / 8 conv3x3_stream<8> / <16>, 7 pw_conv,
# 4 gemm64, 11 / 12 edge convs, 14 wgrad3x3_ws, 6 wgrad3x3 (patch-stationary)
W1_VARIANTS = {13, 10, 8, 7, 4, 11, 12, 14, 6}
FP32 = ("W5", "W6", "W7", "W8", "W19", "W21", "W23")
# recorded launches of the fp32 workloads that may pass a dtype other than fp32 (none: every operand of the fp32 mode is fp32)
FP32_DTYPE_EXEMPT = {}


def _table(key, rows):
    print(f"\n== {key}: {LR.WORKLOADS[key][0]} — {len(rows)} replayed signatures")
    for sig, var, r in rows:
        print(f"  {LR.short(sig):<150s} v{'' if var is None else var:<3} {r.where:<10s} err/bar {r.worst:.3f}")


def _check_fp32_mode(key, rec, variants):
    for s in rec.sigs:
        i = LR.dtype_index(s[0])
        if i is not None and s[0] not in FP32_DTYPE_EXEMPT:
            assert s[1][i] == LR.F32, f"{key}: fp32 mode launched {LR.short(s)} with dtype {s[1][i]}"
    bf16_only = sorted(set(variants) & LR.BF16_ONLY)
    assert not bf16_only, f"{key}: fp32 signatures dispatched to bf16-only kernels {bf16_only}"
    assert "ddpm_softmax_fwd" in rec.names, f"{key}: fp32 attention ran no ddpm_softmax_fwd"
    if key in ("W5", "W7", "W19", "W21", "W23"):
        assert "ddpm_softmax_bwd" in rec.names, f"{key}: fp32 attention backward ran no ddpm_softmax_bwd"


def _check_w9(rec):
    """At B = 32 the pixel-count thresholds of the 3x3 dispatch fall at other levels than at B = 128."""
    moved = []
    for s in rec.sigs:
        w = s[1]
        if s[0] == "ddpm_conv2d_nhwc" and w[17] == 3 and w[18] == 3:
            at128 = LR.variant_of((s[0], w[:10] + (128,) + w[11:]))
            if at128 != LR.variant_of(s):
                moved.append((s, LR.variant_of(s), at128))
    for s, v, v128 in moved:
        print(f"W9: {LR.short(s)}  B=32 -> v{v}, B=128 -> v{v128}")
    assert moved, "W9: every 3x3 conv dispatches as it does at B = 128"


# kernels a non-square step must still reach: 13 / 10 conv3x3 in 1 x 3 patches of 16 x 16 and of 8 x 8, 14 wgrad3x3_ws, 11 / 12 edge convs
W14_VARIANTS = {13, 10, 14, 11, 12}


def _check_w14(rec, variants):
    """16 x 48 at B = 22 keeps the patch kernels (tiles_x = 3, tiles_y = 1) and the fused attention pair, at 8 x 24 = 192 tokens."""
    assert W14_VARIANTS <= set(variants), f"W14 did not reach variants {sorted(W14_VARIANTS - set(variants))}"
    for name in ("ddpm_attention_fwd_lse", "ddpm_attention_bwd"):
        at = sorted({s[1][-5:-2] for s in rec.sigs if s[0] == name})          # (B, L, C)
        print(f"W14: {name[5:]} at (B, L, C) = {at}")
        assert any(L == 192 for _, L, _ in at), f"W14: no {name} over 192 tokens"


def _check_w17(rec):
    """12 x 10 = 120 tokens: a multiple of 8 but not of 16, so the bf16 step runs gemm + softmax + gemm instead of the fused pair."""
    assert "ddpm_softmax_fwd" in rec.names and "ddpm_softmax_bwd" in rec.names, "W17: no ddpm_softmax_fwd / _bwd"
    assert "ddpm_attention_fwd_lse" not in rec.names and "ddpm_attention_bwd" not in rec.names
    sm = sorted({s[1][-3:] for s in rec.sigs if s[0] == "ddpm_softmax_fwd"})
    assert all(L == 120 and dt == LR.BF16 for _, L, dt in sm), sm


def _check_w12(rec):
    gn = [s for s in rec.sigs if s[0] == "ddpm_groupnorm_silu_bwd" and s[1][13] == 64 * 64]
    assert gn, "W12: no GroupNorm backward at HW = 4096"

    def pixels_3x3_wgrad(s):
        w = s[1]
        if s[0] in ("ddpm_conv3x3_wgrad_nhwc", "ddpm_conv3x3_wgrad_up_nhwc"):
            return w[8] * w[9] * w[10]
        if s[0] == "ddpm_conv2d_wgrad_nhwc" and w[15] == 3 and w[16] == 3:
            return w[6] * w[11] * w[12]
        return 0
    wg = [s for s in rec.sigs if pixels_3x3_wgrad(s) == 128 * 64 * 64]
    assert wg, "W12: no 3x3 weight gradient over B*64*64 pixels"
    print(f"W12: {len(gn)} GroupNorm backward signature(s) at HW = 4096, {len(wg)} 3x3 weight gradient(s) over 128*64*64 pixels")


# (in, out) channels of the edge-channel workloads, and the kernels their bf16 edge convs must reach: 11 few-output-channel kernel at
# N = 1, 4, 12; 12 few-input-channel kernel while the image fits one 8-lane vector (also out_conv's data gradient at Np = 8); at 12
# channels (16 lanes) in_conv and out_conv's data gradient are the tile GEMM 3.  6: out_conv's weight gradient (Nreal < N) on the patch
# kernel; 2: in_conv's (Creal < C) on the generic one.
EDGE_CHANNELS_OF = {"W18": (1, 1), "W19": (1, 1), "W20": (4, 4), "W21": (4, 4), "W22": (12, 12), "W23": (12, 12), "W24": (12, 12)}


def _check_edge_channels(key, rec, variants):
    cin, cout = EDGE_CHANNELS_OF[key]
    convs = [s for s in rec.sigs if s[0] == "ddpm_conv2d_nhwc" and s[1][17] == 3]
    staged = sorted({(s[1][3], s[1][5]) for s in rec.sigs if s[0] == "ddpm_nchw_to_nhwc"})               # (C, Cp) of every NCHW -> NHWC staging
    print(f"{key}: staged (C, Cp) {staged}; edge convs " + ", ".join(f"C{s[1][13]}->N{s[1][16]} mode {s[1][25]} v{LR.variant_of(s)}"
                                                                     for s in convs if s[1][13] <= 16 or s[1][16] <= 16))
    assert any(s[1][13] == -(-cin // (4 if key in FP32 else 8)) * (4 if key in FP32 else 8) and s[1][16] == 64 for s in convs), f"{key}: no in_conv"
    assert any(s[1][16] == cout and s[1][25] == 3 for s in convs), f"{key}: no out_conv into NCHW"
    if key in FP32:
        return
    want = {11, 12} if cin <= 8 else {11, 3}
    if key != "W24":
        want |= {6, 2}
    assert want <= set(variants), f"{key} did not reach variants {sorted(want - set(variants))}"


def _check_tail(key, rec, rows, took):
    """The table-driven launches of the optimizer tail: a training step must have replayed its update, its fused unpack, its weight
    packs and its time-bias gather on the geometry of the tables it built; W1's update is the CIFAR trainer's own table."""
    tail = [(s, r) for s, _, r in rows if s[0] in LR.TABLE_ARG]
    assert all(LR.is_table(s[1][LR.TABLE_ARG[s[0]][0]]) for s, _ in tail)
    names = {s[0] for s, _ in tail}
    if "ddpm_mt_adam_ema" in rec.names:
        assert {"ddpm_mt_adam_ema", "ddpm_wgrad_unpack_sumsq", "ddpm_pack_weight_multi", "ddpm_mt_gather_f32"} <= names, f"{key}: replayed of the tail only {sorted(names)}"
    for s, r in tail:
        n_rows = len(s[1][LR.TABLE_ARG[s[0]][0]][1])
        print(f"{key}: tail {s[0][5:]:<20s} {n_rows:4d} rows  {r.where:<14s} err/bar {r.worst:.3f}  replayed in {took[s]:.2f} s"
              + ("" if r.depth is None else f"  (chain length {r.depth})"))
    others = [t for s, t in took.items() if s[0] not in LR.TABLE_ARG]
    if tail and others:
        print(f"{key}: slowest tail replay {max(took[s] for s, _ in tail):.2f} s, slowest other replay {max(others):.2f} s")
    if key == "W1":
        adam = next(s for s, _ in tail if s[0] == "ddpm_mt_adam_ema")
        assert len(adam[1][0][1]) >= 300, f"W1: the update's table has {len(adam[1][0][1])} rows"


@pytest.mark.parametrize("key", list(LR.WORKLOADS))
def test_every_launch_of_the_step_matches_float64(key, monkeypatch):
    t0 = time.perf_counter()
    torch.cuda.reset_peak_memory_stats()
    rec = LR.record(monkeypatch, key, DEV)
    torch.cuda.empty_cache()
    unaccounted = sorted(set(rec.names) - set(LR.REPLAY) - set(LR.COVERED_ELSEWHERE))
    assert not unaccounted, f"{key}: recorded entries neither replayed nor mapped to a covering test: {unaccounted}"
    variants = collections.Counter()
    for s in rec.sigs:
        v = LR.variant_of(s)
        if v is not None:
            assert v > 0, f"{key}: dispatch query rejects the recorded {LR.short(s)} ({v})"
            variants[v] += 1
    print(f"\n{key}: entries {rec.names}\n{key}: dispatched variants {dict(sorted(variants.items()))}")
    if key == "W1":
        assert W1_VARIANTS <= set(variants), f"W1 did not reach variants {sorted(W1_VARIANTS - set(variants))}"
        assert any(s[0] == "ddpm_conv1x1_wgrad_nhwc" for s in rec.sigs), "W1 ran no 1x1 slab weight gradient"
    if key in FP32:
        _check_fp32_mode(key, rec, variants)
    if key == "W9":
        _check_w9(rec)
    if key == "W12":
        _check_w12(rec)
    if key == "W14":
        _check_w14(rec, variants)
    if key == "W17":
        _check_w17(rec)
    if key in LR.EDGE_CHANNEL_WORKLOADS:
        _check_edge_channels(key, rec, variants)
    rows, bad, seen, took = [], [], set(), {}
    for i, s in enumerate(rec.sigs):
        if s[0] not in LR.REPLAY or LR.geometry(s) in seen:
            continue
        seen.add(LR.geometry(s))
        t1 = time.perf_counter()
        r = LR.replay(s, DEV, seed=i)
        torch.cuda.empty_cache()
        took[s] = time.perf_counter() - t1
        rows.append((s, LR.variant_of(s), r))
        if r.worst > 1.0:
            bad.append(f"{LR.short(s)}: {r.where} err/bar {r.worst:.3g}")
    _table(key, rows)
    biggest = max(rows, key=lambda x: x[2].max_bytes)
    worst = max(rows, key=lambda x: x[2].worst)
    print(f"{key}: {len(rec.sigs)} recorded / {len(rows)} replayed signatures, worst err/bar {worst[2].worst:.3f} ({LR.short(worst[0])[:60]}, "
          f"{worst[2].where}), largest operand {biggest[2].max_bytes / 2 ** 30:.2f} GiB ({LR.short(biggest[0])[:60]}), "
          f"peak device memory {torch.cuda.max_memory_allocated() / 1e9:.1f} GB, record + replay {time.perf_counter() - t0:.1f} s")
    _check_tail(key, rec, rows, took)
    if key == "W13":
        assert biggest[2].max_bytes >= 2 ** 30, f"W13: largest replayed operand {biggest[2].max_bytes} bytes < 1 GiB"
    assert not bad, f"{key}: {len(bad)} signature(s) beyond their bar:\n" + "\n".join(bad)


def test_edge_channel_signatures_match_float64():
    """launch_replay.EDGE_CHANNELS: what in_conv and out_conv launch at 1, 4 and 12 channels, hand-written (the workloads W18-W24 record
    the same geometries live), each on the kernel the table names."""
    rows, bad = [], []
    for i, (sig, variant) in enumerate(LR.EDGE_CHANNELS):
        got = LR.variant_of(sig)
        assert got == variant, f"{LR.short(sig)}: dispatched to {got}, the table names {variant}"
        r = LR.replay(sig, DEV, seed=i)
        rows.append((sig, variant, r))
        if r.worst > 1.0:
            bad.append(f"{LR.short(sig)}: {r.where} err/bar {r.worst:.3g}")
    print(f"\n== edge channel counts: {len(rows)} replayed signatures")
    for sig, var, r in rows:
        print(f"  {LR.short(sig):<130s} v{'' if var is None else var:<3} {r.where:<10s} err/bar {r.worst:.3f}")
    assert not bad, "\n".join(bad)


def test_synthetic_signatures_match_float64():
    """The replayed entries at edge geometries of their own (launch_replay.SYNTHETIC): ddpm_gather_rows_f32 and ddpm_add_rows are
    launched by none of the workloads above."""
    bad = []
    for i, s in enumerate(LR.SYNTHETIC):
        r = LR.replay(s, DEV, seed=i)
        print(f"  {LR.short(s):<90s} {r.where:<10s} err/bar {r.worst:.3f}")
        if r.worst > 1.0:
            bad.append(f"{LR.short(s)}: {r.where} err/bar {r.worst:.3g}")
    assert not bad, "\n".join(bad)


# ------------------------------------------------------------------------------------------------------------------ the optimizer tail
TAIL_ENTRIES = sorted({s[0] for s in LR.TAIL})


@pytest.mark.parametrize("name", TAIL_ENTRIES)
def test_tail_rows_match_float64_and_repeat_bit_for_bit(name):
    """launch_replay.TAIL: hand-written tables of the optimizer tail (numel 0 .. 512 x 512 x 9, every packing and alignment, EMA and
    clipping on and off, steps 1 .. 10^6, scalars by value and through hyper_dev).  Every output within its bar (the layout entries: bit
    for bit), nothing outside the rows' tensors touched, and a second launch on the same inputs gives the same bits (no atomics)."""
    bad = []
    for i, s in [(i, s) for i, s in enumerate(LR.TAIL) if s[0] == name]:
        r = LR.replay(s, DEV, seed=i)
        again = LR.replay(s, DEV, seed=i)
        print(f"  {LR.short(s)[:120]:<120s} {r.where:<14s} err/bar {r.worst:.3f}" + ("" if r.depth is None else f"  chain {r.depth}"))
        if r.worst > 1.0:
            bad.append(f"{LR.short(s)}: {r.where} err/bar {r.worst:.3g}")
        assert set(r.outputs) == set(again.outputs)
        for k, (t, _) in r.outputs.items():
            assert LR.same_bits(t, again.outputs[k][0]), f"{LR.short(s)}: {k} differs between two launches on the same inputs"
    assert not bad, "\n".join(bad)


def test_tail_planted_sums_of_squares_are_exact():
    """launch_replay.TAIL_PLANTED: gradients that are zero except for distinct powers of two at the first, last and tail elements, either
    side of one grid sweep, in the first and the last row — total_sq[0] must be the planted sum bit for bit (one element dropped or
    counted twice changes it), lanes 1..63 zero.  ddpm_mt_grad_sumsq and ddpm_wgrad_unpack_sumsq (power-of-two scale)."""
    for i, s in enumerate(LR.TAIL_PLANTED):
        r = LR.replay(s, DEV, seed=i)
        assert r.worst == 0.0, f"{LR.short(s)}: {r.where} err/bar {r.worst:.3g}"


def test_tail_identities_hold_bit_for_bit():
    """launch_replay.tail_identities: the scalar path (one of p, g, m, v, shadow at 4, 8, 12 bytes modulo 16) against the aligned run,
    hyper_dev against scalars by value, a norm below max_norm against no clipping, the fused unpack against the plain one."""
    cache = {}

    def run(sig):
        if sig not in cache:
            cache[sig] = LR.replay(sig, DEV, seed=11)
        return cache[sig]
    for what, a, b, cols in LR.tail_identities():
        LR.assert_same_tensors(run(a), run(b), cols, what)
        if what.startswith("norm below"):
            assert run(a).clip == 1.0 and a[1][3] == 1.0, "the coefficient of a norm below max_norm is exactly 1"


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_chained_tail_on_the_real_tables_matches_float64(dtype):
    """launch_replay.chained_tail: three steps of unpack + norm -> Adam / EMA -> re-pack -> time-bias gather on the tables Trainer and
    UNet build for the reduced network, as Trainer.step issues them."""
    for step, r in LR.chained_tail(DEV, dtype):
        print(f"  chained tail, step {step}: worst err/bar {r.worst:.3f} ({r.where}), clip coefficient {r.clip:.4g}")
        assert r.worst <= 1.0, f"step {step}: {r.where} err/bar {r.worst:.3g}"
        assert r.clip < 1.0
