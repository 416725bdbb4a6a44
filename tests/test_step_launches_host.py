"""Host check (CPU) of tests/launch_replay.py, the replay-against-float64 machinery of tests/test_step_launches_gpu.py.

The benchmarked workloads of the GPU test, their fp32 twins, the non-square workloads W14-W17 and the edge-channel workloads W18-W24
(1, 4 and 12 image channels) run through the host-emulated engine
(tests/abi_emulator.py) at batch 2 (CelebA-HQ at 128x128 instead of 256x256: its geometry does not change how the contract is read),
their launches are recorded, and every recorded signature of a
replayed entry is replayed against the emulator.  This shows, before any GPU time, that the replay builders size their buffers, read
pitches, epilogue terms, output modes and slab workspaces the way include/ddpm_hip.h states them — two independent restatements
(the emulator and the float64 references) must agree within the per-element bars — and that no emulated write leaves the extents the
builders computed (the guard bands and the untouched elements are checked after every launch).  Every recorded entry is accounted for.

The optimizer tail (at the end of this module): the recorded table-driven signatures carry the tables Trainer and UNet built and are
replayed with the rest; the hand-written tables launch_replay.TAIL / TAIL_PLANTED, the bit identities and the three-step chain on the
real tables run on the emulated ABI; and eight faults wrapped round the emulator's entries — eps before the division, the EMA from the
old p, a skipped tail element, the clip on m, an unwritten shadow, a planted element counted twice, an untransposed unpack row, a
float past numel — must each be rejected by the replay."""
import os
import time

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from ddpm_torch import _hip
from tests import abi_emulator
from tests import launch_replay as LR

pytestmark = pytest.mark.skipif(not os.path.exists(_hip.LIB_PATH), reason="libddpm_hip.so not built")

# The emulator is itself an fp32 restatement (torch's CPU group-norm backward forms dgamma as sum(dz x) - mean sum(dz), which cancels
# where |mean| >> std): its own rounding may exceed a bar written for the kernels by a small factor.  A misread pitch, operand or
# epilogue term is off by the size of the value itself, 10^3..10^7 bars.
HOST_SLACK = 4.0
HOST_SIZE = {"W1": (2, 32), "W2": (2, 32), "W3": (2, 128), "W4": (2, 64), "W5": (2, 32), "W6": (2, 32), "W7": (2, 128), "W8": (2, 64),
             "W14": (2, (16, 48)), "W15": (2, (16, 48)), "W16": (2, (48, 16)), "W17": (2, (24, 20)),      # the non-square workloads
             # edge channel counts 1, 4 and 12 (train.py --dataset mnist / --block-size 2), bf16 and fp32, and the 12-channel sampling step
             "W18": (2, 32), "W19": (2, 32), "W20": (2, 16), "W21": (2, 16), "W22": (2, 16), "W23": (2, 16), "W24": (2, 16)}
assert set(LR.EDGE_CHANNEL_WORKLOADS) <= set(HOST_SIZE)


def test_replay_builders_agree_with_the_emulator_on_every_recorded_signature(monkeypatch):
    abi_emulator.install(monkeypatch, _hip)
    t0 = time.perf_counter()
    sigs, names = {}, set()
    for key, (B, size) in HOST_SIZE.items():
        rec = LR.record(monkeypatch, key, "cpu", B, size)
        names |= set(rec.names)
        for s in rec.sigs:
            sigs.setdefault(LR.geometry(s, offsets=False), key)
    unaccounted = sorted(names - set(LR.REPLAY) - set(LR.COVERED_ELSEWHERE))
    assert not unaccounted, f"recorded entries neither replayed nor mapped to a covering test: {unaccounted}"
    for must in ("ddpm_conv2d_nhwc", "ddpm_groupnorm_silu_fwd", "ddpm_groupnorm_silu_bwd", "ddpm_attention_fwd_lse", "ddpm_attention_bwd",
                 "ddpm_q_sample", "ddpm_p_sample_step"):
        assert must in names, must
    worst = []
    for s, key in sigs.items():
        if s[0] not in LR.REPLAY:
            continue
        r = LR.replay(s, "cpu")
        worst.append((r.worst, key, LR.short(s), r.where))
        assert r.worst <= HOST_SLACK, f"{key} {LR.short(s)}: {r.where} err/bar {r.worst:.3g}"
    worst.sort(reverse=True)
    for w in worst[:8]:
        print(f"{w[1]} {w[2]} -> {w[3]} err/bar {w[0]:.3f}")
    print(f"{len(worst)} signatures replayed in {time.perf_counter() - t0:.1f} s")


@pytest.mark.parametrize("sig", LR.SYNTHETIC, ids=LR.short)
def test_synthetic_signatures_agree_with_the_emulator(sig, monkeypatch):
    """Every replayer, including those of entries no recorded workload launches, meets the emulator at its edge geometries."""
    abi_emulator.install(monkeypatch, _hip)
    assert sig[0] in LR.REPLAY and sig[0] not in LR.COVERED_ELSEWHERE
    r = LR.replay(sig, "cpu")
    assert r.worst <= HOST_SLACK, f"{LR.short(sig)}: {r.where} err/bar {r.worst:.3g}"


@pytest.mark.parametrize("row", LR.ODD_GEOMETRY, ids=lambda row: LR.short(row[0]))
def test_odd_geometry_signatures_agree_with_the_emulator_and_name_their_kernel(row, monkeypatch):
    """launch_replay.ODD_GEOMETRY (non-square images, pixel and token counts that are no power of two) before any GPU time: the float64
    replayers meet the emulator at these shapes, and the dispatch queries (pure host functions) send each row to the kernel the table
    names, so that the GPU test of the same rows runs the kernels it means to."""
    sig, variant = row
    abi_emulator.install(monkeypatch, _hip)
    assert sig[0] in LR.REPLAY
    assert LR.variant_of(sig) == variant, f"{LR.short(sig)}: dispatched to {LR.variant_of(sig)}, the table names {variant}"
    r = LR.replay(sig, "cpu")
    assert r.worst <= HOST_SLACK, f"{LR.short(sig)}: {r.where} err/bar {r.worst:.3g}"


@pytest.mark.parametrize("row", LR.EDGE_CHANNELS, ids=lambda row: LR.short(row[0]))
def test_edge_channel_signatures_agree_with_the_emulator_and_name_their_kernel(row, monkeypatch):
    """launch_replay.EDGE_CHANNELS (what in_conv and out_conv launch at 1, 4 and 12 channels) before any GPU time, like the odd-geometry
    rows above: the replayers meet the emulator with Creal < C and Nreal < N, and the dispatch queries name the kernel the table names."""
    sig, variant = row
    abi_emulator.install(monkeypatch, _hip)
    assert sig[0] in LR.REPLAY
    assert LR.variant_of(sig) == variant, f"{LR.short(sig)}: dispatched to {LR.variant_of(sig)}, the table names {variant}"
    r = LR.replay(sig, "cpu")
    assert r.worst <= HOST_SLACK, f"{LR.short(sig)}: {r.where} err/bar {r.worst:.3g}"


def test_keep_mask_restatement_is_bit_equal_to_the_numpy_hash():
    for seed in (0, 12345, 0x5DEECE66D + 977, (1 << 63) + 99):
        idx = np.concatenate([np.arange(70000, dtype=np.uint64), np.uint64(1 << 33) + np.arange(5000, dtype=np.uint64)])
        for p in (0.1, 0.5):
            want = abi_emulator._keep_mask(seed, idx, abi_emulator._thresh(p))
            got = LR.keep_mask(seed, torch.from_numpy(idx.astype(np.int64)), p).numpy()
            assert (got == want).all(), (seed, p)


def test_guard_band_and_untouched_elements_catch_a_stray_write():
    """The checks the replays rely on: a write one element past a pitched row, or into a guard band, is reported."""
    A = LR.Arena("cpu", 0)
    b = A.buf("m", LR.pitched(4, 8, 16), LR.F32, 48)
    assert b.ptr % 256 == 48
    b.fill(torch.zeros(b.n))
    b.out(4, 8, 16)
    A.snapshot()
    b.mat(4, 8, 16)[...] = 1.0
    A.check()                                          # writes inside the declared output: fine
    b.t[8] = 2.0                                       # pitch gap
    with pytest.raises(AssertionError, match="outside the contract"):
        A.check()
    b.t[8] = 0.0
    A.check()
    b.raw[b.start + b.nbytes + 5] = 0
    with pytest.raises(AssertionError, match="guard band"):
        A.check()


def test_error_model_bars_bite_at_the_scale_of_a_one_percent_kernel_error(monkeypatch):
    """A conv result off by 2^-4 of one bias term in one output channel must exceed its bar: the bars are per element, not a fraction of
    the tensor maximum."""
    emu = abi_emulator.install(monkeypatch, _hip)
    sig = ("ddpm_conv2d_nhwc", (("p", False, 0), 64, ("p", False, 0), ("p", False, 0), 64, ("p", False, 0), ("p", True, 0), 0,
                                ("p", False, 0), 64, 2, 8, 8, 64, 8, 8, 64, 3, 3, 1, 1, 1, 0, 0, 0, 0, 1, ("p", True, 0),
                                ("p", True, 0), 1))
    assert LR.replay(sig, "cpu").worst <= 1.0
    real = emu.ddpm_conv2d_nhwc

    def skewed(*a):
        real(*a)
        bias, y, y_ld = a[5], a[3], a[4]
        ys = abi_emulator.Mat(y, 2 * 64, 64, y_ld, abi_emulator.BF16)
        v = ys.get()
        v[:, 63] += abi_emulator.f32(bias, 64)[63] * 2.0 ** -4
        ys.set(v)
    monkeypatch.setattr(emu, "ddpm_conv2d_nhwc", skewed)
    assert LR.replay(sig, "cpu").worst > 1.0


def test_conv_bar_bites_on_height_and_width_swapped(monkeypatch):
    """A 3x3 conv that reads its 16 x 48 image as 48 x 16 (H and W swapped: same pixel count, same extents, nothing out of bounds) must
    exceed its bar; on a square image the swap is invisible, which is why the non-square rows exist."""
    emu = abi_emulator.install(monkeypatch, _hip)
    sig = next(s for s, _ in LR.ODD_GEOMETRY if s[0] == "ddpm_conv2d_nhwc" and s[1][11:13] == (16, 48))
    assert LR.replay(sig, "cpu").worst <= 1.0
    real = emu.ddpm_conv2d_nhwc

    def swapped(*a):
        a = list(a)
        a[11], a[12], a[14], a[15] = a[12], a[11], a[15], a[14]          # H <-> W, Ho <-> Wo
        real(*a)
    monkeypatch.setattr(emu, "ddpm_conv2d_nhwc", swapped)
    assert LR.replay(sig, "cpu").worst > 1.0


def _round_bits(a, bits):
    """a rounded to `bits` significant bits (round half to even), as float32"""
    m, e = np.frexp(np.asarray(a, dtype=np.float64))
    return np.ldexp(np.round(m * 2.0 ** bits), e - bits).astype(np.float32)


def test_fp32_conv_bar_bites_on_operands_rounded_to_11_bits(monkeypatch):
    """An fp32 conv whose product ran on operands rounded to 11 significant bits (an fp16-like or tf32-like path, ~5e-4 per operand)
    must exceed its bar; the same signature computed from the unrounded operands must pass."""
    emu = abi_emulator.install(monkeypatch, _hip)
    B, H, W, C, N = 2, 8, 8, 64, 64
    sig = ("ddpm_conv2d_nhwc", (("p", False, 0), C, ("p", False, 0), ("p", False, 0), N, ("p", False, 0), ("p", True, 0), 0,
                                ("p", True, 0), 0, B, H, W, C, H, W, N, 3, 3, 1, 1, 1, 0, 0, 0, 0, 1, ("p", True, 0), ("p", True, 0),
                                abi_emulator.F32))
    assert LR.replay(sig, "cpu").worst <= 1.0
    real = emu.ddpm_conv2d_nhwc

    def rounded(*a):
        real(*a)
        x, w, y = a[0], a[2], a[3]
        xin = abi_emulator.Mat(x, B * H * W, C, C, abi_emulator.F32).get()
        wt = abi_emulator.f32(w, N * 9 * C)

        def conv(xv, wv):
            xt = torch.from_numpy(xv.astype(np.float64)).reshape(B, H, W, C).permute(0, 3, 1, 2)
            wk = torch.from_numpy(wv.astype(np.float64)).reshape(N, 3, 3, C).permute(0, 3, 1, 2)
            return F.conv2d(xt, wk, padding=1).permute(0, 2, 3, 1).reshape(B * H * W, N).numpy()
        ys = abi_emulator.Mat(y, B * H * W, N, N, abi_emulator.F32)
        ys.set(ys.get() + (conv(_round_bits(xin, 11), _round_bits(wt, 11)) - conv(xin, wt)))
    monkeypatch.setattr(emu, "ddpm_conv2d_nhwc", rounded)
    assert LR.replay(sig, "cpu").worst > 1.0


def test_softmax_bar_bites_on_one_row_normaliser_off_by_2_to_the_minus_12(monkeypatch):
    """ddpm_softmax_fwd (fp32) with one row's normaliser off by 2^-12 relative must exceed the per-element bar; exact rows pass."""
    emu = abi_emulator.install(monkeypatch, _hip)
    rows, L = 512, 256
    sig = ("ddpm_softmax_fwd", (("p", False, 0), ("p", False, 0), rows, L, abi_emulator.F32))
    assert LR.replay(sig, "cpu").worst <= 1.0
    real = emu.ddpm_softmax_fwd

    def skewed(s, p, rows_, L_, dt, st):
        real(s, p, rows_, L_, dt, st)
        abi_emulator.f32(p, rows_ * L_)[77 * L_:78 * L_] /= np.float32(1.0 + 2.0 ** -12)
    monkeypatch.setattr(emu, "ddpm_softmax_fwd", skewed)
    assert LR.replay(sig, "cpu").worst > 1.0


# ------------------------------------------------------------------------------------------------------------------ the optimizer tail
def _tail_id(sig):
    return LR.short(sig)[:90]


@pytest.mark.parametrize("i", range(len(LR.TAIL) + len(LR.TAIL_PLANTED)), ids=lambda i: f"{i}-{_tail_id((LR.TAIL + LR.TAIL_PLANTED)[i])}")
def test_tail_rows_agree_with_the_emulator(i, monkeypatch):
    """launch_replay.TAIL and TAIL_PLANTED (the hand-written tables of the optimizer tail) before any GPU time: the float64 references
    — torch.optim.Adam on the handed state, the indexing references of the layout entries, the exact planted sums — meet the emulator,
    and no emulated write leaves the tensors the builders carved out of the guarded buffers."""
    abi_emulator.install(monkeypatch, _hip)
    sig = (LR.TAIL + LR.TAIL_PLANTED)[i]
    assert sig[0] in LR.REPLAY and sig[0] not in LR.COVERED_ELSEWHERE
    r = LR.replay(sig, "cpu", seed=i)
    assert r.worst <= 1.0, f"{LR.short(sig)}: {r.where} err/bar {r.worst:.3g}"


def test_covered_elsewhere_keeps_only_the_exact_helpers():
    assert set(LR.COVERED_ELSEWHERE) == {"ddpm_stream_order", "ddpm_fill_zero", "ddpm_pack_weight", "ddpm_gather_i64", "ddpm_add_i64"}
    assert not set(LR.COVERED_ELSEWHERE) & set(LR.REPLAY)
    assert set(LR.TABLE_ARG) <= set(LR.REPLAY)


@pytest.mark.parametrize("case", LR.tail_identities(), ids=lambda c: c[0])
def test_tail_identities_hold_on_the_emulator(case, monkeypatch):
    abi_emulator.install(monkeypatch, _hip)
    what, a, b, cols = case
    ra, rb = LR.replay(a, "cpu", seed=11), LR.replay(b, "cpu", seed=11)
    LR.assert_same_tensors(ra, rb, cols, what)
    if what.startswith("norm below"):
        assert ra.clip == 1.0 and a[1][3] == 1.0, "the coefficient of a norm below max_norm is exactly 1"


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_chained_tail_on_the_real_tables_agrees_with_the_emulator(dtype, monkeypatch):
    abi_emulator.install(monkeypatch, _hip)
    for step, r in LR.chained_tail("cpu", dtype):
        assert r.worst <= 1.0, f"step {step}: {r.where} err/bar {r.worst:.3g}"
        assert r.clip < 1.0, "the drawn gradients do not clip"


def test_recorded_tail_signatures_carry_the_tables_of_trainer_and_unet(monkeypatch):
    """A recorded step's table-driven signatures hold the geometry of the tables Trainer / UNet built: one row per parameter in the
    update's table, the flat gradient's slices 16-byte aligned and packed with the rounding to 4 floats, every conv in the pack table;
    a table address that belongs to none of the owners fails the recording."""
    abi_emulator.install(monkeypatch, _hip)
    rec = LR.record(monkeypatch, "W14", "cpu", 2, (16, 48))
    by = {}
    for s in rec.sigs:
        by.setdefault(s[0], []).append(s)
    for name in ("ddpm_wgrad_unpack_sumsq", "ddpm_mt_adam_ema", "ddpm_pack_weight_multi", "ddpm_mt_gather_f32"):
        assert name in by and all(LR.is_table(s[1][LR.TABLE_ARG[name][0]]) for s in by[name]), name
    adam = by["ddpm_mt_adam_ema"][0][1]
    rows = adam[0][1]
    assert len(rows) == adam[1] > 50
    for n, cols in rows[:-1]:
        assert cols[1][:2] == (False, 0) and cols[1][2] == 4 * (-n % 4), (n, cols[1])        # g: slices of one flat buffer
        assert all(c[1] == 0 for c in cols)
    unp = by["ddpm_wgrad_unpack_sumsq"][0][1]
    assert sum(r[2] * r[3] * r[4] for r in unp[2][1]) >= sum(n for n, _ in rows)
    rec2 = LR.Recorder(None)
    sig = LR.signature("ddpm_mt_gather_f32", [12345, 1, 0])
    rec2.sigs[sig], rec2.tables[sig] = None, 12345
    with pytest.raises(AssertionError, match="none of"):
        LR.resolve_tables(rec2, None, None)


# ---- the bars bite: each fault below, wrapped round the emulator's entry, must be rejected by the replay (a bar exceeded, a planted
# sum missed, or the guard / untouched-element check), while the unwrapped emulator passes the same row at the same seed
def _rejected(sig, seed):
    try:
        return LR.replay(sig, "cpu", seed=seed).worst > 1.0
    except AssertionError:
        return True


def _faulty_adam(fault):
    def run(table, n, total, max_norm, lr, b1, b2, eps, bc1, bc2, ema_w, hyper, st):
        f32, i64 = abi_emulator.f32, abi_emulator.i64
        max_norm, lr, b1, b2, eps, bc1, bc2, ema_w = (np.float32(x) for x in (max_norm, lr, b1, b2, eps, bc1, bc2, ema_w))
        if hyper:
            lr, bc1, bc2, ema_w = f32(hyper, 4)
        clip = np.float32(1.0)
        if total and max_norm > 0:
            c = np.float32(max_norm / (np.sqrt(f32(total, 64).sum(dtype=np.float32)) + np.float32(1e-6)))
            clip = np.float32(1.0) if c >= 1 else c
        one = np.float32(1.0)
        for row in i64(table, 6 * n).reshape(n, 6):
            p_, g_, m_, v_, sh_, numel = (int(v) for v in row)
            p, g, m, v = f32(p_, numel), f32(g_, numel), f32(m_, numel), f32(v_, numel)
            g = g * clip if fault != "clip_on_m" else g
            m[...] = b1 * m + (one - b1) * g
            if fault == "clip_on_m":
                m[...] = m * clip
            v[...] = b2 * v + (one - b2) * g * g
            denom = (np.sqrt(v) + eps) / np.sqrt(bc2) if fault == "eps_first" else np.sqrt(v) / np.sqrt(bc2) + eps
            old = p.copy()
            p[...] = p - (lr / bc1) * (m / denom)
            if sh_:
                sh = f32(sh_, numel)
                sh[...] = sh + ema_w * ((old if fault == "ema_old_p" else p) - sh)
    return run


def _row(pred):
    return next((i, s) for i, s in enumerate(LR.TAIL) if pred(s))


def _is_adam(s, **opts):
    return s[0] == "ddpm_mt_adam_ema" and all(dict(s[1][0][2]).get(k) == v for k, v in opts.items())


@pytest.mark.parametrize("fault,pred", [
    ("none", lambda s: _is_adam(s, g="loguniform", step=1)),
    ("eps_first", lambda s: _is_adam(s, g="loguniform", step=1)),                                   # (a)
    ("ema_old_p", lambda s: _is_adam(s, g="loguniform", step=1000, ema_w=1e-4)),                     # (b)
    ("clip_on_m", lambda s: _is_adam(s, step=2) and not LR._opt(s[1][-1])),                         # (d)
], ids=lambda v: v if isinstance(v, str) else "")
def test_adam_bar_bites_on_arithmetic_faults(fault, pred, monkeypatch):
    """(a) eps added before the division by sqrt(bc2) at step 1, (b) the EMA taken from the parameter before the update at ema_w = 1e-4,
    (d) the clip coefficient applied to m instead of g — and the same fp32 restatement without a fault passes."""
    emu = abi_emulator.install(monkeypatch, _hip)
    i, sig = _row(pred)
    assert not _rejected(sig, i)
    monkeypatch.setattr(emu, "ddpm_mt_adam_ema", _faulty_adam(fault))
    assert _rejected(sig, i) == (fault != "none")


def _table_fault(emu, monkeypatch, name, edit):
    """run `name` on a copy of its table that `edit` changed"""
    real = getattr(emu, name)
    ti, ni, width = LR.TABLE_ARG[name]

    def run(*a):
        a = list(a)
        t = abi_emulator.i64(a[ti], width * a[ni]).reshape(a[ni], width).copy()
        edit(t)
        a[ti] = t.ctypes.data
        real(*a)
    monkeypatch.setattr(emu, name, run)


def test_adam_replay_rejects_a_skipped_tail_element_and_an_unwritten_shadow(monkeypatch):
    """(c) the last scalar-tail element of one row skipped, (e) shadow of one row not written"""
    i, sig = _row(lambda s: _is_adam(s, step=2) and not LR._opt(s[1][-1]))
    for edit in (lambda t: t.__setitem__((2, 5), t[2, 5] - 1), lambda t: t.__setitem__((3, 4), 0)):
        with pytest.MonkeyPatch.context() as mp:
            emu = abi_emulator.install(mp, _hip)
            assert not _rejected(sig, i)
            _table_fault(emu, mp, "ddpm_mt_adam_ema", edit)
            assert _rejected(sig, i)


def test_planted_sum_rejects_an_element_counted_twice_or_not_at_all(monkeypatch):
    """(f) one planted element of the sum of squares counted twice (and one not at all): 2^-19 of the total at most, far below any
    relative bar — the planted draw sees it exactly.  Both reductions."""
    for sig in (LR.TAIL_PLANTED[1], next(s for s in LR.TAIL_PLANTED if s[0] == "ddpm_wgrad_unpack_sumsq")):
        for delta in (+1.0, -1.0):                       # the element that holds 2^0
            with pytest.MonkeyPatch.context() as mp:
                emu = abi_emulator.install(mp, _hip)
                assert LR.replay(sig, "cpu", seed=3).worst <= 1.0
                real = getattr(emu, sig[0])
                scale2 = LR._f(sig[1][4]) ** 2 if sig[0] == "ddpm_wgrad_unpack_sumsq" else 1.0

                def run(*a, real=real, delta=delta, scale2=scale2, tot=5 if sig[0] == "ddpm_wgrad_unpack_sumsq" else 2):
                    real(*a)
                    abi_emulator.f32(a[tot], 1)[0] += np.float32(delta * scale2)
                mp.setattr(emu, sig[0], run)
                with pytest.raises(AssertionError, match="planted sum"):
                    LR.replay(sig, "cpu", seed=3)


def test_unpack_replay_rejects_a_row_left_in_the_packed_layout(monkeypatch):
    """(g) unpack writing [N][R*S][C] unchanged for one row"""
    emu = abi_emulator.install(monkeypatch, _hip)
    i, sig = _row(lambda s: s[0] == "ddpm_wgrad_unpack" and s[1][4] == 0.5)
    assert not _rejected(sig, i)
    real = emu.ddpm_wgrad_unpack

    def run(gpack, gflat, descs, n, scale, st):
        real(gpack, gflat, descs, n, scale, st)
        src, dst, N, C, RS = (int(v) for v in abi_emulator.i64(descs, 5 * n).reshape(n, 5)[1])
        abi_emulator.f32(gflat + 4 * dst, N * C * RS)[...] = abi_emulator.f32(gpack + 4 * src, N * C * RS) * np.float32(scale)
    monkeypatch.setattr(emu, "ddpm_wgrad_unpack", run)
    assert _rejected(sig, i)


@pytest.mark.parametrize("name", ["ddpm_mt_adam_ema", "ddpm_wgrad_unpack", "ddpm_mt_gather_f32", "ddpm_pack_weight_multi"])
def test_tail_replays_reject_one_float_written_past_numel(name, monkeypatch):
    """(h) one float written past numel of the table's last row (the pad behind it or the guard band): the bits it held, plus one."""
    for i, sig in [(i, s) for i, s in enumerate(LR.TAIL) if s[0] == name][:4]:
        with pytest.MonkeyPatch.context() as mp:
            emu = abi_emulator.install(mp, _hip)
            assert not _rejected(sig, i)
            real = getattr(emu, name)

            def run(*a, real=real):
                real(*a)
                ti, ni, width = LR.TABLE_ARG[name]
                row = [int(v) for v in abi_emulator.i64(a[ti], width * a[ni]).reshape(a[ni], width)[-1]]      # nothing of the table lies behind the last row
                if name == "ddpm_mt_adam_ema":
                    at = row[0] + 4 * row[5]
                elif name == "ddpm_mt_gather_f32":
                    at = row[2] + 4 * row[3]
                elif name == "ddpm_wgrad_unpack":
                    at = a[1] + 4 * (row[1] + row[2] * row[3] * row[4])
                else:
                    es = 2 if a[2] == LR.BF16 else 4
                    at = row[1] + LR._pack_extents(*row[3:8], es)[1]
                abi_emulator._np(at, 1, __import__("ctypes").c_uint16, np.uint16)[0] += 1
            mp.setattr(emu, name, run)
            with pytest.raises(AssertionError, match="outside the contract|guard band"):
                LR.replay(sig, "cpu", seed=i)
