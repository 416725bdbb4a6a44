"""Host check (CPU) of tests/launch_replay.py, the replay-against-float64 machinery of tests/test_step_launches_gpu.py.

The benchmarked workloads of the GPU test, their fp32 twins, the non-square workloads W14-W17 and the edge-channel workloads W18-W24
(1, 4 and 12 image channels) run through the host-emulated engine
(tests/abi_emulator.py) at batch 2 (CelebA-HQ at 128x128 instead of 256x256: its geometry does not change how the contract is read),
their launches are recorded, and every recorded signature of a
replayed entry is replayed against the emulator.  This shows, before any GPU time, that the replay builders size their buffers, read
pitches, epilogue terms, output modes and slab workspaces the way include/ddpm_hip.h states them — two independent restatements
(the emulator and the float64 references) must agree within the per-element bars — and that no emulated write leaves the extents the
builders computed (the guard bands and the untouched elements are checked after every launch).  Every recorded entry is accounted for."""
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
