"""Host check (CPU) of the hostile-input replays of tests/test_hostile_inputs_gpu.py: the same rows (launch_replay.ODD_GEOMETRY,
SYNTHETIC, EXTRA_SMALL and EDGE_CHANNELS) in the same modes (poison, then every value profile of launch_replay.PROFILES), through the host-emulated
ABI (tests/abi_emulator.py), the way tests/test_step_launches_host.py drives replay().

What it shows before any GPU time:
  * the poison bookkeeping of the replay builders is the contract's: an emulator that read a pitch gap, a guard band, the prior content
    of an overwritten output or an unspecified workspace would turn NaN or change its output bits against the plain run — so
    tests/abi_emulator.py itself stays inside include/ddpm_hip.h;
  * the float64 references follow every profile (two independent restatements agree within the bars, HOST_SLACK as in the sibling);
  * the yardstick — the plain fp32 torch composition of each non-linear family on the same stored inputs — stays at or below
    YARD_BAR = 0.5 of the unchanged bars at the profile intensities of launch_replay.PROFILES: the bars leave a careful fp32
    implementation a factor of two, so a kernel beyond 1.0 is a finding in the kernel;
  * the new checks bite: an emulated conv that reads one channel past C (times a zero weight) fails the poison run, an emulated
    GroupNorm that takes single-pass fp32 moments about 0 fails far_mean, a NaN-swallowing softmax fails nonfinite_nan."""
import os

import numpy as np
import pytest
import torch

from ddpm_torch import _hip
from tests import abi_emulator
from tests import launch_replay as LR

pytestmark = pytest.mark.skipif(not os.path.exists(_hip.LIB_PATH), reason="libddpm_hip.so not built")

HOST_SLACK = 4.0                    # tests/test_step_launches_host.py: the emulator is itself an fp32 restatement
YARD_BAR = 0.5
ROWS = LR.hostile_rows()
_PLAIN = {}


def test_every_hand_written_entry_belongs_to_a_hostile_family_and_profiles_name_replayed_entries():
    names = {n for fam in LR.HOSTILE_FAMILIES.values() for n in fam}
    assert {s[0] for _, s in ROWS} == names
    for prof, (_, roles, entries) in LR.PROFILES.items():
        assert roles and set(entries) <= names, prof


@pytest.mark.parametrize("family,mode", LR.hostile_cases(), ids=lambda v: v)
def test_hostile_rows_agree_with_the_emulator(family, mode, monkeypatch):
    abi_emulator.install(monkeypatch, _hip)
    entries = None if mode == "poison" else LR.PROFILES[mode][2]
    rows = [(i, s) for i, s in ROWS if s[0] in LR.HOSTILE_FAMILIES[family] and (entries is None or s[0] in entries)]
    assert rows
    bad, worst, yard = [], 0.0, None
    for i, sig in rows:
        r = LR.hostile_replay(sig, "cpu", i, mode, _PLAIN)
        worst = max(worst, r.worst)
        if r.worst > HOST_SLACK:
            bad.append(f"{LR.short(sig)}: {r.where} emulator err/bar {r.worst:.3g}")
        if r.yard is not None:
            yard = max(yard or 0.0, r.yard)
            if r.yard > YARD_BAR:
                bad.append(f"{LR.short(sig)}: {r.yard_where} yardstick err/bar {r.yard:.3g}")
        if mode.startswith("nonfinite"):
            assert sum(r.planted.values()) > 0, f"{LR.short(sig)}: the planted value reached no output of the reference"
    print(f"\nhostile, {family} x {mode}: {len(rows)} rows, emulator worst err/bar {worst:.3f}, yardstick "
          + ("-" if yard is None else f"{yard:.3f}"))
    assert not bad, f"{family} x {mode}:\n" + "\n".join(bad)


# ------------------------------------------------------------------------------------------------------------------ the checks bite
def test_poison_run_bites_on_a_conv_that_reads_one_channel_past_C(monkeypatch):
    """A K-tail that reads channel C of a wider buffer and multiplies it by a zero-padded weight: invisible on finite memory (the plain
    run passes, bit-equal), NaN under poison."""
    emu = abi_emulator.install(monkeypatch, _hip)
    i, sig = next((i, s) for i, s in ROWS if s[0] == "ddpm_conv2d_nhwc" and s[1][1] > s[1][13])          # x_ld > C: there is a gap
    LR.hostile_replay(sig, "cpu", i, "poison", {})
    real = emu.ddpm_conv2d_nhwc

    def over_read(*a):
        real(*a)
        x, x_ld, y, y_ld, B, H, W, C, Ho, Wo, N, dt = a[0], a[1], a[3], a[4], a[10], a[11], a[12], a[13], a[14], a[15], a[16], a[29]
        assert (H, W) == (Ho, Wo)
        past = abi_emulator.Mat(x + C * (2 if dt == abi_emulator.BF16 else 4), B * H * W, 1, x_ld, dt).get()       # channel C of every pixel
        ys = abi_emulator.Mat(y, B * Ho * Wo, N, y_ld, dt)
        ys.set(ys.get() + past * np.float32(0.0))
    monkeypatch.setattr(emu, "ddpm_conv2d_nhwc", over_read)
    assert LR.replay(sig, "cpu", i).worst <= 1.0                       # finite gaps: nothing to see
    with pytest.raises(AssertionError, match="non-finite output"):
        LR.replay(sig, "cpu", i, poison=True)


def test_far_mean_bites_on_single_pass_fp32_moments_about_zero(monkeypatch):
    """A GroupNorm whose variance is E[x^2] - E[x]^2 in fp32 (no pivot, one pass) loses all of it at 50 +- 0.1; the plain draw
    (mean 1.5, std 1) hides that."""
    emu = abi_emulator.install(monkeypatch, _hip)
    i, sig = next((i, s) for i, s in ROWS if s[0] == "ddpm_groupnorm_silu_fwd" and s[1][-1] == LR.F32 and s[1][9] == 2304)

    def single_pass(x, x_ld, y, y_ld, gamma, beta, stats, ws, B, HW, C, G, eps, silu, drop_p, seed, seed_dev, dt, st):
        assert drop_p == 0 or seed_dev
        xin = abi_emulator.Mat(x, B * HW, C, x_ld, dt).get().reshape(B, HW, G, C // G)
        n = np.float32(HW * (C // G))
        s1 = np.cumsum(xin.transpose(0, 2, 1, 3).reshape(B, G, -1), -1, dtype=np.float32)[..., -1]               # sequential fp32 sums
        s2 = np.cumsum((xin * xin).transpose(0, 2, 1, 3).reshape(B, G, -1), -1, dtype=np.float32)[..., -1]
        mean = s1 / n
        rstd = np.float32(1.0) / np.sqrt(np.maximum(s2 / n - mean * mean, np.float32(0.0)) + np.float32(eps))
        t = (xin - mean[:, None, :, None]) * rstd[:, None, :, None]
        t = t.reshape(B * HW, C) * abi_emulator.f32(gamma, C)[None] + abi_emulator.f32(beta, C)[None]
        out = torch.from_numpy(t)
        out = torch.nn.functional.silu(out) if silu else out
        if drop_p > 0:
            sd = (seed + int(abi_emulator._np(seed_dev, 1, abi_emulator.ctypes.c_uint64, np.uint64)[0])) & ((1 << 64) - 1)
            keep = abi_emulator._keep_mask(sd, np.arange(B * HW * C, dtype=np.uint64), abi_emulator._thresh(drop_p))
            out = out * torch.from_numpy(keep.astype(np.float32)).reshape(B * HW, C) / (1.0 - drop_p)
        abi_emulator.Mat(y, B * HW, C, y_ld, dt).set(out.numpy())
        if stats:
            s = abi_emulator.f32(stats, B * G * 2).reshape(B, G, 2)
            s[..., 0], s[..., 1] = mean, rstd
    monkeypatch.setattr(emu, "ddpm_groupnorm_silu_fwd", single_pass)
    assert LR.replay(sig, "cpu", i).worst <= HOST_SLACK
    assert LR.replay(sig, "cpu", i, profile="far_mean").worst > HOST_SLACK


def test_nonfinite_parity_bites_on_a_softmax_whose_maximum_and_sum_swallow_nan(monkeypatch):
    """fmaxf-style maxima and a sum that skips NaN leave one NaN element in a row whose every probability the reference makes NaN."""
    emu = abi_emulator.install(monkeypatch, _hip)
    i, sig = next((i, s) for i, s in ROWS if s[0] == "ddpm_softmax_fwd" and s[1][-1] == LR.F32)
    assert sum(LR.replay(sig, "cpu", i, profile="nonfinite_nan").planted.values()) == sig[1][3]          # the row, nothing else

    def swallowing(s, p, rows, L, dt, st):
        v = abi_emulator.f32(s, rows * L).reshape(rows, L)
        e = np.exp(v - np.nanmax(v, -1, keepdims=True))
        abi_emulator.Mat(p, rows, L, L, dt).set(e / np.nansum(e, -1, keepdims=True))
    monkeypatch.setattr(emu, "ddpm_softmax_fwd", swallowing)
    assert LR.replay(sig, "cpu", i).worst <= HOST_SLACK
    with pytest.raises(AssertionError, match="finite where the reference is not"):
        LR.replay(sig, "cpu", i, profile="nonfinite_nan")
