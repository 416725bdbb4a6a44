"""-m gpu: the HIP kernels on poisoned memory and on hostile value distributions.

Every other replay draws N(0, 1)-like operands into buffers whose unreadable parts (guard bands, pitch gaps, overwritten outputs,
workspaces) hold finite, harmless values.  Here every hand-written signature of tests/launch_replay.py (ODD_GEOMETRY, SYNTHETIC,
EXTRA_SMALL — the smallest shapes at which each kernel is dispatched — and EDGE_CHANNELS, the edge convs at 1, 4 and 12 channels) is replayed against the same float64 references under the same,
unchanged per-element bars, one test per family x mode:

  poison          everything include/ddpm_hip.h does not let the call read holds 0xFF bytes (NaN in fp32 and bf16): both guard bands,
                  pitch gaps and channel-slice neighbours of inputs, the prior content of overwritten outputs, the pitch gaps of
                  outputs (unchanged afterwards), unspecified workspaces.  Outputs must be finite, within their bars, and — every
                  entry but the fp32-atomic accumulation targets — bit-equal to the plain run of the same seed.
  value profiles  launch_replay.PROFILES: scaled_up / scaled_down (bit-exactly 2^+-30 times the plain run on the linear families),
                  sparse, corner_outlier, far_mean, constant_group, saturating, wide / flat / offset logits.  The non-linear families
                  also put a yardstick — the plain fp32 torch composition on the same stored inputs — through the same bars;
                  tests/test_hostile_inputs_host.py holds it to 0.5 on the CPU, the kernel is held to 1.0 here.
  nonfinite_*     one NaN / one +inf planted in a data operand: exactly the outputs the float64 reference makes non-finite are
                  non-finite (the receptive field of a conv over all N channels, the GEMM row, the (sample, group) of a GroupNorm and
                  its statistics, the softmax / attention row, the sample's loss, the element of q_sample), everything else is finite
                  and within its bar.
tests/test_kernels_gpu.py holds the optimizer kernels to torch on NaN, overflowing, zero and tiny gradients; the rows of
launch_replay.TAIL put them, the gradient unpack, the weight packs and the time-bias gather through the same modes here (`grad` is the
role of the gradient operand: with a NaN gradient and clipping on, every p, m, v and shadow of every row is NaN).

Measured on the MI355X (worst kernel err/bar | the yardstick's, per family x mode; the whole module runs in 6 s, the GPU suite in 4 min):
  conv            poison, scaled_up, scaled_down, sparse, nonfinite_nan, nonfinite_inf: 0.249 each (bit relations hold on every row)
  wgrad           poison, scaled_up, scaled_down 0.401 (wgrad_reduce, 3 x 4100 floats)   sparse 0.052
  gemm, atb       poison, scaled_up, scaled_down 0.354 (atb 130 x 70 x 37)   sparse 0.466   nonfinite_nan / _inf 0.327
  reduce          poison, scaled_up, scaled_down 0.250 (add_rows)
  groupnorm_fwd   poison 0.249   scaled_up 0.249 | 0.249   scaled_down 0.239 | 0.239   corner_outlier 0.249 | 0.249   far_mean 0.234 | 0.234
                  constant_group 0.209 | 0.209   saturating 0.247 | 0.247   nonfinite_nan / _inf 0.249
  groupnorm_bwd   poison 0.413   scaled_up 0.413 | 0.349   scaled_down 0.598 | 0.248 (dgamma)   sparse 0.446 | 0.365 and the known finding
                  below 1.342 | 0.189   corner_outlier 0.439 | 0.281   far_mean 0.333 | 0.242   constant_group 0.357 | 0.248   saturating 0.389 | 0.249
  attention       poison 0.437   sparse 0.397 | 0.176   wide_logits 0.291 | 0.226   flat_logits 0.436 | 0.222   offset_logits 0.309 | 0.267
                  nonfinite_nan / _inf 0.193
  softmax         poison 0.249   wide_logits 0.242 | 0.242   flat_logits 0.246 | 0.246   offset_logits 0.249 | 0.249   nonfinite_nan / _inf 0.248
  silu            poison 0.117   saturating 0.137 | 0.114
  diffusion       poison 0.299   nonfinite_nan / _inf 0.228        misc  poison 0.248
  optimizer       poison 0.125   scaled_up / scaled_down / sparse 0.125 | 0.125   nonfinite_nan 0.124   nonfinite_inf 0.125 (the store of shadow)
  layout          poison 0.265 (the 4 x 4 dgrad pack, fp32; everything else bit-exact)   scaled_up / scaled_down / sparse 0.023 (the unpack's
                  norm)   nonfinite_nan / _inf: the planted element and the norm, nothing else
Profile intensities are the ones launch_replay.PROFILES states (none had to be halved: the yardstick's worst figure on the CPU is 0.373).
What the rows found when they first ran, and what was done ("Hostile inputs"):
  * GroupNorm forward, corner_outlier: rstd beyond its bar in all eight forms and both dtypes, 2.3 .. 25 bars (y up to 18.7; yardstick
    0.25) — the pivot of the single-pass moments was the group's first element.  csrc/norm.hip gn_pivot now takes the median of three
    elements (first, middle, last pixel): 0.249.
  * GroupNorm forward, nonfinite: the saved rstd of the poisoned group was finite (1000: fmaxf(var, 0) swallowed the NaN) while mean
    and y were NaN.  The clamp is a select now.  Dropped elements of a NaN group are 0, not NaN: the dropout is a select by contract
    (include/ddpm_hip.h says so now) and the reference follows.
  * GroupNorm backward, constant_group, fp32 with SiLU: dx 2.5 .. 22.5 bars (yardstick 0.08) in the four staged forms — z was formed
    as x (rstd gamma) + (beta - mean rstd gamma), two terms of 10^3 that cancel at rstd = eps^-1/2.  Now (x - mean) (rstd gamma) +
    beta, at the same instruction count: 0.357.
  * GroupNorm backward, sparse, fp32, HW 9, C 128: dx 1.34 bars on 0.14 % of the elements (yardstick 0.19) — the group's one
    gradient sits at z = -1.251, next to the zero of silu', and the 2e-8 the kernel's silu' is off by (3.6e-6 of its value) reaches the
    whole group.  Not fixed: KNOWN_FINDINGS.
  * ddpm_adam_ema_step / ddpm_mt_adam_ema: a NaN gradient norm gave clip = 1 (tests/test_kernels_gpu.py); fixed in csrc/optim.hip.
  * poison: nothing.  No kernel reads a guard band, a pitch gap, an overwritten output or its workspace before writing it.
Training step, alternating runs of bench.py on one machine, parent's library | this one: --steps 100 9.002 / 9.003 / 9.008 / 9.000 |
9.008 / 9.006 / 8.999 / 9.009 ms; on another machine, --steps 40: 8.549 / 8.558 / 8.505 | 8.493 / 8.599 / 8.543 ms.
"""
import time

import pytest

from tests import launch_replay as LR
from tests.test_unet_gpu import DEV

pytestmark = pytest.mark.gpu

ROWS = LR.hostile_rows()
_PLAIN = {}
# Rows a kernel does not pass yet: (family, mode) -> {row: reason with the measured err/bar}.  They run as a case of their own, strictly
# expected to fail, so that the rest of the family x mode stays asserted and a fix shows up as an unexpected pass.  DESIGN.md, "Hostile inputs".
KNOWN_FINDINGS = {
    ("groupnorm_bwd", "sparse"): {
        "groupnorm_silu_bwd(@0,144,@0,136,@0,152,@0,@0,@0,@0,@0,@0,3,9,128,32,1,0,1114,-,0,-,0,-,0,0)":
            "fp32, HW 9, C 128 (36 elements a group, one of them with a gradient): dx err/bar 1.34 on 0.14 % of the elements, yardstick 0.19",
    },
}


def _cases():
    out = []
    for family, mode in LR.hostile_cases():
        out.append(pytest.param(family, mode, False, id=f"{family}-{mode}"))
        known = KNOWN_FINDINGS.get((family, mode))
        if known:
            out.append(pytest.param(family, mode, True, id=f"{family}-{mode}-known-finding",
                                    marks=pytest.mark.xfail(strict=True, reason="; ".join(known.values()))))
    return out


def test_every_hand_written_entry_belongs_to_a_hostile_family():
    assert {s[0] for _, s in ROWS} == {n for fam in LR.HOSTILE_FAMILIES.values() for n in fam}


@pytest.mark.parametrize("family,mode,known", _cases())
def test_hostile_rows_match_float64(family, mode, known):
    t0 = time.perf_counter()
    entries = None if mode == "poison" else LR.PROFILES[mode][2]
    findings = KNOWN_FINDINGS.get((family, mode), {})
    rows = [(i, s) for i, s in ROWS if s[0] in LR.HOSTILE_FAMILIES[family] and (entries is None or s[0] in entries)
            and (LR.short(s) in findings) == known]
    assert rows
    done, bad = [], []
    for i, sig in rows:
        try:
            r = LR.hostile_replay(sig, DEV, i, mode, _PLAIN)
        except AssertionError as e:                        # finiteness, guards, bit equality, non-finite parity: report every row
            bad.append(f"{LR.short(sig)}: {e}")
            continue
        done.append((sig, r))
        if r.worst > 1.0:
            bad.append(f"{LR.short(sig)}: {r.where} err/bar {r.worst:.3g}" + ("" if r.yard is None else f" (yardstick {r.yard:.3g})"))
        if mode.startswith("nonfinite") and not sum(r.planted.values()):
            bad.append(f"{LR.short(sig)}: the planted value reached no output of the reference")
    print(f"\n== hostile inputs, {family} x {mode}: {len(rows)} signatures")
    for sig, r in done:
        print(f"  {LR.short(sig):<150s} {r.where:<10s} err/bar {r.worst:.3f}  yardstick " + ("-" if r.yard is None else f"{r.yard:.3f} ({r.yard_where})"))
    if done:
        w = max(done, key=lambda x: x[1].worst)
        yards = [r.yard for _, r in done if r.yard is not None]
        print(f"hostile inputs, {family} x {mode}: worst err/bar {w[1].worst:.3f} ({LR.short(w[0])[:80]}, {w[1].where}), yardstick "
              + (f"{max(yards):.3f}" if yards else "-") + f", {time.perf_counter() - t0:.1f} s")
    assert not bad, f"{family} x {mode}: {len(bad)} finding(s):\n" + "\n".join(bad)
