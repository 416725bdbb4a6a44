"""-m gpu: every launch of the benchmarked steps, replayed on the MI355X against a float64 reference at the geometry the step uses.

The workloads (tests/launch_replay.py WORKLOADS, bf16 compute mode) are recorded live through ddpm_torch._hip._invoke — the geometry
list is taken from the step every time the test runs, not from a committed snapshot.  Each distinct signature of a replayed entry is
(dropout seeds aside) re-issued once on fresh random inputs (same pitches, pointer offsets modulo 256, optional operands, modes, splits and workspaces) and
every output element is held to its own error-model bar; the float64 references run in torch on the GPU, over every image.
Every recorded entry must be either replayed or mapped to the existing test that covers it (launch_replay.COVERED_ELSEWHERE)."""
import collections

import pytest
import torch

from ddpm_torch import _hip
from tests import launch_replay as LR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# kernels the benchmark line is made of (include/ddpm_hip_debug.h): 13 conv3x3_pc, 10 / 8 conv3x3_stream<8> / <16>, 7 pw_conv,
# 4 gemm64, 11 / 12 edge convs, 14 wgrad3x3_ws, 6 wgrad3x3 (patch-stationary)
W1_VARIANTS = {13, 10, 8, 7, 4, 11, 12, 14, 6}


def _table(key, rows):
    print(f"\n== {key}: {LR.WORKLOADS[key][0]} — {len(rows)} replayed signatures")
    for sig, var, r in rows:
        print(f"  {LR.short(sig):<150s} v{'' if var is None else var:<3} {r.where:<10s} err/bar {r.worst:.3f}")


@pytest.mark.parametrize("key", list(LR.WORKLOADS))
def test_every_launch_of_the_step_matches_float64(key, monkeypatch):
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
    rows, bad, seen = [], [], set()
    for i, s in enumerate(rec.sigs):
        if s[0] not in LR.REPLAY or LR.geometry(s) in seen:
            continue
        seen.add(LR.geometry(s))
        r = LR.replay(s, DEV, seed=i)
        rows.append((s, LR.variant_of(s), r))
        if r.worst > 1.0:
            bad.append(f"{LR.short(s)}: {r.where} err/bar {r.worst:.3g}")
    _table(key, rows)
    assert not bad, f"{key}: {len(bad)} signature(s) beyond their bar:\n" + "\n".join(bad)
