"""CPU, C ABI emulated: the engine that reads the network's order and concat geometry from one layout (``_Engine.steps`` /
``_Engine.bufs``) launches, and tabulates, what the engine did whose forward, admission check, scratch sizing and conv tables each walked
the levels themselves.

tests/golden/engine_layout.json holds, for five topologies (three levels with and without resampling convs, one level, four levels of
three blocks with equal widths, two levels with every option on), the launches of a train mode forward, its backward and an eval forward
on the commit before that change — the convolution, GroupNorm and resample launches in full, with the byte offset of every pointer into
its activation buffer (the concat slice a launch reads or writes), the whole list as its length and sha256 — and the engine's derived
tables.  tests/golden/make_engine_layout.py records it and states the cases and the file's form."""
import json
import os

import pytest

from ddpm_torch import _hip
from tests.golden import make_engine_layout as rec

pytestmark = pytest.mark.skipif(not os.path.exists(_hip.LIB_PATH), reason="libddpm_hip.so not built")
# where B, HW, C stand in a GroupNorm launch (entry name included); the element type is the argument in front of the stream
GN_DIMS = {"ddpm_groupnorm_silu_fwd": 9, "ddpm_groupnorm_mod_silu_fwd": 9, "ddpm_groupnorm_silu_bwd": 13, "ddpm_groupnorm_mod_silu_bwd": 13}
WS_NEED = {"three_n2_rwc": 2048, "three_n2_pool": 4352, "one_level": 640, "four_equal_n3": 1152, "two_all_options": 3200}


@pytest.fixture(scope="module")
def golden():
    with open(rec.PATH) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def recorded():
    """case -> (the legs in the fixture's form with their own "launches" table, the tables), each case run once"""
    done = {}

    def get(case):
        if case not in done:
            done[case] = rec.record(case)[1:]
        return done[case]
    return get


@pytest.mark.parametrize("case", list(rec.CASES))
def test_the_launches_are_the_parent_commits(case, golden, recorded):
    mine = recorded(case)[0]
    table = golden["launches"]
    for leg, want in golden["cases"][case]["legs"].items():
        have = mine["legs"][case][leg]
        full = [mine["launches"][i] for i in have["core"]]               # the conv, GroupNorm and resample launches, one by one ...
        assert len(full) == len(want["core"]), (leg, len(full), len(want["core"]))
        for i, (g, w) in enumerate(zip(full, (table[j] for j in want["core"]))):
            assert g == w, (leg, i, g, w)
        assert (have["n"], have["sha256"]) == (want["n"], want["sha256"]), leg      # ... and the leg's whole list, every other entry included


@pytest.mark.parametrize("case", list(rec.CASES))
def test_the_tables_are_the_parent_commits(case, golden, recorded):
    have, want = json.loads(json.dumps(recorded(case)[1])), golden["cases"][case]["tables"]
    assert set(have) == set(want)
    for k in want:
        assert have[k] == want[k], k


@pytest.mark.parametrize("case", list(rec.CASES))
def test_the_groupnorm_scratch_is_the_largest_any_groupnorm_launch_asks_for(case, golden, recorded):
    """``_ws_need`` against ddpm_gn_workspace_floats over the GroupNorm launches of the three legs: as large as the largest, and no larger."""
    mine, tabs = recorded(case)
    need = 0
    for r in mine["launches"]:                                           # every distinct full launch of the three legs
        if r[0] in GN_DIMS:
            b, hw, c, g = r[GN_DIMS[r[0]]:GN_DIMS[r[0]] + 4]
            need = max(need, _hip.lib().ddpm_gn_workspace_floats(b, hw, c, g, r[-2]))
    assert {r[0] for r in mine["launches"]} >= {"ddpm_groupnorm_silu_fwd", "ddpm_groupnorm_silu_bwd"}
    assert tabs["ws_need"] == need == WS_NEED[case] == golden["cases"][case]["tables"]["ws_need"]
