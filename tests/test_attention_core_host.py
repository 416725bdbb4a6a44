"""CPU, C ABI emulated: the engine's attention core issues, launch for launch, what it issued before its path choice moved into one
function (``_ops.attention_path``) and its two materialised sequences into one, and the tape carries the chosen path.

tests/golden/attention_core_launches.json holds the ordered launch list (entry name, every non-pointer argument, null / non-null per pointer)
of the host-emulated engine on the commit before that change, for one network per path: train mode forward and backward, and an eval
forward — the attention core's launches in full, the whole list as its length and sha256.  tests/golden/make_attention_core_launches.py
records it and states the cases and the file's form."""
import json
import os

import pytest
import torch

from ddpm_torch import _hip
from ddpm_torch import _ops as ops
from tests.golden import make_attention_core_launches as rec

pytestmark = pytest.mark.skipif(not os.path.exists(_hip.LIB_PATH), reason="libddpm_hip.so not built")
# what a block's attention core leaves in the log: one attention entry, or the one softmax launch of the materialised sequence
CORE = {"ddpm_attention_fwd_lse": "flash", "ddpm_attention_bwd": "flash", "ddpm_attention_fwd": "fused",
        "ddpm_attention_stream_fwd": "stream", "ddpm_attention_stream_bwd": "stream", "ddpm_attention_mh_fwd": "stream",
        "ddpm_attention_mh_bwd": "stream", "ddpm_softmax_fwd": "mat", "ddpm_softmax_bwd": "mat"}
PARTNER = {"ddpm_attention_bwd": "ddpm_attention_fwd_lse", "ddpm_attention_stream_bwd": "ddpm_attention_stream_fwd",
           "ddpm_attention_mh_bwd": "ddpm_attention_mh_fwd", "ddpm_softmax_bwd": "ddpm_softmax_fwd"}
# per case: the paths of the seven blocks (four of the WIDE network) in forward order; the eval forward's where they differ
F, S, M = "flash", "stream", "mat"
PATHS = {"bf16_8x8": [F, F, F, F, F, F, F], "bf16_12x10": [M, S, S, S, S, M, M], "bf16_10x10": [S] * 7, "bf16_32x16_hid128": [S] * 4,
         "fp32_8x8": [M] * 7, "bf16_heads2": [S] * 7, "bf16_head_channels16": [M] * 7, "fp32_heads2": [M] * 7}
EVAL_PATHS = dict(PATHS, bf16_32x16_hid128=["fused"] * 4)


@pytest.fixture(scope="module")
def golden():
    with open(rec.PATH) as f:
        return json.load(f)


def _core(launches):
    return [r[0] for r in launches if r[0] in CORE]


@pytest.mark.parametrize("case", list(rec.CASES))
def test_the_launches_are_the_parent_commits(case, golden, monkeypatch):
    _, launches = rec.spy(monkeypatch)
    m, got, _ = rec.run(case, launches)
    got = json.loads(json.dumps(got))                                    # (tuples -> lists, as the recorded lists went through)
    table = golden["launches"]
    for leg, want in golden["legs"][case].items():
        mine = rec.pack({case: {leg: got[leg]}})
        have = mine["legs"][case][leg]
        core = [mine["launches"][i] for i in have["core"]]               # the attention core's launches, one by one ...
        assert len(core) == len(want["core"]), (leg, len(core), len(want["core"]))
        for i, (g, w) in enumerate(zip(core, (table[j] for j in want["core"]))):
            assert g == w, (leg, i, g, w)
        assert (have["n"], have["sha256"]) == (want["n"], want["sha256"]), leg      # ... and the leg's whole list, every other entry included
    # the tape names, per block, the path whose entries the log holds: forward in order, backward in reverse, and the backward ran
    # the partner of the forward's entry
    tape = [r for r in m.engine().last_tape if r[0] == "attn"]
    assert [r[-1] for r in tape] == PATHS[case]
    assert [CORE[n] for n in _core(got["train_fwd"])] == PATHS[case]
    assert [CORE[n] for n in _core(got["train_bwd"])] == PATHS[case][::-1]
    assert [PARTNER[n] for n in _core(got["train_bwd"])] == _core(got["train_fwd"])[::-1]
    assert [CORE[n] for n in _core(got["eval"])] == EVAL_PATHS[case]
    heads = {r[1].num_heads for r in tape}
    assert any("_mh_" in n for n in _core(got["train_fwd"])) == (PATHS[case][0] == S and heads != {1})
    for r in tape:                                                       # fields 0-9 are where they were
        assert len(r) == 11 and (r[7] is None) == (r[-1] != M) and (r[9] is None) == (r[-1] == M)


def test_fp32_over_25_tokens_is_still_refused_in_the_same_words(monkeypatch):
    """10 x 10 in the fp32 mode: level 1 sees 25 tokens, no multiple of 4."""
    rec.spy(monkeypatch)
    m, x, t, _ = rec.make(rec.RED, torch.float32, 10, 10, {})
    with pytest.raises(NotImplementedError) as e:
        m.eval()(x, t)
    assert str(e.value) == ("attention over 25 tokens in the fp32 mode: this path needs a token count that is a multiple of 4 (the bf16 mode "
                            "attends over any token count when the channel count is a multiple of 32 up to 512)")


def test_the_chooser_states_the_rules_once():
    """The rules as the engine had them, spelled per head count, against the one function — over every combination of a grid that
    holds each threshold and its neighbours."""
    BF, FP = _hip.BF16, _hip.F32

    def before(H, C, d, dt, B, Lk, ld, save):
        if H > 1:
            return S if dt == BF and d % 32 == 0 and d <= 512 and B * H <= 65535 and Lk * ld * 2 <= 0x7ffffff0 else M
        flash = dt == BF and Lk <= 256 and Lk % 16 == 0 and C <= 512 and C % 32 == 0
        fused = not save and not flash and dt == BF and Lk % 128 == 0 and C in (128, 256)
        stream = (dt == BF and not flash and not fused and (Lk > 256 or Lk % 8) and C <= 512 and C % 32 == 0 and Lk * ld * 2 <= 0x7ffffff0
                  and B <= 65535)                                         # (the one permitted difference: B * H <= 65535 at one head too)
        return F if flash else "fused" if fused else S if stream else M
    seen = set()
    for H in (1, 2, 4):
        for C in (32, 64, 96, 128, 256, 512, 544, 1024, 2048):
            if C % H:
                continue
            for dt in (BF, FP):
                for B in (2, 16384, 32768, 65535, 65536):
                    for Lk in (16, 25, 30, 64, 100, 120, 128, 240, 256, 264, 272, 384, 512, 1000, 1024, 1 << 20):
                        for save in (False, True):
                            args = (H, C, C // H, dt, B, Lk, 3 * C, save)
                            got = ops.attention_path(*args)
                            assert got == before(*args), args
                            seen.add((H > 1, got))
    assert seen == {(False, F), (False, "fused"), (False, S), (False, M), (True, S), (True, M)}
    assert ops.attention_path(1, 64, 64, BF, 65536, 100, 192, True) == M, "B > 65535 at one head: materialised, where the C entry refused"
