"""Record what the host-emulated engine (tests/abi_emulator.py + the mha, adagn and cond emulators) launches, and the tables it builds, on
five network topologies, and write them to tests/golden/engine_layout.json:

    python -m tests.golden.make_engine_layout

The fixture was recorded on the commit BEFORE the engine got its one network layout (``_Engine.steps`` / ``_Engine.bufs``: forward,
admission, scratch sizing and the conv tables had each walked the levels themselves), with this file and the ``pointer`` / ``core``
parameters of tests/golden/make_attention_core_launches.py's ``spy`` / ``pack`` copied into that tree; tests/test_engine_layout_host.py
replays the cases and demands the same lists and tables.  A launch is [entry name, arguments...]: every non-pointer argument as it was
passed; a pointer into an activation buffer (one ``View.new`` made) as "ptr+<byte offset into the most recent such buffer that holds
it>", which is what shows the channel slice of a concat buffer a launch reads or writes; any other pointer as "ptr" or "null".  Per case
and leg (train mode forward, its backward, an eval forward) the file keeps the convolution, GroupNorm and resample launches in full —
"launches" lists each distinct one once, a leg's "core" is its ordered list of indices into that — and of the leg's whole ordered list
the length "n" and the sha256 of its JSON text.  "tables" holds, per case, the engine's derived tables (see ``tables``).
"""
import hashlib
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for _p in (ROOT, os.path.join(ROOT, "ddpm-torch_amd")):                          # (tests/conftest.py does this under pytest)
    if _p not in sys.path:
        sys.path.insert(0, _p)

import ddpm_torch  # noqa: E402
from ddpm_torch import _ops  # noqa: E402
from oracle import unet_ref as U  # noqa: E402
from tests import adagn_emulator, cond_emulator  # noqa: E402
from tests.golden import make_attention_core_launches as core  # noqa: E402
from tests.golden.recipes import rnd  # noqa: E402

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "engine_layout.json")
B = 2
FULL = ('["ddpm_conv2d_nhwc"', '["ddpm_groupnorm_', '["ddpm_resample2x')       # how the JSON text of a launch kept in full begins
BF16, FP32 = torch.bfloat16, torch.float32
THREE = dict(in_channels=3, hid_channels=32, out_channels=3, ch_multipliers=[1, 2, 2], num_res_blocks=2, apply_attn=[False, True, False], drop_rate=0.0)
# id: (config, mode, image height, width, class labels)
CASES = {
    "three_n2_rwc": (THREE, BF16, 16, 16, None),
    "three_n2_pool": (dict(THREE, resample_with_conv=False, drop_rate=0.1), FP32, 24, 16, None),
    # no resampling at all
    "one_level": (dict(THREE, ch_multipliers=[1], num_res_blocks=1, apply_attn=[True]), BF16, 8, 8, None),
    # identity skips in the encoder, equal widths across levels; level 3 attends over 2 x 1 tokens (streaming)
    "four_equal_n3": (dict(THREE, ch_multipliers=[1, 1, 2, 2], num_res_blocks=3, apply_attn=[False, False, True, True]), BF16, 16, 8, None),
    "two_all_options": (dict(in_channels=9, hid_channels=64, out_channels=6, ch_multipliers=[1, 2], num_res_blocks=1, apply_attn=[True, True],
                             drop_rate=0.1, num_classes=3, use_scale_shift_norm=True, num_heads=2), BF16, 12, 10, [1, 3]),
}


def make(cfg, dtype, H, W, labels):
    torch.manual_seed(11)
    m = ddpm_torch.UNet(**cfg)
    m.load_state_dict(U.randomize_state_dict(m.state_dict(), 23))
    m.set_compute_dtype(dtype)
    y = None if labels is None else torch.tensor(labels)
    return m, rnd(B, cfg["in_channels"], H, W, seed=1), torch.tensor([3, 977]), y, rnd(B, cfg["out_channels"], H, W, seed=2)


def spy(monkeypatch):
    """core.spy with the option emulators attached and activation pointers written as offsets.  Returns (emulator, the launch list, the
    list of (address, bytes, tensor) of every activation buffer made — the tensor is held so that its memory is not handed out again
    while the list is — oldest first)."""
    made, inner = [], _ops.View.new

    def new(*args):
        v = inner(*args)
        made.append((v.ptr, v.base.numel() * v.base.element_size(), v.base))
        return v

    def pointer(a):
        if not a:
            return "null"
        for p, n, _ in reversed(made):
            if p <= a < p + n:
                return f"ptr+{a - p}"
        return "ptr"
    monkeypatch.setattr(_ops.View, "new", staticmethod(new))
    emu, launches = core.spy(monkeypatch, pointer)
    return cond_emulator.attach(adagn_emulator.attach(emu)), launches, made


def tables(m, H, W):
    """The engine's derived tables after a backward, in a form that JSON keeps."""
    eng = m.engine()
    names = {id(mod): name for name, mod in m.named_modules()}
    rows = eng._wgrad_table().tolist()
    return dict(convs=[[names[id(cw.mod)], bool(cw.up)] for cw in eng.convs.values()],
                res_blocks=[names[id(rb)] for rb in eng.res_blocks],
                tb_off=[eng.tb_off[id(rb)] for rb in eng.res_blocks], tb_total=eng.tb_total,
                chunks=[[a, b, len(mem)] for a, b, mem in eng.chunks], ptotal=eng.ptotal,
                wdesc_sha256=hashlib.sha256(json.dumps(rows, separators=(",", ":")).encode()).hexdigest(),
                plan_fwd=sorted(map(list, eng.operand_plan(H, W, False))), plan_bwd=sorted(map(list, eng.operand_plan(H, W, True))),
                max_batch=eng.max_batch(H, W), ws_need=eng._ws_need[(B, H, W)])


def run(case, launches, made):
    """Train mode forward + backward, then an eval forward.  Returns (the model, {"train_fwd" | "train_bwd" | "eval": launches})."""
    m, x, t, y, gy = make(*CASES[case])
    m.train()
    del launches[:], made[:]
    out = m(x, t) if y is None else m(x, t, y)
    fwd = list(launches)
    (out * gy).sum().backward()
    bwd = launches[len(fwd):]
    m.eval()
    del launches[:], made[:]
    with torch.no_grad():
        m(x, t) if y is None else m(x, t, y)
    return m, dict(train_fwd=fwd, train_bwd=bwd, eval=list(launches))


def record(case):
    """(the model, the case's legs in the fixture's form with their own "launches" table, its tables)"""
    with pytest.MonkeyPatch.context() as mp:
        _, launches, made = spy(mp)
        m, legs = run(case, launches, made)
        return m, core.pack({case: json.loads(json.dumps(legs))}, FULL), tables(m, *CASES[case][2:4])


def main():
    table, cases = {}, {}
    for case in CASES:
        _, packed, tabs = record(case)
        for leg in packed["legs"][case].values():                                # this case's indices -> indices into the file's one table
            leg["core"] = [table.setdefault(json.dumps(packed["launches"][i], separators=(",", ":")), len(table)) for i in leg["core"]]
        cases[case] = dict(legs=packed["legs"][case], tables=tabs)
    with open(PATH, "w") as f:                                                   # one distinct launch, one leg, one table per line
        f.write('{"launches": [\n' + ",\n".join(table) + '\n], "cases": {\n'
                + ",\n".join(json.dumps(c) + ": {\n" + ",\n".join(
                    json.dumps(part) + ": {\n" + ",\n".join(json.dumps(k) + ": " + json.dumps(v, separators=(",", ":")) for k, v in by[part].items()) + "\n}"
                    for part in ("legs", "tables")) + "\n}" for c, by in cases.items()) + "\n}}\n")
    print(PATH, os.path.getsize(PATH), "bytes")


if __name__ == "__main__":
    main()
