"""Record the launches of the host-emulated engine (tests/abi_emulator.py + tests/mha_emulator.py) over one network per path of the
attention core, and write them to tests/golden/attention_core_launches.json:

    python -m tests.golden.make_attention_core_launches [--hashes]

The fixture was recorded on the commit BEFORE the attention core got its one path chooser (``_ops.attention_path``) and its one
materialised sequence, with this file and tests/mha_emulator.py's streaming pair copied into that tree; tests/test_attention_core_host.py
replays the cases and demands the same list, launch for launch.  A launch is [entry name, arguments...]: every non-pointer argument as it
was passed, a pointer as "ptr" or "null" (allocator addresses are not stable).  The file keeps the launches of the attention core (the
attention, softmax and gemm entries) in full — "launches" lists each distinct one once, a leg's "core" is its ordered list of indices into
that — and of a leg's whole ordered list, every other entry included, the length "n" and the sha256 of its JSON text.  --hashes prints a sha256 of the output and of every parameter
gradient per case instead (the emulator is deterministic float64 numpy: equal between two trees on one machine, not across BLAS builds).
"""
import ctypes
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
from ddpm_torch import _hip  # noqa: E402
from oracle import unet_ref as U  # noqa: E402
from tests import abi_emulator, mha_emulator  # noqa: E402
from tests.golden.recipes import rnd  # noqa: E402

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "attention_core_launches.json")
# the reduced two-level network of tests/test_mha_host.py: attention on both levels and in the middle
RED = dict(in_channels=3, hid_channels=64, out_channels=3, ch_multipliers=[1, 2], num_res_blocks=1, apply_attn=[True, True], drop_rate=0.0)
WIDE = dict(RED, hid_channels=128, ch_multipliers=[1], apply_attn=[True])
B = 2
CORE = ('["ddpm_attention', '["ddpm_softmax', '["ddpm_gemm"')                  # how an attention-core launch's JSON text begins
BF16, FP32 = torch.bfloat16, torch.float32
# id: (config, mode, image height, width, head arguments)                         tokens per level: path
CASES = {
    "bf16_8x8": (RED, BF16, 8, 8, {}),                                          # 64 / 16: flash
    "bf16_12x10": (RED, BF16, 12, 10, {}),                                      # 120: materialised, 30: stream
    "bf16_10x10": (RED, BF16, 10, 10, {}),                                      # 100 / 25: stream
    "bf16_32x16_hid128": (WIDE, BF16, 32, 16, {}),                              # 512 at C = 128: stream in training, fused in eval
    "fp32_8x8": (RED, FP32, 8, 8, {}),                                          # materialised
    "bf16_heads2": (RED, BF16, 8, 8, dict(num_heads=2)),                        # head-indexed streaming, d = 32 and 64
    "bf16_head_channels16": (RED, BF16, 8, 8, dict(num_head_channels=16)),      # materialised per head: d is no multiple of 32
    "fp32_heads2": (RED, FP32, 8, 8, dict(num_heads=2)),                        # materialised per head
}


def make(cfg, dtype, H, W, heads):
    torch.manual_seed(11)
    m = ddpm_torch.UNet(**cfg, **heads)
    m.load_state_dict(U.randomize_state_dict(m.state_dict(), 23))
    m.set_compute_dtype(dtype)
    return m, rnd(B, 3, H, W, seed=1), torch.tensor([3, 977]), rnd(B, 3, H, W, seed=2)


def spy(monkeypatch, pointer=lambda a: "ptr" if a else "null"):
    """Install the emulator; returns (emulator, list that receives one record per launch).  ``pointer``: what a record keeps of an address."""
    emu = mha_emulator.attach(abi_emulator.install(monkeypatch, _hip))
    launches, inner = [], _hip._invoke

    def invoke(name, args):
        launches.append([name] + [pointer(a) if T in (ctypes.c_void_p, ctypes.c_char_p) else a
                                  for T, a in zip(_hip.PROTOTYPES[name], args)])
        inner(name, args)
    monkeypatch.setattr(_hip, "_invoke", invoke)
    return emu, launches


def run(case, launches):
    """Train mode forward + backward, then an eval forward.  Returns (the model, {"train_fwd" | "train_bwd" | "eval": launches},
    {name: tensor} of the outputs and every parameter gradient)."""
    m, x, t, gy = make(*CASES[case])
    m.train()
    m.engine().debug_keep_tape = True
    del launches[:]
    y = m(x, t)
    fwd = list(launches)
    (y * gy).sum().backward()
    bwd = launches[len(fwd):]
    out = {"train.y": y.detach()}
    out.update(("grad." + k, p.grad) for k, p in m.named_parameters())
    m.eval()
    del launches[:]
    with torch.no_grad():
        out["eval.y"] = m(x, t)
    return m, dict(train_fwd=fwd, train_bwd=bwd, eval=list(launches)), out


def pack(res, full=CORE):
    """{case: {leg: launches}} -> the fixture's form (see the module docstring).  ``full``: how the JSON text of a launch kept in full begins."""
    table, legs = {}, {}
    for case, by in res.items():
        legs[case] = {}
        for leg, launches in by.items():
            text = [json.dumps(r, separators=(",", ":")) for r in launches]
            core = [table.setdefault(t, len(table)) for t in text if t.startswith(full)]
            legs[case][leg] = dict(n=len(text), sha256=hashlib.sha256("\n".join(text).encode()).hexdigest(), core=core)
    return dict(launches=[json.loads(t) for t in table], legs=legs)


def main(argv):
    with pytest.MonkeyPatch.context() as mp:
        _, launches = spy(mp)
        res = {}
        for case in CASES:
            _, res[case], out = run(case, launches)
            if "--hashes" in argv:
                h = hashlib.sha256()
                for k in sorted(out):
                    h.update(k.encode() + out[k].detach().contiguous().view(torch.uint8).numpy().tobytes())
                print(case, h.hexdigest(), flush=True)
    if "--hashes" not in argv:
        write(pack(res))


def write(packed):
    with open(PATH, "w") as f:                                                   # one distinct launch, one leg per line
        f.write('{"launches": [\n' + ",\n".join(json.dumps(r, separators=(",", ":")) for r in packed["launches"]) + '\n], "legs": {\n'
                + ",\n".join(json.dumps(c) + ": {\n" + ",\n".join(json.dumps(k) + ": " + json.dumps(v, separators=(",", ":")) for k, v in by.items()) + "\n}"
                             for c, by in packed["legs"].items()) + "\n}}\n")
    print(PATH, os.path.getsize(PATH), "bytes")


if __name__ == "__main__":
    main(sys.argv[1:])
