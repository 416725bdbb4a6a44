"""Host checks of the 2 GiB operand limit: the extent arithmetic of every launch_replay.LARGE_OPERANDS row in pure Python (window
membership, the neighbour outside, the refusal of the neighbour by the library's host-side validation, which needs no GPU), and the
UNet engine's admission check on the emulated ABI: a batch whose operands would exceed the limit raises a ValueError naming the layer,
the operand's bytes and the largest admissible batch before the first launch, instead of DDPM_ERR_SHAPE from a layer in the middle of
the forward.

max_batch of the shipped configurations (training: forward + backward; the values INTEGRATION.md quotes):
    celebahq.json, 256 x 256: bf16 63, fp32 31      celeba.json, 64 x 64: bf16 682, fp32 341      cifar10.json, 32 x 32: bf16 2730, fp32 1365
By hand: the widest operand is the first decoder concatenation of level 0, read whole by that block's conv1 and 1x1 skip projection:
128 + 128 = 256 channels at 256 x 256 (celebahq), 256 + 128 = 384 channels at 64 x 64 (celeba) and 32 x 32 (cifar10), and
floor(floor(0x7ffffff0 / es) / (H W C)) is 63 / 31, 682 / 341 and 2730 / 1365.
"""
import json
import os

import pytest
import torch

import ddpm_torch
from ddpm_torch import _hip, _ops
from tests import abi_emulator
from tests import launch_replay as LR
from tests.golden import make_engine_layout as EL
from tests.golden.recipes import rnd
from tests.test_host_emulated import TINY, make

pytestmark = pytest.mark.skipif(not os.path.exists(_hip.LIB_PATH), reason="libddpm_hip.so not built")
CONFIGS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ddpm-torch_amd", "configs")


def test_the_python_limit_is_the_kernels_limit():
    src = open(os.path.join(os.path.dirname(CONFIGS), "csrc", "gfx950.h")).read()
    assert f"BUF_OOB = {hex(LR.BUF_OOB)}u" in src and _ops.BUF_OOB == LR.BUF_OOB


@pytest.mark.parametrize("i", range(len(LR.LARGE_OPERANDS)))
def test_row_extent_is_in_the_window_and_its_neighbour_outside(i):
    sig, variant, neighbour, expect, amp = LR.LARGE_OPERANDS[i]
    operand, extent, unit = LR.largest_extent(sig, amp and amp[1])
    assert LR.BUF_OOB - unit < extent <= LR.BUF_OOB, (LR.short(sig), operand, extent, unit)
    assert all(e <= LR.BUF_OOB for e, _ in LR.guarded_extents(sig).values())
    assert LR.largest_extent(neighbour)[1] > LR.BUF_OOB, LR.short(neighbour)
    got = LR.variant_of(sig)                       # the dry dispatch query: host code
    assert variant is None or got == variant, (LR.short(sig), got)
    if expect == "refused":
        assert LR.refusal_status(neighbour) == LR.ERR_SHAPE
    else:
        assert LR.variant_of(neighbour) == expect


def test_every_guarded_entry_has_a_row():
    assert {r[0][0] for r in LR.LARGE_OPERANDS} == {
        "ddpm_conv2d_nhwc", "ddpm_conv3x3_wgrad_nhwc", "ddpm_conv3x3_wgrad_up_nhwc", "ddpm_conv1x1_wgrad_nhwc", "ddpm_conv2d_wgrad_nhwc",
        "ddpm_gemm", "ddpm_attention_fwd", "ddpm_attention_fwd_lse", "ddpm_attention_bwd", "ddpm_attention_mh_fwd", "ddpm_attention_mh_bwd"}
    conv_variants = {r[1] for r in LR.LARGE_OPERANDS if r[0][0] == "ddpm_conv2d_nhwc"}
    assert conv_variants >= {13, 8, 10, 7, 4, 11, 12, 5, 3}, conv_variants
    assert {r[1] for r in LR.LARGE_OPERANDS if r[0][0].startswith("ddpm_conv3x3_wgrad")} == {14, 6}


class _Plan:
    """stands in for a recording launch plan: counts what _hip.call would append"""
    retains = False

    def __init__(self):
        self.entries, self.keep = [], []

    def add(self, name, args):
        self.entries.append(name)


def _bytes(eng, B, H, W, backward):
    return max(((B * hw - 1) * ld + C) * eng.es for _, _, hw, C, ld in eng.operand_plan(H, W, backward))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_forward_raises_before_the_first_launch(monkeypatch, dtype):
    emu = abi_emulator.install(monkeypatch, _hip)
    m, _ = make(TINY, dtype=dtype)
    m.eval()
    eng = m.engine()
    limit = _bytes(eng, 2, 16, 16, False)          # the limit patched down to what two 16 x 16 images need: a few hundred KiB
    monkeypatch.setattr(_ops, "BUF_OOB", limit)
    assert eng.max_batch(16, 16, backward=False) == 2
    plan = _Plan()
    seen = len(emu.log)
    prev = _hip.record_into(plan)
    try:
        with torch.no_grad(), pytest.raises(ValueError) as err:
            m(rnd(3, 3, 16, 16, seed=1), torch.tensor([3, 500, 977]))
    finally:
        _hip.record_into(prev)
    assert len(emu.log) == seen and not plan.entries, (emu.log[seen:], plan.entries)
    text = str(err.value)
    over = _bytes(eng, 3, 16, 16, False)
    assert str(over) in text and "largest admissible batch is 2" in text and "batch 3 of 16 x 16" in text
    assert any(name and name in text for name, _ in m.named_modules())
    with torch.no_grad():                          # one batch smaller runs
        y = m(rnd(2, 3, 16, 16, seed=1), torch.tensor([3, 977]))
    assert y.shape == (2, 3, 16, 16) and bool(torch.isfinite(y).all()) and len(emu.log) > seen


def test_training_forward_counts_the_backward_operands(monkeypatch):
    """With a tape the dense gradient buffers count too: project_in's [3C] output gradient is wider than any forward operand of TINY's
    attention level, and the admission check of a training forward sees it."""
    abi_emulator.install(monkeypatch, _hip)
    m, _ = make(TINY)
    eng = m.engine()
    fwd, both = eng.operand_plan(16, 16, False), eng.operand_plan(16, 16, True)
    assert set(fwd) < set(both) and any(what == "output gradient" and C == 3 * 64 for _, what, _, C, _ in both)
    assert eng.max_batch(16, 16, True) <= eng.max_batch(16, 16, False)


@pytest.mark.parametrize("name,size,bf16,fp32", [("celebahq.json", 256, 63, 31), ("celeba.json", 64, 682, 341), ("cifar10.json", 32, 2730, 1365)])
def test_max_batch_of_the_shipped_configurations(monkeypatch, name, size, bf16, fp32):
    abi_emulator.install(monkeypatch, _hip)
    cfg = {k: v for k, v in json.load(open(os.path.join(CONFIGS, name)))["model"].items() if k != "block_size"}
    cfg.setdefault("out_channels", cfg["in_channels"])
    got = {}
    with torch.device("meta"):                     # shapes only: the plan reads no weight
        m = ddpm_torch.UNet(**cfg)
    for dtype in (torch.bfloat16, torch.float32):
        m._eng = None
        m.compute_dtype = dtype
        got[dtype] = m.engine().max_batch(size, size)
    print(f"\nmax_batch {name} {size} x {size}: bf16 {got[torch.bfloat16]}, fp32 {got[torch.float32]}")
    assert (got[torch.bfloat16], got[torch.float32]) == (bf16, fp32)


# ------------------------------------------------------------------------------------------- the plan against the engine's own launches
GUARDED = ("ddpm_conv2d_nhwc", "ddpm_conv2d_wgrad_nhwc", "ddpm_conv3x3_wgrad_nhwc", "ddpm_conv3x3_wgrad_up_nhwc", "ddpm_conv1x1_wgrad_nhwc", "ddpm_gemm")


def _recorded(monkeypatch, m, B, size, labels=None):
    """Every distinct launch signature of one training forward + backward at batch B, with nothing launched and nothing computed: the
    C-ABI calls are recorded and dropped, and every activation view stands on one small buffer (a signature keeps pitches, shapes and
    pointer alignment, which is all the launchers' validation and the dispatch queries read)."""
    rec = LR.Recorder(lambda name, args: None)
    monkeypatch.setattr(_hip, "_invoke", rec)
    bases = {}

    def new(B_, H, W, C, dtype, device):
        return _ops.View(bases.setdefault(dtype, torch.zeros(64, dtype=dtype)), B_, H, W, C)
    monkeypatch.setattr(_ops.View, "new", staticmethod(new))
    H, W = size
    x = torch.zeros(B, m.in_channels, H, W)
    y = m(x, torch.arange(B) % 1000, *(() if labels is None else (torch.arange(B) % (m.num_classes + 1),)))
    y.sum().backward()
    return [s for s in rec.sigs if s[0] in GUARDED]


def _dry(sig):
    """-status or the kernel id from the dry dispatch query (entries that have a pitch-aware one), else None"""
    if sig[0] in ("ddpm_conv2d_nhwc", "ddpm_conv2d_wgrad_nhwc", "ddpm_gemm"):
        return LR.variant_of(LR.geometry(sig, offsets=False))
    return None


def _plan_against_signatures(monkeypatch, m, eng, H, W, label, labels=None):
    B = eng.max_batch(H, W)
    sigs = _recorded(monkeypatch, m, B, (H, W), labels)
    assert len(sigs) > 50
    worst = max(LR.largest_extent(s)[1] for s in sigs)
    assert worst <= LR.BUF_OOB and worst == _bytes(eng, B, H, W, True), (worst, _bytes(eng, B, H, W, True))
    refused = [s for s in sigs if (_dry(s) or 0) < 0]
    assert not refused, [LR.short(s) for s in refused[:3]]
    monkeypatch.setattr(eng, "admit", lambda *a, **k: None)
    over = _recorded(monkeypatch, m, B + 1, (H, W), labels)
    beyond = [s for s in over if LR.largest_extent(s)[1] > LR.BUF_OOB]
    assert beyond and max(LR.largest_extent(s)[1] for s in over) == _bytes(eng, B + 1, H, W, True)
    assert all(_dry(s) in (None, -LR.ERR_SHAPE) for s in beyond) and any(_dry(s) == -LR.ERR_SHAPE for s in beyond)
    print(f"\n{label} {H} x {W}: max_batch {B}, {len(sigs)} guarded signatures, largest operand {worst} B; at {B + 1}: {len(beyond)} refused")


@pytest.mark.parametrize("name,size", [("celebahq.json", 256), ("celeba.json", 64)])
def test_plan_matches_the_signatures_the_engine_emits(monkeypatch, name, size):
    """At max_batch every conv, weight-gradient and GEMM signature the engine really emits (forward + backward, both compute modes) is
    within the limit by the launchers' own extent arithmetic and admitted by the dry dispatch queries; at max_batch + 1 (the
    admission check switched off) at least one is refused; and the largest operand of operand_plan is the largest the engine emits."""
    abi_emulator.install(monkeypatch, _hip)
    cfg = {k: v for k, v in json.load(open(os.path.join(CONFIGS, name)))["model"].items() if k != "block_size"}
    cfg.setdefault("out_channels", cfg["in_channels"])
    m = ddpm_torch.UNet(**cfg)
    m.train()
    for dtype in ((torch.bfloat16, torch.float32) if size == 256 else (torch.bfloat16,)):
        m.set_compute_dtype(dtype)
        _plan_against_signatures(monkeypatch, m, m.engine(), size, size, f"{name} {dtype}")


# the topologies of tests/golden/make_engine_layout.py.  Two of them on a larger image than there, because at max_batch the path chooser
# (batch x heads > 65535) sends their attention to the materialised path, which refuses token counts that are no multiple of 8:
# four_equal_n3 at 32 x 16, not 16 x 8 (max_batch 131071, 2 tokens on level 3); two_all_options at 16 x 12, not 12 x 10 (max_batch 46603
# of two heads, 30 tokens on level 1; at 16 x 12 max_batch x 2 stays below 65536 and the head-indexed streaming kernels serve it).
SIZES = {"four_equal_n3": (32, 16), "two_all_options": (16, 12)}
TOPOLOGIES = [(case, dtype) for case in EL.CASES for dtype in (torch.bfloat16, torch.float32)
              if dtype == torch.bfloat16 or case in ("three_n2_rwc", "one_level")]


@pytest.mark.parametrize("case,dtype", TOPOLOGIES, ids=[f"{c}-{'bf16' if d == torch.bfloat16 else 'fp32'}" for c, d in TOPOLOGIES])
def test_plan_matches_the_signatures_on_other_topologies(monkeypatch, case, dtype):
    """The same on networks that are not the shipped ones: one level, four levels of three blocks with equal widths, conv-free
    resampling, every option on — at B = max_batch and max_batch + 1, where the activations decide (at a small B the weight operands
    are the largest, and the plan does not list them)."""
    abi_emulator.install(monkeypatch, _hip)
    cfg, _, H, W, labels = EL.CASES[case]
    H, W = SIZES.get(case, (H, W))
    m = ddpm_torch.UNet(**cfg)
    m.train()
    m.set_compute_dtype(dtype)
    _plan_against_signatures(monkeypatch, m, m.engine(), H, W, f"{case} {dtype}", labels=labels)


# ------------------------------------------------------------------------------------------- GroupNorm: the new refusal
def _gn_status(B, HW, C, x_ld, y_ld, bwd=False, dx_ld=None):
    fake, lib = 0x10000, _hip.lib()
    if bwd:
        return lib.ddpm_groupnorm_silu_bwd(fake, x_ld, fake, y_ld, fake, dx_ld or C, fake, fake, fake, fake, fake, fake, B, HW, C, 32, 1, 0.0, 0, 0, 0,
                                           0, 0, 0, 0, 1, 0)
    return lib.ddpm_groupnorm_silu_fwd(fake, x_ld, fake, y_ld, fake, fake, 0, fake, B, HW, C, 32, 1e-6, 1, 0.0, 0, 0, 1, 0)


def test_groupnorm_refuses_an_operand_of_2_31_elements_before_any_launch():
    """csrc/norm.hip gn_operand_ok: (B*HW - 1) * ld + C must stay below 2^31 elements for every operand.  Only refused sizes go through
    the launching entry (it returns before any launch); the largest admitted size is not launched here."""
    B, HW, C = 4, 1 << 20, 512                                  # dense: 2^31 elements exactly
    assert (B * HW - 1) * C + C == 1 << 31
    assert _gn_status(B, HW, C, C, C) == LR.ERR_SHAPE
    assert _gn_status(B, HW, C, C, C, bwd=True) == LR.ERR_SHAPE
    ld = -(-((1 << 31) - 64) // (3 * 192 - 1) // 8) * 8         # stretched: 576 rows of 64 channels, the last one ending past 2^31
    assert (3 * 192 - 1) * ld + 64 >= 1 << 31
    assert _gn_status(3, 192, 64, ld, 64) == LR.ERR_SHAPE and _gn_status(3, 192, 64, 64, ld) == LR.ERR_SHAPE
    assert _gn_status(3, 192, 64, 64, 64, bwd=True, dx_ld=ld) == LR.ERR_SHAPE and _gn_status(3, 192, 64, 64, ld, bwd=True) == LR.ERR_SHAPE
