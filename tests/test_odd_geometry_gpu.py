"""-m gpu: the HIP kernels and the UNet on non-square images and on pixel / token counts that are no power of two.

Every other GPU test of a geometry-dependent kernel passes square images with a power-of-two side, where tiles_x == tiles_y, Ho == Wo,
no GroupNorm iteration is ragged and a swapped H / W or a wrong row pitch is invisible.  Here:

  * every row of launch_replay.ODD_GEOMETRY — the smallest shapes at which each conv / weight-gradient kernel is still dispatched, the
    six GroupNorm forms with a ragged last iteration in both dtypes, the fused attention pair at L = 48 .. 240 — is replayed on fresh
    random inputs against the float64 restatement of include/ddpm_hip.h, every output element held to its own error-model bar
    (err/bar <= 1, the bars tests/launch_replay.py defines), after the dispatch query has named the kernel the table expects;
  * a reduced UNet (hid 64, multipliers [1, 2, 2], one res block, attention at 8 x 24 and in the middle block, dropout 0.1) runs
    forward + backward at B = 22 on 16 x 48 and 48 x 16 images against oracle.unet_ref with the bars of tests/test_unet_gpu.py and
    tests/test_configs_gpu.py (the errors of the square 32 x 32, B = 17 twin are printed next to them);
  * a 10-step ancestral chain on 48 x 16 in fp32: the graph-replayed loop equals the eager loop bit for bit and stays within FP32_BAR
    of oracle.diffusion_ref on the same noise.
The non-square workloads W14-W17 of launch_replay.WORKLOADS go through tests/test_step_launches_gpu.py.

Measured on the MI355X (worst err/bar per family; record + replay time as the workload test's summary line prints it):
  ODD_GEOMETRY, worst err/bar:  conv 0.249 (1x1, 24 x 16, C128 -> N192, residual)   weight gradients / reductions 0.249 (upsample2x_bwd)
                                GroupNorm 0.413 (backward, HW 144, C 512, bf16)      attention 0.437 (backward dk, L 80, C 128)
  workloads, worst err/bar and record + replay:  W14 0.445, 0.7 s   W15 0.480, 0.7 s   W16 0.249, 0.1 s   W17 0.431, 0.2 s
                                                 (W9 on the same machine: 2.5 s)
  reduced UNet, forward / worst gradient:  16 x 48 fp32 1.8e-6 / 3.5e-6, bf16 1.4e-2 / 3.0e-2;  48 x 16 fp32 1.7e-6 / 3.6e-6, bf16 1.4e-2 / 3.0e-2;
                                           32 x 32 twin fp32 1.8e-6 / 5.1e-6, bf16 1.2e-2 / 3.9e-2;  10-step chain 1.2e-6 of the oracle's.
What the rows found when they first ran: the fused attention pair was wrong (err/bar 3e2 .. 1.4e4) at every L whose padded length
Lpad = 96, 160 or 192 is no power of two — L = 80, 96, 144, 192, so also W14 and W16 and the bf16 UNet above (forward error 1.2 of the
output range) — because the score tile's XOR swizzle key min(Lpad / 8, 16) - 1 was no mask that maps a row's chunks onto themselves;
csrc/attention.hip carve() now takes the largest power of two that divides the row's chunk count (unchanged for Lpad = 32 .. 256 powers of two).
"""
import functools
import time

import pytest
import torch

import ddpm_torch
from oracle import diffusion_ref as D
from oracle import unet_ref as U
from tests import launch_replay as LR
from tests.golden.recipes import check, rnd
from tests.test_configs_gpu import _grad_report, _masks_from_tape
from tests.test_unet_gpu import DEV, FP32_BAR, make

pytestmark = pytest.mark.gpu

FAMILIES = {
    "conv": ("ddpm_conv2d_nhwc",),
    "wgrad": ("ddpm_conv3x3_wgrad_nhwc", "ddpm_conv3x3_wgrad_up_nhwc", "ddpm_conv2d_wgrad_nhwc", "ddpm_conv1x1_wgrad_nhwc",
              "ddpm_upsample2x_bwd", "ddpm_colsum"),
    "groupnorm": ("ddpm_groupnorm_silu_fwd", "ddpm_groupnorm_silu_bwd"),
    "attention": ("ddpm_attention_fwd_lse", "ddpm_attention_bwd"),
}
REDUCED = dict(in_channels=3, hid_channels=64, out_channels=3, ch_multipliers=[1, 2, 2], num_res_blocks=1, apply_attn=[False, True, False],
               drop_rate=0.1)


def test_every_odd_geometry_row_belongs_to_a_family():
    names = {n for fam in FAMILIES.values() for n in fam}
    assert {s[0] for s, _ in LR.ODD_GEOMETRY} == names


@pytest.mark.parametrize("family", list(FAMILIES))
def test_odd_geometry_rows_match_float64(family):
    t0 = time.perf_counter()
    rows, bad = [], []
    for i, (sig, variant) in enumerate(LR.ODD_GEOMETRY):
        if sig[0] not in FAMILIES[family]:
            continue
        got = LR.variant_of(sig)
        assert got == variant, f"{LR.short(sig)}: dispatched to {got}, the table names {variant}"
        r = LR.replay(sig, DEV, seed=i)
        rows.append((sig, variant, r))
        if r.worst > 1.0:
            bad.append(f"{LR.short(sig)}: {r.where} err/bar {r.worst:.3g}")
    assert rows
    print(f"\n== odd geometry, {family}: {len(rows)} replayed signatures")
    for sig, var, r in rows:
        print(f"  {LR.short(sig):<150s} v{'' if var is None else var:<3} {r.where:<10s} err/bar {r.worst:.3f}")
    worst = max(rows, key=lambda x: x[2].worst)
    print(f"odd geometry, {family}: worst err/bar {worst[2].worst:.3f} ({LR.short(worst[0])[:80]}, {worst[2].where}), "
          f"{time.perf_counter() - t0:.1f} s")
    assert not bad, f"{family}: {len(bad)} signature(s) beyond their bar:\n" + "\n".join(bad)


# ------------------------------------------------------------------------------------------------------------------ end to end
def _forward_backward_errors(B, H, W, dtype):
    """(forward error relative to the oracle's largest output, per-tensor gradient rows worst first) of the reduced UNet in train mode,
    the dropout masks the engine drew injected into the oracle."""
    m, sd = make(REDUCED, dtype=dtype)
    m.train()
    m.engine().debug_keep_tape = True
    x, gy = rnd(B, 3, H, W, seed=3), rnd(B, 3, H, W, seed=4)
    t = (torch.arange(B) * 47 + 5) % 1000
    y = m(x.to(DEV), t.to(DEV))
    (y * gy.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    masks = _masks_from_tape(m, REDUCED["drop_rate"])
    p = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    ref = U.unet_forward(p, REDUCED, x, t, training=True, masks=masks)
    (ref * gy).sum().backward()
    rel = float((y.detach().cpu() - ref.detach()).abs().max() / ref.detach().abs().max())
    rows, _ = _grad_report(m, p, 0.02 if dtype == torch.float32 else 0.1)
    return rel, rows


@functools.lru_cache(maxsize=None)
def _square_twin(dtype):
    return _forward_backward_errors(17, 32, 32, dtype)


@pytest.mark.parametrize("dtype,fwd_bar,grad_bar", [(torch.float32, FP32_BAR, 3e-3), (torch.bfloat16, 6e-2, 5e-2)], ids=["fp32", "bf16"])
@pytest.mark.parametrize("H,W", [(16, 48), (48, 16)])
def test_reduced_unet_forward_backward_vs_oracle(H, W, dtype, fwd_bar, grad_bar):
    """B = 22: level 0 has 16 896 pixels (the 16 x 16-patch kernels in 1 x 3 / 3 x 1 patches, both edge convs, the wave-specialised
    weight gradient), level 1 4224 (8 x 8 patches, attention over 192 tokens), level 2 is 4 x 12 / 12 x 4 (48 tokens).  Per-tensor
    gradient error relative to the tensor's largest gradient, floored at 2 % (fp32) / 10 % (bf16) of the median tensor scale."""
    rel, rows = _forward_backward_errors(22, H, W, dtype)
    rel_sq, rows_sq = _square_twin(dtype)
    print(f"\nreduced UNet {H}x{W} B=22 {dtype}: fwd rel {rel:.3e}; worst grads " + ", ".join(f"{k}={e:.2e}" for e, k in rows[:4]))
    print(f"  32x32 B=17 twin:                 fwd rel {rel_sq:.3e}; worst grads " + ", ".join(f"{k}={e:.2e}" for e, k in rows_sq[:4]))
    assert rel < fwd_bar, rel
    assert rows[0][0] < grad_bar, rows[:4]


def test_ancestral_chain_48x16_graph_equals_eager_and_matches_oracle(monkeypatch):
    """10 ancestral steps on 48 x 16 images in fp32: the hipGraph-replayed loop against the eager loop (bit for bit, on injected noise and
    on a device seed), and against oracle.diffusion_ref's loop over oracle.unet_ref on the same (x_T, z_1..z_10)."""
    cfg = dict(REDUCED, drop_rate=0.0)
    m, sd = make(cfg)
    m.eval()
    steps, shape = 10, (4, 3, 48, 16)
    dif = ddpm_torch.GaussianDiffusion(ddpm_torch.get_beta_schedule("linear", 1e-4, 0.02, steps), "eps", "fixed-large", "mse")
    g = torch.Generator("cpu").manual_seed(31)
    x_T = torch.empty(shape).normal_(generator=g)
    zs = [torch.empty(shape).normal_(generator=g) for _ in range(steps)]
    outs = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("DDPM_TORCH_AMD_GRAPH", mode)
        with torch.inference_mode():
            outs[mode] = dif._sample_loop(m, shape, DEV, x_T, None, z_stream=iter(zs))
        outs[mode + "s"] = dif.p_sample(m, shape=shape, device=DEV, seed=77)
    assert getattr(dif, "_sample_graphs", None), "the sampling step was not captured"
    assert torch.equal(outs["1"], outs["0"]), float((outs["1"] - outs["0"]).abs().max())
    assert torch.equal(outs["1s"], outs["0s"]), float((outs["1s"] - outs["0s"]).abs().max())
    T = D.ddpm_tables(D.beta_schedule("linear", 1e-4, 0.02, steps), "fixed-large")
    with torch.no_grad():
        ref = D.sample_loop(T, lambda x, t: U.unet_forward(sd, cfg, x, t), x_T, zs)
    err = check(outs["1"], ref, FP32_BAR, name="chain 48x16")
    print(f"\n10-step chain 48x16 fp32: rel err {err:.3e} vs oracle; graph == eager")
