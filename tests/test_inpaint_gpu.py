"""-m gpu: inpainting and image editing on the device — `ddpm_p_sample_step_masked` and `ddpm_q_jump` (csrc/inpaint.hip) against the entries
they are built from and against tests/inpaint_ref.py in float64 on the same fp32 inputs and fp32 tables, and ``GaussianDiffusion.inpaint`` /
``edit`` on the reduced UNet of tests/test_cond_gpu.py end to end: replayed against eager, both against the float64 RePaint chain.

Known answers (bit for bit) tie the new kernels to the old ones: a mask of 0 is `ddpm_p_sample_step` / `ddpm_p_sample_step_lv` on the same
inputs whatever ``x_known`` and ``e`` hold (NaN is planted there), a mask of 1 is the fp32 torch evaluation ``a * x_known + b * e`` whatever
``x_t``, ``model_out`` and ``z`` hold, a 0 / 1 checkerboard selects between the two per pixel across all channels, and `ddpm_q_jump` is the
fp32 torch evaluation of its expression.  Soft masks are held to the per-element bar derived in tests/inpaint_ref.py (a worst-case bound,
err / bar <= 1 for every element; the worst ratio is printed).

Networks: FP32_BAR = 1e-3 of the largest reference value, the project's bar for an fp32 network against the float64 oracle.  bf16: the
inpainting chain is allowed twice the error the plain ``p_sample`` chain of the same network and the same number of network calls shows
against its own float64 chain, measured in the same test (the factor 2 is how this project sets its other bf16 bars); both figures go to
profiles/inpaint.log.

Measured on the MI355X: soft masks at most 0.740 of the bar (a worst-case bound, not a multiple of a measured error); chains 7.1e-7
(T = 6, j = 2, r = 2), 7.6e-7 (DDIM-4, j = 1, r = 2), 7.3e-7 (conditional), 7.6e-7 (learned-range) of the float64 chain's largest value
(bar 1e-3); bf16 1.32e-2 beside the plain chain's 1.64e-2 (bar 3.28e-2).  The same figures are in DESIGN.md §4 "Inpainting and image
editing"."""
import functools
import json
import os
import sys

import pytest
import torch

import ddpm_torch
from ddpm_torch import _hip
from oracle import diffusion_ref as D
from oracle import unet_ref as U
from tests import cond_ref as CR
from tests import inpaint_ref as R
from tests import learned_var_ref as LR
from tests.golden.recipes import check
from tests.test_cond_gpu import FP32_BAR, REDUCED, Guarded, bits, model_of, weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "ddpm-torch_amd")
if PKG not in sys.path:
    sys.path.insert(0, PKG)
import ddim  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
T_STEP = 1000
MEAN = ("sqrt_recip_alphas_bar", "sqrt_recip_m1_alphas_bar", "posterior_mean_coef1", "posterior_mean_coef2")
PREV = ("sqrt_alphas_bar_prev", "sqrt_one_minus_alphas_bar_prev")


def r(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


# ------------------------------------------------------------------------------------------------------------------ tables
@functools.lru_cache(maxsize=None)
def tabs64():
    """fp32-rounded tables carried in float64: what the kernels read, as the float64 reference reads it."""
    tb = LR.tables(D.beta_schedule("linear", 1e-4, 0.02, T_STEP))
    tb["fixed_model_logvar"] = tb["model_logvar_max"]
    ka, kb = R.prev_tables(torch.cumprod(1.0 - D.beta_schedule("linear", 1e-4, 0.02, T_STEP), 0))
    tb[PREV[0]], tb[PREV[1]] = ka.float().double(), kb.float().double()
    return tb


@functools.lru_cache(maxsize=None)
def dev_tab(name):
    return tabs64()[name].float().to(DEV)


def masked_tables(var_mode):
    lo = {0: "fixed_model_logvar", 1: None, 2: "posterior_logvar_clipped"}[var_mode]
    hi = "model_logvar_max" if var_mode == 2 else None
    return [dev_tab(k).data_ptr() for k in MEAN] + [dev_tab(k).data_ptr() if k else 0 for k in (lo, hi)] + [dev_tab(k).data_ptr() for k in PREV]


# ------------------------------------------------------------------------------------------------------------------ ddpm_p_sample_step_masked
VARIANTS = ((0, 1), (0, 2), (1, 2), (2, 2))                  # (var_mode, row pitch of the network output in units of n)


@functools.lru_cache(maxsize=None)
def step_case(B, C, hw, t):
    g = dict(B=B, C=C, hw=hw, n=C * hw, t=torch.tensor(t))
    g["xt"], g["out2"], g["z"] = r(B, C, hw, seed=hw + 1), r(B, 2 * C, hw, seed=hw + 2) * 0.8, r(B, C, hw, seed=hw + 3)
    g["xk"], g["e"] = torch.rand(B, C, hw, generator=torch.Generator().manual_seed(hw + 4)) * 2 - 1, r(B, C, hw, seed=hw + 5)
    g["out1"] = g["out2"][:, :C].contiguous()
    return g


class Inputs:
    """The guarded device copies of a case's inputs (and an all-NaN twin of each) at one offset from the 16-byte grid."""

    def __init__(self, c, offset):
        mk = lambda key: Guarded(tuple(c[key].shape), values=c[key], offset=offset)          # noqa: E731
        self.c = c
        self.g = {key: mk(key) for key in ("xt", "out1", "out2", "z", "xk", "e")}
        self.nan = {key: Guarded(tuple(c[key].shape), offset=offset) for key in ("xt", "out1", "out2")}
        self.offset = offset

    def check_intact(self):
        assert all(g.intact() for g in self.g.values()) and all(g.intact() for g in self.nan.values()), "a guard region was written"
        assert all(bits(g.t.cpu(), self.c[key]) for key, g in self.g.items()), "an input was written"
        assert all(bool(torch.isnan(g.t).all()) for g in self.nan.values())


def run_masked(inp, mask, mean_type, clip, var_mode, pitch, t=None, inplace=False, plant=None):
    """One launch.  ``plant``: "known" puts NaN into x_known and e, "step" into x_t, model_out and z."""
    c = inp.c
    B, n, hw = c["B"], c["n"], c["hw"]
    pick = lambda key, planted: (inp.nan[{"z": "xt", "xk": "xt", "e": "xt"}.get(key, key)] if planted else inp.g[key]).t        # noqa: E731
    out_key = "out1" if pitch == 1 else "out2"
    x = pick("xt", plant == "step")
    if inplace:
        own = Guarded(tuple(x.shape), values=x, offset=inp.offset)
        x, dst = own.t, own
    else:
        dst = Guarded(tuple(x.shape), offset=inp.offset)
    mk = Guarded(tuple(mask.shape), values=mask, offset=inp.offset)
    tt = (c["t"] if t is None else t).to(DEV)
    _hip.call("ddpm_p_sample_step_masked", x.data_ptr(), pick(out_key, plant == "step").data_ptr(), pick("z", plant == "step").data_ptr(),
              pick("xk", plant == "known").data_ptr(), pick("e", plant == "known").data_ptr(), mk.t.data_ptr(), tt.data_ptr(), *masked_tables(var_mode),
              dst.t.data_ptr(), B, n, hw, mask.shape[0], pitch * n, mean_type, clip, var_mode, T_STEP, _hip.stream())
    torch.cuda.synchronize()
    assert dst.intact() and mk.intact() and bits(mk.t.cpu(), mask), "a guard region or the mask was written"
    inp.check_intact()
    return dst.t.cpu()


def run_plain(inp, mean_type, clip, var_mode, pitch):
    """`ddpm_p_sample_step` (rows of n) / `ddpm_p_sample_step_lv` (rows of 2n) on the same inputs."""
    c = inp.c
    B, n = c["B"], c["n"]
    x, z, tt = inp.g["xt"].t, inp.g["z"].t, c["t"].to(DEV)
    dst = torch.empty_like(x)
    tb = masked_tables(var_mode)
    if pitch == 1:
        _hip.call("ddpm_p_sample_step", x.data_ptr(), inp.g["out1"].t.data_ptr(), z.data_ptr(), tt.data_ptr(), *tb[:5], dst.data_ptr(), 0, B, n, mean_type,
                  clip, T_STEP, _hip.stream())
    else:
        _hip.call("ddpm_p_sample_step_lv", x.data_ptr(), inp.g["out2"].t.data_ptr(), z.data_ptr(), tt.data_ptr(), *tb[:6], dst.data_ptr(), 0, B, n, mean_type,
                  clip, var_mode, T_STEP, _hip.stream())
    return dst.cpu()


def renoised(c, t=None):
    """a * x_known + b * e in fp32 on the CPU: two products and a sum, each rounded."""
    t = c["t"] if t is None else t
    a, b = tabs64()[PREV[0]].float()[t][:, None, None], tabs64()[PREV[1]].float()[t][:, None, None]
    return a * c["xk"] + b * c["e"]


def masks_of(rows, hw, seed):
    g = torch.Generator().manual_seed(seed)
    board = ((torch.arange(hw)[None, :] + torch.arange(rows)[:, None]) % 2).float()
    soft = {"0.25": torch.full((rows, hw), 0.25), "0.5": torch.full((rows, hw), 0.5), "random": torch.rand(rows, hw, generator=g)}
    return torch.zeros(rows, hw), torch.ones(rows, hw), board, soft


WORST = {"ratio": 0.0}


@pytest.mark.parametrize("per_sample", [False, True])
@pytest.mark.parametrize("C,hw", [(1, 1), (3, 1), (1, 3), (3, 5), (3, 63), (3, 64), (3, 65), (3, 480), (1, 3072)])
@pytest.mark.parametrize("B", [1, 3])
def test_masked_step_known_answers_and_float64(B, C, hw, per_sample):
    """Every mean type, clip on and off, var_mode 0 / 1 / 2, rows of n and of 2n floats, t = 0 and T - 1 among the samples (B = 1: each in
    turn).  hw % 4 != 0, a per-sample mask row off the grid and a base one float off the 16-byte grid take the element-wise path: the bit
    comparisons hold on both."""
    rows = B if per_sample else 1
    zero, one, board, soft = masks_of(rows, hw, seed=B * hw)
    pix = lambda m: m[:, None, :].expand(B, C, hw)                                          # noqa: E731  (one row for the batch, or one per sample)
    for t in ([(0,), (T_STEP - 1,)] if B == 1 else [(0, 1, T_STEP - 1)]):
        c = step_case(B, C, hw, t)
        inp, off = Inputs(c, 0), Inputs(c, 1)
        known = renoised(c)
        x64 = {k: c[k].double() for k in ("xt", "out1", "out2", "z", "xk", "e")}
        for mean_type in range(3):
            for clip in (0, 1):
                for var_mode, pitch in VARIANTS:
                    tag = (t, mean_type, clip, var_mode, pitch)
                    plain = run_plain(inp, mean_type, clip, var_mode, pitch)
                    got0 = run_masked(inp, zero, mean_type, clip, var_mode, pitch, plant="known")
                    assert bits(got0, plain), ("a mask of 0 is the plain step", tag)
                    got1 = run_masked(inp, one, mean_type, clip, var_mode, pitch, plant="step")
                    assert bits(got1, known), ("a mask of 1 is a * x_known + b * e", tag)
                    at0 = c["t"] == 0
                    assert torch.equal(got1[at0], c["xk"][at0]), ("at t = 0 the known region is the source itself", tag)
                    gotb = run_masked(inp, board, mean_type, clip, var_mode, pitch)
                    assert bits(gotb, torch.where(pix(board) == 1, known, plain)), ("a 0 / 1 mask selects per pixel, across all channels", tag)
                    assert bits(run_masked(off, board, mean_type, clip, var_mode, pitch), gotb), ("a base off the 16-byte grid", tag)
                    out64 = x64["out1"] if pitch == 1 else x64["out2"]
                    for name, m in soft.items():
                        got = run_masked(inp, m, mean_type, clip, var_mode, pitch)
                        args = (tabs64(), x64["xt"], c["t"], out64, x64["z"], x64["xk"], x64["e"], m.double(), bool(clip))
                        ref = R.masked_step(args[0], R.MEAN_TYPES[mean_type], R.VAR_TYPES[var_mode], *args[1:])
                        bar = R.masked_bar(args[0], mean_type, var_mode, *args[1:])
                        ratio = float(((got.double() - ref).abs() / bar.clamp_min(1e-300)).max())
                        WORST["ratio"] = max(WORST["ratio"], ratio)
                        assert ratio <= 1.0, (name, tag, ratio)
                        if name == "random":
                            assert bits(run_masked(inp, m, mean_type, clip, var_mode, pitch, inplace=True), got), ("in place", tag)
                            assert bits(run_masked(off, m, mean_type, clip, var_mode, pitch), got), ("off the grid", tag)
    print(f"\n  B={B} C={C} hw={hw} mask rows={rows}: worst err/bar so far {WORST['ratio']:.3f}")


@pytest.mark.parametrize("C,hw", [(3, 1), (3, 64), (3, 65), (3, 480)])
def test_masked_step_bad_t_poisons_its_own_sample_only(C, hw):
    c = step_case(3, C, hw, (0, 1, T_STEP - 1))
    inp = Inputs(c, 0)
    m = masks_of(3, hw, seed=1)[3]["random"]
    for var_mode, pitch in ((0, 1), (2, 2)):
        good = run_masked(inp, m, 0, 1, var_mode, pitch)
        for bad in (-1, T_STEP, 1 << 40):
            t = c["t"].clone()
            t[1] = bad
            got = run_masked(inp, m, 0, 1, var_mode, pitch, t=t)
            assert bool(torch.isnan(got[1]).all()) and bits(got[[0, 2]], good[[0, 2]])


# ------------------------------------------------------------------------------------------------------------------ ddpm_q_jump
@pytest.mark.parametrize("n", [1, 3, 5, 771, 3072])
@pytest.mark.parametrize("B", [1, 3])
def test_q_jump_is_the_fp32_expression_in_place_off_grid_and_with_a_bad_t(B, n):
    S, j = 50, 10
    ab = torch.cumprod(1.0 - D.beta_schedule("linear", 1e-4, 0.02, 1000), 0)[D.selection_schedule("linear", S, 1000)]
    ja, jb = (v.float() for v in R.jump_tables(ab, j))
    jad, jbd = ja.to(DEV), jb.to(DEV)
    x, z = r(B, n, seed=n), r(B, n, seed=n + 1)
    t = torch.tensor([S - 1, j - 1, 30][:B])
    want = ja[t][:, None] * x + jb[t][:, None] * z

    def run(tt, offset=0, inplace=False):
        xs, zs = Guarded((B, n), values=x, offset=offset), Guarded((B, n), values=z, offset=offset)
        dst = xs if inplace else Guarded((B, n), offset=offset)
        td = tt.to(DEV)
        _hip.call("ddpm_q_jump", xs.t.data_ptr(), zs.t.data_ptr(), td.data_ptr(), jad.data_ptr(), jbd.data_ptr(), dst.t.data_ptr(), B, n, S, _hip.stream())
        torch.cuda.synchronize()
        assert xs.intact() and zs.intact() and dst.intact() and bits(zs.t.cpu(), z) and (inplace or bits(xs.t.cpu(), x))
        return dst.t.cpu()

    got = run(t)
    assert bits(got, want) and bits(run(t, inplace=True), got) and bits(run(t, offset=1), got) and bits(run(t, offset=1, inplace=True), got)
    for bad in (-1, S, 1 << 40, j - 2):                                                      # (j - 2: inside the table, where its entries are NaN)
        tb = t.clone()
        tb[B // 2] = bad
        gb = run(tb)
        keep = [b for b in range(B) if b != B // 2]
        assert bool(torch.isnan(gb[B // 2]).all()) and bits(gb[keep], got[keep])


# ------------------------------------------------------------------------------------------------------------------ the engine
SHAPE = (3, 3, 16, 16)
H = W = 16


def half_mask():
    m = torch.zeros(H, W)
    m[:, :W // 2] = 1
    return m


def per_sample_mask():
    m = half_mask()
    c = torch.ones(H, W)
    c[4:12, 4:12] = 0
    return torch.stack([m, m.t().contiguous(), c])[:, None]


def source():
    return torch.rand(SHAPE, generator=torch.Generator().manual_seed(8)) * 2 - 1


def draws(ops, seed=41):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(SHAPE, generator=g) for _ in range(1 + sum(2 if op == "down" else 1 for op in ops))]


ROWS = {
    #            sampler, T, DDIM size, j, r, mask,            network
    "ddpm":     ("ddpm", 6, None, 2, 2, "half", "plain"),
    "ddim4":    ("ddim", 8, 4, 1, 2, "per-sample", "plain"),
    "cond":     ("ddpm", 6, None, 2, 2, "half", "cond"),
    "range":    ("ddpm", 6, None, 2, 2, "per-sample", "learned-range"),
}
LABELS = (2, 0, 1)


@functools.lru_cache(maxsize=None)
def weights_2c():
    from tests.test_learned_var_gpu import REDUCED as REDUCED_2C
    torch.manual_seed(5)
    sd = U.randomize_state_dict(ddpm_torch.UNet(**REDUCED_2C).state_dict(), 17)
    return REDUCED_2C, sd, {k: v.double() for k, v in sd.items()}


def process_of(row):
    sampler, T, size, j, r_, _, net = ROWS[row]
    betas = ddpm_torch.get_beta_schedule("linear", 1e-4, 0.02, T)
    if sampler == "ddim":
        return ddim.DDIM(betas, "eps", "fixed-small", "mse", eta=0.0, subsequence=ddim.get_selection_schedule("linear", size=size, timesteps=T))
    return ddpm_torch.GaussianDiffusion(betas, "eps", "learned-range" if net == "learned-range" else "fixed-large", "hybrid" if net == "learned-range" else "mse")


def network_of(row, dtype=torch.float32):
    net = ROWS[row][6]
    if net == "learned-range":
        cfg, sd, _ = weights_2c()
        m = ddpm_torch.UNet(**cfg)
        m.load_state_dict(sd)
        return m.to(DEV).set_compute_dtype(dtype).eval()
    return model_of(weights()[0], dtype, conditional=net == "cond").eval()


def mask_of(row):
    return half_mask() if ROWS[row][5] == "half" else per_sample_mask()


@functools.lru_cache(maxsize=None)
def chain_reference(row):
    """The float64 RePaint chain of a row on the oracle UNet, once."""
    sampler, T, size, j, r_, _, net = ROWS[row]
    betas = D.beta_schedule("linear", 1e-4, 0.02, T)
    sub = D.selection_schedule("linear", size, T) if sampler == "ddim" else None
    S = T if sub is None else size
    ops = R.schedule(S, j, r_)
    dr = draws(ops)
    if net == "learned-range":
        cfg, _, sd64 = weights_2c()
        tb, var_type = LR.tables(betas), "learned-range"
        tb = {k: v for k, v in tb.items()}
        tb["alphas_bar"] = torch.cumprod(1.0 - betas, 0)
        fn = lambda x, t: U.unet_forward(sd64, cfg, x, t)                                    # noqa: E731
    else:
        tb, var_type = (D.ddim_tables(betas, "fixed-small", 0.0, sub) if sub is not None else D.ddpm_tables(betas, "fixed-large")), None
        sd64 = weights()[1]
        if net == "cond":
            y = torch.tensor(LABELS)
            fn = lambda x, t: CR.unet_forward(sd64, REDUCED, x, t, y)                        # noqa: E731
        else:
            plain64 = {k: v for k, v in sd64.items() if k != CR.TABLE}
            fn = lambda x, t: U.unet_forward(plain64, REDUCED, x, t)                         # noqa: E731
    with torch.no_grad():
        ref = R.chain(R.with_prev(tb), "eps", var_type, fn, source().double(), mask_of(row).double().reshape(-1, H * W), [d.double() for d in dr],
                      j=j, r=r_, timestep_map=sub)
    return ops, dr, ref


def kinds_of(proc):
    return {k[3][3] for k in getattr(proc, "_sample_graphs", {}) if len(k[3]) > 3}


@pytest.mark.parametrize("row", list(ROWS))
def test_inpainting_chain_replayed_equals_eager_and_matches_the_float64_chain(row, monkeypatch):
    """B = 3, 16 x 16, injected draws: the replayed chain equals the eager one bit for bit (with injected draws and with a seed), both are
    within FP32_BAR of the float64 chain, the known region is the source exactly, and the two graphs sit in the cache under their own kind."""
    _, T, size, j, r_, _, net = ROWS[row]
    ops, dr, ref = chain_reference(row)
    proc, m = process_of(row), network_of(row)
    x0, mask = source().to(DEV), mask_of(row)
    kw = dict(jump_length=j, resamples=r_)
    if net == "cond":
        kw["y"] = torch.tensor(LABELS, device=DEV)
    outs = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("DDPM_TORCH_AMD_GRAPH", mode)
        outs[mode] = proc.inpaint(m, x0, mask, z_stream=iter(dr), **kw)
        outs[mode + "s"] = proc.inpaint(m, x0, mask, seed=77, **kw)
    rows = 1 if mask.ndim == 2 else mask.shape[0]
    kind = ("inpaint", j, rows, ("cond",) if net == "cond" else None)
    assert kind in kinds_of(proc), (kind, kinds_of(proc))
    assert outs["1"].shape == SHAPE and outs["1"].dtype == torch.float32
    assert torch.equal(outs["1"], outs["0"]) and torch.equal(outs["1s"], outs["0s"]) and not torch.equal(outs["1"], outs["1s"])
    err = check(outs["1"], ref, FP32_BAR, name=row)
    keep = (mask.reshape(-1, 1, H, W) == 1).expand(SHAPE)
    for out in outs.values():
        assert torch.equal(out.cpu()[keep], x0.cpu()[keep]), "the known region is the source image"
        assert bool(torch.isfinite(out).all())
    print(f"\n  {row}: {ops.count('down')} network calls, {ops.count('up')} jumps, rel err {err:.3e}")
    if row == "ddpm":
        # the cached inpainting entry is not served to p_sample (which captures its own step), and edit is inpaint with a zero mask
        monkeypatch.setenv("DDPM_TORCH_AMD_GRAPH", "1")
        before = len(proc._sample_graphs)
        a = proc.p_sample(m, shape=SHAPE, device=DEV, seed=5)
        assert len(proc._sample_graphs) == before + 1
        monkeypatch.setenv("DDPM_TORCH_AMD_GRAPH", "0")
        assert torch.equal(a, proc.p_sample(m, shape=SHAPE, device=DEV, seed=5))
        for mode in ("1", "0"):
            monkeypatch.setenv("DDPM_TORCH_AMD_GRAPH", mode)
            start = T - 2
            g = torch.Generator(DEV).manual_seed(9)
            ed = [torch.empty(SHAPE, device=DEV).normal_(generator=g)]
            for _ in range(start + 1):
                ed += [torch.empty(SHAPE, device=DEV).normal_(generator=g), torch.zeros(SHAPE, device=DEV)]
            edited = proc.edit(m, x0, start, seed=9)
            assert torch.equal(edited, proc.inpaint(m, x0, torch.zeros(H, W), start=start, z_stream=iter(ed))), mode
            outs["e" + mode] = edited
        assert torch.equal(outs["e1"], outs["e0"])


def test_bf16_chain_against_twice_the_plain_chains_own_error(monkeypatch):
    """bf16 compute: replayed equals eager, the known region is exact, everything is finite, and the error against the float64 chain is at
    most twice what the plain ``p_sample`` chain of the same network with the same number of network calls (T = 10) shows against its own
    float64 chain.  Both figures are written to profiles/inpaint.log."""
    ops, dr, ref = chain_reference("ddpm")
    calls = ops.count("down")
    m = network_of("ddpm", torch.bfloat16)
    x0, mask = source().to(DEV), half_mask()
    proc = process_of("ddpm")
    outs = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("DDPM_TORCH_AMD_GRAPH", mode)
        outs[mode] = proc.inpaint(m, x0, mask, jump_length=2, resamples=2, z_stream=iter(dr))
    assert torch.equal(outs["1"], outs["0"]) and bool(torch.isfinite(outs["1"]).all())
    keep = (mask == 1).expand(SHAPE)
    assert torch.equal(outs["1"].cpu()[keep], x0.cpu()[keep])
    # the yardstick: the plain chain of the parent code, bf16 against float64, on `calls` network calls
    betas = D.beta_schedule("linear", 1e-4, 0.02, calls)
    g = torch.Generator().manual_seed(43)
    x_T, zs = torch.randn(SHAPE, generator=g), torch.randn((calls,) + SHAPE, generator=g)
    plain64 = {k: v for k, v in weights()[1].items() if k != CR.TABLE}
    with torch.no_grad():
        ref_plain = D.sample_loop(D.ddpm_tables(betas, "fixed-large"), lambda x, t: U.unet_forward(plain64, REDUCED, x, t), x_T.double(), zs.double())
    plain = ddpm_torch.GaussianDiffusion(ddpm_torch.get_beta_schedule("linear", 1e-4, 0.02, calls), "eps", "fixed-large", "mse")
    monkeypatch.setenv("DDPM_TORCH_AMD_GRAPH", "1")
    with torch.inference_mode():
        got_plain = plain._sample_loop(m, SHAPE, DEV, x_T, None, z_stream=iter(zs))
    rel = lambda a, b: float((a.cpu().double() - b).abs().max() / b.abs().max())             # noqa: E731
    err_plain, err = rel(got_plain, ref_plain), rel(outs["1"], ref)
    line = json.dumps({"network_calls": calls, "plain_p_sample_bf16_rel_err": err_plain, "inpaint_bf16_rel_err": err, "bar": 2 * err_plain,
                       "device": torch.cuda.get_device_name(0)})
    print("\n  " + line)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "inpaint.log"), "w") as f:
        f.write("bf16 inpainting chain (T = 6, j = 2, r = 2, reduced UNet, B = 3, 16 x 16) against the float64 chain, beside the plain p_sample chain of the\n"
                "same network and the same number of network calls against its own float64 chain (tests/test_inpaint_gpu.py; relative to the reference's\n"
                "largest value; the bar is twice the plain chain's error)\n" + line + "\n")
    assert err <= 2 * err_plain, (err, err_plain)


def test_generate_inpaint_center_on_the_device(tmp_path):
    import importlib
    import numpy as np
    from PIL import Image
    cfg = {"dataset": "cifar10",
           "diffusion": {"timesteps": 40, "beta_start": 1e-4, "beta_end": 0.02, "beta_schedule": "linear", "model_mean_type": "eps",
                         "model_var_type": "fixed-large", "loss_type": "mse"},
           "model": {"in_channels": 3, "hid_channels": 32, "ch_multipliers": [1, 2], "num_res_blocks": 1, "apply_attn": [False, True], "drop_rate": 0.0}}
    (tmp_path / "tiny.json").write_text(json.dumps(cfg))
    torch.manual_seed(0)
    net = ddpm_torch.UNet(out_channels=3, **cfg["model"])
    torch.save(U.randomize_state_dict(net.state_dict(), 3), tmp_path / "tiny.pt")
    src = tmp_path / "src.pt"
    torch.save(torch.randint(0, 256, (3, 3, 32, 32), dtype=torch.uint8, generator=torch.Generator().manual_seed(0)), src)
    gen = importlib.import_module("generate")
    out = gen.main(["--config-path", str(tmp_path / "tiny.json"), "--device", DEV, "--chkpt-path", str(tmp_path / "tiny.pt"), "--use-ddim", "--subseq-size", "8",
                    "--compute", "fp32", "--inpaint", "center", "--source", str(src), "--batch-size", "2", "--seed", "3", "--jump-length", "2",
                    "--resamples", "2", "--save-dir", str(tmp_path / "out")])
    assert sorted(os.listdir(out)) == ["inpaint_00000.png", "inpaint_00001.png", "inpaint_00002.png"]
    im = np.asarray(Image.open(os.path.join(out, "inpaint_00001.png")))
    assert im.shape == (36, 3 * 34 + 2, 3)
    a, b, c = (im[2:34, 2 + 34 * k:34 + 34 * k] for k in range(3))
    keep = np.ones((32, 32), dtype=bool)
    keep[8:24, 8:24] = False
    assert np.array_equal(a[keep], b[keep]) and np.array_equal(a[keep], c[keep]) and (b[~keep] == 128).all() and not np.array_equal(a[~keep], c[~keep])
