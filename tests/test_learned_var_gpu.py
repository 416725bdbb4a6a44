"""-m gpu: the learned reverse-process variance — `ddpm_p_sample_step_lv`, `ddpm_vlb_terms_lv`, `ddpm_bpd_terms_lv`, `ddpm_learned_loss`
(csrc/elementwise.hip) against tests/learned_var_ref.py in float64 on the same fp32 inputs and fp32 tables, and
``GaussianDiffusion(model_var_type="learned" | "learned-range")`` end to end on the reduced UNet of tests/test_odd_geometry_gpu.py with
``out_channels = 2C``: sampling and bits/dim graph-replayed against eager, three hybrid ``Trainer.step``s eager against launch plan,
DDIM on the 2C-channel model.

Inputs of the kernel tests are those of tests/test_bpd_gpu.py (its module docstring says why): the mean half of the network output is the
exact target of its parameterisation plus a perturbation that moves the model mean by 0.3 sigma_t per unit normal (capped at 0.05); row 0
carries the four tail values of G16.  The v half: var_mode 2, 0.8 x a unit normal (so f leaves [0, 1]); var_mode 1, the middle of
[lv_min, lv_max] at the sample's t plus 0.3 x a unit normal.

Bars, derived as tests/test_bpd_gpu.py derives its own — from the float64 reference and from the fp32 torch evaluation of the same
reference, with that file's margin of 8:
  per-sample values (loss, losses, mses columns): per entry the larger of 5e-5 x max |ref| over the tensor (the `losses` figure of
      test_bpd_gpu) and 8 x |ref32 - ref64| of that entry;
  per-element outputs (x_prev, pred_x0, both gradient halves): per ROW the larger of 2e-5 x the row's max |ref| (the `mses` figure) and
      8 x the row's max |ref32 - ref64|.  Per row, not per element: d = true_mean - model_mean is a difference of O(1) numbers of size
      0.3 sigma_t ~ 2e-3 at t = 1, so a gradient element carries ~3e-5 of relative rounding noise that the kernel and torch draw
      independently; element by element the torch draw is no bound for the kernel's.
Known answers (bit for bit) tie the new kernels to the fixed-variance ones; see each test.
Measured on the MI355X, worst err / bar over every kernel case of this file: per-row outputs 0.151 (mean-half gradient of kl, n = 768,
T = 8; x_prev 0.010, pred_x0 0.138, d/dv 0.133), per-sample values 0.125 (the decoder tails / floor case; 0.004 elsewhere, mses 0.012).
End to end: chain 3.0e-6 / 6.1e-7 of the oracle's largest value (learned / learned-range), bits/dim outputs <= 4.6e-7.  The same figures
are in DESIGN.md §4 "Learned reverse-process variance".
"""
import functools

import pytest
import torch

import ddpm_torch
from ddpm_torch import _hip
from oracle import diffusion_ref as D
from oracle import unet_ref as U
from tests import learned_var_ref as R
from tests.golden.recipes import check, check_state

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FP32_BAR = 1e-3                       # tests/test_unet_gpu.py: the project's bar for an fp32 network against the float64 oracle
MEAN = ("sqrt_recip_alphas_bar", "sqrt_recip_m1_alphas_bar", "posterior_mean_coef1", "posterior_mean_coef2")
LV = MEAN + ("posterior_logvar_clipped", "model_logvar_max")
SHAPES = {"n35": (3, 35), "n768": (5, 768), "n16640": (2, 16640)}          # (B, C*H*W) of (3,1,5,7), (5,3,16,16), (2,1,128,130)
NAN = float("nan")


def r(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


@functools.lru_cache(maxsize=None)
def tabs64(T):
    """fp32-rounded tables carried in float64, with both fixed log-variance tables under the names the old kernels' callers use."""
    betas = D.beta_schedule("linear", 1e-4, 0.02, T)
    tb = R.tables(betas)
    tb["fixed-large"], tb["fixed-small"] = tb["model_logvar_max"], tb["posterior_logvar_clipped"]
    return tb


def tabs_as(T, dtype):
    return {k: (v.to(dtype) if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in tabs64(T).items()}


@functools.lru_cache(maxsize=None)
def dev_tabs(T, names):
    return [tabs64(T)[k].float().to(DEV) for k in names]


@functools.lru_cache(maxsize=None)
def case(key, T, var_mode):
    """Inputs shared by every test of one geometry (never modified)."""
    B, n = SHAPES[key]
    f = tabs_as(T, torch.float32)
    t = {3: [0, 1, T - 1], 5: [0, 0, 1, T // 2, T - 1], 2: [0, T - 1]}[B]
    t = torch.tensor(t)
    x0 = (r(B, n, seed=1) * 0.5).clamp(-1, 1)
    x0[0, :4] = torch.tensor([1.0, -1.0, 0.9995, -0.9995])
    noise, z = r(B, n, seed=2), r(B, n, seed=3)
    xt = f["sqrt_alphas_bar"][t][:, None] * x0 + f["sqrt_one_minus_alphas_bar"][t][:, None] * noise
    c1, c2, rm1 = (f[k][t][:, None] for k in ("posterior_mean_coef1", "posterior_mean_coef2", "sqrt_recip_m1_alphas_bar"))
    lmin, lmax = f["posterior_logvar_clipped"][t][:, None], f["model_logvar_max"][t][:, None]
    sigma = torch.exp(0.5 * lmax)
    pert = r(B, n, seed=7)
    v = 0.8 * r(B, n, seed=8) if var_mode != 1 else 0.5 * (lmin + lmax) + 0.3 * r(B, n, seed=8)
    outs, targets = {}, {}
    for mt, target, gain in (("eps", noise, c1 * rm1), ("x_0", x0, c1), ("mean", c1 * x0 + c2 * xt, torch.ones_like(c1))):
        targets[mt] = target.contiguous()
        outs[mt] = torch.cat([target + torch.minimum(0.3 * sigma / gain, torch.full_like(sigma, 0.05)) * pert, v], dim=1).contiguous()
    return dict(t=t, x0=x0, xt=xt, z=z, outs=outs, targets=targets, B=B, n=n, T=T)


def on_dev(x, offset=0):
    """A device copy whose base address is ``offset`` floats past a 16-byte boundary."""
    if not offset:
        return x.to(DEV).contiguous()
    buf = torch.empty(x.numel() + 4, dtype=x.dtype, device=DEV)
    view = buf[offset:offset + x.numel()].view(x.shape)
    view.copy_(x)
    return view


# ------------------------------------------------------------------------------------------------------------------ launchers
def step_lv(c, out, mean_type, clip, var_mode, t=None, inplace=False, tables=None, want_pred=True, offset=0):
    T = c["T"]
    x_t, o, z = on_dev(c["xt"]).clone(), on_dev(out, offset), on_dev(c["z"])
    tt = on_dev(c["t"] if t is None else t)
    if tables is None:
        tables = dev_tabs(T, LV) if var_mode else dev_tabs(T, MEAN + ("fixed-large",)) + [None]
    x_prev = x_t if inplace else torch.full_like(x_t, NAN)
    pred = torch.full_like(x_t, NAN) if want_pred else None
    _hip.call("ddpm_p_sample_step_lv", x_t.data_ptr(), o.data_ptr(), z.data_ptr(), tt.data_ptr(), *[_hip.ptr(v) for v in tables], x_prev.data_ptr(),
              _hip.ptr(pred), c["B"], c["n"], mean_type, clip, var_mode, T, _hip.stream())
    return x_prev.cpu(), (pred.cpu() if want_pred else None)


def step_old(c, out_mean, mean_type, clip, logvar_name):
    T = c["T"]
    x_t, o, z, tt = on_dev(c["xt"]), on_dev(out_mean), on_dev(c["z"]), on_dev(c["t"])
    x_prev, pred = torch.empty_like(x_t), torch.empty_like(x_t)
    _hip.call("ddpm_p_sample_step", x_t.data_ptr(), o.data_ptr(), z.data_ptr(), tt.data_ptr(), *[v.data_ptr() for v in dev_tabs(T, MEAN + (logvar_name,))],
              x_prev.data_ptr(), pred.data_ptr(), c["B"], c["n"], mean_type, clip, T, _hip.stream())
    return x_prev.cpu(), pred.cpu()


def vlb_lv(c, out, mean_type, clip, var_mode, t=None, offset=0):
    x0, xt, o, tt = on_dev(c["x0"]), on_dev(c["xt"]), on_dev(out, offset), on_dev(c["t"] if t is None else t)
    loss, pred = torch.full((c["B"],), NAN, device=DEV), torch.full_like(x0, NAN)
    _hip.call("ddpm_vlb_terms_lv", x0.data_ptr(), xt.data_ptr(), o.data_ptr(), tt.data_ptr(), *[v.data_ptr() for v in dev_tabs(c["T"], LV)],
              loss.data_ptr(), pred.data_ptr(), c["B"], c["n"], mean_type, clip, var_mode, c["T"], _hip.stream())
    return loss.cpu(), pred.cpu()


def bpd_lv(c, out, mean_type, clip, var_mode, t=None, offset=0):
    """One launch on NaN-filled [B, ld] tables -> (losses, mses) on the host."""
    ld = c["T"] + 8
    x0, xt, o, tt = on_dev(c["x0"]), on_dev(c["xt"]), on_dev(out, offset), on_dev(c["t"] if t is None else t)
    losses, mses = torch.full((c["B"], ld), NAN, device=DEV), torch.full((c["B"], ld), NAN, device=DEV)
    _hip.call("ddpm_bpd_terms_lv", x0.data_ptr(), xt.data_ptr(), o.data_ptr(), tt.data_ptr(), *[v.data_ptr() for v in dev_tabs(c["T"], LV)],
              losses.data_ptr(), mses.data_ptr(), c["B"], c["n"], ld, mean_type, clip, 0, var_mode, c["T"], _hip.stream())
    return losses.cpu(), mses.cpu()


def old_terms(c, out_mean, mean_type, clip, logvar_name, name):
    T, ld = c["T"], c["T"] + 8
    x0, xt, o, tt = on_dev(c["x0"]), on_dev(c["xt"]), on_dev(out_mean), on_dev(c["t"])
    tb = [v.data_ptr() for v in dev_tabs(T, MEAN + ("fixed-small", logvar_name))]
    if name == "ddpm_vlb_terms":
        loss = torch.empty(c["B"], device=DEV)
        _hip.call(name, x0.data_ptr(), xt.data_ptr(), o.data_ptr(), tt.data_ptr(), *tb, loss.data_ptr(), 0, c["B"], c["n"], mean_type, clip, T, _hip.stream())
        return loss.cpu()
    losses, mses = torch.full((c["B"], ld), NAN, device=DEV), torch.full((c["B"], ld), NAN, device=DEV)
    _hip.call(name, x0.data_ptr(), xt.data_ptr(), o.data_ptr(), tt.data_ptr(), *tb, losses.data_ptr(), mses.data_ptr(), c["B"], c["n"], ld, mean_type, clip,
              0, T, _hip.stream())
    rows = torch.arange(c["B"])
    return losses.cpu()[rows, c["t"]], mses.cpu()[rows, c["t"]]


def learned_loss(c, out, target, mean_type, var_mode, w_mse, w_vlb, detach, gloss=None, t=None, want_grad=True, offset=0):
    B, n, T = c["B"], c["n"], c["T"]
    x0, xt, o, tt = on_dev(c["x0"]), on_dev(c["xt"]), on_dev(out, offset), on_dev(c["t"] if t is None else t)
    tg = on_dev(target) if target is not None else None
    gl = on_dev(gloss if gloss is not None else torch.full((B,), 1.0 / B))
    loss = torch.full((B,), NAN, device=DEV)
    gout = torch.full((B, 2 * n), NAN, device=DEV) if want_grad else None
    _hip.call("ddpm_learned_loss", x0.data_ptr(), xt.data_ptr(), o.data_ptr(), _hip.ptr(tg), tt.data_ptr(), *[v.data_ptr() for v in dev_tabs(T, LV)],
              gl.data_ptr(), loss.data_ptr(), _hip.ptr(gout), B, n, mean_type, var_mode, detach, T, w_mse, w_vlb, _hip.stream())
    return loss.cpu(), (gout.cpu() if want_grad else None)


# ------------------------------------------------------------------------------------------------------------------ bars
WORST = {}


def hold_vals(got, r64, r32, tag, rel=5e-5):
    bar = torch.maximum(torch.full_like(r64, rel * float(r64.abs().max())), 8 * (r32.double() - r64).abs())
    ratio = float(((got.double() - r64).abs() / bar).max())
    WORST["vals"] = max(WORST.get("vals", 0.0), ratio)
    print(f"  {tag}: err/bar {ratio:.3f}")
    assert ratio <= 1.0, (tag, ratio)


def hold_rows(got, r64, r32, tag, rel=2e-5):
    bar = torch.maximum(rel * r64.abs().amax(1, keepdim=True), 8 * (r32.double() - r64).abs().amax(1, keepdim=True)).clamp_min(1e-30)
    ratio = float(((got.double() - r64).abs() / bar).max())
    WORST["rows"] = max(WORST.get("rows", 0.0), ratio)
    print(f"  {tag}: err/bar {ratio:.3f}")
    assert ratio <= 1.0, (tag, ratio)


def ref_step(c, out, mean_type, clip, var_mode, dtype):
    tb = tabs_as(c["T"], dtype)
    if var_mode == 0:
        tb = dict(tb, fixed_model_logvar=tb["fixed-large"])
    return R.step(tb, R.MEAN_TYPES[mean_type], R.VAR_TYPES[var_mode], c["xt"].to(dtype), c["t"], out.to(dtype), c["z"].to(dtype), bool(clip))


def ref_terms(c, out, mean_type, clip, var_mode, dtype):
    return R.terms(tabs_as(c["T"], dtype), R.MEAN_TYPES[mean_type], R.VAR_TYPES[var_mode], c["x0"].to(dtype), c["xt"].to(dtype), c["t"], out.to(dtype), bool(clip))


def ref_loss(c, out, target, mean_type, var_mode, w_mse, w_vlb, detach, gloss, dtype):
    """(loss [B], d (sum_b gloss_b loss_b) / d out) by autograd on the reference."""
    o = out.detach().to(dtype).clone().requires_grad_(True)
    loss = R.weighted_loss(tabs_as(c["T"], dtype), R.MEAN_TYPES[mean_type], R.VAR_TYPES[var_mode], c["x0"].to(dtype), c["xt"].to(dtype), c["t"], o,
                           None if target is None else target.to(dtype), w_mse, w_vlb, bool(detach))
    loss = loss + 0.0 * o.sum(1)
    (loss * gloss.to(dtype)).sum().backward()
    return loss.detach(), o.grad


CASES = [("n35", 1000), ("n768", 1000), ("n768", 8), ("n16640", 1000)]


# ------------------------------------------------------------------------------------------------------------------ the step
@pytest.mark.parametrize("key,T", CASES, ids=[f"{k}-T{T}" for k, T in CASES])
def test_step_against_float64_and_the_fixed_variance_kernel(key, T):
    """Both learned modes against the reference, all mean types, clip on and off, in place == out of place; and bit for bit: var_mode 2
    with v = +1 / -1 is `ddpm_p_sample_step` on the fixed-large / fixed-small table, var_mode 1 with v = the broadcast table entry is too,
    var_mode 0 with any v is the old kernel on the de-interleaved mean half."""
    print()
    for var_mode in (1, 2):
        c = case(key, T, var_mode)
        n = c["n"]
        for mean_type in (0, 1, 2):
            out = c["outs"][R.MEAN_TYPES[mean_type]]
            for clip in (0, 1):
                x_prev, pred = step_lv(c, out, mean_type, clip, var_mode)
                assert not torch.isnan(x_prev).any() and not torch.isnan(pred).any()          # NaN-filled outputs fully overwritten
                (x64, p64), (x32, p32) = ref_step(c, out, mean_type, clip, var_mode, torch.float64), ref_step(c, out, mean_type, clip, var_mode, torch.float32)
                tag = f"{key} T={T} mode {var_mode} {R.MEAN_TYPES[mean_type]} clip={clip}"
                hold_rows(x_prev, x64, x32, tag + " x_prev")
                hold_rows(pred, p64, p32, tag + " pred_x0")
                inpl, _ = step_lv(c, out, mean_type, clip, var_mode, inplace=True, want_pred=False)
                assert torch.equal(inpl, x_prev)
    c = case(key, T, 2)
    B, n = c["B"], c["n"]
    lmax, lmin = (tabs64(T)[k].float()[c["t"]][:, None].expand(B, n) for k in ("model_logvar_max", "posterior_logvar_clipped"))
    for mean_type in (0, 1, 2):
        mean_half = c["outs"][R.MEAN_TYPES[mean_type]][:, :n].contiguous()
        with_v = lambda v: torch.cat([mean_half, v], dim=1).contiguous()                   # noqa: E731
        for clip in (0, 1):
            large, small = step_old(c, mean_half, mean_type, clip, "fixed-large"), step_old(c, mean_half, mean_type, clip, "fixed-small")
            for got, want, what in ((step_lv(c, with_v(torch.ones(B, n)), mean_type, clip, 2), large, "v=+1"),
                                    (step_lv(c, with_v(-torch.ones(B, n)), mean_type, clip, 2), small, "v=-1"),
                                    (step_lv(c, with_v(lmax), mean_type, clip, 1), large, "v=lv_max"),
                                    (step_lv(c, with_v(lmin), mean_type, clip, 1), small, "v=lv_min"),
                                    (step_lv(c, c["outs"][R.MEAN_TYPES[mean_type]], mean_type, clip, 0), large, "mode 0")):
                assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), (what, mean_type, clip)


def test_step_out_of_range_t_poisons_the_sample_alone_and_misaligned_rows():
    c = case("n768", 1000, 2)
    out = c["outs"]["eps"]
    good = step_lv(c, out, 0, 1, 2)
    t_bad = c["t"].clone()
    t_bad[1], t_bad[3] = -1, 1000
    x_prev, pred = step_lv(c, out, 0, 1, 2, t=t_bad)
    for b in range(c["B"]):
        if b in (1, 3):
            assert torch.isnan(x_prev[b]).all() and torch.isnan(pred[b]).all()
        else:
            assert torch.equal(x_prev[b], good[0][b]) and torch.equal(pred[b], good[1][b])
    off = step_lv(c, out, 0, 1, 2, offset=1)                                            # model_out one float past a 16-byte boundary
    assert torch.equal(off[0], good[0]) and torch.equal(off[1], good[1])


# ------------------------------------------------------------------------------------------------------------------ bound term, column form
@pytest.mark.parametrize("key,T", CASES, ids=[f"{k}-T{T}" for k, T in CASES])
def test_bound_term_and_column_form_against_float64(key, T):
    """`ddpm_vlb_terms_lv` (always the 256-thread layout) and `ddpm_bpd_terms_lv` (a wave per row at n = 35, 256 threads at n = 768, 1024
    threads with 16-byte loads at n = 16640 — and its scalar form when model_out sits one float off) against the reference, and against
    each other: bit for bit at n = 768, where both run the 256-thread layout, within the `losses` bar elsewhere (the reduction order differs
    between the layouts)."""
    print()
    rows = None
    for var_mode in (1, 2):
        c = case(key, T, var_mode)
        B, n, t = c["B"], c["n"], c["t"]
        rows = torch.arange(B)
        for mean_type in (0, 1, 2):
            out = c["outs"][R.MEAN_TYPES[mean_type]]
            for clip in (0, 1):
                (l64, m64), (l32, m32) = ref_terms(c, out, mean_type, clip, var_mode, torch.float64), ref_terms(c, out, mean_type, clip, var_mode, torch.float32)
                tag = f"{key} T={T} mode {var_mode} {R.MEAN_TYPES[mean_type]} clip={clip}"
                loss, pred = vlb_lv(c, out, mean_type, clip, var_mode)
                hold_vals(loss, l64, l32, tag + " vlb")
                p64 = ref_step(c, out, mean_type, clip, var_mode, torch.float64)[1]
                hold_rows(pred, p64, ref_step(c, out, mean_type, clip, var_mode, torch.float32)[1], tag + " pred_x0")
                for offset in ((0, 1) if n >= 16384 else (0,)):
                    losses, mses = bpd_lv(c, out, mean_type, clip, var_mode, offset=offset)
                    written = torch.zeros(B, T + 8, dtype=torch.bool)
                    written[rows, t] = True
                    assert torch.equal(~torch.isnan(losses), written) and torch.equal(~torch.isnan(mses), written)
                    hold_vals(losses[rows, t], l64, l32, tag + f" bpd losses off={offset}")
                    hold_vals(mses[rows, t], m64, m32, tag + f" bpd mses off={offset}", rel=2e-5)
                    if key == "n768" and offset == 0:                   # both are the 256-thread layout: one element order, one reduction tree
                        assert torch.equal(losses[rows, t], loss)
                    assert float((losses[rows, t] - loss).abs().max()) <= 5e-5 * float(l64.abs().max())     # the layouts agree


@pytest.mark.parametrize("key", ["n35", "n768", "n16640"])
def test_bound_term_with_v_at_the_table_entries_is_the_fixed_variance_kernel(key):
    """v = +1 / -1 (var_mode 2) and v = the broadcast table entry (var_mode 1): within the `losses` bar (5e-5 x max) and the `mses` floor
    (2e-5 x max) of `ddpm_vlb_terms` / `ddpm_bpd_terms` on the fixed-large / fixed-small tables."""
    T = 1000
    c = case(key, T, 2)
    B, n = c["B"], c["n"]
    lmax, lmin = (tabs64(T)[k].float()[c["t"]][:, None].expand(B, n) for k in ("model_logvar_max", "posterior_logvar_clipped"))
    rows = torch.arange(B)
    for mean_type in (0, 1, 2):
        mean_half = c["outs"][R.MEAN_TYPES[mean_type]][:, :n].contiguous()
        for v, var_mode, name in ((torch.ones(B, n), 2, "fixed-large"), (-torch.ones(B, n), 2, "fixed-small"), (lmax, 1, "fixed-large"), (lmin, 1, "fixed-small")):
            out = torch.cat([mean_half, v], dim=1).contiguous()
            old_vlb = old_terms(c, mean_half, mean_type, 1, name, "ddpm_vlb_terms")
            old_l, old_m = old_terms(c, mean_half, mean_type, 1, name, "ddpm_bpd_terms")
            new_vlb, _ = vlb_lv(c, out, mean_type, 1, var_mode)
            losses, mses = bpd_lv(c, out, mean_type, 1, var_mode)
            scale = float(old_vlb.abs().max())
            assert float((new_vlb - old_vlb).abs().max()) <= 5e-5 * scale, (key, mean_type, name)
            assert float((losses[rows, c["t"]] - old_l).abs().max()) <= 5e-5 * scale, (key, mean_type, name)
            assert float((mses[rows, c["t"]] - old_m).abs().max()) <= 2e-5 * float(old_m.abs().max()), (key, mean_type, name)


def test_terms_out_of_range_t():
    c = case("n768", 1000, 2)
    out = c["outs"]["eps"]
    t_bad = c["t"].clone()
    t_bad[1], t_bad[3] = -1, 1000
    good_loss, good_pred = vlb_lv(c, out, 0, 1, 2)
    loss, pred = vlb_lv(c, out, 0, 1, 2, t=t_bad)
    good_l, good_m = bpd_lv(c, out, 0, 1, 2)
    losses, mses = bpd_lv(c, out, 0, 1, 2, t=t_bad)
    for b in range(c["B"]):
        if b in (1, 3):
            assert torch.isnan(loss[b]) and torch.isnan(pred[b]).all()
            assert torch.isnan(losses[b]).all() and torch.isnan(mses[b]).all()             # no column: untouched
        else:
            assert loss[b] == good_loss[b] and torch.equal(pred[b], good_pred[b])
            assert torch.equal(losses[b].nan_to_num(7.0), good_l[b].nan_to_num(7.0)) and torch.equal(mses[b].nan_to_num(7.0), good_m[b].nan_to_num(7.0))


# ------------------------------------------------------------------------------------------------------------------ the loss
@pytest.mark.parametrize("key,T", CASES, ids=[f"{k}-T{T}" for k, T in CASES])
def test_learned_loss_value_and_both_gradient_halves_against_float64_autograd(key, T):
    """Hybrid (1, 0.37, detach) and kl (0, 1, full gradient), both modes, all mean types; two launches give the same bits; NaN-filled
    outputs are fully overwritten."""
    print()
    for var_mode in (1, 2):
        c = case(key, T, var_mode)
        B, n = c["B"], c["n"]
        gloss = torch.linspace(0.5, 1.5, B) / B
        for mean_type in ((0, 1, 2) if n < 16384 else (0,)):
            mt = R.MEAN_TYPES[mean_type]
            out, target = c["outs"][mt], c["targets"][mt]
            # the MSE against the exact target would be the perturbation alone: move the target so that both terms carry weight
            target = target + 0.1 * r(B, n, seed=11)
            for name, (w_mse, w_vlb, detach) in (("hybrid", (1.0, 0.37, 1)), ("kl", (0.0, 1.0, 0))):
                tg = target if w_mse else None
                loss, gout = learned_loss(c, out, tg, mean_type, var_mode, w_mse, w_vlb, detach, gloss)
                assert not torch.isnan(loss).any() and not torch.isnan(gout).any()
                w32 = (float(torch.tensor(w_mse, dtype=torch.float32)), float(torch.tensor(w_vlb, dtype=torch.float32)))
                l64, g64 = ref_loss(c, out, tg, mean_type, var_mode, *w32, detach, gloss, torch.float64)
                l32, g32 = ref_loss(c, out, tg, mean_type, var_mode, *w32, detach, gloss, torch.float32)
                tag = f"{key} T={T} mode {var_mode} {mt} {name}"
                hold_vals(loss, l64, l32, tag + " loss")
                hold_rows(gout[:, :n], g64[:, :n], g32[:, :n], tag + " d/d mean half")
                hold_rows(gout[:, n:], g64[:, n:], g32[:, n:], tag + " d/dv")
                again = learned_loss(c, out, tg, mean_type, var_mode, w_mse, w_vlb, detach, gloss)
                assert torch.equal(again[0], loss) and torch.equal(again[1], gout)
                alone, _ = learned_loss(c, out, tg, mean_type, var_mode, w_mse, w_vlb, detach, want_grad=False)
                assert torch.equal(alone, loss)                                             # gout = NULL: the forward of the autograd node


def test_learned_loss_known_answers():
    """detach_mean = 1: the mean-half gradient is `ddpm_mse_bwd`'s, bit for bit, and with w_vlb = 0 the loss is `ddpm_mse_fwd`'s to its
    bar (1e-5, tests/test_kernels_gpu.py) and the v half exactly 0.0; a one-hot gloss leaves every other row zero; (0, 1, 0) is
    `ddpm_vlb_terms_lv`."""
    for key in ("n35", "n768", "n16640"):
        c = case(key, 1000, 2)
        B, n = c["B"], c["n"]
        out, target = c["outs"]["eps"], c["targets"]["eps"] + 0.1 * r(B, n, seed=11)
        gloss = torch.linspace(0.5, 1.5, B) / B
        mean_half, tg, gl = on_dev(out[:, :n].contiguous()), on_dev(target), on_dev(gloss)
        g_mse, l_mse = torch.empty(B, n, device=DEV), torch.empty(B, device=DEV)
        _hip.call("ddpm_mse_bwd", mean_half.data_ptr(), tg.data_ptr(), gl.data_ptr(), g_mse.data_ptr(), B, n, _hip.stream())
        _hip.call("ddpm_mse_fwd", mean_half.data_ptr(), tg.data_ptr(), l_mse.data_ptr(), B, n, _hip.stream())
        loss, gout = learned_loss(c, out, target, 0, 2, 1.0, 0.37, 1, gloss)
        assert torch.equal(gout[:, :n], g_mse.cpu())
        loss0, gout0 = learned_loss(c, out, target, 0, 2, 1.0, 0.0, 1, gloss)
        assert torch.equal(gout0[:, :n], g_mse.cpu()) and bool((gout0[:, n:] == 0.0).all())
        assert float((loss0 - l_mse.cpu()).abs().max()) <= 1e-5 * float(l_mse.abs().max())
        hot = torch.zeros(B)
        hot[B - 1] = 1.0
        _, g_hot = learned_loss(c, out, target, 0, 2, 1.0, 0.37, 0, hot)
        assert bool((g_hot[:B - 1] == 0.0).all()) and bool((g_hot[B - 1] != 0.0).any())
        kl, _ = learned_loss(c, out, None, 0, 2, 0.0, 1.0, 0, gloss)
        assert float((kl - vlb_lv(c, out, 0, 0, 2)[0]).abs().max()) <= 5e-5 * float(kl.abs().max())


def test_learned_loss_decoder_tails_and_floor():
    """t = 0 for every sample, var_mode 1: x_0 at and beyond +-0.999 (open tails: row 0 of the case, and planted here) and v = -40 on a
    stretch of elements (sigma = e^-20: the likelihood is at its 1e-12 floor wherever the model mean is more than 1/255 off, and 1 where
    it is not) — value and gradients against float64 autograd, which cuts the gradient in the same places."""
    c0 = case("n768", 1000, 1)
    B, n = c0["B"], c0["n"]
    c = dict(c0, t=torch.zeros(B, dtype=torch.int64))
    f = tabs_as(1000, torch.float32)
    x0 = c0["x0"].clone()
    x0[1, :6] = torch.tensor([0.999, -0.999, 0.99901, -0.99901, 0.9989, -0.9989])
    c["x0"] = x0
    c["xt"] = f["sqrt_alphas_bar"][0] * x0 + f["sqrt_one_minus_alphas_bar"][0] * r(B, n, seed=2)
    sigma = float(torch.exp(0.5 * f["model_logvar_max"][0]))
    v = f["model_logvar_max"][0] + 0.3 * r(B, n, seed=8)
    v[:, 100:200] = -40.0
    mean_half = x0 + 0.3 * sigma * r(B, n, seed=7)
    mean_half[:, 150:200] = x0[:, 150:200]                                                # the model mean exactly on x_0: likelihood 1
    out = torch.cat([mean_half, v], dim=1).contiguous()                                   # mean_type 1: at t = 0 the model mean is the output
    gloss = torch.full((B,), 1.0 / B)
    print()
    for w in ((1.0, 0.37, 1), (0.0, 1.0, 0)):
        tg = x0 + 0.1 * r(B, n, seed=11) if w[0] else None
        loss, gout = learned_loss(c, out, tg, 1, 1, *w, gloss)
        w32 = (float(torch.tensor(w[0], dtype=torch.float32)), float(torch.tensor(w[1], dtype=torch.float32)), w[2])
        l64, g64 = ref_loss(c, out, tg, 1, 1, *w32, gloss, torch.float64)
        l32, g32 = ref_loss(c, out, tg, 1, 1, *w32, gloss, torch.float32)
        assert bool(torch.isfinite(l64).all()) and bool(torch.isfinite(g64).all())
        hold_vals(loss, l64, l32, f"tails/floor {w} loss")
        hold_rows(gout[:, :n], g64[:, :n], g32[:, :n], f"tails/floor {w} d/d mean half")
        hold_rows(gout[:, n:], g64[:, n:], g32[:, n:], f"tails/floor {w} d/dv")
        assert bool((gout[:, n + 100:n + 200] == 0.0).all())                               # floor and saturated CDF: no gradient to v


def test_learned_loss_out_of_range_t_poisons_its_own_row():
    c = case("n768", 1000, 2)
    B, n = c["B"], c["n"]
    out, target = c["outs"]["eps"], c["targets"]["eps"]
    good = learned_loss(c, out, target, 0, 2, 1.0, 0.37, 1)
    t_bad = c["t"].clone()
    t_bad[1], t_bad[3] = -1, 1000
    loss, gout = learned_loss(c, out, target, 0, 2, 1.0, 0.37, 1, t=t_bad)
    for b in range(B):
        if b in (1, 3):
            assert torch.isnan(loss[b]) and torch.isnan(gout[b]).all()
        else:
            assert loss[b] == good[0][b] and torch.equal(gout[b], good[1][b])


# ------------------------------------------------------------------------------------------------------------------ hostile values
def same_places(got, ref64, tag):
    """Non-finite results fall where the float64 reference has them (NaN on NaN, +-inf on the same infinity)."""
    assert torch.equal(torch.isnan(got), torch.isnan(ref64)), tag
    inf = torch.isinf(ref64)
    assert torch.equal(torch.isinf(got), inf) and torch.equal(got[inf].double(), ref64[inf]), tag


def test_hostile_v_and_planted_nan():
    """var_mode 1 with v = +-1e4 (e^{+-5000} and e^{+-1e4} overflow / underflow in float64 as they do in fp32) on the first 16 elements of
    every row, var_mode 2 with v = +-50 (log-variances of about +-20 at t = 1: finite in both precisions): non-finite results exactly
    where the float64 reference has them; a NaN planted in sample 1 stays there.  (No accuracy bar here: with e^{+-20} variances eight
    elements carry a row and their 3e-5 of rounding noise is the row's.)"""
    print()
    for var_mode, big in ((1, 1e4), (2, 50.0)):
        c = case("n768", 1000, var_mode)
        B, n = c["B"], c["n"]
        out = c["outs"]["eps"].clone()
        out[:, n:n + 8], out[:, n + 8:n + 16] = big, -big
        x_prev, pred = step_lv(c, out, 0, 1, var_mode)
        x64, p64 = ref_step(c, out, 0, 1, var_mode, torch.float64)
        same_places(x_prev, x64, f"step mode {var_mode}")
        same_places(pred, p64, f"pred_x0 mode {var_mode}")
        loss, _ = vlb_lv(c, out, 0, 1, var_mode)
        l64, m64 = ref_terms(c, out, 0, 1, var_mode, torch.float64)
        same_places(loss, l64, f"vlb mode {var_mode}")
        losses, mses = bpd_lv(c, out, 0, 1, var_mode)
        rows = torch.arange(B)
        same_places(losses[rows, c["t"]], l64, f"bpd mode {var_mode}")
        same_places(mses[rows, c["t"]], m64, f"bpd mses mode {var_mode}")
        print(f"  mode {var_mode}, v = +-{big:g}: non-finite x_prev {int((~torch.isfinite(x64)).sum())}, non-finite L_t rows {int((~torch.isfinite(l64)).sum())} of {B}")
        lo, gout = learned_loss(c, out, c["targets"]["eps"], 0, var_mode, 1.0, 0.37, 1)
        l64h, _ = ref_loss(c, out, c["targets"]["eps"], 0, var_mode, 1.0, float(torch.tensor(0.37, dtype=torch.float32)), 1, torch.full((B,), 1.0 / B), torch.float64)
        same_places(lo, l64h, f"loss mode {var_mode}")
        # a NaN in sample 1 (mean half and v half) stays in sample 1
        clean = c["outs"]["eps"]
        bad = clean.clone()
        bad[1, 5], bad[1, n + 9] = NAN, NAN
        for fn in (lambda o: step_lv(c, o, 0, 1, var_mode), lambda o: vlb_lv(c, o, 0, 1, var_mode), lambda o: bpd_lv(c, o, 0, 1, var_mode),
                   lambda o: learned_loss(c, o, c["targets"]["eps"], 0, var_mode, 1.0, 0.37, 0)):
            a, b = fn(clean), fn(bad)
            for u, w in zip(a, b):
                keep = [i for i in range(B) if i != 1]
                assert torch.equal(u[keep].nan_to_num(7.0), w[keep].nan_to_num(7.0))
            # ... and shows there (sample 1 sits at t = 0, where the decoder's floor, fmaxf(p, 0) as in `ddpm_vlb_terms`, swallows it in
            # L_t itself: the x_0 estimate, the mses column and the gradient carry it)
            assert any(bool(torch.isnan(w[1]).any()) for w in b)


# ------------------------------------------------------------------------------------------------------------------ end to end
REDUCED = dict(in_channels=3, hid_channels=64, out_channels=6, ch_multipliers=[1, 2, 2], num_res_blocks=1, apply_attn=[False, True, False],
               drop_rate=0.0)
E2E_T, E2E_SHAPE = 8, (3, 3, 16, 16)


@functools.lru_cache(maxsize=None)
def e2e_reference(var_type):
    """The oracle UNet under tests/learned_var_ref.py on the CPU, once per variance type: the sampling chain and the bits/dim loop."""
    torch.manual_seed(5)
    m = ddpm_torch.UNet(**REDUCED)
    sd = U.randomize_state_dict(m.state_dict(), 17)
    g = torch.Generator().manual_seed(41)
    x_T = torch.randn(E2E_SHAPE, generator=g)
    zs = torch.randn((E2E_T,) + E2E_SHAPE, generator=g)
    x_0 = torch.rand(E2E_SHAPE, generator=g) * 2 - 1
    tb = R.tables(D.beta_schedule("linear", 1e-4, 0.02, E2E_T))
    sd64 = {k: v.double() for k, v in sd.items()}
    net = lambda x, t: U.unet_forward(sd64, REDUCED, x, t)                                # noqa: E731
    with torch.no_grad():
        chain = R.sample_chain(tb, "eps", var_type, net, x_T.double(), zs.double())
        bpd = R.all_bpd(tb, "eps", var_type, x_0.double(), zs.double(), net, True)
    return sd, x_T, zs, x_0, chain, bpd, sd64


def e2e_model(sd):
    m = ddpm_torch.UNet(**REDUCED)
    m.load_state_dict(sd)
    return m.to(DEV).set_compute_dtype(torch.float32)


@pytest.mark.parametrize("var_type", ["learned", "learned-range"])
def test_sampling_and_bpd_graph_replayed_equal_eager_and_match_the_oracle(var_type, monkeypatch):
    """T = 8, B = 3, 16 x 16: the replayed chain and evaluation loop equal the eager ones bit for bit, and both stay within FP32_BAR
    (1e-3 of the largest reference value, the project's bar for an fp32 network) of the oracle UNet under the float64 reference."""
    sd, x_T, zs, x_0, chain, bpd, _ = e2e_reference(var_type)
    m = e2e_model(sd).eval()
    dif = ddpm_torch.GaussianDiffusion(ddpm_torch.get_beta_schedule("linear", 1e-4, 0.02, E2E_T), "eps", var_type, "kl")
    outs, evals = {}, {}
    for mode in ("1", "0"):
        monkeypatch.setenv("DDPM_TORCH_AMD_GRAPH", mode)
        with torch.inference_mode():
            outs[mode] = dif._sample_loop(m, E2E_SHAPE, DEV, x_T, None, z_stream=iter(zs))
        outs[mode + "s"] = dif.p_sample(m, shape=E2E_SHAPE, device=DEV, seed=77)
        evals[mode] = dif.calc_all_bpd(m, x_0.to(DEV), noise_stream=iter([z.to(DEV) for z in zs]))
    assert getattr(dif, "_sample_graphs", None) and any(k[3][2] is not None for k in dif._sample_graphs), "the steps were not captured"
    assert torch.equal(outs["1"], outs["0"]) and torch.equal(outs["1s"], outs["0s"])
    assert all(torch.equal(a, b) for a, b in zip(evals["1"], evals["0"]))
    err = check(outs["1"], chain, FP32_BAR, name="chain")
    errs = {k: float((v.cpu() - bpd[k]).abs().max() / bpd[k].abs().max()) for v, k in zip(evals["1"], ("total", "losses", "prior", "mses"))}
    print(f"\n{var_type}: chain rel err {err:.3e}; bpd " + ", ".join(f"{k} {e:.3e}" for k, e in errs.items()))
    assert max(errs.values()) <= FP32_BAR, errs


def test_ddim4_on_the_2c_channel_model():
    """DDIM (eta = 0, 4 of 8 steps) built from the learned-range process reads the mean half alone on its own tables: the same bits as a
    fixed-small DDIM on a network that is the mean half of this one, and FP32_BAR from the oracle."""
    import os
    import sys
    pkg = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ddpm-torch_amd")
    if pkg not in sys.path:
        sys.path.insert(0, pkg)
    import ddim
    sd, x_T, zs, x_0, _, _, sd64 = e2e_reference("learned-range")
    m = e2e_model(sd).eval()
    betas = ddpm_torch.get_beta_schedule("linear", 1e-4, 0.02, E2E_T)
    sub = ddim.get_selection_schedule("linear", size=4, timesteps=E2E_T)
    dd = ddim.DDIM.from_ddpm(ddpm_torch.GaussianDiffusion(betas, "eps", "learned-range", "hybrid"), eta=0.0, subsequence=sub)
    plain = ddim.DDIM(betas, "eps", "fixed-small", "mse", eta=0.0, subsequence=sub)
    zero = [torch.zeros(E2E_SHAPE) for _ in range(4)]
    with torch.inference_mode():
        got = dd._sample_loop(m, E2E_SHAPE, DEV, x_T, None, z_stream=iter(zero))
        want = plain._sample_loop(lambda x, t: m(x, t)[:, :3].contiguous(), E2E_SHAPE, DEV, x_T, None, z_stream=iter(zero))
    assert torch.equal(got, want)
    tb = D.ddim_tables(D.beta_schedule("linear", 1e-4, 0.02, E2E_T), "fixed-small", 0.0, sub)
    with torch.no_grad():
        ref = D.sample_loop(tb, lambda x, t: U.unet_forward(sd64, REDUCED, x, t)[:, :3], x_T.double(), [z.double() for z in zero], timestep_map=sub)
    check(got, ref, FP32_BAR, name="DDIM-4")
    lat = dd.encode(m, x_0.to(DEV))
    assert lat.shape == x_0.shape and bool(torch.isfinite(lat).all())


TRAIN_LR = 1e-3


def _train_images(B):
    g = torch.Generator().manual_seed(21)
    return [torch.rand(B, 3, 16, 16, generator=g) * 2 - 1 for _ in range(3)]


@functools.lru_cache(maxsize=None)
def hybrid_runs(B, slabs):
    """Three hybrid ``Trainer.step``s (learned-range, 16 x 16, lr 1e-3, the reference's CPU (t, noise) stream) in the eager form, in the
    eager form again and in the launch-plan form (step 2 records, step 3 replays): {name: (losses, parameters, EMA shadow)}.  ``slabs``:
    the engine's deterministic weight-gradient reduction (``unet._WGRAD_SLABS``, the switch DDPM_WGRAD_SLABS initialises)."""
    from ddpm_torch.models import unet as unet_mod
    from ddpm_torch.utils import train as train_mod
    from tests import channels_accum as CA
    sd = e2e_reference("learned-range")[0]
    lr, xs = TRAIN_LR, _train_images(B)
    runs = {}
    was = train_mod._TRAIN_GRAPH, unet_mod._WGRAD_SLABS
    unet_mod._WGRAD_SLABS = slabs
    try:
        for name, form in (("eager", False), ("eager again", False), ("plan", "plan")):
            train_mod._TRAIN_GRAPH = form
            m = e2e_model(sd)
            dif = ddpm_torch.GaussianDiffusion(ddpm_torch.get_beta_schedule("linear", 1e-4, 0.02, 1000), "eps", "learned-range", "hybrid")
            opt = torch.optim.Adam(m.parameters(), lr=lr, betas=(0.9, 0.999))
            tr = ddpm_torch.Trainer(m, opt, dif, epochs=1, trainloader=None, scheduler=None, use_ema=True, grad_norm=1.0, shape=(3, 16, 16),
                                    device=torch.device(DEV), ema_decay=0.9999)
            draw = CA.reference_stream()

            def fill(t_buf, noise_buf, draw=draw):
                t, noise = draw(noise_buf)
                t_buf.copy_(t)
                noise_buf.copy_(noise)
            tr.input_source = fill
            m.train()
            losses = []
            for i, x in enumerate(xs):
                tr.stats.reset()
                tr.step(x, global_steps=i + 1)
                losses.append(tr.current_stats["loss"])
            torch.cuda.synchronize()
            ds = next(iter(tr._direct.values()))
            assert ds.last_kind == ("plan" if form == "plan" else "eager")
            runs[name] = (losses, {k: v.detach().cpu().clone() for k, v in m.state_dict().items()},
                          {k: v.detach().cpu().clone() for k, v in tr.ema.shadow.items()})
    finally:
        train_mod._TRAIN_GRAPH, unet_mod._WGRAD_SLABS = was
    return runs


def _hold_to_the_oracle_trainer(runs, B, names):
    """Bars of tests/test_channels_accum_gpu.py: losses rtol 5e-4; states 1e-3 with an Adam slack of 0.25 lr per update."""
    sd = e2e_reference("learned-range")[0]
    oracle = R.oracle_trainer(sd, REDUCED, TRAIN_LR, "eps", "learned-range", 1.0)
    ref = torch.tensor([oracle.step(x)[0] for x in _train_images(B)], dtype=torch.float64)
    slack = 0.25 * TRAIN_LR * 3
    for name in names:
        losses = torch.tensor(runs[name][0], dtype=torch.float64)
        print(f"\nB = {B} hybrid losses ({name}) {losses.tolist()} vs oracle {ref.tolist()}")
        assert torch.allclose(losses, ref, rtol=5e-4), (name, losses, ref)
        check_state(runs[name][1], oracle.state(), 1e-3, "param", adam_slack=slack)
        check_state(runs[name][2], oracle.shadow, 1e-3, "shadow", adam_slack=slack)


def test_three_hybrid_trainer_steps_eager_and_launch_plan_match_the_oracle_trainer():
    """B = 4, the engine as it ships (split-K weight gradients added with atomics): both forms take the autograd-free step (eager launches /
    a recorded plan replayed by csrc/plan.hip), and in both the losses and the parameters follow the float64 oracle trainer.  The first
    step's loss — one forward on identical weights — is the same bits in both."""
    runs = hybrid_runs(4, False)
    assert runs["eager"][0][0] == runs["plan"][0][0]
    _hold_to_the_oracle_trainer(runs, 4, ("eager", "plan"))


def test_three_hybrid_trainer_steps_eager_and_launch_plan_same_bits():
    """The two forms issue the same launches with the same arguments (the plan bakes in `w_mse`, `vlb_weight`, `var_mode`, every pointer),
    so three steps leave the same bits: losses, parameters, EMA shadow — and follow the float64 oracle trainer.

    The shape this is asked at, and why.  `Trainer.step` does not repeat its own bits from run to run on this engine, whatever the loss
    (tests/test_device_loader_gpu.py says the same of the `mse` step): split-K weight-gradient slices, GroupNorm's dgamma / dbeta and the
    bias column sums add with fp32 atomics in an order the hardware picks.  Measured with this network at B = 4, three steps, eager
    against a second EAGER run: `mse` / fixed-large 150 of 166 tensors differ (worst 5.4e-5 of a tensor's largest entry), `hybrid` /
    learned-range 151 of 166 (3.7e-5); eager against plan 147 and 149.  There a comparison of two forms says nothing about the forms.
    It does where a run repeats itself: with the engine's deterministic weight-gradient reduction (`unet._WGRAD_SLABS`) and B = 1 no
    address receives more than two unordered contributions (measured: eager against eager 0 of 166 tensors at 8 x 8 and 16 x 16; at
    B = 2 the cross-sample atomics are back, 151 of 166).  So: B = 1, slabs on; first that a second eager run gives the first one's
    bits — the premise — then that the plan run does."""
    runs = hybrid_runs(1, True)
    for other in ("eager again", "plan"):
        assert runs["eager"][0] == runs[other][0], (other, runs["eager"][0], runs[other][0])
        for part in (1, 2):
            for k, v in runs["eager"][part].items():
                assert torch.equal(v, runs[other][part][k]), (other, k)
    _hold_to_the_oracle_trainer(runs, 1, ("eager", "plan"))
