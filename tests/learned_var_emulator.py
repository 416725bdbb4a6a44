"""TEST INFRASTRUCTURE for the learned reverse-process variance (csrc/elementwise.hip: ``ddpm_p_sample_step_lv``, ``ddpm_vlb_terms_lv``,
``ddpm_bpd_terms_lv``, ``ddpm_learned_loss``): restatements of the four entry points as include/ddpm_hip.h states them, over the raw host
pointers the product passes, for the host emulator (tests/abi_emulator.py; ``attach`` hangs them on the Emulator instance ``install``
returns).  fp32 arithmetic like the kernels', through tests/learned_var_ref.py on numpy views (the loss gradient by autograd on those
expressions, as abi_emulator does for ``ddpm_vlb_terms_bwd``).  They say nothing about the kernels themselves — tests/test_learned_var_gpu.py
holds those to float64."""
import numpy as np
import torch

from tests import learned_var_ref as R
from tests.abi_emulator import f32, i64

NAN = float("nan")


def _rows(ptr, B, n):
    return torch.from_numpy(f32(ptr, B * n).reshape(B, n).copy())


def _tables(recip, recip_m1, c1, c2, lo, hi, T, var_mode):
    g = lambda p: torch.from_numpy(f32(p, T).copy()) if p else None                        # noqa: E731
    tb = dict(sqrt_recip_alphas_bar=g(recip), sqrt_recip_m1_alphas_bar=g(recip_m1), posterior_mean_coef1=g(c1), posterior_mean_coef2=g(c2),
              alphas_bar=torch.zeros(T))
    if var_mode == 0:
        tb["fixed_model_logvar"] = g(lo)
    else:
        tb["posterior_logvar_clipped"], tb["model_logvar_max"] = g(lo), g(hi)
    return tb


def _times(t, B, T):
    """(t clamped into the tables, which samples are inside them)."""
    tt = torch.from_numpy(i64(t, B).copy())
    return tt.clamp(0, T - 1), (tt >= 0) & (tt < T)


def _put(ptr, B, n, values, ok):
    f32(ptr, B * n).reshape(B, n)[...] = torch.where(ok[:, None], values, torch.full_like(values, NAN)).numpy()


def ddpm_p_sample_step_lv(x_t, out, z, t, recip, recip_m1, c1, c2, lo, hi, x_prev, pred, B, n, mean_type, clip, var_mode, T, st):
    assert x_t and out and z and t and x_prev and 0 <= var_mode <= 2 and (var_mode == 1 or lo) and (var_mode != 2 or hi)
    tb, (tc, ok) = _tables(recip, recip_m1, c1, c2, lo, hi, T, var_mode), _times(t, B, T)
    with torch.no_grad():
        nxt, x0 = R.step(tb, R.MEAN_TYPES[mean_type], R.VAR_TYPES[var_mode], _rows(x_t, B, n), tc, _rows(out, B, 2 * n), _rows(z, B, n), bool(clip))
    _put(x_prev, B, n, nxt, ok)                   # (the inputs were copied: x_prev may be x_t)
    if pred:
        _put(pred, B, n, x0, ok)


def ddpm_vlb_terms_lv(x_0, x_t, out, t, recip, recip_m1, c1, c2, lv_min, lv_max, loss, pred_x0, B, n, mean_type, clip, var_mode, T, st):
    assert x_0 and x_t and out and t and loss and lv_min and var_mode in (1, 2) and (var_mode == 1 or lv_max)
    tb, (tc, ok) = _tables(recip, recip_m1, c1, c2, lv_min, lv_max, T, var_mode), _times(t, B, T)
    with torch.no_grad():
        term, pred = R.loss_term(tb, R.MEAN_TYPES[mean_type], R.VAR_TYPES[var_mode], _rows(x_0, B, n), _rows(x_t, B, n), tc, _rows(out, B, 2 * n), bool(clip))
    f32(loss, B)[...] = torch.where(ok, term, torch.full_like(term, NAN)).numpy()
    if pred_x0:
        _put(pred_x0, B, n, pred, ok)


def ddpm_bpd_terms_lv(x_0, x_t, out, t, recip, recip_m1, c1, c2, lv_min, lv_max, losses, mses, B, n, ld, mean_type, clip, decoder, var_mode, T, st):
    assert x_0 and x_t and out and t and losses and mses and lv_min and ld >= T and decoder == 0 and var_mode in (1, 2) and (var_mode == 1 or lv_max)
    tb, (tc, ok) = _tables(recip, recip_m1, c1, c2, lv_min, lv_max, T, var_mode), _times(t, B, T)
    with torch.no_grad():
        term, mse = R.terms(tb, R.MEAN_TYPES[mean_type], R.VAR_TYPES[var_mode], _rows(x_0, B, n), _rows(x_t, B, n), tc, _rows(out, B, 2 * n), bool(clip))
    lo, ms = f32(losses, B * ld).reshape(B, ld), f32(mses, B * ld).reshape(B, ld)
    for b in range(B):
        if ok[b]:                                  # a sample outside the tables has no column
            lo[b, int(tc[b])], ms[b, int(tc[b])] = float(term[b]), float(mse[b])


def ddpm_learned_loss(x_0, x_t, out, target, t, recip, recip_m1, c1, c2, lv_min, lv_max, gloss, loss, gout, B, n, mean_type, var_mode, detach_mean, T,
                      w_mse, w_vlb, st):
    assert x_0 and x_t and out and t and loss and lv_min and var_mode in (1, 2) and (var_mode == 1 or lv_max)
    assert (target or w_mse == 0) and (gloss or not gout)
    tb, (tc, ok) = _tables(recip, recip_m1, c1, c2, lv_min, lv_max, T, var_mode), _times(t, B, T)
    o = _rows(out, B, 2 * n).requires_grad_(bool(gout))
    with torch.enable_grad():                      # (also called from inside an autograd backward, where grad mode is off)
        val = R.weighted_loss(tb, R.MEAN_TYPES[mean_type], R.VAR_TYPES[var_mode], _rows(x_0, B, n), _rows(x_t, B, n), tc, o,
                              _rows(target, B, n) if target else None, np.float32(w_mse).item(), np.float32(w_vlb).item(), bool(detach_mean))
        val = val + 0.0 * o.sum(1)                 # (both weights 0: still a function of the leaf)
        if gout:
            (val * torch.from_numpy(f32(gloss, B).copy())).sum().backward()
    f32(loss, B)[...] = torch.where(ok, val.detach(), torch.full_like(val.detach(), NAN)).numpy()
    if gout:
        _put(gout, B, 2 * n, o.grad, ok)


def ddpm_bpd_finish(x_0, losses, prior, total, B, n, T, ld, sqrt_ab_last, log_1m_ab_last, st):
    """(`calc_all_bpd` ends in it; abi_emulator itself has no restatement of it.)"""
    x = f32(x_0, B * n).reshape(B, n).astype(np.float64)
    m, lv = np.float32(sqrt_ab_last) * x, float(np.float32(log_1m_ab_last))
    pr = (0.5 * ((-1.0 - lv) + m * m + np.exp(lv))).mean(1) / np.log(2.0)
    f32(prior, B)[...] = pr
    f32(total, B)[...] = f32(losses, B * ld).reshape(B, ld)[:, :T].astype(np.float64).sum(1) + pr


def attach(emu):
    """Add the four entry points to an ``abi_emulator.Emulator`` instance (its ``call`` is ``getattr(self, name)``)."""
    if not hasattr(emu, "ddpm_bpd_finish"):
        emu.ddpm_bpd_finish = ddpm_bpd_finish
    emu.ddpm_p_sample_step_lv = ddpm_p_sample_step_lv
    emu.ddpm_vlb_terms_lv = ddpm_vlb_terms_lv
    emu.ddpm_bpd_terms_lv = ddpm_bpd_terms_lv
    emu.ddpm_learned_loss = ddpm_learned_loss
    return emu
