"""TEST INFRASTRUCTURE: the float64 restatement of inpainting by RePaint (Lugmayr et al., CVPR 2022, Algorithm 1 and the jump schedule of
its §4.2), composed from the pinned oracle only.  Nothing of it exists upstream, so it is stated from the paper on top of what the fixtures
pin: the reverse step is ``oracle.diffusion_ref.model_mean_from_output`` plus the noise term of ``p_step_from_eps`` (through
tests/learned_var_ref.py ``step`` for a per-element log-variance), the re-noising of the known region and the jump are ``q_sample``'s
expression on the tables of the level they arrive at, and the network is the oracle UNet (tests/cond_ref.py for a conditional one).

    x_known_{i-1} = sqrt(ab_{i-1}) x_0 + sqrt(1 - ab_{i-1}) e           (Algorithm 1 line 4; ab_{-1} = 1: the source image itself)
    x_unknown_{i-1} = the reverse step on x_i                          (lines 5-6)
    x_{i-1} = m x_known_{i-1} + (1 - m) x_unknown_{i-1}                 (line 7)
    x_{i+j} = sqrt(ab_{i+j} / ab_i) x_i + sqrt(1 - ab_{i+j} / ab_i) z    (line 9, j single steps composed into one Gaussian)

Everything follows the dtype of its inputs: float64 inputs give the reference, float32 inputs the fp32 evaluation.

The per-element error bars of the masked step (U24 = 2^-24, one rounding unit per fp32 operation, times the magnitude it rounds; first
order, in the manner of ``step_bar`` of tests/test_cond_gpu.py, with the network output exact — there is no guided combination in front):
  eps:  x0 = a xt - b o                 E_0 = 2u (|a xt| + |b o|)
  x_0:  x0 = o                          E_0 = 0
  mean: x0 = fma(-xt, c2/c1, o/c1)      E_0 = 2u (|o / c1| + |xt c2 / c1|)
  clip is 1-Lipschitz.                  mean = c1 x0 + c2 xt: E_m = c1 E_0 + 2u (|c1 x0| + |c2 xt|)     (mean type: E_m = 0)
  log-variance: a table entry or v itself is exact; var_mode 2, lv = f lmax + (1 - f) lmin with f = (v + 1) / 2:
        E_f = u |f|,   E_lv = E_f |lmax| + (E_f + u |1 - f|) |lmin| + 2u (|f lmax| + |(1 - f) lmin|)
  u' = fma(z, mask sd, mean)            E_u = E_m + u (terms + noise) + (3u + E_lv / 2) noise,   noise = mask sd |z|   (0.5 lv exact; expf
                                              within 2 ulp, one more for the product; d sd / sd = d lv / 2)
  k = ka xk + kb e                      E_k = 2u (|ka xk| + |kb e|)                              two products and a sum
  out = m k + (1 - m) u'                E = m E_k + r E_u + 2u (|m k| + |r u'|) + u r |u'|       r = 1 - m (one rounding), two products, a sum
"""
import torch

from oracle import diffusion_ref as D
from tests import learned_var_ref as LR

MEAN_TYPES = LR.MEAN_TYPES
VAR_TYPES = LR.VAR_TYPES
U24 = 2.0 ** -24


def prev_tables(ab):
    """(sqrt(ab_prev), sqrt(1 - ab_prev)) with ab_prev[i] = ab[i-1], ab_prev[0] = 1, in ab's dtype."""
    ab_prev = torch.cat([torch.ones(1, dtype=ab.dtype), ab[:-1]])
    return ab_prev.sqrt(), (1.0 - ab_prev).sqrt()


def jump_tables(ab, j):
    """(ja, jb) indexed by the arrival index i, NaN where i - j < -1."""
    ext = torch.cat([torch.ones(1, dtype=ab.dtype), ab])
    ja, jb = torch.full_like(ab, float("nan")), torch.full_like(ab, float("nan"))
    for i in range(len(ab)):
        if i - j >= -1:
            a = ext[i + 1] / ext[i - j + 1]
            ja[i], jb[i] = a.sqrt(), (1.0 - a).sqrt()
    return ja, jb


def _rows(v, t, x):
    return D._gather(v, t, x)


def _mask_like(mask, x):
    """[rows][hw] or [rows, 1, H, W] -> broadcastable against x ([B, C, ...]): one row for the batch or one per sample, every channel."""
    m = mask.to(x.dtype)
    return m.reshape((m.shape[0], 1) + tuple(x.shape[2:]))


def reverse_step(T, mean_type, var_type, x_t, t, out, z, clip):
    """The unknown region's update: the plain step for a C-channel output (or a 2C-channel one read on the fixed table, var_type None),
    the learned-variance step otherwise."""
    if out.shape[1] == 2 * x_t.shape[1]:
        return LR.step(T, mean_type, var_type, x_t, t, out, z, clip)[0]
    assert var_type is None
    mean, _ = D.model_mean_from_output(T, mean_type, x_t, t, out, clip)
    mask = (t > 0).reshape((-1,) + (1,) * (x_t.ndim - 1)).to(x_t)
    return mean + mask * torch.exp(0.5 * _rows(T["fixed_model_logvar"], t, x_t)) * z


def masked_step(T, mean_type, var_type, x_t, t, out, z, x_known, e, mask, clip):
    """Algorithm 1 lines 4-7 at level t: T holds "sqrt_alphas_bar_prev" / "sqrt_one_minus_alphas_bar_prev" beside the step's tables."""
    u = reverse_step(T, mean_type, var_type, x_t, t, out, z, clip)
    k = _rows(T["sqrt_alphas_bar_prev"], t, x_t) * x_known + _rows(T["sqrt_one_minus_alphas_bar_prev"], t, x_t) * e
    m = _mask_like(mask, x_t)
    return m * k + (1.0 - m) * u


def jump(ja, jb, x, t, z):
    return _rows(ja, t, x) * x + _rows(jb, t, x) * z


def schedule(S, j=1, r=1, start=None):
    """RePaint's jump schedule, written as its authors' sampler walks it: a table of the jumps still to take from each index, consumed as
    the chain passes."""
    top = S - 1 if start is None else start
    left = {i: r - 1 for i in range(0, top - j + 1) if (top - i) % j == 0} if r > 1 else {}
    ops, i = [], top
    while i >= 0:
        i -= 1
        ops.append("down")
        if left.get(i, 0) > 0:
            left[i] -= 1
            i += j
            ops.append("up")
    return ops


def network_calls(S, j, r, start=None):
    top = S - 1 if start is None else start
    return (top + 1) + (r - 1) * j * (top // j)


def chain(T, mean_type, var_type, net, x_known, mask, draws, j=1, r=1, start=None, clip=True, timestep_map=None):
    """The whole chain with injected draws in the product's order: the initial draw, then per reverse step z, then e, one draw per jump.
    ``net(x, t)`` is the network (labels bound by the caller); T holds the prev tables and, for jumps, is given ``alphas_bar``."""
    draws = iter(draws)
    S = len(T["posterior_mean_coef1"])
    top = S - 1 if start is None else start
    B = len(x_known)
    full = lambda i: torch.full((B,), i, dtype=torch.int64)                                  # noqa: E731
    first = next(draws).to(x_known)
    x = first if start is None else D.q_sample(T, x_known, full(top), first)
    ja, jb = jump_tables(T["alphas_bar"], j)
    i = top
    for op in schedule(S, j, r, start):
        if op == "down":
            t = full(i)
            out = net(x, t if timestep_map is None else timestep_map.gather(0, t))
            z, e = next(draws).to(x), next(draws).to(x)
            x = masked_step(T, mean_type, var_type, x, t, out, z, x_known, e, mask, clip)
            i -= 1
        else:
            i += j
            x = jump(ja, jb, x, full(i), next(draws).to(x))
    assert i == -1
    return x


def with_prev(T):
    """T with the two tables of the level a step arrives at, from its own ``alphas_bar``."""
    T = dict(T)
    T["sqrt_alphas_bar_prev"], T["sqrt_one_minus_alphas_bar_prev"] = prev_tables(T["alphas_bar"])
    return T


# ------------------------------------------------------------------------------------------------------------------ error bars
def step_bar(T, mean_type, var_mode, x_t, t, out, z):
    """(E_u, |u'|-free terms are inside) of the module docstring, float64, from the float64 reference's own intermediate values."""
    g_ = lambda k: _rows(T[k], t, x_t)                                                       # noqa: E731
    C = x_t.shape[1]
    o, v = out[:, :C], (out[:, C:] if out.shape[1] == 2 * C else None)
    a, b, c1, c2 = g_("sqrt_recip_alphas_bar"), g_("sqrt_recip_m1_alphas_bar"), g_("posterior_mean_coef1"), g_("posterior_mean_coef2")
    if mean_type == 0:
        x0 = a * x_t - b * o
        e_0 = 2 * U24 * ((a * x_t).abs() + (b * o).abs())
    elif mean_type == 1:
        x0, e_0 = o, torch.zeros_like(o)
    else:
        x0 = o / c1 - c2 / c1 * x_t
        e_0 = 2 * U24 * ((o / c1).abs() + (x_t * c2 / c1).abs())
    if mean_type == 2:
        terms, e_m = o.abs(), torch.zeros_like(o)
    else:
        terms = (c1 * x0).abs() + (c2 * x_t).abs()                                           # (|x0| before the clip bounds |x0| after it)
        e_m = c1 * e_0 + 2 * U24 * terms
    e_lv = torch.zeros_like(o)
    if var_mode == 0:
        lv = g_("fixed_model_logvar")
    elif var_mode == 1:
        lv = v
    else:
        lmin, lmax = g_("posterior_logvar_clipped"), g_("model_logvar_max")
        f = (v + 1.0) / 2.0
        lv = f * lmax + (1.0 - f) * lmin
        e_f = U24 * f.abs()
        e_lv = e_f * lmax.abs() + (e_f + U24 * (1.0 - f).abs()) * lmin.abs() + 2 * U24 * ((f * lmax).abs() + ((1.0 - f) * lmin).abs())
    noise = (t > 0).to(x_t).reshape((-1,) + (1,) * (x_t.ndim - 1)) * torch.exp(0.5 * lv) * z.abs()
    return e_m + U24 * (terms + noise) + (3 * U24 + 0.5 * e_lv) * noise


def masked_bar(T, mean_type, var_mode, x_t, t, out, z, x_known, e, mask, clip):
    """E of the module docstring for every element, float64."""
    e_u = step_bar(T, mean_type, var_mode, x_t, t, out, z)
    u = reverse_step(T, MEAN_TYPES[mean_type], VAR_TYPES[var_mode], x_t, t, out, z, clip)
    ka, kb = _rows(T["sqrt_alphas_bar_prev"], t, x_t), _rows(T["sqrt_one_minus_alphas_bar_prev"], t, x_t)
    k = ka * x_known + kb * e
    e_k = 2 * U24 * ((ka * x_known).abs() + (kb * e).abs())
    m = _mask_like(mask, x_t)
    r = 1.0 - m
    return m * e_k + r * e_u + 2 * U24 * ((m * k).abs() + (r * u).abs()) + U24 * r * u.abs()
