"""-m gpu: class conditioning and classifier-free guidance on the device — `ddpm_class_embed_fwd`, `ddpm_class_embed_bwd` and
`ddpm_p_sample_step_cfg` (csrc/guidance.hip) against tests/cond_ref.py in float64 on the same fp32 inputs and fp32 tables, and the
class-conditional reduced UNet of tests/test_learned_var_gpu.py (``num_classes = 3``) end to end: forward, every parameter's gradient, guided
chains graph-replayed against eager, three conditional ``Trainer.step``s against the float64 oracle trainer.

Known answers (bit for bit) tie the new kernels to the old ones: ``s`` of the embedding kernel is `ddpm_silu_fwd(pre)`, a zero table row
leaves ``pre`` = ``t_emb``, ``scale`` 1 / 0 of the guided step are `ddpm_p_sample_step` on the conditional / unconditional half, a zeroed
class table makes the conditional network the unconditional one.

Bars, all derived (u = 2^-24, one rounding unit per fp32 operation, times the sum of the absolute terms it rounds):
  table gradient: a sum of B terms added one by one makes B - 1 roundings of partial sums no larger than S = sum_b |dpre[b][e]|:
      (B - 1) u S per element.  Integer-valued ``dpre`` sums exactly: tested for equality.
  guided step, per element, first order, propagated through the expression the kernel evaluates (``step_bar``):
      g = s oc + r ou                       E_g = 2u (|s oc| + |r ou|)                        two products, one sum
      eps:  x0 = a xt - b g                 E_0 = b E_g + 2u (|a xt| + |b g|)
      x_0:  x0 = g                          E_0 = E_g
      mean: x0 = fma(-xt, c2/c1, g/c1)      E_0 = E_g / c1 + 2u (|g / c1| + |xt c2 / c1|)     two divisions, one fma
      clip is 1-Lipschitz: E_0 stays.       mean = c1 x0 + c2 xt: E_m = c1 E_0 + 2u (|c1 x0| + |c2 xt|)   (mean type: E_m = E_g)
      x_prev = fma(z, mask sd, mean)        E_x = E_m + u (|c1 x0| + |c2 xt| + |z| mask sd) + 3u |z| mask sd   (0.5 lv is exact; expf within
                                                  2 ulp, one more for the product)
  networks: FP32_BAR = 1e-3 of the largest reference value, the project's bar for an fp32 network against the float64 oracle, which
      tests/test_learned_var_gpu.py uses for its forwards and chains (the class path adds one fp32 add); parameter gradients at the bar of
      tests/test_unet_gpu.py (3e-3 of a tensor's largest gradient, tensors below 2 % of the median scale measured against that floor);
      the trainer at the bars tests/test_learned_var_gpu.py uses at B = 4 (losses rtol 5e-4, states 1e-3 with an Adam slack of 0.25 lr per
      update).
Measured on the MI355X, worst error / bar: table gradient 0.329 (B = 7, E = 300; 0.008 at B = 257), guided step 0.875 (x_prev) and 0.926
(pred_x0) — the bar is a worst-case bound, not a multiple of a measured error; conditional forward 9.2e-7, worst gradient 1.7e-6, guided
chain 1.0e-6, guided DDIM-4 8.5e-7 of the reference's largest value (bar 1e-3 / 3e-3); trainer losses within 1.7e-6 (bar 5e-4).  The same
figures are in DESIGN.md §4 "Class conditioning and classifier-free guidance"."""
import functools
import os
import sys

import pytest
import torch

import ddpm_torch
from ddpm_torch import _hip
from oracle import diffusion_ref as D
from oracle import unet_ref as U
from tests import cond_ref as R
from tests import learned_var_ref as LR
from tests.golden.recipes import check, check_state

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ddpm-torch_amd")
if PKG not in sys.path:
    sys.path.insert(0, PKG)
import ddim  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U24 = 2.0 ** -24
NAN = float("nan")
FP32_BAR = 1e-3
STEP = ("sqrt_recip_alphas_bar", "sqrt_recip_m1_alphas_bar", "posterior_mean_coef1", "posterior_mean_coef2", "fixed_model_logvar")
GUARD = 64                                            # floats of NaN on either side of every guarded buffer


def r(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


class Guarded:
    """A device buffer of ``shape`` between two guard regions of NaN bytes; ``offset`` floats move its base off the 16-byte grid."""

    def __init__(self, shape, fill=NAN, offset=0, values=None):
        n = 1
        for s in shape:
            n *= s
        self.buf = torch.full((n + 2 * GUARD + 4,), NAN, device=DEV)
        self.lo, self.hi = GUARD + offset, GUARD + offset + n
        self.t = self.buf[self.lo:self.hi].view(shape)
        if values is not None:
            self.t.copy_(values)
        elif fill == fill:
            self.t.fill_(fill)

    def intact(self):
        return bool(torch.isnan(self.buf[:self.lo]).all()) and bool(torch.isnan(self.buf[self.hi:]).all())


def bits(a, b):
    """Equal as bit patterns (NaN payloads included)."""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ------------------------------------------------------------------------------------------------------------------ ddpm_class_embed_fwd
def embed_fwd(t_emb, table, y):
    B, E = t_emb.shape
    te, tb = Guarded((B, E), values=t_emb), Guarded(tuple(table.shape), values=table)
    pre, s = Guarded((B, E)), Guarded((B, E))
    yd = y.to(DEV)
    _hip.call("ddpm_class_embed_fwd", te.t.data_ptr(), tb.t.data_ptr(), yd.data_ptr(), pre.t.data_ptr(), s.t.data_ptr(), B, E, table.shape[0], _hip.stream())
    torch.cuda.synchronize()
    assert all(g.intact() for g in (te, tb, pre, s)) and bits(te.t.cpu(), t_emb) and bits(tb.t.cpu(), table)
    return pre.t.clone(), s.t.clone()


@pytest.mark.parametrize("K1", [2, 11])
@pytest.mark.parametrize("E", [64, 512])
@pytest.mark.parametrize("B", [1, 5, 128])
def test_class_embed_fwd_is_the_fp32_sum_and_the_shared_silu(B, E, K1):
    t_emb, table = r(B, E, seed=B + E), r(K1, E, seed=K1)
    table[K1 - 1] = 0.0                                                              # a zero row: pre = t_emb to the bit
    y = torch.randint(0, K1, (B,), generator=torch.Generator().manual_seed(B * K1))
    y[-1] = K1 - 1
    pre, s = embed_fwd(t_emb, table, y)
    want = t_emb.to(DEV) + table.to(DEV)[y.to(DEV)]
    assert bits(pre, want)
    assert bits(pre[-1].cpu(), t_emb[-1])
    silu = torch.full_like(pre, NAN)
    _hip.call("ddpm_silu_fwd", pre.data_ptr(), silu.data_ptr(), B * E, _hip.stream())
    assert bits(s, silu)
    # a label outside [0, K1) poisons its own two rows and nothing else
    for bad in (K1, -1, 1 << 40):
        yb = y.clone()
        yb[B // 2] = bad
        pre_b, s_b = embed_fwd(t_emb, table, yb)
        assert bool(torch.isnan(pre_b[B // 2]).all()) and bool(torch.isnan(s_b[B // 2]).all())
        keep = [b for b in range(B) if b != B // 2]
        assert bits(pre_b[keep], pre[keep]) and bits(s_b[keep], s[keep])


# ------------------------------------------------------------------------------------------------------------------ ddpm_class_embed_bwd
def embed_bwd(dpre, y, K1, poison=NAN):
    B, E = dpre.shape
    d, out = Guarded((B, E), values=dpre), Guarded((K1, E), fill=poison)
    yd = y.to(DEV)
    outs = []
    for _ in range(2):
        _hip.call("ddpm_class_embed_bwd", d.t.data_ptr(), yd.data_ptr(), out.t.data_ptr(), B, E, K1, _hip.stream())
        outs.append(out.t.cpu().clone())
    assert d.intact() and out.intact() and bits(d.t.cpu(), dpre)
    assert bits(outs[0], outs[1]), "a second launch repeats the bits"
    return outs[0]


def label_cases(B, K1):
    g = torch.Generator().manual_seed(B)
    mixed = torch.randint(0, K1, (B,), generator=g)
    mixed[mixed == 1] = 0                                                             # class 1 has no sample
    stray = mixed.clone()
    stray[0] = -1                                                                     # out of range: contributes nothing
    if B > 1:
        stray[B - 1] = K1
    return {"all equal": torch.full((B,), 2), "a class without a sample": mixed, "all null": torch.full((B,), K1 - 1), "out of range": stray}


@pytest.mark.parametrize("E", [64, 300])
@pytest.mark.parametrize("B", [1, 7, 257])
def test_class_embed_bwd_fixed_order_sums(B, E):
    K1 = 4
    ints = torch.randint(-8, 9, (B, E), generator=torch.Generator().manual_seed(E)).float()
    rand = r(B, E, seed=B) * torch.logspace(-3, 3, E)[None, :]
    worst = 0.0
    for name, y in label_cases(B, K1).items():
        own = (y[:, None] == torch.arange(K1)[None, :]).double()                      # [B, K1]
        got = embed_bwd(ints, y, K1)
        assert torch.equal(got.double(), own.T @ ints.double()), name                 # exact, and 0.0 (not the poison) where no sample is
        got = embed_bwd(rand, y, K1)
        want, mag = own.T @ rand.double(), own.T @ rand.double().abs()
        bar = (B - 1) * U24 * mag
        err = (got.double() - want).abs()
        assert bool((err <= bar).all()), (name, float((err / bar.clamp_min(1e-300)).max()))
        worst = max(worst, float((err / bar.clamp_min(1e-300))[bar > 0].max()) if bool((bar > 0).any()) else 0.0)
        empty = own.sum(0) == 0
        assert bool((got[empty] == 0).all()) and not bool(torch.isnan(got).any())
    print(f"\n  B={B} E={E}: worst err/bar {worst:.3f}")


# ------------------------------------------------------------------------------------------------------------------ ddpm_p_sample_step_cfg
T_STEP = 1000


@functools.lru_cache(maxsize=None)
def tabs64():
    tb = LR.tables(D.beta_schedule("linear", 1e-4, 0.02, T_STEP))                     # fp32-rounded tables carried in float64
    tb["fixed_model_logvar"] = tb["model_logvar_max"]
    return tb


@functools.lru_cache(maxsize=None)
def dev_tabs():
    return [tabs64()[k].float().to(DEV) for k in STEP]


@functools.lru_cache(maxsize=None)
def step_case(B, n, t):
    return dict(B=B, n=n, t=torch.tensor(t), xt=r(B, n, seed=n + 1), out2=r(2 * B, n, seed=n + 2) * 0.8, z=r(B, n, seed=n + 3))


def step_cfg(c, scale, mean_type, clip, dup, t=None, inplace=False, want_pred=True, offset=0):
    B, n = c["B"], c["n"]
    rows = 2 * B if dup else B
    x = Guarded((rows, n), offset=offset)
    x.t[:B].copy_(c["xt"])
    o2, z = Guarded((2 * B, n), values=c["out2"], offset=offset), Guarded((B, n), values=c["z"], offset=offset)
    dst = x if inplace else Guarded((rows, n), offset=offset)
    pred = Guarded((B, n), offset=offset) if want_pred else None
    tt = (c["t"] if t is None else t).to(DEV)
    _hip.call("ddpm_p_sample_step_cfg", x.t.data_ptr(), o2.t.data_ptr(), z.t.data_ptr(), tt.data_ptr(), *[v.data_ptr() for v in dev_tabs()], float(scale),
              dst.t.data_ptr(), pred.t.data_ptr() if want_pred else 0, B, n, mean_type, clip, dup, T_STEP, _hip.stream())
    torch.cuda.synchronize()
    assert all(g.intact() for g in (x, o2, z, dst) + ((pred,) if want_pred else ())), "a guard region was written"
    assert bits(o2.t.cpu(), c["out2"]) and bits(z.t.cpu(), c["z"])
    if not inplace:
        assert bits(x.t[:B].cpu(), c["xt"]) and (not dup or bool(torch.isnan(x.t[B:]).all())), "x_t was written, or its second half read as state"
    return dst.t.cpu(), (pred.t.cpu() if want_pred else None)


def step_plain(c, half, mean_type, clip):
    B, n = c["B"], c["n"]
    x, o, z, tt = c["xt"].to(DEV), c["out2"][half * B:(half + 1) * B].contiguous().to(DEV), c["z"].to(DEV), c["t"].to(DEV)
    x_prev, pred = torch.empty_like(x), torch.empty_like(x)
    _hip.call("ddpm_p_sample_step", x.data_ptr(), o.data_ptr(), z.data_ptr(), tt.data_ptr(), *[v.data_ptr() for v in dev_tabs()], x_prev.data_ptr(),
              pred.data_ptr(), B, n, mean_type, clip, T_STEP, _hip.stream())
    return x_prev.cpu(), pred.cpu()


def step_bar(c, scale, mean_type):
    """(E_x, E_0) of the module docstring, in float64 from the float64 reference's own intermediate values."""
    tb, t = tabs64(), c["t"]
    g_ = lambda k: tb[k][t][:, None]                                                       # noqa: E731
    xt, z, B = c["xt"].double(), c["z"].double(), c["B"]
    oc, ou = c["out2"][:B].double(), c["out2"][B:].double()
    rest = float(torch.tensor(1.0) - torch.tensor(scale, dtype=torch.float32))
    g = scale * oc + rest * ou
    e_g = 2 * U24 * ((scale * oc).abs() + (rest * ou).abs())
    a, b, c1, c2 = g_("sqrt_recip_alphas_bar"), g_("sqrt_recip_m1_alphas_bar"), g_("posterior_mean_coef1"), g_("posterior_mean_coef2")
    if mean_type == 0:
        x0 = a * xt - b * g
        e_0 = b * e_g + 2 * U24 * ((a * xt).abs() + (b * g).abs())
    elif mean_type == 1:
        x0, e_0 = g, e_g
    else:
        x0 = g / c1 - c2 / c1 * xt
        e_0 = e_g / c1 + 2 * U24 * ((g / c1).abs() + (xt * c2 / c1).abs())
    if mean_type == 2:
        terms, e_m = g.abs(), e_g
    else:
        terms = (c1 * x0).abs() + (c2 * xt).abs()                             # (|x0| before the clip bounds |x0| after it)
        e_m = c1 * e_0 + 2 * U24 * terms
    noise = (t > 0).double()[:, None] * torch.exp(0.5 * g_("fixed_model_logvar")) * z.abs()
    return e_m + U24 * (terms + noise) + 3 * U24 * noise, e_0


STEP_WORST = {"x_prev": 0.0, "pred_x0": 0.0}


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("n", [1, 3, 63, 64, 65, 1440, 3072])
def test_guided_step_known_answers_and_float64(B, n):
    """Every mean type, clip on and off, dup 0 and 1, t = 0 among the samples (B = 1: t = 0 and t = T - 1 in turn); odd n takes the
    element-wise path for b > 0, and a base one float off the 16-byte grid takes it for every sample — the same bits."""
    for t in ([(0,), (T_STEP - 1,)] if B == 1 else [(0, 1, T_STEP - 1)]):
        c = step_case(B, n, t)
        for mean_type in range(3):
            for clip in (0, 1):
                plain = [step_plain(c, half, mean_type, clip) for half in (0, 1)]
                for dup in (0, 1):
                    for scale, half in ((1.0, 0), (0.0, 1)):                         # the bits of ddpm_p_sample_step on that half
                        x_prev, pred = step_cfg(c, scale, mean_type, clip, dup)
                        assert bits(x_prev[:B], plain[half][0]) and bits(pred, plain[half][1]), (mean_type, clip, dup, scale)
                        assert not dup or bits(x_prev[B:], x_prev[:B])
                for scale in (0.5, 3.0, 7.5):
                    x_prev, pred = step_cfg(c, scale, mean_type, clip, 1)
                    x64, p64 = R.guided_step(tabs64(), R.MEAN_TYPES[mean_type], c["xt"].double(), c["t"], c["out2"][:B].double(), c["out2"][B:].double(),
                                             c["z"].double(), scale, bool(clip))
                    e_x, e_0 = step_bar(c, scale, mean_type)
                    rx, rp = float(((x_prev[:B].double() - x64).abs() / e_x).max()), float(((pred.double() - p64).abs() / e_0).max())
                    STEP_WORST["x_prev"], STEP_WORST["pred_x0"] = max(STEP_WORST["x_prev"], rx), max(STEP_WORST["pred_x0"], rp)
                    assert rx <= 1.0 and rp <= 1.0, (mean_type, clip, scale, rx, rp)
                    assert bits(x_prev[B:], x_prev[:B])
                    # in place equals out of place; no pred_x0 buffer; a base off the 16-byte grid
                    assert bits(step_cfg(c, scale, mean_type, clip, 1, inplace=True, want_pred=False)[0], x_prev)
                    off = step_cfg(c, scale, mean_type, clip, 1, offset=1)
                    assert bits(off[0], x_prev) and bits(off[1], pred)
    print(f"\n  n={n} B={B}: worst err/bar so far x_prev {STEP_WORST['x_prev']:.3f}, pred_x0 {STEP_WORST['pred_x0']:.3f}")


@pytest.mark.parametrize("n", [3, 64, 1440])
def test_guided_step_bad_t_poisons_both_rows_of_its_sample_only(n):
    c = step_case(3, n, (0, 1, T_STEP - 1))
    good = step_cfg(c, 3.0, 0, 1, 1)
    for bad in (-1, T_STEP, 1 << 40):
        t = c["t"].clone()
        t[1] = bad
        x_prev, pred = step_cfg(c, 3.0, 0, 1, 1, t=t)
        assert bool(torch.isnan(x_prev[1]).all()) and bool(torch.isnan(x_prev[4]).all()) and bool(torch.isnan(pred[1]).all())
        keep = [0, 2, 3, 5]
        assert bits(x_prev[keep], good[0][keep]) and bits(pred[[0, 2]], good[1][[0, 2]])


# ------------------------------------------------------------------------------------------------------------------ the conditional UNet
K = 3
REDUCED = dict(in_channels=3, hid_channels=64, out_channels=3, ch_multipliers=[1, 2, 2], num_res_blocks=1, apply_attn=[False, True, False], drop_rate=0.0)
NET_SHAPE = (4, 3, 16, 16)
LABELS = (0, 2, K, 0)                                   # a class with two samples, one with one, the null class, class 1 with none


@functools.lru_cache(maxsize=None)
def weights():
    torch.manual_seed(5)
    m = ddpm_torch.UNet(**REDUCED, num_classes=K)
    sd = U.randomize_state_dict(m.state_dict(), 17)
    return sd, {k: v.double() for k, v in sd.items()}


def model_of(sd, dtype=torch.float32, conditional=True):
    m = ddpm_torch.UNet(**REDUCED, num_classes=K if conditional else None)
    m.load_state_dict(sd if conditional else {k: v for k, v in sd.items() if k != R.TABLE})
    return m.to(DEV).set_compute_dtype(dtype)


@functools.lru_cache(maxsize=None)
def net_reference():
    """Forward and every parameter's gradient of the conditional oracle network, once."""
    sd, sd64 = weights()
    x, t, y, gy = r(*NET_SHAPE, seed=1), torch.tensor([3, 977, 40, 500]), torch.tensor(LABELS), r(*NET_SHAPE, seed=2)
    p = {k: v.clone().requires_grad_(True) for k, v in sd64.items()}
    out = R.unet_forward(p, REDUCED, x.double(), t, y, training=True)
    (out * gy.double()).sum().backward()
    return x, t, y, gy, out.detach(), {k: v.grad for k, v in p.items()}


def test_conditional_forward_and_every_gradient_against_the_float64_restatement():
    sd, _ = weights()
    x, t, y, gy, out64, grads64 = net_reference()
    m = model_of(sd).train()
    out = m(x.to(DEV), t.to(DEV), y.to(DEV))
    err = check(out, out64, FP32_BAR, name="forward")
    (out * gy.to(DEV)).sum().backward()
    scales = {k: float(v.abs().max()) for k, v in grads64.items()}
    floor = 0.02 * sorted(scales.values())[len(scales) // 2]
    ratios = {k: float((q.grad.cpu().double() - grads64[k]).abs().max()) / max(scales[k], floor) for k, q in m.named_parameters()}
    worst = max(ratios, key=ratios.get)
    print(f"\n  forward rel err {err:.3e}; worst gradient {worst} {ratios[worst]:.3e}; d table {ratios[R.TABLE]:.3e}")
    assert ratios[worst] < 3e-3, (worst, ratios[worst])
    gt = m.class_embed.weight.grad.cpu()
    assert bool((gt[1] == 0).all()) and all(float(gt[k].abs().max()) > 0 for k in (0, 2, 3)), "class 1 has no sample: exactly zero"


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_a_zero_class_table_is_the_unconditional_network_bit_for_bit(dtype):
    sd, _ = weights()
    x, t, y = net_reference()[:3]
    plain = model_of(sd, dtype, conditional=False).eval()
    zero = model_of(dict(sd, **{R.TABLE: torch.zeros_like(sd[R.TABLE])}), dtype).eval()
    with torch.no_grad():
        a, b = plain(x.to(DEV), t.to(DEV)), plain(x.to(DEV), t.to(DEV))
        assert torch.equal(a, b), "the premise: two unconditional forwards repeat their bits"
        assert torch.equal(zero(x.to(DEV), t.to(DEV), y.to(DEV)), a) and torch.equal(zero(x.to(DEV), t.to(DEV)), a)


# ------------------------------------------------------------------------------------------------------------------ samplers
CHAIN_T, CHAIN_SHAPE, CHAIN_Y = 8, (3, 3, 16, 16), (2, 0, 1)


@functools.lru_cache(maxsize=None)
def chain_reference(kind):
    sd, sd64 = weights()
    g = torch.Generator().manual_seed(41)
    x_T, zs = torch.randn(CHAIN_SHAPE, generator=g), torch.randn((CHAIN_T,) + CHAIN_SHAPE, generator=g)
    y = torch.tensor(CHAIN_Y)
    net = lambda x, t, yy: R.unet_forward(sd64, REDUCED, x, t, yy)                         # noqa: E731
    betas = D.beta_schedule("linear", 1e-4, 0.02, CHAIN_T)
    preds = []
    with torch.no_grad():
        if kind == "ddpm":
            ref = R.guided_chain(D.ddpm_tables(betas, "fixed-large"), "eps", net, x_T.double(), zs.double(), y, K, 2.0, preds=preds)
        else:
            sub = D.selection_schedule("linear", 4, CHAIN_T)
            ref = R.guided_chain(D.ddim_tables(betas, "fixed-small", 0.0, sub), "eps", net, x_T.double(), torch.zeros(4, *CHAIN_SHAPE, dtype=torch.float64),
                                 y, K, 2.0, timestep_map=sub)
    return x_T, zs, y, ref, preds


def test_guided_chain_replayed_equals_eager_and_matches_the_float64_chain(monkeypatch):
    """T = 8, scale 2, B = 3 (a 6-row network call per step), injected noise: the replayed chain equals the eager one bit for bit, both
    are within FP32_BAR of the float64 chain, scale 1 with labels is the plain conditional chain, and the progressive sampler returns
    B-row predictions."""
    sd, _ = weights()
    x_T, zs, y, ref, preds64 = chain_reference("ddpm")
    m = model_of(sd).eval()
    dif = ddpm_torch.GaussianDiffusion(ddpm_torch.get_beta_schedule("linear", 1e-4, 0.02, CHAIN_T), "eps", "fixed-large", "mse")
    outs = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("DDPM_TORCH_AMD_GRAPH", mode)
        with torch.inference_mode():
            outs[mode] = dif._sample_loop(m, CHAIN_SHAPE, DEV, x_T, None, z_stream=iter(zs), y=y.to(DEV), guidance_scale=2.0)
            outs[mode + "c"] = dif._sample_loop(m, CHAIN_SHAPE, DEV, x_T, None, z_stream=iter(zs), y=y.to(DEV), guidance_scale=1.0)
        outs[mode + "s"] = dif.p_sample(m, shape=CHAIN_SHAPE, device=DEV, seed=77, y=y.to(DEV), guidance_scale=2.0)
    kinds = {k[3][3] for k in dif._sample_graphs if len(k[3]) > 3}
    assert ("cfg", 2.0, K) in kinds and ("cond",) in kinds, "the guided and the conditional step were not captured under their own keys"
    assert outs["1"].shape == CHAIN_SHAPE and torch.equal(outs["1"], outs["0"]) and torch.equal(outs["1s"], outs["0s"]) and torch.equal(outs["1c"], outs["0c"])
    err = check(outs["1"], ref, FP32_BAR, name="guided chain")
    # scale 1 with y: the B-row conditional call and the existing step kernel, written out
    with torch.inference_mode():
        x = x_T.to(DEV).clone()
        for i, ti in enumerate(range(CHAIN_T - 1, -1, -1)):
            t = torch.full((3,), ti, dtype=torch.int64, device=DEV)
            x, _ = dif._step(x, m(x, t, y.to(DEV)), zs[i].to(DEV), t, dif.clip_sampling, False)
    assert torch.equal(outs["1c"], x)
    monkeypatch.setenv("DDPM_TORCH_AMD_GRAPH", "1")
    xp, preds = dif.p_sample_progressive(m, CHAIN_SHAPE, device=DEV, noise=x_T, pred_freq=4, z_stream=iter(zs), y=y.to(DEV), guidance_scale=2.0)
    assert torch.equal(xp, outs["1"].cpu()) and preds.shape == (2,) + CHAIN_SHAPE
    check(preds[1], preds64[0], FP32_BAR, name="pred_x0 at t = 7")
    check(preds[0], preds64[4], FP32_BAR, name="pred_x0 at t = 3")
    print(f"\n  guided chain rel err {err:.3e}")


def test_guided_ddim4_replayed_equals_eager_and_matches_the_float64_chain(monkeypatch):
    sd, _ = weights()
    x_T, _, y, ref, _ = chain_reference("ddim")
    m = model_of(sd).eval()
    sub = ddim.get_selection_schedule("linear", size=4, timesteps=CHAIN_T)
    dd = ddim.DDIM(ddpm_torch.get_beta_schedule("linear", 1e-4, 0.02, CHAIN_T), "eps", "fixed-small", "mse", eta=0.0, subsequence=sub)
    outs = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("DDPM_TORCH_AMD_GRAPH", mode)
        with torch.inference_mode():                         # (eta = 0: the noise is injected as zeros, as tests/test_learned_var_gpu.py does)
            outs[mode] = dd._sample_loop(m, CHAIN_SHAPE, DEV, x_T, None, z_stream=iter([torch.zeros(CHAIN_SHAPE)] * 4), y=y.to(DEV), guidance_scale=2.0)
    assert any(len(k[3]) > 3 and k[3][3] == ("cfg", 2.0, K) for k in dd._sample_graphs)
    assert torch.equal(outs["1"], outs["0"])
    err = check(outs["1"], ref, FP32_BAR, name="guided DDIM-4")
    print(f"\n  guided DDIM-4 rel err {err:.3e}")
    # the loops without a label input of their own: labels bound to the network, replayed = eager, and not the null-class result
    x_0 = (x_T * 0.5).clamp(-1, 1).to(DEV)
    dif = ddpm_torch.GaussianDiffusion(ddpm_torch.get_beta_schedule("linear", 1e-4, 0.02, CHAIN_T), "eps", "fixed-large", "kl")
    lat, bpd = {}, {}
    for mode in ("1", "0"):
        monkeypatch.setenv("DDPM_TORCH_AMD_GRAPH", mode)
        lat[mode] = dd.encode(m, x_0, y=y.to(DEV))
        bpd[mode] = dif.calc_all_bpd(m, x_0, seed=3, y=y.to(DEV))[0]
    assert torch.equal(lat["1"], lat["0"]) and torch.equal(bpd["1"], bpd["0"]) and bool(torch.isfinite(lat["1"]).all()) and bool(torch.isfinite(bpd["1"]).all())
    assert not torch.equal(lat["1"], dd.encode(m, x_0)) and not torch.equal(bpd["1"], dif.calc_all_bpd(m, x_0, seed=3)[0])


# ------------------------------------------------------------------------------------------------------------------ Trainer
def test_three_conditional_trainer_steps_match_the_float64_oracle_trainer():
    """B = 4, label_drop 0.5, lr 1e-3: the labels the step trained on are reproduced from the trainer's generator (t, noise, then B
    uniforms), the step is the generic autograd step (no launch plan) and follows the float64 oracle trainer."""
    from tests import channels_accum as CA
    sd, _ = weights()
    lr, B = 1e-3, 4
    m = model_of(sd)
    dif = ddpm_torch.GaussianDiffusion(ddpm_torch.get_beta_schedule("linear", 1e-4, 0.02, 1000), "eps", "fixed-large", "mse")
    opt = torch.optim.Adam(m.parameters(), lr=lr, betas=(0.9, 0.999))
    tr = ddpm_torch.Trainer(m, opt, dif, epochs=1, trainloader=None, scheduler=None, use_ema=True, grad_norm=1.0, shape=(3, 16, 16),
                            device=torch.device(DEV), ema_decay=0.9999, label_drop=0.5)
    twin = torch.Generator(DEV).manual_seed(CA.GEN_SEED)                              # the trainer's generator, drawn in step with it
    oracle = R.oracle_trainer(sd, REDUCED, lr, K)
    g = torch.Generator().manual_seed(21)
    m.train()
    losses, ref, dropped = [], [], 0
    for i in range(3):
        x = torch.rand(B, 3, 16, 16, generator=g) * 2 - 1
        y = torch.randint(0, K, (B,), generator=g)
        t = torch.empty((B,), dtype=torch.int64, device=DEV).random_(to=1000, generator=twin)
        noise = torch.empty(B, 3, 16, 16, device=DEV).normal_(generator=twin)
        y_used = R.dropped_labels(y, torch.rand((B,), device=DEV, generator=twin).cpu(), 0.5, K)
        dropped += int((y_used != y).sum())
        tr.stats.reset()
        tr.step((x, y), global_steps=i + 1)
        losses.append(tr.current_stats["loss"])
        ref.append(oracle.step(x, y_used, inputs=(t.cpu(), noise.cpu()))[0])
    assert not tr._direct and tr._direct_unet() is None, "the conditional step must not take the launch plan"
    assert 0 < dropped < 3 * B
    print(f"\n  losses {losses} vs oracle {ref}; {dropped} of {3 * B} labels dropped")
    assert torch.allclose(torch.tensor(losses, dtype=torch.float64), torch.tensor(ref, dtype=torch.float64), rtol=5e-4), (losses, ref)
    slack = 0.25 * lr * 3
    check_state({k: v.cpu() for k, v in m.state_dict().items()}, oracle.state(), 1e-3, "param", adam_slack=slack)
    check_state({k: v.cpu() for k, v in tr.ema.shadow.items()}, oracle.shadow, 1e-3, "shadow", adam_slack=slack)
