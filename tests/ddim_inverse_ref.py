"""TEST INFRASTRUCTURE: a float64 restatement of DDIM inversion and latent interpolation (Song et al. 2020 §4.3, §5.3, eq. 67), written from
the equations — the upstream project has no such code.  The yardstick of tests/test_ddim_inverse_host.py and tests/test_ddim_inverse_gpu.py.

Conventions (those of ddim.py): ``ab[i] = alphas_bar[subsequence[i]]``, ``ab_prev[i] = ab[i-1]``, ``ab_prev[0] = 1``.  Encode step i takes the
state from level i-1 to level i, decode step i takes it back; both evaluate the network at ``subsequence[i]``."""
import torch

F64 = torch.float64


def tables(betas, subsequence, dtype=F64):
    """Every table of the two directions at eta = 0.  ``dtype`` = torch.float32 rounds each table once, like the product's device copies,
    and returns it in float64 again (the kernel tests hold the kernels to float64 arithmetic ON the fp32 tables)."""
    betas = torch.as_tensor(betas, dtype=F64)
    sub = torch.as_tensor(subsequence, dtype=torch.int64)
    ab = torch.cumprod(1.0 - betas, 0)[sub]
    ab_prev = torch.cat([torch.ones(1, dtype=F64), ab[:-1]])
    coef2 = torch.sqrt(1.0 - ab) * torch.sqrt(1.0 - ab_prev) / (1.0 - ab)                 # Song et al. eq. 12 at sigma = 0
    tb = dict(
        ab=ab, ab_prev=ab_prev,
        cx=torch.sqrt(ab / ab_prev),
        ce=torch.sqrt(1.0 - ab) - torch.sqrt(ab * (1.0 - ab_prev) / ab_prev),
        recip_prev=torch.sqrt(1.0 / ab_prev), recip_m1_prev=torch.sqrt(1.0 / ab_prev - 1.0),
        recip=torch.sqrt(1.0 / ab), recip_m1=torch.sqrt(1.0 / ab - 1.0),
        coef1=torch.sqrt(ab_prev) * (1.0 - torch.sqrt(ab / ab_prev) * coef2), coef2=coef2,
    )
    tb = {k: v.to(dtype).to(F64) for k, v in tb.items()}
    tb["subsequence"] = sub
    return tb


def _col(v, x):
    return v.reshape((-1,) + (1,) * (x.ndim - 1))


def encode_step(tb, x, eps, t):
    """(x_next, pred_x0) of one step at the per-sample indices ``t`` ([B] int64); a sample whose index is outside the tables is NaN."""
    S = len(tb["cx"])
    ok = (t >= 0) & (t < S)
    tc = t.clamp(0, S - 1)
    g = lambda k: _col(tb[k][tc], x)                                                      # noqa: E731
    x, eps = x.to(F64), eps.to(F64)
    nxt = g("cx") * x + g("ce") * eps
    pred = g("recip_prev") * x - g("recip_m1_prev") * eps
    bad = _col(~ok, x)
    nan = torch.full_like(x, float("nan"))
    return torch.where(bad, nan, nxt), torch.where(bad, nan, pred)


def decode_step(tb, x_t, eps, t, clip=False):
    """The eta = 0 sampling update (no noise): x_0 = recip x_t - recip_m1 eps (optionally clipped), x_prev = coef1 x_0 + coef2 x_t."""
    g = lambda k: _col(tb[k][t], x_t)                                                     # noqa: E731
    x_t, eps = x_t.to(F64), eps.to(F64)
    x0 = g("recip") * x_t - g("recip_m1") * eps
    if clip:
        x0 = x0.clamp(-1.0, 1.0)
    return g("coef1") * x0 + g("coef2") * x_t


def encode(tb, model, x_0):
    """S encode steps; ``model(x, model_t)`` gets float64 ``x`` and the [B] int64 model timesteps ``subsequence[i]``."""
    x = x_0.to(F64)
    B = x.shape[0]
    for i in range(len(tb["cx"])):
        t = torch.full((B,), i, dtype=torch.int64)
        x, _ = encode_step(tb, x, model(x, tb["subsequence"][t]), t)
    return x


def decode(tb, model, latent, clip=False):
    x = latent.to(F64)
    B = x.shape[0]
    for i in range(len(tb["cx"]) - 1, -1, -1):
        t = torch.full((B,), i, dtype=torch.int64)
        x = decode_step(tb, x, model(x, tb["subsequence"][t]), t, clip)
    return x


def slerp_weights(a, b, alphas):
    """[P, K, 2] float64 weights (w0, w1) of ``slerp``; the linear ones when 1 - |c| < 1e-6 or c is not finite."""
    a, b = a.to(F64).flatten(1), b.to(F64).flatten(1)
    al = torch.as_tensor(alphas).to(F64).reshape(1, -1)
    c = ((a * b).sum(1) / (a.norm(dim=1) * b.norm(dim=1))).clamp(-1.0, 1.0)
    linear = ~((1.0 - c.abs()) >= 1e-6)
    th = torch.acos(torch.where(linear, torch.zeros_like(c), c))[:, None]
    w0 = torch.sin((1.0 - al) * th) / torch.sin(th)
    w1 = torch.sin(al * th) / torch.sin(th)
    w0 = torch.where(linear[:, None], (1.0 - al).expand_as(w0), w0)
    w1 = torch.where(linear[:, None], al.expand_as(w1), w1)
    return torch.stack([w0, w1], dim=-1)


def slerp(a, b, alphas):
    """[P, K, ...] float64: out[p][k] = w0 a[p] + w1 b[p] over the whole flattened sample (NaN operands propagate through the products)."""
    w = slerp_weights(a, b, alphas)
    P, K = w.shape[:2]
    shape = (P, K) + (1,) * (a.ndim - 1)
    return w[..., 0].reshape(shape) * a.to(F64)[:, None] + w[..., 1].reshape(shape) * b.to(F64)[:, None]
