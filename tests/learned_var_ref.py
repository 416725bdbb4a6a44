"""TEST INFRASTRUCTURE: what a ``GaussianDiffusion`` with a learned reverse-process variance computes (model_var_type "learned",
diffusion.py:111-114, and "learned-range", Nichol & Dhariwal 2021 eq. 15; the hybrid loss of eq. 16), composed from ``oracle/diffusion_ref.py``
functions only (``normal_kl``, ``discretized_gaussian_loglik``, ``model_mean_from_output``, ``q_sample``: pinned to the reference by fixtures
G16 / G18).  The network output is ``[B, 2C, ...]``: channels [0, C) the mean output, [C, 2C) v.  Everything follows the dtype of its
inputs: float64 inputs give the reference the kernels are held to, float32 inputs the fp32 torch evaluation whose own error scales a bar.
Gradients come from torch.autograd on these functions; the stop-gradient of the hybrid loss is ``.detach()``.  ``oracle_trainer`` puts the
hybrid loss into the float64 oracle of ``Trainer.step`` that tests/channels_accum.py holds."""
import math

import torch

from oracle import diffusion_ref as D
from tests import bpd_ref

MEAN_TYPES = ("eps", "x_0", "mean")
VAR_TYPES = (None, "learned", "learned-range")           # indexed by the kernels' var_mode (0 = a fixed table, "fixed_model_logvar")
LN2 = math.log(2.0)


def tables(betas, dtype=torch.float64):
    """The fp64 host tables as the kernels see them (rounded to fp32, carried in ``dtype``): oracle ``ddpm_tables`` with the "fixed-large"
    log-variance under the name lv_max goes by in the product, ``model_logvar_max``; lv_min is ``posterior_logvar_clipped``."""
    T = D.ddpm_tables(betas, "fixed-large")
    T["model_logvar_max"] = T.pop("fixed_model_logvar")
    T.pop("fixed_model_var")
    return bpd_ref.tables(T, dtype)


def split(out):
    C = out.shape[1] // 2
    return out[:, :C], out[:, C:]


def model_logvar(T, var_type, v, t):
    if var_type is None:
        return D._gather(T["fixed_model_logvar"], t, v)
    if var_type == "learned":
        return v
    f = (v + 1.0) / 2.0
    return f * D._gather(T["model_logvar_max"], t, v) + (1.0 - f) * D._gather(T["posterior_logvar_clipped"], t, v)


def loss_target(T, mean_type, x_0, x_t, t, noise):
    if mean_type == "eps":
        return noise
    if mean_type == "x_0":
        return x_0
    return D._gather(T["posterior_mean_coef1"], t, x_0) * x_0 + D._gather(T["posterior_mean_coef2"], t, x_0) * x_t


def step(T, mean_type, var_type, x_t, t, out, z, clip):
    """(x_{t-1}, pred_x_0): diffusion.py:107-158 with the per-element log-variance."""
    o, v = split(out)
    mean, pred = D.model_mean_from_output(T, mean_type, x_t, t, o, clip)
    mask = (t > 0).reshape((-1,) + (1,) * (x_t.ndim - 1)).to(x_t)
    return mean + mask * torch.exp(0.5 * model_logvar(T, var_type, v, t)) * z, pred


def loss_term(T, mean_type, var_type, x_0, x_t, t, out, clip, detach_mean=False):
    """`_loss_term_bpd` (diffusion.py:203-215): (L_t [B] in bits/dim, pred_x_0)."""
    o, v = split(out)
    true_mean = D._gather(T["posterior_mean_coef1"], t, x_0) * x_0 + D._gather(T["posterior_mean_coef2"], t, x_0) * x_t
    true_logvar = D._gather(T["posterior_logvar_clipped"], t, x_0)
    mean, pred = D.model_mean_from_output(T, mean_type, x_t, t, o, clip)
    if detach_mean:
        mean = mean.detach()
    lv = model_logvar(T, var_type, v, t)
    kl = D.normal_kl(true_mean, true_logvar, mean, lv).flatten(1).mean(1) / LN2
    nll = (-D.discretized_gaussian_loglik(x_0, mean, log_scale=0.5 * lv)).flatten(1).mean(1) / LN2
    return torch.where(t > 0, kl, nll), pred


def terms(T, mean_type, var_type, x_0, x_t, t, out, clip):
    """(L_t [B], mean (pred_x_0 - x_0)^2 [B]): one column of `calc_all_bpd`."""
    loss, pred = loss_term(T, mean_type, var_type, x_0, x_t, t, out, clip)
    return loss, ((pred - x_0) ** 2).flatten(1).mean(1)


def weighted_loss(T, mean_type, var_type, x_0, x_t, t, out, target, w_mse, w_vlb, detach_mean):
    """w_mse * mean (out_mean - target)^2 + w_vlb * L_t: (1, vlb_weight, True) is the hybrid loss (eq. 16), (0, 1, False) loss_type "kl"."""
    loss = 0.0
    if w_mse != 0:
        loss = loss + w_mse * ((split(out)[0] - target) ** 2).flatten(1).mean(1)
    if w_vlb != 0:
        loss = loss + w_vlb * loss_term(T, mean_type, var_type, x_0, x_t, t, out, False, detach_mean)[0]
    return loss


def all_bpd(T, mean_type, var_type, x_0, noise, net, clip):
    """The loop of diffusion.py:258-268: noise[i] is the draw of loop step i (t = steps-1-i); ``net(x_t, t)`` is the 2C-channel network."""
    B, steps = len(x_0), len(T["alphas_bar"])
    losses, mses = x_0.new_zeros(B, steps), x_0.new_zeros(B, steps)
    for i, ti in enumerate(range(steps - 1, -1, -1)):
        t = torch.full((B,), ti, dtype=torch.int64)
        x_t = D.q_sample(T, x_0, t, noise[i].to(x_0))
        losses[:, ti], mses[:, ti] = terms(T, mean_type, var_type, x_0, x_t, t, net(x_t, t), clip)
    prior = bpd_ref.prior_bpd(T, x_0)
    return dict(losses=losses, mses=mses, prior=prior, total=losses.sum(1) + prior)


def sample_chain(T, mean_type, var_type, net, x_T, zs, clip=True):
    """diffusion.py:160-174 with injected noise: x_T, then zs[i] for loop step i (t = steps-1-i)."""
    x, steps = x_T, len(T["alphas_bar"])
    for i, ti in enumerate(range(steps - 1, -1, -1)):
        t = torch.full((len(x),), ti, dtype=torch.int64)
        x, _ = step(T, mean_type, var_type, x, t, net(x, t), zs[i].to(x), clip)
    return x


def oracle_trainer(sd, cfg, lr, mean_type, var_type, vlb_weight, **kw):
    """tests/channels_accum.py's float64 oracle of ``Trainer.step`` with the hybrid loss in the place of its eps-MSE (everything after the
    loss — accumulation, clip, Adam, scheduler, EMA — is that class's)."""
    from tests import channels_accum as CA

    class HybridOracleTrainer(CA.OracleTrainer):
        def __init__(self):
            super().__init__(sd, cfg, lr, **kw)
            self.lv_tables = tables(self.tables["betas"])

        def step(self, x, masks=None, inputs=None):
            t, noise = self.draw(x) if inputs is None else inputs
            x, noise = x.double(), noise.double()
            T = self.lv_tables
            x_t = D.q_sample(T, x, t, noise)
            out = self.denoise(x_t, t, training=True, masks=masks)
            loss = weighted_loss(T, mean_type, var_type, x, x_t, t, out, loss_target(T, mean_type, x, x_t, t, noise), 1.0, vlb_weight, True).mean()
            (loss / self.num_accum).backward()
            self.calls += 1
            updated = self.calls % self.num_accum == 0
            if updated:
                torch.nn.utils.clip_grad_norm_(list(self.params.values()), max_norm=self.grad_norm)
                self.opt.step()
                self.opt.zero_grad(set_to_none=True)
                if self.sched is not None:
                    self.sched.step()
                self.num_updates += 1
                d = min(self.ema_decay, (1 + self.num_updates) / (10 + self.num_updates))
                with torch.no_grad():
                    for k, p in self.params.items():
                        self.shadow[k] += (1 - d) * (p.data - self.shadow[k])
            return float(loss.detach()), updated

    return HybridOracleTrainer()
