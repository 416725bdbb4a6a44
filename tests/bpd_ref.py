"""TEST INFRASTRUCTURE: what ``GaussianDiffusion.calc_all_bpd`` computes, composed from ``oracle/diffusion_ref.py`` (pinned to the reference
by fixtures G16 / G18) plus the toy pipeline's continuous-Gaussian likelihood.  Everything follows the dtype of its inputs: float64 inputs
give the reference the kernels are held to, float32 inputs give the fp32 torch evaluation whose own error scales a bar."""
import math

import torch

from oracle import diffusion_ref as D


def continuous_gaussian_nll(x, mean, logvar):
    """-continuous_gaussian_loglik (functions.py:68-72)."""
    return 0.5 * ((x - mean) ** 2 * torch.exp(-logvar) + math.log(2 * math.pi) + logvar)


def tables(T, dtype=torch.float64):
    """The fp64 host tables as the kernels see them: rounded to fp32, then carried in ``dtype``."""
    return {k: (v.to(torch.float32).to(dtype) if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in T.items()}


def terms(T, mean_type, x_0, x_t, t, out, clip, decoder=0):
    """(L_t [B] in bits/dim, mean (pred_x_0 - x_0)^2 [B]): `_loss_term_bpd` (diffusion.py:203-215; toy/diffusion.py:52-64 for decoder 1) and
    the MSE of diffusion.py:264."""
    if decoder == 0:
        loss, pred = D.loss_term_bpd(T, mean_type, x_0, x_t, t, out, clip)
    else:
        true_mean = D._gather(T["posterior_mean_coef1"], t, x_0) * x_0 + D._gather(T["posterior_mean_coef2"], t, x_0) * x_t
        mean, pred = D.model_mean_from_output(T, mean_type, x_t, t, out, clip)
        logvar = D._gather(T["fixed_model_logvar"], t, x_t)
        kl = D.normal_kl(true_mean, D._gather(T["posterior_logvar_clipped"], t, x_0), mean, logvar).flatten(1).mean(1) / math.log(2.0)
        nll = continuous_gaussian_nll(x_0, mean, logvar).flatten(1).mean(1) / math.log(2.0)
        loss = torch.where(t > 0, kl, nll)
    return loss, ((pred - x_0) ** 2).flatten(1).mean(1)


def prior_bpd(T, x_0):
    """diffusion.py:245-250 with the tensors it meant."""
    last = len(T["alphas_bar"]) - 1
    t = torch.full((len(x_0),), last, dtype=torch.int64)
    mean = D._gather(T["sqrt_alphas_bar"], t, x_0) * x_0
    logvar = D._gather(torch.log(1.0 - T["alphas_bar"]), t, x_0)
    return D.normal_kl(mean, logvar, torch.zeros_like(mean), torch.zeros_like(logvar)).flatten(1).mean(1) / math.log(2.0)


def all_bpd(T, mean_type, x_0, noise, net, clip, decoder=0):
    """The loop of diffusion.py:258-268: noise[i] is the draw of loop step i (t = steps-1-i); ``net(x_t, t)`` is the network."""
    B, steps = len(x_0), len(T["alphas_bar"])
    losses, mses = x_0.new_zeros(B, steps), x_0.new_zeros(B, steps)
    for i, ti in enumerate(range(steps - 1, -1, -1)):
        t = torch.full((B,), ti, dtype=torch.int64)
        x_t = D.q_sample(T, x_0, t, noise[i].to(x_0))
        losses[:, ti], mses[:, ti] = terms(T, mean_type, x_0, x_t, t, net(x_t, t), clip, decoder)
    prior = prior_bpd(T, x_0)
    return dict(losses=losses, mses=mses, prior=prior, total=losses.sum(1) + prior)
