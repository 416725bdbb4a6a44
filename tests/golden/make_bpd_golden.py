"""Write fixture G18 (tests/golden/g18_bpd.pt): what ``GaussianDiffusion.calc_all_bpd`` means, composed from the LIVE functions of the
reference on the CPU (its own ``calc_all_bpd`` / ``_prior_bpd`` cannot run, diffusion.py:245-268): ``q_sample`` with given noise,
``_loss_term_bpd(clip_denoised, return_pred=True)``, ``flat_mean((pred - x_0)^2)``, ``q_mean_var`` and ``normal_kl`` with tensor zeros as
the prior's ``mean2`` / ``logvar2``.  Run where the reference checkout is available:

    python tests/golden/make_bpd_golden.py
"""
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import load_reference as LR  # noqa: E402


def all_bpd(ref, dif, x_0, noise, w, clip):
    """The loop of diffusion.py:258-268 with the tensors it meant; noise[i] is the draw of loop step i (t = T-1-i), the "network" is
    0.7 x_t + w[t]."""
    B, T = len(x_0), dif.timesteps
    F = ref.functions
    losses, mses = torch.zeros(B, T), torch.zeros(B, T)
    for i, ti in enumerate(range(T - 1, -1, -1)):
        t = torch.full((B,), ti, dtype=torch.int64)
        x_t = dif.q_sample(x_0, t, noise=noise[i])
        loss, pred = dif._loss_term_bpd(lambda x, tt: 0.7 * x + w[ti], x_0, x_t=x_t, t=t, clip_denoised=clip, return_pred=True)
        losses[:, ti] = loss
        mses[:, ti] = F.flat_mean((pred - x_0).pow(2))
    mean, _, logvar = dif.q_mean_var(x_0, (T - 1) * torch.ones((B,), dtype=torch.int64))
    prior = F.flat_mean(F.normal_kl(mean, logvar, torch.zeros_like(mean), torch.zeros_like(logvar))) / math.log(2.)
    return dict(losses=losses, mses=mses, prior=prior, total=losses.sum(dim=1) + prior)


def main():
    ref = LR.load()
    out = {}
    with torch.no_grad():
        g = torch.Generator().manual_seed(1818)
        T = 12
        x_0 = (torch.rand(5, 3, 8, 8, generator=g) * 2 - 1).clamp(-1, 1)
        x_0[0, 0, 0, :4] = torch.tensor([1.0, -1.0, 0.9995, -0.9995])          # both open tails of the discretised likelihood (as G16)
        noise = torch.randn(T, 5, 3, 8, 8, generator=g)
        w = torch.randn(T, 5, 3, 8, 8, generator=g) * 0.3
        # betas of 0.3 .. 0.9: with T = 12 the usual 1e-4 .. 0.02 leaves a decoder of sigma = 0.007 at t = 0, and for the x_0 / mean
        # parameterisations the stand-in network misses x_0 by tens of sigma — the reference's fp32 cdf_upper - cdf_lower is then rounding
        # noise against its 1e-12 floor, which no float64 restatement can reproduce.  Here sigma_0 = 0.44 and every element stays where
        # the fp32 difference is well conditioned (fp32 and float64 evaluations of the oracle agree to 0.3 of the test's bar).
        sched = ("linear", 0.3, 0.9, T)
        img = dict(x_0=x_0, noise=noise, w=w, schedule=sched, records={})
        for mean_type in ("eps", "x_0", "mean"):
            for var_type in ("fixed-small", "fixed-large"):
                dif = ref.GaussianDiffusion(ref.get_beta_schedule(*sched), mean_type, var_type, "kl")
                for clip in (True, False):
                    img["records"][f"{mean_type}/{var_type}/clip{int(clip)}"] = all_bpd(ref, dif, x_0, noise, w, clip)
        out["images"] = img
        T = 10
        x_0 = torch.randn(7, 2, generator=g) * 0.8
        noise = torch.randn(T, 7, 2, generator=g)
        w = torch.randn(T, 7, 2, generator=g) * 0.3
        sched = ("linear", 1e-3, 0.2, T)
        toy = dict(x_0=x_0, noise=noise, w=w, schedule=sched, records={})
        for mean_type in ("eps", "x_0", "mean"):
            for var_type in ("fixed-small", "fixed-large"):
                dif = ref.toy_diffusion.GaussianDiffusion(ref.get_beta_schedule(*sched), mean_type, var_type, "kl")
                toy["records"][f"{mean_type}/{var_type}"] = all_bpd(ref, dif, x_0, noise, w, True)      # (the toy class ignores clip_denoised)
        out["toy"] = toy
    torch.save(out, os.path.join(ROOT, "tests", "golden", "g18_bpd.pt"))


if __name__ == "__main__":
    main()
