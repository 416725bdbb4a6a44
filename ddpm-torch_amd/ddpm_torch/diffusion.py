"""Gaussian diffusion process with the reference's constructor and method contract
(``ddpm_torch/diffusion.py:13-243`` of tqch/ddpm-torch), re-built around device-resident tables.

The reference re-uploads an fp64 table from the host on every ``_extract`` call (two per ``q_sample``,
six or more per sampling step).  Here the fp64 tables are kept as attributes (same names; ``DDIM.from_ddpm``
and checkpoints of hyper-parameters read them), an fp32 copy is uploaded ONCE per device, and each of
``q_sample``, the eps-MSE loss and the ancestral step is a single fused HIP kernel that gathers its
per-sample coefficients by ``t`` on the device:

    x_t      = sqrt(ab_t) x_0 + sqrt(1 - ab_t) eps                                  (diffusion.py:92-97)
    loss_b   = mean_chw (eps - eps_hat)^2                                           (:236-239)
    x_{t-1}  = c1_t clamp(r_t x_t - m_t eps_hat, -1, 1) + c2_t x_t + 1[t>0] exp(logvar_t / 2) z   (:99-158)

Arithmetic is fp32 with the reference's operation order (no fused multiply-add contraction) so identical
(x_t, t, noise) give matching results.  No CPU path: CPU tensors raise.
"""
import contextlib
import os

import torch

from . import _hip
from ._graphs import SegmentedGraph

__all__ = ["get_beta_schedule", "GaussianDiffusion", "repaint_schedule"]

_F64 = torch.float64


def get_beta_schedule(beta_schedule, beta_start, beta_end, timesteps, dtype=_F64):
    """Same schedules and names as diffusion.py:13-29."""
    def ramp(frac):
        out = torch.full((timesteps,), beta_end, dtype=dtype)
        k = int(timesteps * frac)
        out[:k] = torch.linspace(beta_start, beta_end, k, dtype=dtype)
        return out

    table = {
        "quad": lambda: torch.linspace(beta_start ** 0.5, beta_end ** 0.5, timesteps, dtype=dtype) ** 2,
        "linear": lambda: torch.linspace(beta_start, beta_end, timesteps, dtype=dtype),
        "warmup10": lambda: ramp(0.1),
        "warmup50": lambda: ramp(0.5),
        "const": lambda: torch.full((timesteps,), beta_end, dtype=dtype),
        "jsd": lambda: 1.0 / torch.linspace(timesteps, 1, timesteps, dtype=dtype),
    }
    if beta_schedule not in table:
        raise NotImplementedError(beta_schedule)
    betas = table[beta_schedule]()
    assert betas.shape == (timesteps,)
    return betas


def repaint_schedule(S, jump_length=1, resamples=1, start=None):
    """The order of operations of a RePaint chain (Lugmayr et al. 2022, Algorithm 1 with the jumps of its §4.2) on S levels: a list of
    ``"down"`` (one reverse step: a network call, the state goes from index i to i - 1) and ``"up"`` (one forward jump from i to
    i + jump_length).  The chain begins at index ``top`` = S - 1, or ``start``, and ends at -1 (the clean image).  After a reverse step
    arrives at index i it jumps when 0 <= i <= top - j, (top - i) % j == 0 and fewer than ``resamples`` - 1 jumps have been taken from i,
    so every stretch of j levels below ``top`` is walked ``resamples`` times: (top + 1) + (resamples - 1) * j * (top // j) network calls.
    ``resamples`` = 1 is the plain replacement method (no jump)."""
    S, j, r = int(S), int(jump_length), int(resamples)
    top = S - 1 if start is None else int(start)
    if S < 1 or not 0 <= top <= S - 1:
        raise ValueError(f"the chain starts at an index in [0, {S - 1}], got {top}")
    if r < 1 or j < 1:
        raise ValueError(f"resamples and jump_length are at least 1, got resamples={r}, jump_length={j}")
    if r > 1 and j > top:
        raise ValueError(f"a jump of {j} levels does not fit below the starting index {top}")
    ops, taken, i = [], {}, top
    while i >= 0:
        ops.append("down")
        i -= 1
        if r > 1 and 0 <= i <= top - j and (top - i) % j == 0 and taken.get(i, 0) < r - 1:
            taken[i] = taken.get(i, 0) + 1
            ops.append("up")
            i += j
    return ops


_MEAN_CODE = {"eps": 0, "x_0": 1, "mean": 2}
_STEP_TABLES = ("sqrt_recip_alphas_bar", "sqrt_recip_m1_alphas_bar", "posterior_mean_coef1", "posterior_mean_coef2", "fixed_model_logvar")
_VLB_TABLES = ("sqrt_recip_alphas_bar", "sqrt_recip_m1_alphas_bar", "posterior_mean_coef1", "posterior_mean_coef2", "posterior_logvar_clipped",
               "fixed_model_logvar")
# learned variance (the network emits [B, 2C, H, W]: mean output | v): the kernels' var_mode, and the tables of the *_lv entry points —
# the four mean coefficients, then lv_min = posterior_logvar_clipped and lv_max = the "fixed-large" table
_VAR_MODE = {"learned": 1, "learned-range": 2}
_LV_TABLES = ("sqrt_recip_alphas_bar", "sqrt_recip_m1_alphas_bar", "posterior_mean_coef1", "posterior_mean_coef2", "posterior_logvar_clipped",
              "model_logvar_max")


class _AutogradMSE(torch.autograd.Function):
    """Per-sample eps-MSE with a fused backward (d/d pred only; the target is data)."""

    @staticmethod
    def forward(ctx, pred, target):
        B, n = pred.shape[0], pred[0].numel()
        loss = torch.empty(B, dtype=torch.float32, device=pred.device)
        _hip.call("ddpm_mse_fwd", pred.data_ptr(), target.data_ptr(), loss.data_ptr(), B, n, _hip.stream())
        ctx.save_for_backward(pred, target)
        return loss

    @staticmethod
    def backward(ctx, gloss):
        pred, target = ctx.saved_tensors
        B, n = pred.shape[0], pred[0].numel()
        g = torch.empty_like(pred)
        _hip.call("ddpm_mse_bwd", pred.data_ptr(), target.data_ptr(), gloss.contiguous().float().data_ptr(), g.data_ptr(), B, n, _hip.stream())
        return g, None


class _AutogradVLB(torch.autograd.Function):
    """Per-sample variational-bound term (bits / dim) of the network output with a fused backward (d / d model_out only: x_0, x_t are data)."""

    @staticmethod
    def forward(ctx, model_out, x_0, x_t, t, tabs, mean_code, T):
        B, n = model_out.shape[0], model_out[0].numel()
        loss = torch.empty(B, dtype=torch.float32, device=model_out.device)
        _hip.call("ddpm_vlb_terms", x_0.data_ptr(), x_t.data_ptr(), model_out.data_ptr(), t.data_ptr(), *[tb.data_ptr() for tb in tabs],
                  loss.data_ptr(), 0, B, n, mean_code, 0, T, _hip.stream())
        ctx.save_for_backward(model_out, x_0, x_t, t)
        ctx.tabs, ctx.mean_code, ctx.T = tabs, mean_code, T
        return loss

    @staticmethod
    def backward(ctx, gloss):
        model_out, x_0, x_t, t = ctx.saved_tensors
        B, n = model_out.shape[0], model_out[0].numel()
        g = torch.empty_like(model_out)
        _hip.call("ddpm_vlb_terms_bwd", x_0.data_ptr(), x_t.data_ptr(), model_out.data_ptr(), t.data_ptr(), *[tb.data_ptr() for tb in ctx.tabs],
                  gloss.contiguous().float().data_ptr(), g.data_ptr(), B, n, ctx.mean_code, ctx.T, _hip.stream())
        return g, None, None, None, None, None, None


class _AutogradLearnedLoss(torch.autograd.Function):
    """Per-sample loss of a learned-variance model, w_mse * MSE(mean half, target) + w_vlb * L_t (bits / dim), by `ddpm_learned_loss`: the
    forward asks for the loss alone, the backward runs the kernel again for d / d model_out (both halves; x_0, x_t, target are data)."""

    @staticmethod
    def forward(ctx, model_out, x_0, x_t, target, t, launch):
        ctx.save_for_backward(model_out, x_0, x_t, target, t)
        ctx.launch = launch
        return launch(x_0, x_t, model_out, target, t, None, None)

    @staticmethod
    def backward(ctx, gloss):
        model_out, x_0, x_t, target, t = ctx.saved_tensors
        g = torch.empty_like(model_out)
        ctx.launch(x_0, x_t, model_out, target, t, gloss.contiguous().float(), g)
        return g, None, None, None, None, None


class Conditioned(torch.nn.Module):
    """``denoise_fn`` with its class labels bound: ``forward(x, t) = denoise_fn(x, t, y)``.  What the loops without a label input of their own
    (``calc_all_bpd``, ``DDIM.encode`` / ``decode``) evaluate a class-conditional network through, at guidance scale 1.  A module, so the
    engines of the UNets inside it are found; a new object per call, so its captured step is captured for that call."""

    def __init__(self, denoise_fn, y):
        super().__init__()
        self.fn, self.y = denoise_fn, y
        self.training = bool(getattr(denoise_fn, "training", False))

    def forward(self, x, t):
        return self.fn(x, t, self.y)


class GaussianDiffusion:
    # whether the sampling loops (eager and captured) clamp the x_0 estimate to [-1, 1] (diffusion.py:152-158 pass clip_denoised=True);
    # the 2-D toy subclass never clips (toy/diffusion.py:32)
    clip_sampling = True

    def __init__(self, betas, model_mean_type, model_var_type, loss_type, **kwargs):
        assert isinstance(betas, torch.Tensor) and betas.dtype == _F64          # diffusion.py:42-43
        assert (betas > 0).all() and (betas <= 1).all()
        self.betas = betas
        self.model_mean_type = model_mean_type
        self.model_var_type = model_var_type
        self.loss_type = loss_type
        self.timesteps = len(betas)
        # the network's output is [B, 2C, H, W], mean output | v (a DDIM built for such a model keeps this set and samples on fixed tables)
        self.learned_var = model_var_type in _VAR_MODE
        if self.learned_var and loss_type == "mse":
            raise ValueError(f"loss_type 'mse' gives the variance half of a {model_var_type!r} model no gradient (diffusion.py:229); use 'hybrid' or 'kl'")
        if loss_type == "hybrid" and not self.learned_var:
            raise ValueError(f"loss_type 'hybrid' trains a learned variance: model_var_type must be 'learned' or 'learned-range', got {model_var_type!r}")
        # weight of the bound term in the hybrid loss (Nichol & Dhariwal 2021 eq. 16: lambda = 0.001 on the sum of T terms, carried by the one sampled)
        self.vlb_weight = float(kwargs.get("vlb_weight", self.timesteps / 1000.0))
        self._build_tables(betas, torch.cumprod(1.0 - betas, dim=0), eta2=None)

    def _build_tables(self, betas, alphas_bar, eta2):
        """fp64 host tables under the reference's attribute names.

        eta2 is None : DDPM posterior (diffusion.py:49-73).
        eta2 given   : DDIM generalisation on a sub-sequence (ddim.py:61-92): variance scaled by eta^2,
                       logs floored at 1e-20, mean coefficients from Song et al. eq. 12.
        """
        one = torch.ones(1, dtype=_F64)
        ab, ab_prev = alphas_bar, torch.cat([one, alphas_bar[:-1]])
        ddim = eta2 is not None
        self.alphas_bar = ab
        self.sqrt_alphas_bar = ab.sqrt()
        self.sqrt_one_minus_alphas_bar = (1.0 - ab).sqrt()
        # the level a reverse step arrives at (ab[-1] = 1: the clean image): the masked step re-noises the known region to it
        self.alphas_bar_prev = ab_prev
        self.sqrt_alphas_bar_prev = ab_prev.sqrt()
        self.sqrt_one_minus_alphas_bar_prev = (1.0 - ab_prev).sqrt()
        self.sqrt_recip_alphas_bar = (1.0 / ab).sqrt()
        self.sqrt_recip_m1_alphas_bar = (1.0 / ab - 1.0).sqrt()
        self.posterior_var = betas * (1.0 - ab_prev) / (1.0 - ab) * (eta2 if ddim else 1.0)

        def log_patched(head, tail):               # entry 0 takes the value of entry 1 (diffusion.py:65,71)
            v = torch.cat([head, tail])
            return torch.log(v.clip(min=1e-20) if ddim else v)

        self.posterior_logvar_clipped = log_patched(self.posterior_var[1:2], self.posterior_var[1:])
        if ddim:
            alphas = ab / ab_prev
            self.posterior_mean_coef2 = torch.sqrt(1 - ab - eta2 * betas) * torch.sqrt(1 - ab_prev) / (1.0 - ab)
            self.posterior_mean_coef1 = ab_prev.sqrt() * (1.0 - alphas.sqrt() * self.posterior_mean_coef2)
        else:
            self.posterior_mean_coef1 = betas * ab_prev.sqrt() / (1.0 - ab)
            self.posterior_mean_coef2 = (1.0 - betas).sqrt() * (1.0 - ab_prev) / (1.0 - ab)
        self.model_logvar_max = log_patched(self.posterior_var[1:2], betas[1:])          # lv_max of "learned-range"; lv_min = posterior_logvar_clipped
        if self.model_var_type == "fixed-large":
            self.fixed_model_var = betas
            self.fixed_model_logvar = self.model_logvar_max
        elif self.model_var_type == "fixed-small":
            self.fixed_model_var = self.posterior_var
            self.fixed_model_logvar = self.posterior_logvar_clipped
        elif self.model_var_type not in _VAR_MODE:        # the learned types have no fixed_model_var / fixed_model_logvar
            raise KeyError(self.model_var_type)
        self._dev = {}                                  # (table name, device) -> fp32 device copy
        return ab_prev

    # ------------------------------------------------------------------ device tables
    def _tab(self, name, device):
        key = (name, device)
        if key not in self._dev:
            self._dev[key] = getattr(self, name).to(torch.float32).to(device).contiguous()   # cast THEN gather (diffusion.py:83)
        return self._dev[key]

    @staticmethod
    def _extract(arr, t, x, dtype=torch.float32, device=torch.device("cpu"), ndim=4):
        """diffusion.py:75-84 (kept for callers that use it directly; the fused kernels do not)."""
        if x is not None:
            dtype, device, ndim = x.dtype, x.device, x.ndim
        out = torch.as_tensor(arr, dtype=dtype, device=device).gather(0, t)
        return out.reshape((-1,) + (1,) * (ndim - 1))

    @staticmethod
    def _prep(*tensors):
        _hip.require_cuda(*tensors)
        return [None if v is None else v.contiguous().float() for v in tensors]

    # ------------------------------------------------------------------ forward process / loss
    def q_sample(self, x_0, t, noise=None):
        if noise is None:
            noise = torch.randn_like(x_0)
        x_0, noise = self._prep(x_0, noise)
        t = t.contiguous()
        out = _hip.retain(torch.empty_like(x_0))
        B = x_0.shape[0]
        _hip.call("ddpm_q_sample", x_0.data_ptr(), noise.data_ptr(), t.data_ptr(), self._tab("sqrt_alphas_bar", x_0.device).data_ptr(),
             self._tab("sqrt_one_minus_alphas_bar", x_0.device).data_ptr(), out.data_ptr(), B, x_0[0].numel(), len(self.sqrt_alphas_bar), _hip.stream())
        return out

    def q_mean_var(self, x_0, t):
        """diffusion.py:86-90: mean, variance and log-variance of q(x_t | x_0)."""
        e = self._extract
        return e(self.sqrt_alphas_bar, t, x_0) * x_0, e(1.0 - self.alphas_bar, t, x_0), e(torch.log(1.0 - self.alphas_bar), t, x_0)

    def q_posterior_mean_var(self, x_0, x_t, t):
        e = self._extract
        mean = e(self.posterior_mean_coef1, t, x_0) * x_0 + e(self.posterior_mean_coef2, t, x_0) * x_t
        return mean, e(self.posterior_var, t, x_0), e(self.posterior_logvar_clipped, t, x_0)

    def _loss_term_bpd(self, denoise_fn, x_0, x_t, t, clip_denoised, return_pred):
        """diffusion.py:203-215: L_t in bits per dimension — KL(q(x_{t-1}|x_t,x_0) || p(x_{t-1}|x_t)) for t > 0, the discretized-Gaussian decoder
        NLL at t = 0 — per sample, one fused kernel behind the network (csrc/elementwise.hip `vlb_terms_kernel`, compiled for a fixed and
        for a learned variance).  With grad enabled and clip_denoised = False (how `train_losses` calls it) the result carries the fused
        backward to the network output."""
        model_out = denoise_fn(x_t, t)
        x_0, x_t, model_out = self._prep(x_0, x_t, model_out)
        t = t.contiguous()
        entry, tabs, mode = self._bound_entry("ddpm_vlb_terms", x_0.device)
        if self.learned_var:
            self._check_two_halves(model_out, x_0)
        T, code = len(self.posterior_mean_coef1), _MEAN_CODE[self.model_mean_type]
        if torch.is_grad_enabled() and model_out.requires_grad:
            if clip_denoised or return_pred:
                raise NotImplementedError("the differentiable bound term is the training form: clip_denoised=False, return_pred=False")
            if self.learned_var:
                launch = lambda x0, xt, out, tg, tt, gl, g: self.learned_loss(x0, xt, out, None, tt, gl, g, 0.0, 1.0, False)      # noqa: E731
                return _AutogradLearnedLoss.apply(model_out, x_0, x_t, None, t, launch)
            return _AutogradVLB.apply(model_out, x_0, x_t, t, tabs, code, T)
        B, n = x_0.shape[0], x_0[0].numel()
        loss = torch.empty(B, dtype=torch.float32, device=x_0.device)
        pred = torch.empty_like(x_0) if return_pred else None
        _hip.call(entry, x_0.data_ptr(), x_t.data_ptr(), model_out.data_ptr(), t.data_ptr(), *[tb.data_ptr() for tb in tabs],
                  loss.data_ptr(), _hip.ptr(pred), B, n, code, int(bool(clip_denoised)), *mode, T, _hip.stream())
        return (loss, pred) if return_pred else loss

    # ---- learned variance: the *_lv entry points on the network's [B, 2C, H, W] output
    def _var_mode(self):
        """The kernels' var_mode: 1 / 2 for the learned types, 0 = fixed tables (a DDIM on a 2C-channel model: the v half is ignored)."""
        return _VAR_MODE.get(self.model_var_type, 0)

    def _lv_tabs(self, dev):
        return [self._tab(n_, dev).data_ptr() for n_ in _LV_TABLES]

    def _bound_entry(self, name, dev):
        """How this model calls the bound kernel ``name`` (`ddpm_vlb_terms`, `ddpm_bpd_terms`): (entry point, its six tables, the extra
        var_mode argument) — the plain entry on _VLB_TABLES, or the *_lv one on _LV_TABLES with var_mode in front of T."""
        if self.learned_var:
            return name + "_lv", [self._tab(n_, dev) for n_ in _LV_TABLES], [self._var_mode()]
        return name, [self._tab(n_, dev) for n_ in _VLB_TABLES], []

    def _check_two_halves(self, model_out, x):
        if model_out.shape[0] != x.shape[0] or model_out[0].numel() != 2 * x[0].numel():
            raise ValueError(f"a {self.model_var_type!r} model emits twice the channels of its input (mean output | v): got "
                             f"{tuple(model_out.shape)} for an input of {tuple(x.shape)}")

    def learned_loss(self, x_0, x_t, model_out, target, t, gloss, gout, w_mse, w_vlb, detach_mean, loss=None):
        """One `ddpm_learned_loss` launch on prepared fp32 tensors: loss [B] (and gout when given, see include/ddpm_hip.h)."""
        self._check_two_halves(model_out, x_0)
        B, n = x_0.shape[0], x_0[0].numel()
        if loss is None:
            loss = _hip.retain(torch.empty(B, dtype=torch.float32, device=x_0.device))
        _hip.call("ddpm_learned_loss", x_0.data_ptr(), x_t.data_ptr(), model_out.data_ptr(), _hip.ptr(target), t.data_ptr(), *self._lv_tabs(x_0.device),
                  _hip.ptr(gloss), loss.data_ptr(), _hip.ptr(gout), B, n, _MEAN_CODE[self.model_mean_type], self._var_mode(), int(bool(detach_mean)),
                  len(self.posterior_mean_coef1), float(w_mse), float(w_vlb), _hip.stream())
        return loss

    def train_losses(self, denoise_fn, x_0, t, noise=None, y=None):
        """diffusion.py:217-243 -> per-sample losses [B]: "mse" (unweighted), "kl" (the variational-bound term, :222-224) or, for a learned
        variance, "hybrid" (Nichol & Dhariwal 2021 eq. 16): mean (out_mean - target)^2 + vlb_weight * L_t(stopgrad(out_mean), v).
        ``y`` (class-conditional models; not in the reference): int64 [B] labels handed to the network as its third input."""
        if self.loss_type not in ("mse", "kl", "hybrid"):
            raise NotImplementedError(self.loss_type)
        if y is not None:
            net = denoise_fn
            denoise_fn = lambda x, tt: net(x, tt, y)                    # noqa: E731
        if noise is None:
            noise = torch.randn_like(x_0)
        x_t = self.q_sample(x_0, t, noise=noise)
        if self.loss_type == "kl":
            return self._loss_term_bpd(denoise_fn, x_0=x_0, x_t=x_t, t=t, clip_denoised=False, return_pred=False)
        target = self.loss_target(x_0, x_t, t, noise)
        model_out = denoise_fn(x_t, t)
        if self.loss_type == "hybrid":
            x_0, model_out, target = self._prep(x_0, model_out, target)
            launch = lambda x0, xt, out, tg, tt, gl, g: self.learned_loss(x0, xt, out, tg, tt, gl, g, 1.0, self.vlb_weight, True)     # noqa: E731
            return _AutogradLearnedLoss.apply(model_out, x_0, x_t, target, t.contiguous(), launch)
        pred, target = self._prep(model_out, target)
        return _AutogradMSE.apply(pred, target)

    def loss_target(self, x_0, x_t, t, noise):
        """What the model output is regressed on (diffusion.py:225-236)."""
        if self.model_mean_type == "eps":
            return noise
        if self.model_mean_type == "x_0":
            return x_0
        if self.model_mean_type == "mean":
            # posterior mean from the device-resident tables (no host -> device upload: this runs inside captured steps)
            c1 = self._tab("posterior_mean_coef1", x_0.device).gather(0, t).reshape((-1,) + (1,) * (x_0.ndim - 1))
            c2 = self._tab("posterior_mean_coef2", x_0.device).gather(0, t).reshape((-1,) + (1,) * (x_0.ndim - 1))
            return c1 * x_0 + c2 * x_t
        raise NotImplementedError(self.model_mean_type)

    def supports_direct_step(self):
        """True when Trainer may run its autograd-free step: the loss is the plain MSE on a target that does not depend on
        the model (the reference's 'kl' loss would need the variance terms), or the hybrid loss of a learned variance (one fused launch
        forms it and its gradient)."""
        if self.loss_type == "hybrid":
            return self.model_var_type in _VAR_MODE and self.model_mean_type in _MEAN_CODE
        return self.loss_type == "mse" and self.model_mean_type in _MEAN_CODE

    # ------------------------------------------------------------------ reverse process
    def _step(self, x_t, model_out, z, t, clip_denoised, want_pred):
        x_t, model_out, z = self._prep(x_t, model_out, z)
        out = torch.empty_like(x_t)
        pred = torch.empty_like(x_t) if want_pred else None
        self._step_call(x_t, model_out, z, t, out, pred, clip_denoised)
        return out, pred

    def _step_call(self, x_t, model_out, z, t, out, pred, clip_denoised):
        """The launch of one sampling update on prepared fp32 tensors (``out`` may be ``x_t``: each element is read once, then written):
        `ddpm_p_sample_step` on _STEP_TABLES, or, for a [B, 2C, H, W] network output, `ddpm_p_sample_step_lv` — on _LV_TABLES with the
        model's var_mode; at var_mode 0 (a DDIM on such a model) on the sampler's own fixed table and the mean half alone."""
        dev, mode = x_t.device, self._var_mode()
        # a learned type (var_mode 1 | 2) has no fixed table, var_mode 0 has the sampler's own
        tabs = self._lv_tabs(dev) if mode else [self._tab(n_, dev).data_ptr() for n_ in _STEP_TABLES]
        entry, extra = "ddpm_p_sample_step", []
        if self.learned_var:
            self._check_two_halves(model_out, x_t)
            entry, extra = "ddpm_p_sample_step_lv", [mode]
            if not mode:
                tabs = tabs + [0]                                       # nothing in the entry's logvar_hi slot
        _hip.call(entry, x_t.data_ptr(), model_out.data_ptr(), z.data_ptr(), t.data_ptr(), *tabs, out.data_ptr(), _hip.ptr(pred),
                  x_t.shape[0], x_t[0].numel(), _MEAN_CODE[self.model_mean_type], int(bool(clip_denoised)), *extra, len(self.posterior_mean_coef1),
                  _hip.stream())

    def _step_cfg_call(self, state, out2, z, t, scale, pred, B):
        """`ddpm_p_sample_step_cfg` in place on the doubled state ``[2B, ...]``: rows [0, B) are read, both halves are written (dup)."""
        dev = state.device
        tabs = [self._tab(n_, dev).data_ptr() for n_ in _STEP_TABLES]
        _hip.call("ddpm_p_sample_step_cfg", state.data_ptr(), out2.data_ptr(), z.data_ptr(), t.data_ptr(), *tabs, float(scale), state.data_ptr(),
                  _hip.ptr(pred), B, state[0].numel(), _MEAN_CODE[self.model_mean_type], int(bool(self.clip_sampling)), 1,
                  len(self.posterior_mean_coef1), _hip.stream())

    def _mean_half(self, out2, state):
        """What the guided step combines: the network output itself, or — a sampler on fixed tables (var_mode 0) over a 2C-channel model,
        i.e. a DDIM built for a learned-variance one — its mean half as a plain copy, as ``DDIM.encode`` / ``decode`` take it."""
        if not self.learned_var:
            return out2
        self._check_two_halves(out2, state)
        return out2[:, :state.shape[1]].contiguous()

    @staticmethod
    def _null_class(denoise_fn):
        """Index of the null class of the class-conditional network behind ``denoise_fn`` (its ``num_classes``)."""
        k = getattr(denoise_fn, "num_classes", None)
        if k is None and isinstance(denoise_fn, torch.nn.Module):
            k = next((m.num_classes for m in denoise_fn.modules() if getattr(m, "num_classes", None) is not None), None)
        if k is None:
            raise ValueError("classifier-free guidance needs a class-conditional network (an attribute num_classes names its null class)")
        return int(k)

    def _guidance_form(self, denoise_fn, y, guidance_scale):
        """How a sampling loop calls the network and which step kernel follows it: None (no labels: the unconditional call), ``("cond",)``
        (labels at scale 1: a B-row call with ``y`` and the plain step) or ``("cfg", scale, null)`` — classifier-free guidance (Ho & Salimans
        2022): ONE network call on the doubled batch [x | x] with labels [y | null], then `ddpm_p_sample_step_cfg` on
        scale * out_c + (1 - scale) * out_u.  Also the ``kind`` a captured step of the form is cached under."""
        if y is None:
            return None
        scale = float(guidance_scale)
        if scale == 1.0:
            return ("cond",)
        if self._var_mode():                                        # (a DDIM on a 2C-channel model has var_mode 0: its own fixed table, the mean half)
            raise NotImplementedError("classifier-free guidance (guidance_scale != 1) of a learned-variance model: the guided step kernel "
                                      "combines the mean output on a fixed variance table; sample such a model at guidance_scale = 1")
        return ("cfg", scale, self._null_class(denoise_fn))

    def _model_logvar(self, model_out, x_t, t):
        """Per-element log-variance of a learned-variance model from the v half (diffusion.py:113-114; eq. 15 for "learned-range")."""
        v = model_out.contiguous().float().reshape(x_t.shape[0], 2, -1)[:, 1].reshape(x_t.shape)
        if self.model_var_type == "learned":
            return v
        e = lambda name: self._tab(name, x_t.device).gather(0, t).reshape((-1,) + (1,) * (x_t.ndim - 1))        # noqa: E731
        f = (v + 1.0) * 0.5
        return f * e("model_logvar_max") + (1.0 - f) * e("posterior_logvar_clipped")

    def p_mean_var(self, denoise_fn, x_t, t, clip_denoised, return_pred):
        """diffusion.py:107-138 (mean / variance are read off a zero-noise fused step)."""
        out = denoise_fn(x_t, t)
        mean, pred = self._step(x_t, out, torch.zeros_like(x_t), t, clip_denoised, True)
        if self._var_mode():
            logvar = self._model_logvar(out, x_t, t)
            return (mean, torch.exp(logvar), logvar, pred) if return_pred else (mean, torch.exp(logvar), logvar)
        var = self._tab("fixed_model_var", x_t.device).gather(0, t).reshape((-1,) + (1,) * (x_t.ndim - 1))
        logvar = self._tab("fixed_model_logvar", x_t.device).gather(0, t).reshape((-1,) + (1,) * (x_t.ndim - 1))
        return (mean, var, logvar, pred) if return_pred else (mean, var, logvar)

    def p_sample_step(self, denoise_fn, x_t, t, clip_denoised=True, return_pred=False, generator=None):
        """diffusion.py:152-158: one model call, one noise draw (also at t = 0, then masked), one fused update."""
        out = denoise_fn(x_t, t)
        noise = torch.empty_like(x_t).normal_(generator=generator)
        sample, pred = self._step(x_t, out, noise, t, clip_denoised, return_pred)
        return (sample, pred) if return_pred else sample

    def _model_t(self, t):
        return t

    def _sample_loop(self, denoise_fn, shape, device, noise, seed, on_step=None, z_stream=None, y=None, guidance_scale=1.0, edit=None):
        form = self._guidance_form(denoise_fn, y, guidance_scale)
        with self._time_tables(denoise_fn):
            return self._sample_loop_impl(denoise_fn, shape, device, noise, seed, on_step, z_stream, y, form, edit)

    def _sample_loop_impl(self, denoise_fn, shape, device, noise, seed, on_step=None, z_stream=None, y=None, form=None, edit=None):
        """The T-step (or S-step) loop.  ``z_stream`` (parity tests only) is an iterator of per-step noise tensors
        that replaces the generator draws, so an identical (x_T, z_1..z_T) stream can be injected.  ``y`` / ``form``: class labels and
        the way they are used (``_guidance_form``); the RNG consumption of every form is that of the unconditional loop.
        ``edit`` = (x_0, start) (``GaussianDiffusion.edit``): the chain begins at index ``start`` from ``q_sample(x_0, start)``, whose
        draw takes the place of the x_T draw, and runs ``start + 1`` steps.

        The step body (model call, noise draw, fused update, t -= 1) has static shapes, so it is captured ONCE into a
        hipGraph and replayed: at 32x32 the eager loop is bound by ~250 kernel launches per step, not by the GPU.
        The captured step is cached per (denoiser, shape) — later calls only re-seed and replay.
        RNG consumption (x_T first, then one z per step incl. t = 0) and results are identical to the eager loop;
        set DDPM_TORCH_AMD_GRAPH=0 to force eager."""
        device = torch.device(device)
        _hip.require_cuda(torch.empty(0, device=device))        # no CPU fallback: sampling runs on the GPU only
        B = (shape or noise.shape)[0]
        steps = self._num_steps() if edit is None else edit[1] + 1
        if form is not None:
            y = torch.as_tensor(y).to(device=device, dtype=torch.int64).contiguous()
            if y.shape != (B,):
                raise ValueError(f"expected class labels y of shape [{B}], got {tuple(y.shape)}")
        if (on_step is None and steps >= 4 and device.type == "cuda"
                and os.environ.get("DDPM_TORCH_AMD_GRAPH", "1") != "0" and not torch.cuda.is_current_stream_capturing()):
            done = self._graph_loop(denoise_fn, tuple(shape or noise.shape), device, noise, seed, steps, z_stream, y, form, edit)
            if done is not None:
                return done
        rng = torch.Generator(device).manual_seed(seed) if seed is not None else None       # diffusion.py:164-166
        if edit is not None:
            x_t = self._edit_state(edit, rng)
        elif noise is None:
            x_t = torch.empty(shape, device=device).normal_(generator=rng)                  # x_T first, then one z per step
        else:
            x_t = noise.to(device)
        t = torch.full((B,), steps - 1, dtype=torch.int64, device=device)
        x_t = x_t.contiguous().float().clone()
        if form is not None and form[0] == "cfg":
            return self._guided_eager_loop(denoise_fn, x_t, y, form, steps, rng, on_step, z_stream)
        for ti in range(steps - 1, -1, -1):
            t.fill_(ti)
            out = denoise_fn(x_t, self._model_t(t)) if form is None else denoise_fn(x_t, self._model_t(t), y)
            z = torch.empty_like(x_t).normal_(generator=rng) if z_stream is None else next(z_stream).to(x_t)
            x_t, pred = self._step(x_t, out, z, t, self.clip_sampling, on_step is not None)
            if on_step is not None:
                on_step(ti, pred)
        return x_t

    def _guided_eager_loop(self, denoise_fn, x_T, y, form, steps, rng, on_step, z_stream):
        """The guided loop, eagerly: the launches of the captured guided step (``_capture_sample_step``), one by one."""
        _, scale, null = form
        B, dev = x_T.shape[0], x_T.device
        state = torch.cat([x_T, x_T], dim=0)                                                # the doubled state [x | x]; the step keeps both halves
        y2 = torch.cat([y, torch.full_like(y, null)], dim=0)                                # [y | null]
        t = torch.full((2 * B,), steps - 1, dtype=torch.int64, device=dev)
        x_t = state[:B]
        pred = torch.empty_like(x_T) if on_step is not None else None
        for ti in range(steps - 1, -1, -1):
            t.fill_(ti)
            out2 = self._mean_half(denoise_fn(state, self._model_t(t), y2).contiguous().float(), state)
            z = torch.empty_like(x_T).normal_(generator=rng) if z_stream is None else next(z_stream).to(x_T).contiguous()
            self._step_cfg_call(state, out2, z, t, scale, pred, B)
            if on_step is not None:
                on_step(ti, pred)
        return x_t.clone()

    # ---- captured sampling step
    @contextlib.contextmanager
    def _time_tables(self, denoise_fn):
        """While a sampling loop (or the capture of its step) runs, the UNets under ``denoise_fn`` take their per-block time biases from
        the [T][sum Cout] table of all timesteps instead of running the embedding MLP every step (models/unet.py: time_table)."""
        engines = self._engines_of(denoise_fn) if os.environ.get("DDPM_TIME_TABLE", "1") != "0" else None
        for e in engines or ():
            e.enable_time_table(self.timesteps)
            e.tt_on = True
        try:
            yield
        finally:
            for e in engines or ():
                e.tt_on = False

    @staticmethod
    def _engines_of(denoise_fn):
        """Engines of every UNet of this package reachable from ``denoise_fn`` (their derived weight copies must be
        brought up to date eagerly before a captured step is replayed)."""
        from .models.unet import UNet
        if not isinstance(denoise_fn, torch.nn.Module):
            return None
        return [m.engine() for m in denoise_fn.modules() if isinstance(m, UNet)]

    def _graph_entry(self, denoise_fn, shape, device, default_rng, external_z=False, bpd=None, kind=None):
        """Cached captured step for (denoiser, shape), capturing it on first use; None when capture is not possible.
        ``external_z`` (parity tests): the step does not draw its noise, the caller fills the captured ``z`` buffer before every replay.
        ``bpd``: None for the sampling step, ``(clip_denoised,)`` for the bits/dim evaluation step of ``calc_all_bpd``.
        ``kind``: None for those two; a tuple naming another step a subclass captures itself (``_capture_kind_step``; ddim.py: the encode and
        decode steps) — it extends the key, so such a step and a sampling step of the same denoiser and shape never serve each other."""
        cache = self.__dict__.setdefault("_sample_graphs", {})
        engines = self._engines_of(denoise_fn)
        # engine serials: model.to() / .float() / set_compute_dtype() re-create the engine (packed weights, workspaces) — a step
        # captured against the previous one points at freed memory and must never be replayed
        # ... and so is the time-bias table the step gathers from: a sampler with a longer schedule re-allocates it
        key = (id(denoise_fn), shape, str(device), (default_rng, external_z, bpd) + ((kind,) if kind is not None else ()), getattr(denoise_fn, "training", None),
               tuple((e.serial, e.T, e.tt.data_ptr() if e.tt_on and e.tt is not None else 0) for e in engines) if engines else None)
        ent = cache.get(key)
        if ent is not None and ent["ref"]() is not denoise_fn:
            ent = None                                            # the id was recycled by another object
        if ent is None and engines:
            live = {e.serial for e in engines}
            for k in [k for k, v in cache.items() if v["ref"]() is denoise_fn and k[5] and {q[0] for q in k[5]} != live]:
                cache.pop(k)                                      # entries of this denoiser's earlier engines: dead weight (and dead pointers)
        if ent is None:
            if kind is not None:
                ent = self._capture_kind_step(denoise_fn, shape, device, default_rng, external_z, kind)
            elif bpd is None:
                ent = self._capture_sample_step(denoise_fn, shape, device, default_rng, external_z)
            else:
                ent = self._capture_bpd_step(denoise_fn, shape, device, default_rng, external_z, *bpd)
            if ent is not None and engines is not None:           # arbitrary callables are captured per call: nothing tells us when their weights change
                import weakref
                ent["ref"] = weakref.ref(denoise_fn)
                if len(cache) >= 8:
                    cache.pop(next(iter(cache)))
                cache[key] = ent
        return ent

    def _edit_state(self, edit, rng):
        """q_sample(x_0, start) on one draw from ``rng``: where an edited chain begins (``edit`` = (x_0, start))."""
        x_0, start = edit
        t = torch.full((x_0.shape[0],), start, dtype=torch.int64, device=x_0.device)
        return self.q_sample(x_0, t, noise=torch.empty_like(x_0).normal_(generator=rng))

    def _graph_loop(self, denoise_fn, shape, device, noise, seed, steps, z_stream=None, y=None, form=None, edit=None):
        """Replay the captured sampling step ``steps`` times; returns None if capture is not possible (the caller then
        runs the eager loop; no RNG state has been consumed).  ``z_stream`` (parity tests only): per-step noise tensors that are copied
        into the captured step's noise buffer instead of being drawn inside it.  ``form`` (``_guidance_form``) extends the cache key: a
        conditional or guided step (the scale is a kernel argument frozen into it) never serves another form; ``y`` refills the label
        buffer the captured network call reads."""
        ent = self._graph_entry(denoise_fn, shape, device, default_rng=seed is None, external_z=z_stream is not None, kind=form)
        if ent is None:
            return None
        if form is not None:
            ent["y"][:shape[0]].copy_(y)
        x_t, t, rng, graph = ent["x_t"], ent["t"], ent["rng"], ent["graph"]
        for e in self._engines_of(denoise_fn) or ():
            e.ensure_fresh()
        if rng is not None:
            rng.manual_seed(seed)
        if edit is not None:
            x_t.copy_(self._edit_state(edit, rng))                # the draw of q_sample in the place of the x_T draw
        elif noise is None:
            x_t.normal_(generator=rng)                            # x_T first, then one z per step (diffusion.py:166-171)
        else:
            x_t.copy_(noise)
        if ent.get("x_dup") is not None:
            ent["x_dup"].copy_(x_t)                               # the unconditional half of the doubled state; every step then keeps it
        t.fill_(steps - 1)
        for _ in range(steps):
            if z_stream is not None:
                ent["z"].copy_(next(z_stream))
            graph.replay()
        return x_t.clone()

    def _capture_kind_step(self, denoise_fn, shape, device, default_rng, external_z, kind):
        """Capture a step the cache knows under an extended key: here the conditional and the guided sampling step (``_guidance_form``)."""
        if kind[0] in ("cond", "cfg"):
            return self._capture_sample_step(denoise_fn, shape, device, default_rng, external_z, form=kind)
        if kind[0] == "inpaint":
            return self._capture_inpaint_steps(denoise_fn, shape, device, default_rng, external_z, kind)
        raise NotImplementedError(kind)

    def prepare_sampler(self, denoise_fn, shape, device, seeded=True):
        """Capture (and cache) the hipGraph of one sampling step for ``(denoise_fn, shape)`` without running a chain, so that the
        first ``p_sample`` of a serving process does not pay for it.  Returns True when a captured step is ready.  Not in the
        reference (its loop is eager)."""
        device = torch.device(device)
        if device.type != "cuda" or os.environ.get("DDPM_TORCH_AMD_GRAPH", "1") == "0" or self._num_steps() < 4:
            return False
        with torch.inference_mode(), self._time_tables(denoise_fn):
            return self._graph_entry(denoise_fn, tuple(shape), device, default_rng=not seeded) is not None

    def _capture_sample_step(self, denoise_fn, shape, device, default_rng, external_z=False, form=None):
        """``form`` (``_guidance_form``): None, ("cond",) — the network also reads the label buffer ``y`` — or ("cfg", scale, null): state,
        labels and timesteps have 2 B rows ([x | x], [y | null]), the network runs once on all of them and the guided step kernel reads the
        first B rows of the state and writes both halves; ``x_t`` and ``z`` of the entry are the B rows the caller sees."""
        dev = device
        guided = form is not None and form[0] == "cfg"
        B = shape[0]
        rows = 2 * B if guided else B
        state = torch.zeros((rows,) + tuple(shape[1:]), dtype=torch.float32, device=dev)
        x_t = state[:B]
        z = torch.empty(shape, dtype=torch.float32, device=dev)
        t = torch.full((rows,), self._num_steps() - 1, dtype=torch.int64, device=dev)
        y = None if form is None else torch.full((rows,), form[2] if guided else 0, dtype=torch.int64, device=dev)
        rng = None if default_rng else torch.Generator(dev)

        def body(cut=None):
            out = (denoise_fn(state, self._model_t(t)) if y is None else denoise_fn(state, self._model_t(t), y)).contiguous().float()
            if not external_z:
                z.normal_(generator=rng)
            if guided:
                self._step_cfg_call(state, self._mean_half(out, state), z, t, form[1], None, B)
            else:
                self._step_call(x_t, out, z, t, x_t, None, self.clip_sampling)         # in place
            _hip.call("ddpm_add_i64", t.data_ptr(), rows, -1, _hip.stream())

        graph = self._capture_step(dev, rng, body, "sampling")
        if graph is None:
            return None
        return {"x_t": x_t, "t": t, "z": z, "rng": rng, "graph": graph, "ref": lambda: denoise_fn, "y": y, "x_dup": state[B:] if guided else None}

    @staticmethod
    def _capture_step(dev, rng, body, what):
        """Warm ``body`` up on a side stream, then capture it into a SegmentedGraph (None, with a warning, when that is not possible; the
        generator ``body`` draws from — ``rng``, or the device's default one — is left where it was either way)."""
        gen = rng if rng is not None else torch.cuda.default_generators[dev.index if dev.index is not None else torch.cuda.current_device()]
        snap_rng = gen.get_state()
        try:
            # warm-up on a side stream (lazy kernel / cache initialisation) on scratch state: nothing the caller sees is consumed
            side = torch.cuda.Stream(device=dev)
            side.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(side):
                body()
            torch.cuda.current_stream(dev).wait_stream(side)
            gen.set_state(snap_rng)
            graph = SegmentedGraph(dev)
            graph.register_generator(rng)
            graph.capture(body)
        except Exception as e:                                   # capture not possible for this denoise_fn: eager loop instead
            import warnings
            warnings.warn(f"hipGraph capture of the {what} step failed ({type(e).__name__}: {e}); running the eager loop")
            torch.cuda.synchronize(dev)
            gen.set_state(snap_rng)
            return None
        return graph

    def _num_steps(self):
        return self.timesteps

    @torch.inference_mode()
    def p_sample(self, denoise_fn, shape=None, device=torch.device("cpu"), noise=None, seed=None, y=None, guidance_scale=1.0):
        """diffusion.py:160-174.  Not in the reference: ``y`` (int64 [B] class labels of a class-conditional network) and
        ``guidance_scale`` (classifier-free guidance, Ho & Salimans 2022: the step runs on scale * out(x, y) + (1 - scale) * out(x, null);
        1 = plain conditional sampling, any other value evaluates both branches as one 2B-row network call).  Learned-variance models
        are sampled at scale 1 only (NotImplementedError otherwise; a DDIM built for one runs on fixed tables and guides the mean half).
        RNG consumption is that of the unconditional loop."""
        return self._sample_loop(denoise_fn, shape, device, noise, seed, y=y, guidance_scale=guidance_scale)

    @torch.inference_mode()
    def p_sample_progressive(self, denoise_fn, shape, device=torch.device("cpu"), noise=None, pred_freq=10, seed=None, z_stream=None, y=None,
                             guidance_scale=1.0):
        """diffusion.py:176-198: the same loop, also returning pred_x0 of every ``pred_freq``-th step (on the host), filled from
        the back: ``preds[L-1]`` is the first one kept (t = T-1 when T is a multiple of pred_freq), ``preds[0]`` the one at
        t = pred_freq - 1.  The per-step read-back needs the eager loop (no graph replay).  ``z_stream`` (parity tests only): as in
        ``_sample_loop``."""
        shape = tuple(shape or noise.shape)
        B = shape[0]
        L = self._num_steps() // pred_freq
        preds = torch.zeros((L, B) + shape[1:], dtype=torch.float32)
        box = [L]

        def keep(ti, pred):
            if (ti + 1) % pred_freq == 0:
                box[0] -= 1
                preds[box[0]] = pred.cpu()

        x = self._sample_loop(denoise_fn, shape, device, noise, seed, on_step=keep, z_stream=z_stream, y=y, guidance_scale=guidance_scale)
        return x.cpu(), preds

    # ------------------------------------------------------------------ inpainting and image editing (not in the reference)
    # RePaint (Lugmayr et al., CVPR 2022, Algorithm 1) as a sampling-loop feature.  Index convention of every loop here: the device ``t``
    # buffer is the index of the current state (S - 1 at the start, -1 when clean); a reverse step at t = i takes the state from i to i - 1
    # and re-noises the known region to i - 1; a jump adds j to t, then applies `ddpm_q_jump` at the new index.
    def _jump_tables(self, j, device):
        """(ja, jb) of `ddpm_q_jump` for jumps of ``j`` levels, indexed by the arrival index i: ja[i] = sqrt(ab[i] / ab[i-j]),
        jb[i] = sqrt(1 - ab[i] / ab[i-j]) with ab[-1] = 1, NaN where i - j < -1.  Formed in fp64 (the ratio of two fp32 table entries
        would lose about three digits of 1 - a at small betas); the fp32 device copies are cached per (j, device) by ``_tab``."""
        names = (f"repaint_jump_a_{j}", f"repaint_jump_b_{j}")
        if not hasattr(self, names[0]):
            ab = torch.cat([torch.ones(1, dtype=_F64), self.alphas_bar.to(_F64)])           # ab[i] sits at i + 1
            i = torch.arange(len(self.alphas_bar))
            src = i - j + 1
            ratio = torch.where(src >= 0, ab[i + 1] / ab[src.clamp_min(0)], torch.full((len(i),), float("nan"), dtype=_F64))
            setattr(self, names[0], ratio.sqrt())
            setattr(self, names[1], (1.0 - ratio).sqrt())
        return [self._tab(n_, device) for n_ in names]

    @staticmethod
    def _inpaint_mask(mask, shape, device):
        """The mask as the kernel reads it: fp32 [1 or B][H * W], 1 = keep the known pixel, 0 = generate, from ``[H, W]``, ``[1, 1, H, W]``
        or ``[B, 1, H, W]`` of dtype bool, uint8 or float.  ValueError for another shape, NaN or a value outside [0, 1]."""
        B, _, H, W = shape
        m = torch.as_tensor(mask)
        if tuple(m.shape) == (H, W):
            m = m.reshape(1, H * W)
        elif tuple(m.shape) in ((1, 1, H, W), (B, 1, H, W)):
            m = m.reshape(m.shape[0], H * W)
        else:
            raise ValueError(f"expected a mask of shape [{H}, {W}], [1, 1, {H}, {W}] or [{B}, 1, {H}, {W}], got {tuple(m.shape)}")
        if not (m.dtype in (torch.bool, torch.uint8) or m.dtype.is_floating_point):
            raise ValueError(f"expected a bool, uint8 or floating-point mask, got {m.dtype}")
        m = m.to(torch.float32)
        if not bool(((m >= 0) & (m <= 1)).all()):                                           # (NaN compares false)
            raise ValueError("mask values lie in [0, 1]: 1 = keep the known pixel, 0 = generate")
        return m.to(device).contiguous()

    def _inpaint_state(self, denoise_fn, shape, dev, rng, external_z, kind):
        """Buffers and the two step bodies of an inpainting chain.  "down": network, two draws (z of the reverse step, then e of the
        re-noising), the masked step in place, t -= 1.  "up" (kind's j > 0): t += j, one draw, `ddpm_q_jump` in place."""
        _, j, mask_rows, form = kind
        B, n, hw = shape[0], shape[1] * shape[2] * shape[3], shape[2] * shape[3]
        S = self._num_steps()
        x_t = torch.zeros(shape, dtype=torch.float32, device=dev)
        z, e, x_known = torch.zeros_like(x_t), torch.zeros_like(x_t), torch.zeros_like(x_t)
        mask = torch.zeros((mask_rows, hw), dtype=torch.float32, device=dev)
        t = torch.full((B,), S - 1, dtype=torch.int64, device=dev)
        y = None if form is None else torch.zeros((B,), dtype=torch.int64, device=dev)
        mode = self._var_mode()
        tabs = self._lv_tabs(dev) if mode else [self._tab(n_, dev).data_ptr() for n_ in _STEP_TABLES] + [0]
        tabs = tabs + [self._tab(n_, dev).data_ptr() for n_ in ("sqrt_alphas_bar_prev", "sqrt_one_minus_alphas_bar_prev")]
        code, clip, T = _MEAN_CODE[self.model_mean_type], int(bool(self.clip_sampling)), len(self.posterior_mean_coef1)
        jump = [tb.data_ptr() for tb in self._jump_tables(j, dev)] if j else None

        def down(cut=None):
            out = (denoise_fn(x_t, self._model_t(t)) if y is None else denoise_fn(x_t, self._model_t(t), y)).contiguous().float()
            if self.learned_var:
                self._check_two_halves(out, x_t)
            elif out.shape != x_t.shape:
                raise ValueError(f"the network returned {tuple(out.shape)} for an input of {tuple(x_t.shape)}")
            if not external_z:
                z.normal_(generator=rng)
                e.normal_(generator=rng)
            _hip.call("ddpm_p_sample_step_masked", x_t.data_ptr(), out.data_ptr(), z.data_ptr(), x_known.data_ptr(), e.data_ptr(), mask.data_ptr(),
                      t.data_ptr(), *tabs, x_t.data_ptr(), B, n, hw, mask_rows, out[0].numel(), code, clip, mode, T, _hip.stream())    # in place
            _hip.call("ddpm_add_i64", t.data_ptr(), B, -1, _hip.stream())

        def up(cut=None):
            _hip.call("ddpm_add_i64", t.data_ptr(), B, j, _hip.stream())
            if not external_z:
                z.normal_(generator=rng)
            _hip.call("ddpm_q_jump", x_t.data_ptr(), z.data_ptr(), t.data_ptr(), *jump, x_t.data_ptr(), B, n, T, _hip.stream())       # in place

        return {"x_t": x_t, "z": z, "e": e, "x_known": x_known, "mask": mask, "t": t, "y": y, "rng": rng, "down": down, "up": up if j else None,
                "ref": lambda: denoise_fn}

    def _capture_inpaint_steps(self, denoise_fn, shape, device, default_rng, external_z, kind):
        """One cache entry, two graphs over the same buffers, replayed by the host in schedule order."""
        rng = None if default_rng else torch.Generator(device)
        ent = self._inpaint_state(denoise_fn, shape, device, rng, external_z, kind)
        for name in ("down", "up"):
            if ent[name] is not None:
                graph = self._capture_step(device, rng, ent[name], "inpainting " + name)
                if graph is None:
                    return None
                ent[name] = graph.replay
        return ent

    def inpaint(self, denoise_fn, x_known, mask, jump_length=1, resamples=1, start=None, seed=None, noise=None, y=None, z_stream=None):
        """Fill the region of ``x_known`` ([B, C, H, W] in [-1, 1]) where ``mask`` is 0 and keep it where ``mask`` is 1 (RePaint, Lugmayr
        et al. 2022): ``[B, C, H, W]`` float32 on ``x_known``'s device, whose known region is the source image itself.  ``mask``: ``[H, W]``,
        ``[1, 1, H, W]`` or ``[B, 1, H, W]``, bool, uint8 or float in [0, 1] (a soft value blends the two regions), broadcast over channels.
        At every level the known region is re-noised from ``x_known`` and the unknown one comes from the reverse step — one fused kernel
        behind the network (csrc/inpaint.hip).  ``jump_length`` / ``resamples``: the chain jumps back up ``jump_length`` levels and comes
        down again ``resamples`` times so that the two regions harmonise (``repaint_schedule``; 1 = the plain replacement method).
        ``start`` = None: the state begins as x_T (a draw, or ``noise``) at index S - 1; ``start`` = i: as ``q_sample(x_known, i)`` on one
        draw (or ``noise``) in place of the x_T draw.  RNG order: the initial draw, then per reverse step z, then e, and one draw per
        jump, from a generator seeded with ``seed`` on the device (else the default one); ``z_stream`` (parity tests) supplies exactly
        those tensors in that order.  ``y``: class labels of a class-conditional network at guidance scale 1.  Learned-variance models are
        served.  The two step bodies are captured once and replayed in schedule order like the sampling step (same cache, same fallback to
        the eager loop, which issues the same launches one by one and gives the same bits)."""
        form = self._guidance_form(denoise_fn, y, 1.0)              # None or ("cond",), by the rule p_sample and edit go through
        with torch.inference_mode(), self._time_tables(denoise_fn):
            return self._inpaint_impl(denoise_fn, x_known, mask, int(jump_length), int(resamples), start, seed, noise, y, z_stream, form)

    def _inpaint_impl(self, denoise_fn, x_known, mask, j, r, start, seed, noise, y, z_stream, form):
        x_known, = self._prep(x_known)
        if x_known.ndim != 4:
            raise ValueError(f"expected x_known of shape [B, C, H, W], got {tuple(x_known.shape)}")
        if noise is not None and z_stream is not None:
            raise ValueError("z_stream supplies the initial draw as its first tensor: give noise or z_stream, not both")
        dev, shape, S = x_known.device, tuple(x_known.shape), self._num_steps()
        B = shape[0]
        ops = repaint_schedule(S, j, r, start)
        top = S - 1 if start is None else int(start)
        m = self._inpaint_mask(mask, shape, dev)
        if form is not None:
            y = torch.as_tensor(y).to(device=dev, dtype=torch.int64).contiguous()
            if y.shape != (B,):
                raise ValueError(f"expected class labels y of shape [{B}], got {tuple(y.shape)}")
        kind = ("inpaint", j if "up" in ops else 0, m.shape[0], form)
        external = z_stream is not None
        ent = None
        if (ops.count("down") >= 4 and dev.type == "cuda" and os.environ.get("DDPM_TORCH_AMD_GRAPH", "1") != "0"
                and not torch.cuda.is_current_stream_capturing()):
            ent = self._graph_entry(denoise_fn, shape, dev, default_rng=seed is None, external_z=external, kind=kind)
        if ent is not None:
            for eng in self._engines_of(denoise_fn) or ():
                eng.ensure_fresh()
        else:
            ent = self._inpaint_state(denoise_fn, shape, dev, torch.Generator(dev) if seed is not None else None, external, kind)
        rng = ent["rng"]
        if rng is not None:
            rng.manual_seed(seed)
        x_t, z = ent["x_t"], ent["z"]
        ent["x_known"].copy_(x_known)
        ent["mask"].copy_(m)
        if form is not None:
            ent["y"].copy_(y)
        if external:
            first = next(z_stream).to(x_t)
        elif noise is not None:
            first = noise.to(x_t)
        else:
            first = z.normal_(generator=rng)                      # the initial draw first, then z and e per reverse step, one draw per jump
        ent["t"].fill_(top)
        if start is None:
            x_t.copy_(first)
        else:
            x_t.copy_(self.q_sample(x_known, ent["t"], noise=first.contiguous()))
        for op in ops:
            if external:
                z.copy_(next(z_stream))
                if op == "down":
                    ent["e"].copy_(next(z_stream))
            ent[op]()
        return x_t.clone()

    def edit(self, denoise_fn, x_0, start, seed=None, y=None):
        """SDEdit-style editing: ``q_sample(x_0, start)`` on one draw, then the sampling step from index ``start`` down — the existing
        (captured) sampling step with ``t`` filled to ``start`` and run ``start + 1`` times.  RNG order: the q_sample draw, then one z
        per step.  Equals ``inpaint`` with an all-zero mask and the same ``start`` bit for bit when both are given the same draws.
        ``y``: class labels at guidance scale 1.  Returns ``[B, C, H, W]`` float32 on ``x_0``'s device."""
        x_0, = self._prep(x_0)
        start = int(start)
        if not 0 <= start <= self._num_steps() - 1:
            raise ValueError(f"the chain starts at an index in [0, {self._num_steps() - 1}], got {start}")
        with torch.inference_mode():
            return self._sample_loop(denoise_fn, tuple(x_0.shape), x_0.device, None, seed, y=y, edit=(x_0, start))

    # ------------------------------------------------------------------ negative log-likelihood in bits per dimension
    # t = 0 likelihood of the evaluation: 0 = discretized Gaussian (functions.py:49-65); the 2-D toy subclass uses 1, the continuous one
    bpd_decoder = 0

    def _bpd_finish(self, x_0, losses):
        """(prior [B], total [B]) from x_0 and the [B, T] table of bound terms: one launch (csrc/elementwise.hip `bpd_finish_kernel`)."""
        B, n = x_0.shape[0], x_0[0].numel()
        T, last = losses.shape[1], self.timesteps - 1
        prior = torch.empty(B, dtype=torch.float32, device=x_0.device)
        total = torch.empty_like(prior)
        _hip.call("ddpm_bpd_finish", x_0.data_ptr(), losses.data_ptr(), prior.data_ptr(), total.data_ptr(), B, n, T, losses.stride(0),
                  float(self.sqrt_alphas_bar[last].to(torch.float32)), float(torch.log(1.0 - self.alphas_bar[last]).to(torch.float32)), _hip.stream())
        return prior, total

    @torch.inference_mode()
    def _prior_bpd(self, x_0):
        """diffusion.py:245-250 with the tensors it meant: KL(q(x_T | x_0) || N(0, I)) in bits per dimension, per sample [B]."""
        x_0, = self._prep(x_0)
        # the prior is one output of ddpm_bpd_finish: give it a [B, 1] table of zeros to sum, and take the prior alone
        return self._bpd_finish(x_0, torch.zeros((x_0.shape[0], 1), dtype=torch.float32, device=x_0.device))[0]

    def _bpd_state(self, denoise_fn, shape, dev, rng, external_z, clip_denoised):
        """Buffers of the evaluation loop and its step body: draw eps, q_sample, network, bound term + MSE into column t, t -= 1."""
        x_0 = torch.zeros(shape, dtype=torch.float32, device=dev)
        z, x_t = torch.zeros_like(x_0), torch.empty_like(x_0)       # zeros: with external noise the capture's warm-up runs before the first copy
        B, n, T = shape[0], x_0[0].numel(), self.timesteps
        t = torch.full((B,), T - 1, dtype=torch.int64, device=dev)
        losses = torch.full((B, T), float("nan"), dtype=torch.float32, device=dev)
        mses = torch.full_like(losses, float("nan"))
        qtabs = [self._tab(n_, dev) for n_ in ("sqrt_alphas_bar", "sqrt_one_minus_alphas_bar")]
        entry, tabs, mode = self._bound_entry("ddpm_bpd_terms", dev)
        code, clip, decoder = _MEAN_CODE[self.model_mean_type], int(bool(clip_denoised)), self.bpd_decoder

        def body(cut=None):
            if not external_z:
                z.normal_(generator=rng)
            _hip.call("ddpm_q_sample", x_0.data_ptr(), z.data_ptr(), t.data_ptr(), *[tb.data_ptr() for tb in qtabs], x_t.data_ptr(), B, n, T, _hip.stream())
            out = denoise_fn(x_t, self._model_t(t)).contiguous().float()
            if self.learned_var:
                self._check_two_halves(out, x_0)
            _hip.call(entry, x_0.data_ptr(), x_t.data_ptr(), out.data_ptr(), t.data_ptr(), *[tb.data_ptr() for tb in tabs],
                      losses.data_ptr(), mses.data_ptr(), B, n, T, code, clip, decoder, *mode, T, _hip.stream())
            _hip.call("ddpm_add_i64", t.data_ptr(), B, -1, _hip.stream())

        return {"x_0": x_0, "z": z, "t": t, "losses": losses, "mses": mses, "rng": rng, "body": body, "ref": lambda: denoise_fn}

    def _capture_bpd_step(self, denoise_fn, shape, device, default_rng, external_z, clip_denoised):
        rng = None if default_rng else torch.Generator(device)
        ent = self._bpd_state(denoise_fn, shape, device, rng, external_z, clip_denoised)
        ent["graph"] = self._capture_step(device, rng, ent["body"], "bits/dim evaluation")
        return ent if ent["graph"] is not None else None

    def calc_all_bpd(self, denoise_fn, x_0, clip_denoised=True, seed=None, noise_stream=None, y=None):
        """``y``: int64 [B] class labels of a class-conditional network, evaluated conditionally (no guidance).
        diffusion.py:252-268 as it was meant: ``(total_bpd [B], losses [B, T], prior_bpd [B], mses [B, T])`` with
        ``total = L_T + sum_t L_t``, float32 ON ``x_0``'s DEVICE (the reference preallocates on the host and would synchronise T times).

        For t = T-1 ... 0: one standard-normal draw of x_0's shape (from a generator seeded with ``seed`` on x_0's device, else the default
        one; ``noise_stream`` — parity tests — is an iterator of per-step noise tensors that replaces the draws), q_sample, the network, and
        one fused kernel that puts L_t and mean (pred_x_0 - x_0)^2 into column t.  The step is captured once and replayed T times like the
        sampling step (same cache, same fallback to the eager loop; DDPM_TORCH_AMD_GRAPH=0 forces eager); both forms give the same bits."""
        if y is not None:
            denoise_fn = Conditioned(denoise_fn, y.to(x_0.device))
        with torch.inference_mode(), self._time_tables(denoise_fn):
            return self._calc_all_bpd_impl(denoise_fn, x_0, clip_denoised, seed, noise_stream)

    def _calc_all_bpd_impl(self, denoise_fn, x_0, clip_denoised, seed, noise_stream):
        x_0, = self._prep(x_0)
        dev, shape, T = x_0.device, tuple(x_0.shape), self.timesteps
        clip_denoised, external = bool(clip_denoised), noise_stream is not None
        ent = None
        if (T >= 4 and dev.type == "cuda" and os.environ.get("DDPM_TORCH_AMD_GRAPH", "1") != "0"
                and not torch.cuda.is_current_stream_capturing()):
            ent = self._graph_entry(denoise_fn, shape, dev, default_rng=seed is None, external_z=external, bpd=(clip_denoised,))
        if ent is not None:
            for e in self._engines_of(denoise_fn) or ():
                e.ensure_fresh()
            step = ent["graph"].replay
        else:
            ent = self._bpd_state(denoise_fn, shape, dev, torch.Generator(dev) if seed is not None else None, external, clip_denoised)
            step = ent["body"]
        if ent["rng"] is not None:
            ent["rng"].manual_seed(seed)
        ent["x_0"].copy_(x_0)
        ent["t"].fill_(T - 1)
        ent["losses"].fill_(float("nan"))          # a sample the kernel refuses (t outside the tables) shows in every total
        ent["mses"].fill_(float("nan"))
        for _ in range(T):
            if external:
                ent["z"].copy_(next(noise_stream))
            step()
        losses, mses = ent["losses"].clone(), ent["mses"].clone()
        prior, total = self._bpd_finish(x_0, losses)
        return total, losses, prior, mses
