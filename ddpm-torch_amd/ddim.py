"""DDIM sampler (Song et al. 2020) with the reference's module-level contract (``ddim.py:30-120`` of
tqch/ddpm-torch): ``get_selection_schedule`` and ``DDIM(GaussianDiffusion)`` incl. ``from_ddpm``.

Only the tables differ from the ancestral sampler; the loop and the fused device step are inherited from
``ddpm_torch.GaussianDiffusion``.  The model is evaluated at ``subsequence[t]`` (ddim.py:101) via a device gather.

Not in the reference: the deterministic (eta = 0) sampler run the other way (Song et al. 2020 §4.3, §5.3, §5.4) — ``DDIM.encode`` takes
an image to the latent that regenerates it, ``DDIM.decode`` is the sampling loop started from a given latent, ``DDIM.reconstruct`` their
composition, ``slerp`` the spherical interpolation of latents (eq. 67) and ``DDIM.interpolate`` encode -> slerp -> decode.  Conventions,
with ``ab[i] = alphas_bar[subsequence[i]]``, ``ab_prev[i] = ab[i-1]``, ``ab_prev[0] = 1``: encode step i (i = 0 ... S-1) takes the state from
level i-1 to level i on the network output at ``subsequence[i]``, the timestep the sampling step i evaluates,

    x_next = cx[i] x + ce[i] eps,    cx = sqrt(ab / ab_prev),    ce = sqrt(1 - ab) - sqrt(ab (1 - ab_prev) / ab_prev)

(the two-coefficient form: no sqrt(1 / ab)-sized cancellation through an x_0 estimate), never clips, and exists for eta = 0 and the eps
parameterisation only.  One fused kernel behind the network per step (csrc/ddim.hip), captured once and replayed like the sampling step.
"""
import math
import os

import torch

import ddpm_torch
from ddpm_torch import _hip

__all__ = ["get_selection_schedule", "DDIM", "slerp"]

_ENCODE_TABLES = ("ddim_encode_cx", "ddim_encode_ce", "sqrt_recip_alphas_bar_prev", "sqrt_recip_m1_alphas_bar_prev")


def get_selection_schedule(schedule, size, timesteps):
    """Sub-sequence of original timesteps (ddim.py:30-44).  NB 'quadratic' can repeat an entry (size 50 -> two zeros)."""
    assert schedule in {"linear", "quadratic"}
    if schedule == "linear":
        return torch.arange(0, timesteps, timesteps // size)
    return torch.pow(torch.linspace(0, math.sqrt(timesteps * 0.8), size), 2).round().to(torch.int64)


def slerp(z_a, z_b, alphas):
    """Spherical interpolation (Song et al. 2020 eq. 67) of the latent pairs ``z_a[p], z_b[p]`` ([P, ...] CUDA tensors of one shape) at
    every ``alphas[k]`` (a tensor or a sequence of K numbers): ``[P, K, ...]`` float32.  The angle of a pair is that of its two whole
    flattened samples; a pair that is (anti)parallel to 1e-6 in the cosine, or whose cosine is not finite, is interpolated linearly
    (include/ddpm_hip.h `ddpm_slerp`).  Two launches, bit-reproducible."""
    _hip.require_cuda(z_a, z_b)
    if z_a.shape != z_b.shape or z_a.ndim < 1:
        raise ValueError(f"slerp needs two batches of one shape, got {tuple(z_a.shape)} and {tuple(z_b.shape)}")
    z_a, z_b = z_a.contiguous().float(), z_b.contiguous().float()
    al = torch.as_tensor(alphas, dtype=torch.float32).reshape(-1).to(z_a.device).contiguous()
    P, K = z_a.shape[0], al.numel()
    n = z_a[0].numel() if P else 0
    out = torch.empty((P, K) + tuple(z_a.shape[1:]), dtype=torch.float32, device=z_a.device)
    if P == 0 or K == 0 or n == 0:
        return out
    ws = torch.empty(int(_hip.lib().ddpm_slerp_workspace_floats(P, n)), dtype=torch.float32, device=z_a.device)
    _hip.call("ddpm_slerp", z_a.data_ptr(), z_b.data_ptr(), al.data_ptr(), out.data_ptr(), ws.data_ptr(), P, K, n, _hip.stream())
    return out


class DDIM(ddpm_torch.GaussianDiffusion):
    def __init__(self, betas, model_mean_type, model_var_type, loss_type, eta, subsequence):
        super().__init__(betas, model_mean_type, model_var_type, loss_type)
        self.eta = eta
        eta2 = eta ** 2
        if (eta2 != 1.0 and model_var_type != "fixed-small") or self.learned_var:
            # silent coercion, as ddim.py:53-59.  A learned-variance model is sampled on these eta-scaled tables too, at any eta: its mean
            # half alone is read (``learned_var`` stays set: the network output is [B, 2C, H, W]; var_mode 0 of ddpm_p_sample_step_lv)
            self.model_var_type = "fixed-small"
        ab = self.alphas_bar[subsequence]
        ab_prev = torch.cat([torch.ones(1, dtype=torch.float64), ab[:-1]], dim=0)
        self.alphas = ab / ab_prev
        self.betas = 1.0 - self.alphas
        self._build_tables(self.betas, ab, eta2=eta2)             # (also alphas_bar_prev and sqrt_alphas_bar_prev, ddim.py:66-67)
        self.subsequence = torch.as_tensor(subsequence)
        self._sub_dev = {}
        # the encoder's tables (fp64 like every other one; _tab casts them to fp32 once per device)
        self.ddim_encode_cx = torch.sqrt(ab / ab_prev)
        self.ddim_encode_ce = torch.sqrt(1.0 - ab) - torch.sqrt(ab * (1.0 - ab_prev) / ab_prev)
        self.sqrt_recip_alphas_bar_prev = torch.sqrt(1.0 / ab_prev)
        self.sqrt_recip_m1_alphas_bar_prev = torch.sqrt(1.0 / ab_prev - 1.0)

    def _num_steps(self):
        return len(self.subsequence)

    def _model_t(self, t):
        dev = t.device
        if dev not in self._sub_dev:
            self._sub_dev[dev] = self.subsequence.to(torch.int64).to(dev).contiguous()
        out = torch.empty_like(t)
        _hip.call("ddpm_gather_i64", t.data_ptr(), self._sub_dev[dev].data_ptr(), out.data_ptr(), t.numel(), _hip.stream())
        return out

    def p_sample_step(self, denoise_fn, x_t, t, clip_denoised=True, return_pred=False, generator=None):
        return super().p_sample_step(lambda x, tt: denoise_fn(x, self._model_t(tt)), x_t, t, clip_denoised, return_pred, generator)

    @torch.inference_mode()
    def p_sample(self, denoise_fn, shape, device=torch.device("cpu"), noise=None, seed=None, y=None, guidance_scale=1.0):
        """ddim.py:96-113: S = len(subsequence) steps, same RNG consumption order as the ancestral loop.  ``y`` / ``guidance_scale``
        (not in the reference): class labels and classifier-free guidance as in ``GaussianDiffusion.p_sample`` — the guided step kernel on
        this sampler's own tables."""
        return self._sample_loop(denoise_fn, shape, device, noise, seed, y=y, guidance_scale=guidance_scale)

    # ------------------------------------------------------------------ the sampler's ODE in both directions
    def _check_invertible(self):
        if self.eta != 0:
            raise ValueError(f"DDIM.encode inverts the deterministic sampler: eta must be 0, got {self.eta}")
        if self.model_mean_type != "eps":
            raise NotImplementedError(
                f"DDIM.encode is defined for model_mean_type 'eps', got {self.model_mean_type!r}: written through an x_0 estimate the step is "
                "x_next = sqrt(ab) x_0 + sqrt(1 - ab) (x - sqrt(ab_prev) x_0) / sqrt(1 - ab_prev), which is 0 / 0 at step 0 (ab_prev = 1)")

    def _ode_state(self, denoise_fn, shape, dev, kind, want_pred=False):
        """Buffers and step body of a deterministic-direction loop.  ``kind`` = ("encode",): network, fused encode update in place, t += 1;
        ("decode", clip): network, the sampling update in place with that clip flag, t -= 1 (its noise is a buffer of zeros at eta = 0 —
        no generator is touched — and a draw from the default generator otherwise)."""
        x_t = torch.zeros(shape, dtype=torch.float32, device=dev)
        pred = torch.empty_like(x_t) if want_pred else None
        B, n, S = shape[0], x_t[0].numel(), self._num_steps()
        encode = kind[0] == "encode"
        t = torch.full((B,), 0 if encode else S - 1, dtype=torch.int64, device=dev)
        if encode:
            tabs = [self._tab(n_, dev) for n_ in _ENCODE_TABLES]
            z = None
        else:
            tabs = [self._tab(n_, dev) for n_ in ddpm_torch.diffusion._STEP_TABLES]
            z = torch.zeros_like(x_t)
            mean_code, clip = ddpm_torch.diffusion._MEAN_CODE[self.model_mean_type], int(bool(kind[1]))
        C = shape[1] if len(shape) > 1 else None

        def body(cut=None):
            out = denoise_fn(x_t, self._model_t(t))
            if self.learned_var:                       # a 2C-channel model: the mean half, as a plain copy
                self._check_two_halves(out, x_t)
                out = out[:, :C]
            out = out.contiguous().float()
            if encode:
                _hip.call("ddpm_ddim_encode_step", x_t.data_ptr(), out.data_ptr(), t.data_ptr(), *[tb.data_ptr() for tb in tabs],
                          x_t.data_ptr(), _hip.ptr(pred), B, n, S, _hip.stream())             # in place: each element is read once, then written
                _hip.call("ddpm_add_i64", t.data_ptr(), B, 1, _hip.stream())
            else:
                if self.eta != 0:
                    z.normal_()
                _hip.call("ddpm_p_sample_step", x_t.data_ptr(), out.data_ptr(), z.data_ptr(), t.data_ptr(), *[tb.data_ptr() for tb in tabs],
                          x_t.data_ptr(), _hip.ptr(pred), B, n, mean_code, clip, S, _hip.stream())
                _hip.call("ddpm_add_i64", t.data_ptr(), B, -1, _hip.stream())

        return {"x_t": x_t, "t": t, "z": z, "pred": pred, "rng": None, "body": body, "ref": lambda: denoise_fn}

    def _capture_kind_step(self, denoise_fn, shape, device, default_rng, external_z, kind):
        if kind[0] not in ("encode", "decode"):                    # the conditional / guided sampling step: the base class captures it
            return super()._capture_kind_step(denoise_fn, shape, device, default_rng, external_z, kind)
        ent = self._ode_state(denoise_fn, shape, device, kind)
        ent["graph"] = self._capture_step(device, None, ent["body"], "DDIM " + kind[0])
        return ent if ent["graph"] is not None else None

    def _ode_loop(self, denoise_fn, x, kind, on_step=None):
        """S steps of ``kind`` from ``x``: the captured step replayed, or the eager loop under the conditions the sampler runs it
        (DDPM_TORCH_AMD_GRAPH=0, fewer than 4 steps, a capture in progress, a per-step read-back)."""
        x, = self._prep(x)
        dev, shape, S = x.device, tuple(x.shape), self._num_steps()
        ent = None
        if (on_step is None and S >= 4 and dev.type == "cuda" and os.environ.get("DDPM_TORCH_AMD_GRAPH", "1") != "0"
                and not torch.cuda.is_current_stream_capturing()):
            ent = self._graph_entry(denoise_fn, shape, dev, default_rng=True, kind=kind)
        if ent is not None:
            for e in self._engines_of(denoise_fn) or ():
                e.ensure_fresh()
            step = ent["graph"].replay
        else:
            ent = self._ode_state(denoise_fn, shape, dev, kind, want_pred=on_step is not None)
            step = ent["body"]
        ent["x_t"].copy_(x)
        ent["t"].fill_(0 if kind[0] == "encode" else S - 1)
        for i in range(S):
            step()
            if on_step is not None:
                on_step(i, ent["pred"])
        return ent["x_t"].clone()

    def encode(self, denoise_fn, x_0, return_pred=False, y=None):
        """The latent x_T that the eta = 0 sampler takes back to ``x_0`` (up to the discretisation error of S steps): S network
        evaluations at ``subsequence[0 ... S-1]`` with the fused update of the module docstring behind each.  No clipping, no RNG.
        ``return_pred``: also the x_0 estimates of the S steps, ``[S, B, ...]`` on the device (this per-step read-back runs the eager
        loop).  Raises ValueError for eta != 0 and NotImplementedError for the x_0 / mean parameterisations.  ``y``: class labels of a
        class-conditional network, evaluated conditionally (guidance scale 1; guided inversion is not served)."""
        self._check_invertible()
        if y is not None:
            denoise_fn = ddpm_torch.diffusion.Conditioned(denoise_fn, y.to(x_0.device))
        preds = []
        keep = (lambda i, pred: preds.append(pred.clone())) if return_pred else None
        with torch.inference_mode(), self._time_tables(denoise_fn):
            latent = self._ode_loop(denoise_fn, x_0, ("encode",), on_step=keep)
            return (latent, torch.stack(preds)) if return_pred else latent

    def decode(self, denoise_fn, latent, clip_denoised=True, y=None):
        """The sampling loop started from ``latent`` (level S-1) with an explicit clip flag: x_0, float32 on the latent's device.  At
        eta = 0 it is deterministic and touches no generator.  ``y``: as in ``encode``."""
        if y is not None:
            denoise_fn = ddpm_torch.diffusion.Conditioned(denoise_fn, y.to(latent.device))
        with torch.inference_mode(), self._time_tables(denoise_fn):
            return self._ode_loop(denoise_fn, latent, ("decode", bool(clip_denoised)))

    def reconstruct(self, denoise_fn, x_0, clip_denoised=False, y=None):
        """``decode(encode(x_0))`` -> ``(x_rec, latent)`` (Song et al. 2020 §5.4, Table 2)."""
        latent = self.encode(denoise_fn, x_0, y=y)
        return self.decode(denoise_fn, latent, clip_denoised, y=y), latent

    def interpolate(self, denoise_fn, x_a, x_b, num=9, encoded=False, clip_denoised=True, batch_size=None):
        """Semantic interpolation of the pairs ``x_a[p], x_b[p]`` (Song et al. 2020 §5.3): both ends are encoded in one batch of 2 P
        (``encoded=True``: they already are latents), the latents are slerped at ``linspace(0, 1, num)`` and the P * num results decoded in
        batches of ``batch_size`` (default: all at once).  Returns ``[P, num, C, H, W]``."""
        if x_a.shape != x_b.shape:
            raise ValueError(f"interpolate needs two batches of one shape, got {tuple(x_a.shape)} and {tuple(x_b.shape)}")
        P = x_a.shape[0]
        if encoded:
            z_a, z_b = x_a, x_b
        else:
            z = self.encode(denoise_fn, torch.cat([x_a, x_b], dim=0))
            z_a, z_b = z[:P], z[P:]
        z = slerp(z_a, z_b, torch.linspace(0.0, 1.0, num)).reshape((P * num,) + tuple(x_a.shape[1:]))
        step = batch_size or max(P * num, 1)
        out = [self.decode(denoise_fn, z[i:i + step], clip_denoised) for i in range(0, P * num, step)]
        return torch.cat(out, dim=0).reshape((P, num) + tuple(x_a.shape[1:]))

    def calc_all_bpd(self, denoise_fn, x_0, clip_denoised=True, seed=None, noise_stream=None):
        raise NotImplementedError("the variational bound is defined on the full chain; DDIM's tables are those of a sub-sequence — "
                                  "evaluate bits/dim with the GaussianDiffusion the sampler was derived from")

    @classmethod
    def from_ddpm(cls, diffusion, eta, subsequence):
        keys = ("betas", "model_mean_type", "model_var_type", "loss_type")
        return cls(**{k: diffusion.__dict__.get(k, None) for k in keys}, eta=eta, subsequence=subsequence)
