"""The 2-D toy diffusion of upstream ``ddpm_torch/toy/diffusion.py``: the image process of this package on [B, D] data, except that
the x_0 estimate is never clipped (toy/diffusion.py:32) and only the "mse" loss is served."""
from .. import diffusion
from .toy_model import Decoder

__all__ = ["GaussianDiffusion"]


class GaussianDiffusion(diffusion.GaussianDiffusion):
    clip_sampling = False
    bpd_decoder = 1            # t = 0 term of the bound: continuous Gaussian likelihood (toy/diffusion.py:61)

    def __init__(self, betas, model_mean_type, model_var_type, loss_type, **kwargs):
        if model_var_type in ("learned", "learned-range"):
            raise NotImplementedError(f"model_var_type {model_var_type!r} is not served for the toy pipeline (its fused decoder emits the mean "
                                      "output alone); use 'fixed-small' or 'fixed-large'")
        if loss_type == "kl":
            raise NotImplementedError("loss_type='kl' is not served for the toy pipeline (its t = 0 term is the continuous-Gaussian "
                                      "decoder likelihood); use loss_type='mse'")
        if loss_type != "mse":
            raise NotImplementedError(loss_type)
        super().__init__(betas, model_mean_type, model_var_type, loss_type, **kwargs)

    def _bind(self, denoise_fn):
        """Size the toy decoders' time tables to this schedule."""
        mods = denoise_fn.modules() if hasattr(denoise_fn, "modules") else ()
        for m in mods:
            if isinstance(m, Decoder):
                m.timesteps = self.timesteps

    def _step(self, x_t, model_out, z, t, clip_denoised, want_pred):
        return super()._step(x_t, model_out, z, t, False, want_pred)

    def train_losses(self, denoise_fn, x_0, t, noise=None):
        self._bind(denoise_fn)
        return super().train_losses(denoise_fn, x_0, t, noise=noise)

    def p_mean_var(self, denoise_fn, x_t, t, clip_denoised, return_pred):
        self._bind(denoise_fn)
        return super().p_mean_var(denoise_fn, x_t, t, clip_denoised, return_pred)

    def p_sample_step(self, denoise_fn, x_t, t, clip_denoised=True, return_pred=False, generator=None):
        self._bind(denoise_fn)
        return super().p_sample_step(denoise_fn, x_t, t, clip_denoised, return_pred, generator)

    def _sample_loop(self, denoise_fn, shape, device, noise, seed, on_step=None, z_stream=None, y=None, guidance_scale=1.0):
        if y is not None:
            raise NotImplementedError("the 2-D toy decoder is unconditional: it takes no class labels")
        self._bind(denoise_fn)
        return super()._sample_loop(denoise_fn, shape, device, noise, seed, on_step, z_stream)

    def calc_all_bpd(self, denoise_fn, x_0, clip_denoised=True, seed=None, noise_stream=None):
        """The image loop with the continuous-Gaussian decoder at t = 0; the x_0 estimate is never clipped (toy/diffusion.py:31)."""
        self._bind(denoise_fn)
        return super().calc_all_bpd(denoise_fn, x_0, clip_denoised=False, seed=seed, noise_stream=noise_stream)
