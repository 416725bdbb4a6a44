"""The 2-D toy pipeline (upstream ``ddpm_torch/toy``): the MLP denoiser on the fused HIP decoder, the non-clipping diffusion, the toy
datasets and the toy trainer / histogram-KL evaluator — the names upstream's ``train_toy.py`` imports with ``from ddpm_torch.toy import *``."""
from ..diffusion import get_beta_schedule
from .diffusion import GaussianDiffusion
from .toy_data import DataStreamer
from .toy_model import Decoder
from .toy_utils import Evaluator, Trainer

__all__ = ["GaussianDiffusion", "get_beta_schedule", "DataStreamer", "Decoder", "Trainer", "Evaluator"]
