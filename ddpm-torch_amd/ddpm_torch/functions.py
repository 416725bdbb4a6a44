"""Host-side functional helpers mirroring ``ddpm_torch/functions.py`` of the reference for the hot path:
``get_timestep_embedding`` (functions.py:10-26) and ``flat_mean`` (functions.py:99-101), plus the toy evaluator's NumPy histograms
``hist2d`` / ``discrete_klv2d`` (functions.py:75-97).  Device work goes through the C-ABI; CPU tensors raise (no fallback)."""
import math

import numpy as np

import torch

from . import _hip

_freq_cache = {}


def _freqs(embed_dim, device):
    key = (embed_dim, device)
    if key not in _freq_cache:
        half = embed_dim // 2
        rate = math.log(10000) / (half - 1)
        _freq_cache[key] = torch.exp(-torch.arange(half, dtype=torch.float32) * rate).to(device)
    return _freq_cache[key]


def get_timestep_embedding(timesteps, embed_dim, dtype=torch.float32):
    """[B] int64 -> [B, embed_dim] fp32: cat(sin(t f_i), cos(t f_i)), f_i = exp(-i ln(1e4)/(half-1)); zero-padded if odd."""
    if dtype != torch.float32:
        raise TypeError("the timestep embedding is fp32-only (as in the reference, functions.py:11)")
    _hip.require_cuda(timesteps)
    t = timesteps.reshape(-1).to(torch.int64).contiguous()
    out = torch.empty((t.numel(), embed_dim), dtype=torch.float32, device=t.device)
    _hip.call("ddpm_timestep_embedding", t.data_ptr(), _freqs(embed_dim, t.device).data_ptr(), out.data_ptr(), t.numel(), embed_dim, _hip.stream())
    return out


def flat_mean(x, start_dim=1):
    return torch.mean(x, dim=list(range(start_dim, x.ndim)))


def _axis_ranges(value_range):
    """None | r (both axes [-r, r]) | (lo, hi) for both axes | ((xlo, xhi), (ylo, yhi))  ->  numpy.histogram2d's ``range``."""
    if value_range is None:
        return None
    if isinstance(value_range, (int, float)):
        return ((-value_range, value_range), (-value_range, value_range))
    first = next(iter(value_range))
    return tuple(value_range) if hasattr(first, "__iter__") else (tuple(value_range), tuple(value_range))


def hist2d(data, bins, value_range=None):
    """Counts of the 2-D points ``data`` [N, 2] on a bins x bins grid (``bins="auto"``: floor(sqrt(N // 10)))."""
    pts = np.asarray(data)
    nb = math.floor(math.sqrt(len(pts) // 10)) if bins == "auto" else bins
    counts, _, _ = np.histogram2d(pts[:, 0], pts[:, 1], bins=nb, range=_axis_ranges(value_range))
    return counts


def discrete_klv2d(hist1, hist2, eps=1e-9):
    """KL(hist2 || hist1) of two normalised histograms, each cell regularised by ``eps``."""
    log_ratio = np.log(hist2 + eps) - np.log(hist1 + eps)
    return np.sum(hist2 * log_ratio)
