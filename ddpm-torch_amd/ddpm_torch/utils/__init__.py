"""Config / seeding glue with the reference's names (``ddpm_torch/utils/__init__.py:39-59,62-94,96-101``)."""
import random

import numpy as np
import torch

__all__ = ["seed_all", "get_param", "ConfigDict", "save_image_grid", "infer_range", "save_scatterplot"]


def seed_all(seed):
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    if torch.cuda.is_available():
        torch.cuda.manual_seed_all(seed)


def get_param(param, obj_1, obj_2):
    """Look ``param`` up in obj_1 (JSON section), falling back to obj_2 (argparse namespace)."""
    def get(obj, attr):
        return obj[attr] if hasattr(obj, "__getitem__") else getattr(obj, attr)
    try:
        return get(obj_1, param)
    except (KeyError, AttributeError):
        return get(obj_2, param)


class ConfigDict(dict):
    """dict with attribute access; missing keys read as None."""

    def __getattr__(self, name):
        return self.get(name, None)


def save_image_grid(x, path, nrow=8, pad=2):
    """Write a batch of images in [-1, 1] ([N, C, H, W]) as one grid picture — the role torchvision's ``save_image(normalize=True,
    value_range=(-1, 1))`` plays in the reference (utils/train.py:60).  Needs Pillow; without it the tensor is saved next to the
    requested name as ``.pt``."""
    x = x.detach().float().cpu().clamp(-1, 1)
    n, c, h, w = x.shape
    nrow = max(1, min(nrow, n))
    rows = (n + nrow - 1) // nrow
    grid = torch.zeros(c, rows * (h + pad) + pad, nrow * (w + pad) + pad)
    for i in range(n):
        r, q = divmod(i, nrow)
        grid[:, pad + r * (h + pad): pad + r * (h + pad) + h, pad + q * (w + pad): pad + q * (w + pad) + w] = x[i]
    arr = (grid * 127.5 + 127.5).round().clamp(0, 255).to(torch.uint8).permute(1, 2, 0).numpy()
    try:
        from PIL import Image
    except ImportError:
        torch.save(x, path.rsplit(".", 1)[0] + ".pt")
        return
    Image.fromarray(arr.squeeze(-1) if c == 1 else arr).save(path)


def infer_range(dataset):
    """Axis limits for evaluating / plotting a 2-D toy dataset: each axis' [min, max] of ``dataset.data`` widened by 5 % of its span
    on both sides.  Returns (xlim, ylim)."""
    lims = []
    for j in (0, 1):
        lo, hi = dataset.data[:, j].min(), dataset.data[:, j].max()
        span = hi - lo
        lims.append((lo - 0.05 * span, hi + 0.05 * span))
    return tuple(lims)


def save_scatterplot(fpath, x, y=None, xlim=None, ylim=None):
    """Scatter plot of 2-D points ``x`` [N, 2] (or of ``y`` against ``x``; a 1-D ``x`` alone is plotted against its index).  Needs
    matplotlib; without it the points are saved next to the requested name as ``.npy``."""
    if hasattr(x, "ndim"):
        if x.ndim == 2:
            x, y = x[:, 0], x[:, 1]
        elif y is None:
            x, y = np.arange(len(x)), x
    try:
        import matplotlib
        matplotlib.use("Agg")
        import matplotlib.pyplot as plt
    except ImportError:
        np.save(fpath.rsplit(".", 1)[0] + ".npy", np.stack([np.asarray(x), np.asarray(y)], axis=1))
        return
    plt.figure(figsize=(6, 6))
    plt.scatter(x, y, s=0.5, alpha=0.7)
    if xlim is not None:
        plt.xlim(*xlim)
    if ylim is not None:
        plt.ylim(*ylim)
    plt.tight_layout()
    plt.savefig(fpath)
    plt.close()
