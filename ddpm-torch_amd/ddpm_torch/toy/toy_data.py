"""Synthetic 2-D point clouds for the toy pipeline (the datasets of upstream ``ddpm_torch/toy/toy_data.py``).

Interface kept from upstream: the class names, ``(size, stdev, random_state)`` constructors and their defaults, ``.data`` as a float32
[size, 2] array scaled to unit variance per axis, ``resample()``, and the random sources — isotropic noise from
``np.random.default_rng(random_state)``; which of the eight Gaussian8 centres a point belongs to from NumPy's GLOBAL generator (so
``seed_all`` makes it reproducible); the swiss roll from scikit-learn, imported only when one is drawn.  ``DataStreamer`` cuts one freshly
drawn set (``random_state=None``) into ``num_batches`` batches per pass."""
import math

import numpy as np
import torch
from torch.utils.data import Dataset

__all__ = ["Gaussian8", "Gaussian25", "SwissRoll", "DataStreamer"]


class ToyDataset(Dataset):
    """Base: subclasses say how to place ``size`` points (``_draw``) and the per-axis standard deviation of that law (``_axis_std``)."""

    def __init__(self, size, stdev, random_state=None):
        self.size, self.noise, self.random_state = size, stdev, random_state
        self.stdev = self._axis_std()
        self.data = self._draw()

    def _axis_std(self):
        raise NotImplementedError

    def _draw(self):
        raise NotImplementedError

    def resample(self):
        self.data = self._draw()

    def __len__(self):
        return self.size

    def __getitem__(self, i):
        return torch.from_numpy(self.data[i])


class _Mixture(ToyDataset):
    """Equal-weight isotropic Gaussians around fixed centres; ``_assign`` picks each point's centre."""
    scale = 2

    def __init__(self, size, stdev, random_state):
        self.modes = np.float32(self.scale) * np.asarray(self.modes, dtype=np.float32)
        super().__init__(size, stdev, random_state)

    def _assign(self):
        raise NotImplementedError

    def _draw(self):
        jitter = np.random.default_rng(self.random_state).standard_normal((self.size, 2), dtype=np.float32)
        pts = self.noise * jitter
        pts += self.modes[self._assign()]
        return pts / self.stdev


class Gaussian8(_Mixture):
    """Centres at radius 2 on the eight compass directions, chosen uniformly at random."""
    modes = [(math.cos(math.pi * k / 4), math.sin(math.pi * k / 4)) for k in range(8)]

    def __init__(self, size, stdev=0.02, random_state=1234):
        super().__init__(size, stdev, random_state)

    def _axis_std(self):
        # within-mode variance + variance of the centre's coordinate (radius^2 / 2 per axis)
        return math.sqrt(self.noise ** 2 + self.scale ** 2 * 0.5)

    def _assign(self):
        return np.random.choice(8, size=self.size, replace=True)


class Gaussian25(_Mixture):
    """A 5 x 5 lattice of centres, spacing 2, taken in turn (point i sits at centre i mod 25)."""
    modes = [(a, b) for a in (-2, -1, 0, 1, 2) for b in (-2, -1, 0, 1, 2)]

    def __init__(self, size, stdev=0.05, random_state=1234):
        super().__init__(size, stdev, random_state)

    def _axis_std(self):
        # lattice coordinates are uniform on {-4, -2, 0, 2, 4}: variance 8 = scale^2 * 2
        return math.sqrt(self.noise ** 2 + self.scale ** 2 * 2.0)

    def _assign(self):
        return np.arange(self.size) % len(self.modes)


class SwissRoll(ToyDataset):
    """scikit-learn's 3-D swiss roll seen from above (its x and z coordinates)."""

    def __init__(self, size, stdev=0.25, random_state=1234):
        super().__init__(size, stdev, random_state)

    def _axis_std(self):
        # closed-form variance of the roll's x / z coordinate (39 pi^2 / 8 - 4, -+ 1/4) plus the noise variance
        roll = 39 * math.pi ** 2 / 8 - 4
        return np.sqrt(roll + (np.array([[-0.25, 0.25]]) + self.noise ** 2))

    def _draw(self):
        from sklearn.datasets import make_swiss_roll
        xyz, _ = make_swiss_roll(self.size, noise=self.noise, random_state=self.random_state)
        plane = xyz[:, (0, 2)].astype(np.float32)
        plane /= self.stdev
        return plane


_BY_NAME = {"gaussian8": Gaussian8, "gaussian25": Gaussian25, "swissroll": SwissRoll}


class DataStreamer:
    """One pass = ``num_batches`` consecutive [batch_size, 2] slices of a set of ``batch_size * num_batches`` points; ``resample``
    redraws the set after every complete pass."""

    def __init__(self, dataset, batch_size, num_batches, resample=False):
        kind = self.dataset_map(dataset)
        self.batch_size, self.num_batches, self.resample = batch_size, num_batches, resample
        self.dataset = kind(batch_size * num_batches, random_state=None)

    def __len__(self):
        return self.num_batches

    def __iter__(self):
        bs = self.batch_size
        for start in range(0, bs * self.num_batches, bs):
            yield torch.from_numpy(self.dataset.data[start:start + bs])
        if self.resample:
            self.dataset.resample()

    @staticmethod
    def dataset_map(dataset):
        return _BY_NAME.get(dataset)
