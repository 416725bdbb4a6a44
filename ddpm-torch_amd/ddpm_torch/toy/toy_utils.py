"""Training loop and sample-quality score of the toy pipeline (the roles of upstream ``ddpm_torch/toy/toy_utils.py``).

Interface kept from upstream: ``Trainer(model, optimizer, diffusion, epochs, trainloader, scheduler, shape, grad_norm, device,
eval_intv, chkpt_intv)`` with ``step`` / ``train`` / ``load_checkpoint`` / ``save_checkpoint``, ``trainees`` (model, optimizer,
scheduler) and the checkpoint keys {model, optimizer, scheduler, epoch, <statistics of the last epoch>}; the LR schedule advances once
per epoch, before the checkpoint.  ``Evaluator(true_data, eval_batch_size, max_eval_count, value_range, eps)`` scores generated points
by the KL divergence between their 2-D histogram and the training data's on floor(sqrt(max_eval_count // 10)) bins per axis.

The parameter update is the package's fused clip + Adam (``utils/train.py`` ``_FusedUpdate``: two launches, torch's optimiser-state
layout kept) whenever the optimiser qualifies, torch's own ``clip_grad_norm_`` + ``step`` otherwise."""
import math
import os

import numpy as np
import torch
import torch.nn as nn

from ..functions import discrete_klv2d, hist2d
from ..utils import save_scatterplot
from ..utils.train import DummyScheduler, RunningStatistics, _FusedUpdate

__all__ = ["Trainer", "Evaluator"]

_TRAINEES = ("model", "optimizer", "scheduler")


class Trainer:
    def __init__(self, model, optimizer, diffusion, epochs, trainloader, scheduler=None, shape=None, grad_norm=0,
                 device=torch.device("cpu"), eval_intv=1, chkpt_intv=10):
        self.model, self.optimizer, self.diffusion = model, optimizer, diffusion
        self.epochs, self.start_epoch = epochs, 0
        self.trainloader = trainloader
        self.shape = tuple(shape) if shape is not None else tuple(next(iter(trainloader)).shape[1:])
        self.scheduler = scheduler if scheduler is not None else DummyScheduler()
        self.grad_norm, self.device = grad_norm, device
        self.eval_intv, self.chkpt_intv = eval_intv, chkpt_intv
        self.stats = RunningStatistics(loss=None)
        self._fused = _FusedUpdate(optimizer, None)

    # ---- one step
    def loss(self, x):
        n = x.shape[0]
        t = torch.randint(self.diffusion.timesteps, (n,), dtype=torch.int64, device=self.device)
        per_sample = self.diffusion.train_losses(self.model, x_0=x, t=t)
        assert per_sample.shape == (n,)
        return per_sample

    def _update(self):
        if self._fused(self.grad_norm, 0.0):
            return
        if self.grad_norm:
            nn.utils.clip_grad_norm_(self.model.parameters(), max_norm=self.grad_norm)
        self.optimizer.step()

    def step(self, x):
        mean_loss = self.loss(x).mean()
        self.optimizer.zero_grad(set_to_none=True)
        mean_loss.backward()
        self._update()
        self.stats.update(x.shape[0], loss=mean_loss.item() * x.shape[0])

    # ---- epochs
    def sample_fn(self, n):
        out = self.diffusion.p_sample(denoise_fn=self.model, shape=(n, *self.shape), device=self.device, noise=None)
        return out.cpu().numpy()

    def _epoch_summary(self, epoch, evaluator, image_dir, plot_kwargs):
        """Statistics of the finished epoch, with the evaluator's score every ``eval_intv`` epochs (its samples are plotted)."""
        summary = dict(self.current_stats)
        if (epoch + 1) % self.eval_intv == 0 and evaluator is not None:
            self.model.eval()
            scores = evaluator.eval(self.sample_fn)
            points = scores.pop("x_gen", None)
            if points is not None and image_dir:
                save_scatterplot(os.path.join(image_dir, f"{epoch + 1}.jpg"), points, **plot_kwargs)
            summary.update(scores)
        return summary

    def train(self, evaluator=None, chkpt_path=None, image_dir=None, **plot_kwargs):
        try:
            from tqdm import tqdm
        except ImportError:
            tqdm = None
        summary = {}
        for epoch in range(self.start_epoch, self.epochs):
            self.stats.reset()
            self.model.train()
            batches = tqdm(self.trainloader, desc=f"{epoch + 1}/{self.epochs} epochs") if tqdm else self.trainloader
            for x in batches:
                self.step(x.to(self.device))
                if tqdm:
                    batches.set_postfix(self.current_stats)
            summary = self._epoch_summary(epoch, evaluator, image_dir, plot_kwargs)
            if tqdm:
                batches.set_postfix(summary)
                batches.close()
            self.scheduler.step()
            if chkpt_path and (epoch + 1) % self.chkpt_intv == 0:
                self.save_checkpoint(chkpt_path, epoch=epoch + 1, **summary)

    # ---- state
    @property
    def current_stats(self):
        return self.stats.extract()

    @property
    def trainees(self):
        return list(_TRAINEES)

    def named_state_dicts(self):
        return ((name, getattr(self, name).state_dict()) for name in self.trainees)

    def save_checkpoint(self, chkpt_path, **extra_info):
        torch.save({**dict(self.named_state_dicts()), **extra_info}, chkpt_path)

    def load_checkpoint(self, chkpt_path):
        state = torch.load(chkpt_path, map_location=self.device, weights_only=False)
        for name in self.trainees:
            getattr(self, name).load_state_dict(state[name])
        self.start_epoch = state["epoch"]


class Evaluator:
    def __init__(self, true_data, eval_batch_size=500, max_eval_count=30000, value_range=(-3, 3), eps=1e-9):
        self.eval_batch_size, self.max_eval_count = eval_batch_size, max_eval_count
        self.bins = math.floor(math.sqrt(max_eval_count // 10))
        self.value_range, self.eps = value_range, eps
        self.true_hist = self._normalised(self._counts(true_data[i:i + eval_batch_size] for i in range(0, len(true_data), eval_batch_size)))
        self.true_hist.setflags(write=False)

    def _counts(self, chunks):
        total = 0
        for chunk in chunks:
            total = total + hist2d(chunk, bins=self.bins, value_range=self.value_range)
        return total

    def _normalised(self, counts):
        return counts / (np.sum(counts) + self.eps)

    def get_histogram(self, data):
        bs = self.eval_batch_size
        return self._normalised(self._counts(data[i:i + bs] for i in range(0, len(data), bs)))

    def eval(self, sample_fn):
        """Draw ceil((max_eval_count + 1) / eval_batch_size) batches of eval_batch_size points; {"kld", "x_gen"}."""
        rounds = len(range(0, self.max_eval_count + self.eval_batch_size, self.eval_batch_size))
        drawn = [sample_fn(self.eval_batch_size) for _ in range(rounds)]
        gen_hist = self._normalised(self._counts(drawn))
        return {"kld": discrete_klv2d(gen_hist, self.true_hist), "x_gen": np.concatenate(drawn, axis=0)}
