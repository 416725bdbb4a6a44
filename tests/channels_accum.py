"""Shared by tests/test_channels_accum_host.py and tests/test_channels_accum_gpu.py (TEST INFRASTRUCTURE): networks whose edge
channel counts are not 3, a float64 oracle of ``Trainer.step`` with gradient accumulation, and the dropout masks of one forward.

What the shipped command lines build besides the 3 -> 3 network every other test uses: ``train.py --block-size 2`` wraps the UNet in
``ModelWrapper(PixelUnshuffle(2), PixelShuffle(2))`` (12 channels in and out on the RGB data sets, 4 on MNIST), ``--dataset mnist``
gives 1 channel, and ``--num-accum N`` sends every step through the generic autograd branch of ``Trainer.step``."""
import torch
import torch.nn.functional as F

from ddpm_torch import _hip
from oracle import diffusion_ref as D
from oracle import unet_ref as U

TINY = dict(in_channels=3, hid_channels=32, out_channels=3, ch_multipliers=[1, 2], num_res_blocks=1, apply_attn=[False, True], drop_rate=0.0)
GEN_SEED = 8191                              # utils/train.py:115 (rank 0)


def edge(cfg, cin, cout, drop=None):
    """``cfg`` with its edge channel counts (and optionally its dropout rate) overridden."""
    return dict(cfg, in_channels=cin, out_channels=cout, **({} if drop is None else {"drop_rate": drop}))


def masks_from_tape(m, drop_rate, device):
    """{res-block prefix: keep mask [B, C, H, W]} of the forward whose tape the engine kept (``debug_keep_tape``), rebuilt from the
    recorded seeds through ddpm_dropout_mask; the oracle consumes the very masks the engine used."""
    eng, names, masks = m.engine(), {id(mod): name for name, mod in m.named_modules()}, {}
    for rec in eng.last_tape:
        if rec[0] != "res" or drop_rate <= 0:
            continue
        h1, seed = rec[6], rec[9]
        n = h1.B * h1.H * h1.W * h1.C
        mk = torch.empty(n, device=device)
        _hip.call("ddpm_dropout_mask", mk.data_ptr(), n, drop_rate, seed, _hip.stream())
        masks[names[id(rec[1])] + "."] = mk.cpu().reshape(h1.B, h1.H, h1.W, h1.C).permute(0, 3, 1, 2)
    return masks


def reference_stream(seed=GEN_SEED, timesteps=1000):
    """draw(x) -> (t, noise) in the reference's order (utils/train.py:134-141: t first, then noise, from one CPU generator)."""
    gen = torch.Generator("cpu").manual_seed(seed)

    def draw(x):
        t = torch.empty((x.shape[0],), dtype=torch.int64).random_(to=timesteps, generator=gen)
        noise = torch.empty(tuple(x.shape), dtype=torch.float32).normal_(generator=gen)
        return t, noise
    return draw


class OracleTrainer:
    """float64 restatement of utils/train.py:148-170 with ``num_accum`` micro-batches per update: every call backpropagates
    ``loss / num_accum`` into gradients that accumulate; every ``num_accum``-th call clips, runs Adam, the scheduler and the EMA
    (:300-305).  ``block`` > 1: the network sits between pixel-unshuffle and pixel-shuffle (train.py:69-72)."""

    def __init__(self, sd, cfg, lr, num_accum=1, lr_lambda=None, block=1, grad_norm=1.0, ema_decay=0.9999, seed=GEN_SEED, timesteps=1000):
        self.cfg, self.num_accum, self.block, self.grad_norm, self.ema_decay = cfg, num_accum, block, grad_norm, ema_decay
        self.params = {k: v.detach().double().clone().requires_grad_(True) for k, v in sd.items()}
        self.opt = torch.optim.Adam(list(self.params.values()), lr=lr, betas=(0.9, 0.999))
        self.sched = torch.optim.lr_scheduler.LambdaLR(self.opt, lr_lambda=lr_lambda) if lr_lambda is not None else None
        self.shadow = {k: v.detach().clone() for k, v in self.params.items()}
        self.num_updates, self.calls = -1, 0
        self.tables = D.ddpm_tables(D.beta_schedule("linear", 1e-4, 0.02, timesteps), "fixed-large")
        self.draw = reference_stream(seed, timesteps)

    def denoise(self, x, t, training=False, masks=None, params=None):
        y = x if self.block == 1 else F.pixel_unshuffle(x, self.block)
        y = U.unet_forward(self.params if params is None else params, self.cfg, y, t, training=training, masks=masks)
        return y if self.block == 1 else F.pixel_shuffle(y, self.block)

    def step(self, x, masks=None, inputs=None):
        """One ``Trainer.step`` call; returns (mean loss of the micro-batch, whether the parameters were updated)."""
        t, noise = self.draw(x) if inputs is None else inputs
        x, noise = x.double(), noise.double()
        x_t = D.q_sample(self.tables, x, t, noise)
        loss = D.mse_eps_loss(self.denoise(x_t, t, training=True, masks=masks), noise).mean()
        (loss / self.num_accum).backward()
        self.calls += 1
        updated = self.calls % self.num_accum == 0
        if updated:
            torch.nn.utils.clip_grad_norm_(list(self.params.values()), max_norm=self.grad_norm)
            self.opt.step()
            self.opt.zero_grad(set_to_none=True)
            if self.sched is not None:
                self.sched.step()
            self.num_updates += 1
            d = min(self.ema_decay, (1 + self.num_updates) / (10 + self.num_updates))
            with torch.no_grad():
                for k, p in self.params.items():
                    self.shadow[k] += (1 - d) * (p.data - self.shadow[k])
        return float(loss.detach()), updated

    def state(self):
        return {k: v.detach() for k, v in self.params.items()}


def snapshot(model, ema):
    """Bit copies of the live parameters and of the EMA shadow (host tensors)."""
    return ({k: v.detach().cpu().clone() for k, v in model.state_dict().items()},
            {k: v.detach().cpu().clone() for k, v in ema.shadow.items()})


def assert_bit_equal(now, before, what):
    for k, v in before.items():
        assert torch.equal(now[k], v), f"{what}.{k} changed on a call that is not an update"


def strip(sd, prefix="_model."):
    """State dict of a ModelWrapper -> the keys of the UNet inside it."""
    return {(k[len(prefix):] if k.startswith(prefix) else k): v for k, v in sd.items()}
