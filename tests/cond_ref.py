"""TEST INFRASTRUCTURE: the float64 restatement of class conditioning and classifier-free guidance (Ho & Salimans 2022), composed from the
pinned oracle only.  Nothing of it exists upstream, so it is stated from the paper on top of what the fixtures pin:

* the conditional network is ``oracle.unet_ref.unet_forward`` called per sample at batch 1 with ``embed.2.bias`` replaced by
  ``embed.2.bias + table[y_b]`` — exactly ``t_emb + table[y]`` in front of the SiLU every ResidualBlock shares, with no change to the
  oracle (GroupNorm and attention are per sample, so splitting the batch is exact); row ``num_classes`` of the table is the null class;
* gradients come by autograd through it: d table[k] is the sum of the shifted bias's gradients over the samples of class k, which is what
  indexing the table leaf gives;
* the guided step is ``g = scale out_c + (1 - scale) out_u`` followed by ``oracle.diffusion_ref.model_mean_from_output`` and the noise
  term of ``p_step_from_eps`` (all three mean types; both weights sum to one, so eps, x_0 and mean outputs combine alike).

Everything follows the dtype of its inputs: float64 inputs give the reference, float32 inputs the fp32 evaluation whose terms scale a bar."""
import torch

from oracle import diffusion_ref as D
from oracle import unet_ref as U

MEAN_TYPES = ("eps", "x_0", "mean")
TABLE = "class_embed.weight"


def unet_forward(sd, cfg, x, t, y, training=False, masks=None):
    """The class-conditional network: ``sd`` holds the unconditional keys plus ``class_embed.weight`` [num_classes + 1, E]."""
    table = sd[TABLE]
    outs = []
    for b in range(x.shape[0]):
        one = {k: v for k, v in sd.items() if k != TABLE}
        one["embed.2.bias"] = sd["embed.2.bias"] + table[int(y[b])]
        mk = None if not masks else {k: v[b:b + 1] for k, v in masks.items()}
        outs.append(U.unet_forward(one, cfg, x[b:b + 1], t[b:b + 1], training=training, masks=mk))
    return torch.cat(outs, dim=0)


def combine(out_c, out_u, scale):
    return scale * out_c + (1.0 - scale) * out_u


def guided_step(T, mean_type, x_t, t, out_c, out_u, z, scale, clip):
    """(x_{t-1}, pred_x_0) of one guided step on a fixed variance table ``T["fixed_model_logvar"]``."""
    mean, pred = D.model_mean_from_output(T, mean_type, x_t, t, combine(out_c, out_u, scale), clip)
    mask = (t > 0).reshape((-1,) + (1,) * (x_t.ndim - 1)).to(x_t)
    return mean + mask * torch.exp(0.5 * D._gather(T["fixed_model_logvar"], t, x_t)) * z, pred


def guided_chain(T, mean_type, net, x_T, zs, y, null, scale, clip=True, timestep_map=None, preds=None):
    """diffusion.py:160-174 / ddim.py:96-113 with injected noise and guidance: ``net(x, t, y)`` is the conditional network, ``null`` the
    null class, zs[i] the noise of loop step i (t = S-1-i).  ``scale`` 1 evaluates the conditional branch alone."""
    x, S = x_T, len(T["posterior_mean_coef1"])
    y_null = torch.full_like(y, null)
    for i, ti in enumerate(range(S - 1, -1, -1)):
        t = torch.full((len(x),), ti, dtype=torch.int64)
        tm = t if timestep_map is None else timestep_map.gather(0, t)
        out_c = net(x, tm, y)
        out_u = out_c if scale == 1.0 else net(x, tm, y_null)
        x, pred = guided_step(T, mean_type, x, t, out_c, out_u, zs[i].to(x), scale, clip)
        if preds is not None:
            preds.append(pred)
    return x


def dropped_labels(y, u, label_drop, null):
    """The labels a conditional ``Trainer.get_input`` trains on: the null class where ``u < label_drop``."""
    return torch.where(u < label_drop, torch.full_like(y, null), y)


def oracle_trainer(sd, cfg, lr, null, **kw):
    """tests/channels_accum.py's float64 oracle of ``Trainer.step`` with the conditional network in the place of the unconditional one
    (``oracle/train_ref.py``'s step: q_sample, the eps-MSE, clip, Adam, scheduler, EMA).  ``step(x, y)`` takes the labels AFTER the drop."""
    from tests import channels_accum as CA

    class CondOracleTrainer(CA.OracleTrainer):
        def __init__(self):
            super().__init__(sd, cfg, lr, **kw)
            self.y = None

        def denoise(self, x, t, training=False, masks=None, params=None):
            assert self.block == 1
            return unet_forward(self.params if params is None else params, self.cfg, x, t, self.y, training=training, masks=masks)

        def step(self, x, y, masks=None, inputs=None):
            self.y = y
            return super().step(x, masks=masks, inputs=inputs)

    assert null == sd[TABLE].shape[0] - 1
    return CondOracleTrainer()
