"""TEST INFRASTRUCTURE (no test functions): the UNet's constructor options and process types TOGETHER — class conditioning, multi-head
attention, the scale-shift norm, a learned reverse-process variance, dropout, conv-free resampling, both compute modes — as one float64
reference composed of the four single-option ones, and the table of networks the option tests build.

The composed reference.  tests/adagn_ref.py and tests/mha_ref.py rebind two different names of ``oracle.unet_ref`` (``residual_block``,
``attention_core``) for the duration of a ``with`` block; tests/cond_ref.py calls ``oracle.unet_ref.unet_forward`` per sample with the class
row added to ``embed.2.bias``.  ``forward64`` stacks the bindings an option set asks for around the conditional or the plain forward and
binds nothing an option set does not ask for, so with one option on it IS that option's own reference (tests/test_option_rows_host.py holds
it to that with ``torch.equal``).  The learned variance changes no network code: ``out_channels`` is 2C and tests/learned_var_ref.py reads
the two halves.

``ROWS``: one network configuration plus process per row, written out literally.  The factors and their levels are ``FACTORS``; the table
covers every pair of levels of every two factors in 12 rows (tests/test_option_rows_host.py recomputes that and fails when a row is
deleted).  Geometry decides the network, because the engine's attention paths are a function of the token count (``ops.attention_path``,
``_Engine._need_vec_tokens`` / ``_attn_mat``):

  8 x 8    NETS["two"]    64 ch / 64 tokens, 128 ch / 16 tokens, middle 16 tokens
  24 x 18  NETS["two"]    64 ch / 432 tokens (above the on-chip pair's 256), 128 ch / 108 tokens (a multiple of 4, which the fp32 mode
                          needs, and no multiple of 8 — what the streaming pair exists for), middle 108.  Level 1 is 12 x 9: an odd width.
  16 x 16  NETS["three"]  64 ch / 256 tokens (the on-chip pair's last size), 128 ch / 64 tokens, a third level without attention at 4 x 4,
                          middle 16 tokens
  24 x 16  NETS["wide"]   128 ch / 384 tokens, 128 ch / 96 tokens, middle 96: the one geometry at which a single bf16 head reaches the
                          inference-only "fused" kernel (L % 128 == 0, C in {128, 256}, and L > 256 — up to 256 tokens the rule asks for
                          "flash" first).  The network's last level feeds ``out_conv`` at ``hid_channels``, so 128 channels at the
                          image's own size means hid_channels = 128 with multipliers [1, 1]: the one row outside the hid_channels = 64
                          family.  It is no level of the geometry factor; the row that carries it counts for its other factors.

``paths`` of a row is what its author expects ``ops.attention_path`` to answer per token count, (training, inference); the GPU test reads
the training one off the engine's tape.  fp32 rows run "mat" everywhere; a bf16 row with a head index runs the streaming pair ("stream",
the ``mh`` entry points) at every size; a single bf16 head runs "flash" up to 256 tokens in multiples of 16 and "stream" beyond."""
import contextlib
import functools

import torch

from oracle import diffusion_ref as D
from oracle import unet_ref as U
from tests import adagn_ref as AR
from tests import channels_accum as CA
from tests import cond_ref as CR
from tests import ddim_inverse_ref as IR
from tests import learned_var_ref as LV
from tests import mha_ref as MR

K = 3                                               # classes of a conditional row; class K is the null class
B = 3
NETS = {"two": dict(hid_channels=64, ch_multipliers=[1, 2], apply_attn=[True, True]),
        "three": dict(hid_channels=64, ch_multipliers=[1, 2, 2], apply_attn=[True, True, False]),
        "wide": dict(hid_channels=128, ch_multipliers=[1, 1], apply_attn=[True, True])}
NET_OF_SIZE = {(8, 8): "two", (24, 18): "two", (16, 16): "three", (24, 16): "wide"}
FUSED_SIZE = (24, 16)

FACTORS = {
    "cond": [None, K],
    "heads": ["1", "num_heads=2", "num_head_channels=32"],
    "ssn": [False, True],
    "var_loss": [("fixed-large", "mse"), ("learned-range", "hybrid"), ("learned", "kl")],
    "drop": [0.0, 0.1],
    "rwc": [True, False],
    "mode": ["fp32", "bf16"],
    "size": [(8, 8), (24, 18), (16, 16)],
}
HEADS = {"1": {}, "num_heads=2": {"num_heads": 2}, "num_head_channels=32": {"num_head_channels": 32}}
ALL_ON = dict(cond=K, heads="num_head_channels=32", ssn=True, var_loss=("learned-range", "hybrid"), drop=0.1, size=(24, 18))

MAT2 = {64: ("mat", "mat"), 16: ("mat", "mat")}
MAT3 = {256: ("mat", "mat"), 64: ("mat", "mat"), 16: ("mat", "mat")}
MATN = {432: ("mat", "mat"), 108: ("mat", "mat")}
ST2 = {64: ("stream", "stream"), 16: ("stream", "stream")}
ST3 = {256: ("stream", "stream"), 64: ("stream", "stream"), 16: ("stream", "stream")}
STN = {432: ("stream", "stream"), 108: ("stream", "stream")}

ROWS = [
    dict(id="all-on-fp32", cond=K, heads="num_head_channels=32", ssn=True, var_loss=("learned-range", "hybrid"), drop=0.1, rwc=False,
         mode="fp32", size=(24, 18), paths=MATN),
    dict(id="all-on-bf16", cond=K, heads="num_head_channels=32", ssn=True, var_loss=("learned-range", "hybrid"), drop=0.1, rwc=False,
         mode="bf16", size=(24, 18), paths=STN),
    dict(id="fused-1head-ssn-kl-bf16", cond=None, heads="1", ssn=True, var_loss=("learned", "kl"), drop=0.0, rwc=True,
         mode="bf16", size=FUSED_SIZE, paths={384: ("stream", "fused"), 96: ("flash", "flash")}),
    dict(id="cond-2heads-fixed-fp32", cond=K, heads="num_heads=2", ssn=False, var_loss=("fixed-large", "mse"), drop=0.0, rwc=True,
         mode="fp32", size=(16, 16), paths=MAT3),
    dict(id="2heads-ssn-range-bf16", cond=None, heads="num_heads=2", ssn=True, var_loss=("learned-range", "hybrid"), drop=0.0, rwc=True,
         mode="bf16", size=(8, 8), paths=ST2),
    dict(id="1head-kl-drop-fp32", cond=None, heads="1", ssn=False, var_loss=("learned", "kl"), drop=0.1, rwc=False,
         mode="fp32", size=(16, 16), paths=MAT3),
    dict(id="hc32-fixed-drop-bf16", cond=None, heads="num_head_channels=32", ssn=False, var_loss=("fixed-large", "mse"), drop=0.1, rwc=True,
         mode="bf16", size=(24, 18), paths=STN),
    dict(id="cond-hc32-kl-fp32", cond=K, heads="num_head_channels=32", ssn=False, var_loss=("learned", "kl"), drop=0.0, rwc=False,
         mode="fp32", size=(8, 8), paths=MAT2),
    dict(id="cond-1head-ssn-fixed-drop-bf16", cond=K, heads="1", ssn=True, var_loss=("fixed-large", "mse"), drop=0.1, rwc=False,
         mode="bf16", size=(8, 8), paths={64: ("flash", "flash"), 16: ("flash", "flash")}),
    dict(id="2heads-kl-drop-bf16", cond=None, heads="num_heads=2", ssn=False, var_loss=("learned", "kl"), drop=0.1, rwc=False,
         mode="bf16", size=(24, 18), paths=STN),
    dict(id="1head-range-bf16", cond=None, heads="1", ssn=False, var_loss=("learned-range", "hybrid"), drop=0.0, rwc=True,
         mode="bf16", size=(24, 18), paths=STN),
    dict(id="cond-hc32-ssn-range-bf16", cond=K, heads="num_head_channels=32", ssn=True, var_loss=("learned-range", "hybrid"), drop=0.0, rwc=True,
         mode="bf16", size=(16, 16), paths=ST3),
]
ROW = {r["id"]: r for r in ROWS}

# what the package refuses by design, and the cell of variance x loss each refusal empties: the reason ``var_loss`` is ONE factor of three
# levels and not two of three.  (The remaining cells — a fixed variance under "kl", learned-range under "kl", learned under "hybrid" — are
# served; they are no levels of this table.)  The fourth refusal empties no cell of the table: it is why the guided ANCESTRAL chain is run
# on the fixed-variance conditional row alone.
EXCLUDED = {
    (("variance", "fixed-large"), ("loss", "hybrid")): "GaussianDiffusion: ValueError, 'hybrid' trains a learned variance",
    (("variance", "learned-range"), ("loss", "mse")): "GaussianDiffusion: ValueError, 'mse' gives the variance half no gradient",
    (("variance", "learned"), ("loss", "mse")): "GaussianDiffusion: ValueError, 'mse' gives the variance half no gradient",
}
GUIDED_LEARNED = "GaussianDiffusion.p_sample: NotImplementedError, guidance_scale != 1 of a learned-variance model"


def learned(row):
    return row["var_loss"][0] in ("learned", "learned-range")


def var_type(row):
    return row["var_loss"][0] if learned(row) else None


def cfg_of(row):
    """The oracle's configuration (the reference's keys only)."""
    return dict(in_channels=3, out_channels=6 if learned(row) else 3, num_res_blocks=1, drop_rate=row["drop"],
                resample_with_conv=row["rwc"], **NETS[NET_OF_SIZE[row["size"]]])


def opts_of(row):
    """The constructor options that are not the reference's."""
    return dict(num_classes=row["cond"], use_scale_shift_norm=row["ssn"], **HEADS[row["heads"]])


def build(row):
    import ddpm_torch
    return ddpm_torch.UNet(**cfg_of(row), **opts_of(row))


@functools.lru_cache(maxsize=None)
def weights(row_id):
    """(fp32 state dict, its float64 copy) of a row's network, every tensor randomised as the option files do."""
    torch.manual_seed(5)
    sd = U.randomize_state_dict(build(ROW[row_id]).state_dict(), 17)
    return sd, {k: v.double() for k, v in sd.items()}


def r(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


@functools.lru_cache(maxsize=None)
def inputs(row_id):
    """x, t, y, gy of the forward-and-gradient test at B = 3: one sample at t = 0; two different classes, the null class among the three
    labels, class 1 without a sample (``y`` is None on an unconditional row)."""
    row = ROW[row_id]
    H, W = row["size"]
    x, gy = r(B, 3, H, W, seed=1), r(B, cfg_of(row)["out_channels"], H, W, seed=2)
    return x, torch.tensor([0, 977, 40]), (torch.tensor([2, 0, K]) if row["cond"] else None), gy


# --------------------------------------------------------------------------------------------------------------- the composed reference
def forward64(sd, cfg, opts, x, t, y=None, training=False, masks=None):
    """The network of ``cfg`` + ``opts`` in the dtype of its inputs.  ``opts``: num_classes, num_heads, num_head_channels,
    use_scale_shift_norm (missing keys are off).  ``y``: the labels of a conditional network (None: the null class for every sample)."""
    heads, hc = opts.get("num_heads") or 1, opts.get("num_head_channels")
    with contextlib.ExitStack() as stack:
        if opts.get("use_scale_shift_norm"):
            stack.enter_context(AR.bound())
        if heads != 1 or hc is not None:
            stack.enter_context(MR.bound(heads, hc))
        if opts.get("num_classes") is None:
            assert y is None, "labels for an unconditional network"
            return U.unet_forward(sd, cfg, x, t, training=training, masks=masks)
        if y is None:
            y = torch.full((x.shape[0],), opts["num_classes"], dtype=torch.int64)
        return CR.unet_forward(sd, cfg, x, t, y, training=training, masks=masks)


def forward_and_gradients64(row_id, masks=None, training=True):
    """(out, {name: gradient}) of sum(out * gy) on ``inputs(row_id)`` in float64."""
    row = ROW[row_id]
    x, t, y, gy = inputs(row_id)
    p = {k: v.clone().requires_grad_(True) for k, v in weights(row_id)[1].items()}
    out = forward64(p, cfg_of(row), opts_of(row), x.double(), t, y, training=training, masks=masks)
    (out * gy.double()).sum().backward()
    return out.detach(), {k: v.grad for k, v in p.items()}


def host_masks(row_id, seed=9):
    """Keep masks of the rate of the row for a CPU run of the reference (the GPU test rebuilds the engine's own from its tape)."""
    row = ROW[row_id]
    cfg = cfg_of(row)
    if row["drop"] <= 0:
        return None
    g, out = torch.Generator().manual_seed(seed), {}
    H, W = row["size"]
    chs = [cfg["hid_channels"] * m for m in cfg["ch_multipliers"]]
    L = len(chs)
    for p in U.res_block_prefixes(cfg):
        lvl = L - 1 if p.startswith("middle") else int(p.split("level_")[1].split(".")[0])
        out[p] = torch.rand(B, chs[lvl], H >> lvl, W >> lvl, generator=g) >= row["drop"]
    return out


def oracle_trainer(row, lr, **kw):
    """tests/channels_accum.py's float64 oracle of ``Trainer.step`` on the composed network: ``denoise`` is ``forward64`` with the labels
    AFTER the drop (as tests/cond_ref.py's), the loss tests/learned_var_ref.py's hybrid loss when the row's variance is learned (as its
    ``oracle_trainer``; vlb_weight = T / 1000 = 1) and the eps-MSE otherwise.  Everything behind the loss is the base classes'.
    ``step(x, y=None, masks=None, inputs=None)``."""
    sd, cfg, opts = weights(row["id"])[0], cfg_of(row), opts_of(row)
    if row["var_loss"][1] == "kl":
        raise NotImplementedError("no trainer row of the table trains under 'kl'")
    base = type(LV.oracle_trainer(sd, cfg, lr, "eps", row["var_loss"][0], 1.0, **kw)) if learned(row) else CA.OracleTrainer

    class ComposedOracleTrainer(base):
        def __init__(self):
            if learned(row):
                base.__init__(self)
            else:
                base.__init__(self, sd, cfg, lr, **kw)
            self.y = None

        def denoise(self, x, t, training=False, masks=None, params=None):
            assert self.block == 1
            return forward64(self.params if params is None else params, self.cfg, opts, x, t, self.y, training=training, masks=masks)

        def step(self, x, y=None, masks=None, inputs=None):
            assert (y is None) == (opts["num_classes"] is None)
            self.y = y
            return super().step(x, masks=masks, inputs=inputs)

    assert issubclass(ComposedOracleTrainer, CA.OracleTrainer)
    return ComposedOracleTrainer()


# --------------------------------------------------------------------------------------------------------------- chains
def betas(T):
    return D.beta_schedule("linear", 1e-4, 0.02, T)


def net64(row, y=None):
    """``net(x, t)`` of the row in float64 with the labels bound (the conditional branch at guidance scale 1)."""
    sd64, cfg, opts = weights(row["id"])[1], cfg_of(row), opts_of(row)
    return lambda x, t: forward64(sd64, cfg, opts, x, t, y)


def sample_chain64(row, T, x_T, zs, y=None):
    """The ancestral chain with injected noise, labels (if any) at scale 1: tests/learned_var_ref.py's on a learned variance,
    ``oracle.diffusion_ref.sample_loop`` on fixed-large."""
    with torch.no_grad():
        if learned(row):
            return LV.sample_chain(LV.tables(betas(T)), "eps", var_type(row), net64(row, y), x_T.double(), zs.double())
        return D.sample_loop(D.ddpm_tables(betas(T), "fixed-large"), net64(row, y), x_T.double(), zs.double())


def all_bpd64(row, T, x_0, zs, y=None):
    """``calc_all_bpd`` of a learned-variance row: dict(total, losses, prior, mses)."""
    assert learned(row)
    with torch.no_grad():
        return LV.all_bpd(LV.tables(betas(T)), "eps", var_type(row), x_0.double(), zs.double(), net64(row, y), True)


def guided_chain64(row, T, x_T, zs, y, scale, sub=None):
    """tests/cond_ref.py's guided chain on the row's conditional network: the ancestral chain on fixed-large (``sub`` None; a learned
    variance is refused there), or DDIM at eta = 0 over the sub-sequence ``sub`` on its own fixed-small tables — of a 2C-channel network
    the mean half alone, as ``DDIM`` reads it."""
    sd64, cfg, opts = weights(row["id"])[1], cfg_of(row), opts_of(row)
    net = lambda x, t, yy: forward64(sd64, cfg, opts, x, t, yy)[:, :3]                      # noqa: E731
    with torch.no_grad():
        if sub is None:
            assert not learned(row), GUIDED_LEARNED
            return CR.guided_chain(D.ddpm_tables(betas(T), "fixed-large"), "eps", net, x_T.double(), zs.double(), y, K, scale)
        tb = D.ddim_tables(betas(T), "fixed-small", 0.0, sub)
        return CR.guided_chain(tb, "eps", net, x_T.double(), torch.zeros(len(sub), *x_T.shape, dtype=torch.float64), y, K, scale, timestep_map=sub)


def encode_decode64(row, T, sub, x_0, y=None):
    """(latent, reconstruction) of ``DDIM.encode`` then ``decode`` (clip on) at eta = 0: tests/ddim_inverse_ref.py on the mean half."""
    tb = IR.tables(betas(T), sub)
    net = net64(row, y)
    mean = lambda x, t: net(x, t)[:, :3]                                                    # noqa: E731
    with torch.no_grad():
        lat = IR.encode(tb, mean, x_0.double())
        return lat, IR.decode(tb, mean, lat, clip=True)
