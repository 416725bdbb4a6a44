"""CPU: the table of tests/option_rows.py and its composed float64 reference, before tests/test_option_rows_gpu.py relies on either.

* coverage: ``ROWS`` covers every pair of levels of every two factors of ``FACTORS``, holds the all-on row in both compute modes, has at
  most 14 rows, and loses one of these properties when any single row is deleted;
* reduction: with one option on, the composed reference is that option's own reference (tests/cond_ref.py, tests/mha_ref.py,
  tests/adagn_ref.py; the composed oracle trainer against tests/cond_ref.py's and tests/learned_var_ref.py's) — ``torch.equal`` on the
  forward and on every gradient, B = 2 at 8 x 8;
* no dead inputs: on the inputs the GPU test uses, every parameter of every row has a non-zero float64 gradient, two samples carry
  different labels, the null label occurs, a class has no sample, one sample sits at t = 0;
* the refusals ``EXCLUDED`` rests on are pinned, and a guided DDIM built from a learned-variance process runs the guided step on the mean
  half (C ABI emulated: tests/abi_emulator.py + tests/cond_emulator.py)."""
import itertools
import os
import sys

import pytest
import torch

import ddpm_torch
from ddpm_torch import _hip
from oracle import diffusion_ref as D
from oracle import unet_ref as U
from tests import abi_emulator, batch_emulator, cond_emulator, ddim_emulator, learned_var_emulator
from tests import adagn_ref as AR
from tests import cond_ref as CR
from tests import learned_var_ref as LV
from tests import mha_ref as MR
from tests import option_rows as OR
from tests.golden.recipes import check, rnd

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ddpm-torch_amd")
if PKG not in sys.path:
    sys.path.insert(0, PKG)
import ddim  # noqa: E402

CPU = torch.device("cpu")


# --------------------------------------------------------------------------------------------------------------- coverage
def required_pairs():
    return {((a, x), (b, y)) for a, b in itertools.combinations(OR.FACTORS, 2) for x in OR.FACTORS[a] for y in OR.FACTORS[b]}


def covered_pairs(rows):
    """Pairs of LEVELS the rows hold (a value that is no level of its factor — the fused row's geometry — covers nothing)."""
    return {((a, r[a]), (b, r[b])) for r in rows for a, b in itertools.combinations(OR.FACTORS, 2)
            if r[a] in OR.FACTORS[a] and r[b] in OR.FACTORS[b]}


def problems(rows):
    """What a table lacks of the three conditions (empty: nothing)."""
    out = [f"pair not covered: {p}" for p in sorted(required_pairs() - covered_pairs(rows), key=str)]
    for mode in OR.FACTORS["mode"]:
        if not any(r["mode"] == mode and all(r[k] == v for k, v in OR.ALL_ON.items()) for r in rows):
            out.append(f"no all-on row in the {mode} mode")
    if len(rows) > 14:
        out.append(f"{len(rows)} rows")
    return out


def test_the_table_covers_every_pair_holds_the_all_on_row_twice_and_has_at_most_14_rows():
    assert len(required_pairs()) == 157 and not problems(OR.ROWS), problems(OR.ROWS)
    assert len({r["id"] for r in OR.ROWS}) == len(OR.ROWS)
    # the only value outside its factor's levels is the geometry of the one row built to reach the inference-only attention kernel
    odd = [(r["id"], k) for r in OR.ROWS for k in OR.FACTORS if r[k] not in OR.FACTORS[k]]
    assert odd == [("fused-1head-ssn-kl-bf16", "size")] and OR.ROW["fused-1head-ssn-kl-bf16"]["size"] == OR.FUSED_SIZE
    for r in OR.ROWS:
        assert set(r["paths"]) == set(token_counts(r)), (r["id"], token_counts(r))


def test_no_row_can_be_deleted():
    for i, r in enumerate(OR.ROWS):
        assert problems(OR.ROWS[:i] + OR.ROWS[i + 1:]), f"the table loses nothing without {r['id']}"


def test_the_excluded_cells_are_the_refused_ones_and_nothing_else():
    """variance x loss as two factors: the table takes three cells, the package refuses three, and the refusals are those of EXCLUDED."""
    variances, losses = [v for v, _ in OR.FACTORS["var_loss"]], [l for _, l in OR.FACTORS["var_loss"]]
    b = ddpm_torch.get_beta_schedule("linear", 1e-4, 0.02, 8)
    refused = set()
    for v, l in itertools.product(variances, losses):
        try:
            ddpm_torch.GaussianDiffusion(b, "eps", v, l)
        except ValueError:
            refused.add((("variance", v), ("loss", l)))
    assert refused == set(OR.EXCLUDED)
    assert not refused & {(("variance", v), ("loss", l)) for v, l in OR.FACTORS["var_loss"]}


def test_refusals():
    b = ddpm_torch.get_beta_schedule("linear", 1e-4, 0.02, 8)
    for v in ("learned", "learned-range"):
        with pytest.raises(ValueError, match="mse"):
            ddpm_torch.GaussianDiffusion(b, "eps", v, "mse")
    with pytest.raises(ValueError, match="hybrid"):
        ddpm_torch.GaussianDiffusion(b, "eps", "fixed-large", "hybrid")
    two = lambda x, t, yy: torch.cat([0.5 * x, 0.3 * x - 0.2], dim=1)                        # noqa: E731
    two.num_classes = OR.K
    y = torch.tensor([1, 0])
    for v, l in (("learned", "kl"), ("learned-range", "hybrid")):
        with pytest.raises(NotImplementedError, match="learned-variance"):
            ddpm_torch.GaussianDiffusion(b, "eps", v, l).p_sample(two, (2, 2, 4, 4), device=CPU, y=y, guidance_scale=2.0)


def token_counts(row):
    cfg = OR.cfg_of(row)
    H, W = row["size"]
    L = len(cfg["ch_multipliers"])
    return sorted({(H >> i) * (W >> i) for i in range(L) if cfg["apply_attn"][i]} | {(H >> (L - 1)) * (W >> (L - 1))})


def test_geometries_fit_the_engine():
    """What ``_need_vec_tokens`` / ``_attn_mat`` ask of the fp32 mode (token counts and head widths in multiples of 4) holds on every fp32
    row; among the bf16 rows one reaches a token count above 256 and one a count that is no multiple of 8."""
    bf16 = set()
    for r in OR.ROWS:
        cfg, counts = OR.cfg_of(r), token_counts(r)
        H, W = r["size"]
        assert H % (1 << (len(cfg["ch_multipliers"]) - 1)) == 0 and W % (1 << (len(cfg["ch_multipliers"]) - 1)) == 0
        if r["mode"] == "fp32":
            assert all(n % 4 == 0 for n in counts), (r["id"], counts)
            m = OR.build(r)
            assert all((ab.in_channels // ab.num_heads) % 4 == 0 for ab in m.modules() if hasattr(ab, "project_in"))
        else:
            bf16 |= set(counts)
    assert any(n > 256 for n in bf16) and any(n % 8 for n in bf16), sorted(bf16)
    assert max(r["size"][0] * r["size"][1] for r in OR.ROWS) <= 24 * 20


# --------------------------------------------------------------------------------------------------------------- reduction
RED = dict(in_channels=3, out_channels=3, num_res_blocks=1, drop_rate=0.0, **OR.NETS["two"])
SINGLE = {
    "cond": (dict(num_classes=OR.K), lambda p, x, t, y: CR.unet_forward(p, RED, x, t, y, training=True)),
    "num_heads": (dict(num_heads=2), lambda p, x, t, y: MR.unet_forward(p, RED, x, t, num_heads=2, training=True)),
    "num_head_channels": (dict(num_head_channels=32), lambda p, x, t, y: MR.unet_forward(p, RED, x, t, num_head_channels=32, training=True)),
    "ssn": (dict(use_scale_shift_norm=True), lambda p, x, t, y: AR.unet_forward(p, RED, x, t, training=True)),
    "none": (dict(), lambda p, x, t, y: U.unet_forward(p, RED, x, t, training=True)),
}


@pytest.mark.parametrize("name", list(SINGLE))
def test_one_option_alone_is_its_own_reference(name):
    opts, own = SINGLE[name]
    torch.manual_seed(5)
    sd = {k: v.double() for k, v in U.randomize_state_dict(ddpm_torch.UNet(**RED, **opts).state_dict(), 17).items()}
    x, t, gy = OR.r(2, 3, 8, 8, seed=1).double(), torch.tensor([0, 977]), OR.r(2, 3, 8, 8, seed=2).double()
    y = torch.tensor([2, OR.K]) if name == "cond" else None
    res = []
    for fn in (lambda p: OR.forward64(p, RED, opts, x, t, y, training=True), lambda p: own(p, x, t, y)):
        p = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
        out = fn(p)
        (out * gy).sum().backward()
        res.append((out.detach(), {k: v.grad for k, v in p.items()}))
    (a, ga), (b, gb) = res
    assert torch.equal(a, b)
    assert all(g is not None and torch.equal(g, gb[k]) for k, g in ga.items())
    assert U.attention_core.__module__ == "oracle.unet_ref" and U.residual_block.__module__ == "oracle.unet_ref", "a binding was left behind"


@pytest.mark.parametrize("name", ["cond", "learned-range"])
def test_the_composed_oracle_trainer_alone_is_the_option_files_trainer(name):
    row = dict(id="reduction-" + name, cond=OR.K if name == "cond" else None, heads="1", ssn=False,
               var_loss=("fixed-large", "mse") if name == "cond" else ("learned-range", "hybrid"), drop=0.0, rwc=True, mode="fp32", size=(8, 8))
    OR.ROW[row["id"]] = row
    try:
        sd, cfg = OR.weights(row["id"])[0], OR.cfg_of(row)
        x = torch.rand(2, 3, 8, 8, generator=torch.Generator().manual_seed(3)) * 2 - 1
        mine = OR.oracle_trainer(row, 1e-3)
        if name == "cond":
            theirs, y = CR.oracle_trainer(sd, cfg, 1e-3, OR.K), torch.tensor([1, OR.K])
            la, lb = mine.step(x, y), theirs.step(x, y)
        else:
            theirs = LV.oracle_trainer(sd, cfg, 1e-3, "eps", "learned-range", 1.0)
            la, lb = mine.step(x), theirs.step(x)
        assert la == lb and la[1]
        assert all(torch.equal(v, theirs.state()[k]) for k, v in mine.state().items())
        assert all(torch.equal(v, theirs.shadow[k]) for k, v in mine.shadow.items())
    finally:
        del OR.ROW[row["id"]]


# --------------------------------------------------------------------------------------------------------------- no dead inputs
@pytest.mark.parametrize("row", OR.ROWS, ids=[r["id"] for r in OR.ROWS])
def test_every_parameter_has_a_gradient_on_the_inputs_of_the_gpu_test(row):
    x, t, y, gy = OR.inputs(row["id"])
    assert x.shape == (OR.B, 3) + row["size"] and int((t == 0).sum()) == 1
    out, grads = OR.forward_and_gradients64(row["id"], masks=OR.host_masks(row["id"]))
    assert out.shape == gy.shape and bool(torch.isfinite(out).all())
    dead = [k for k, g in grads.items() if g is None or float(g.abs().max()) == 0.0]
    assert not dead and len(grads) == len(OR.weights(row["id"])[0]), dead
    if row["cond"]:
        labels = y.tolist()
        assert OR.K in labels and len(set(labels) - {OR.K}) >= 2 and 1 not in labels
        g = grads[CR.TABLE]
        assert bool((g[1] == 0).all()) and all(float(g[k].abs().max()) > 0 for k in (0, 2, OR.K))
    else:
        assert y is None and CR.TABLE not in grads
    if row["drop"] > 0:                                                    # the masks did something
        assert not torch.equal(out, OR.forward_and_gradients64(row["id"], masks=None, training=False)[0])


# --------------------------------------------------------------------------------------------------------------- guided DDIM on 2C channels
@pytest.mark.skipif(not os.path.exists(_hip.LIB_PATH), reason="libddpm_hip.so not built")
def test_guided_ddim_of_a_learned_variance_process_combines_the_mean_halves(monkeypatch):
    """``DDIM.from_ddpm`` of a learned-range process samples on its own fixed tables (var_mode 0), so classifier-free guidance is served
    there: the guided step runs on the mean half of the 2B-row output — the bits of a fixed-small DDIM on the mean-half network, and the
    float64 guided chain."""
    emu = cond_emulator.attach(batch_emulator.attach(learned_var_emulator.attach(ddim_emulator.attach(abi_emulator.install(monkeypatch, _hip)))))
    T, S, shape, scale = 40, 4, (2, 2, 4, 4), 2.0
    b = ddpm_torch.get_beta_schedule("linear", 1e-4, 0.02, T)
    sub = ddim.get_selection_schedule("linear", size=S, timesteps=T)
    w, c = rnd(T, *shape[1:], seed=4) * 0.3, torch.tensor([0.5, -1.0, 0.25, 0.0])

    def net(x, t, y, dtype=torch.float32):
        return 0.7 * x + w.to(dtype)[t.long()].to(x) + c.to(dtype)[y.long()].reshape(-1, 1, 1, 1).to(x)
    net.num_classes = OR.K
    two = lambda x, t, y: torch.cat([net(x, t, y), 0.3 * x - 0.2], dim=1)                    # noqa: E731
    two.num_classes = OR.K
    x_T, y = rnd(*shape, seed=7), torch.tensor([1, 0])
    dd = ddim.DDIM.from_ddpm(ddpm_torch.GaussianDiffusion(b, "eps", "learned-range", "hybrid"), eta=0.0, subsequence=sub)
    plain = ddim.DDIM(b, "eps", "fixed-small", "mse", eta=0.0, subsequence=sub)
    got = dd.p_sample(two, shape, device=CPU, noise=x_T, y=y, guidance_scale=scale)
    assert emu.log.count("ddpm_p_sample_step_cfg") == S
    assert torch.equal(got, plain.p_sample(net, shape, device=CPU, noise=x_T, y=y, guidance_scale=scale))
    tb = D.ddim_tables(b, "fixed-small", 0.0, sub)
    want = CR.guided_chain(tb, "eps", lambda x, t, yy: net(x, t, yy, torch.float64), x_T.double(), torch.zeros(S, *shape, dtype=torch.float64),
                           y, OR.K, scale, timestep_map=sub)
    check(got, want, 2e-4, name="guided DDIM-4 on 2C channels")
    with pytest.raises(ValueError, match="twice the channels"):
        dd.p_sample(net, shape, device=CPU, noise=x_T, y=y, guidance_scale=scale)
