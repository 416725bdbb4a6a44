"""-m gpu: the UNet's options TOGETHER on the device — every row of tests/option_rows.py (class conditioning x head count x scale-shift
norm x variance / loss x dropout x resampling x compute mode x geometry, pairwise complete, the all-on Improved-DDPM / ADM denoiser in both
modes) through the engine against the composed float64 reference of that file.

What the rows reach that no single-option file does: the concatenated time projection whose width doubles under the scale-shift norm AND
whose rows depend on (t, y); the ``fold`` branch of ``_Engine._res_bwd`` on concat inputs and at geometries the patch-stationary weight
gradient declines (24 x 18, 12 x 9); ``ops.attention_path`` at 2B rows with modulated blocks on either side; the dropout seed derived from
offsets the scale-shift norm moves; the hybrid loss under autograd on a conditional network; conditional learned-variance chains.

Bars are the project's, unchanged: ``MODES`` of tests/test_adagn_gpu.py (forward 1e-3 / 1.5e-1 of the reference's largest value in the
fp32 / bf16 mode, every gradient 3 x that relative to its own largest entry with the floor at 2 % / 10 % of the median tensor scale);
trainers at tests/test_channels_accum_gpu.py's (losses rtol 5e-4, states 1e-3 with an Adam slack of 0.25 lr per update, lr 1e-3) in the fp32
mode and at the bars tests/test_adagn_gpu.py documents for the bf16 mode (lr 1e-4; plan against eager: first loss 1e-5, second 7.5e-3, third
1.2e-1, parameters within 2 lr x steps; against the oracle: losses within 1.5e-1); chains at FP32_BAR = 1e-3 of the float64 chain's largest
value, replayed equal to eager bit for bit.

Every test prints one or more lines that start with ``option-rows``; profiles/option_rows.log keeps those of one run on an MI355X."""
import functools
import os
import sys

import pytest
import torch

import ddpm_torch
from ddpm_torch import _ops as ops
from ddpm_torch.models import unet as unet_mod
from oracle import unet_ref as U
from tests import channels_accum as CA
from tests import cond_ref as CR
from tests import option_rows as OR
from tests.golden.recipes import check, check_state
from tests.test_adagn_gpu import MODES

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ddpm-torch_amd")
if PKG not in sys.path:
    sys.path.insert(0, PKG)
import ddim  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DT = {"fp32": MODES[0][0], "bf16": MODES[1][0]}
BAR = {"fp32": MODES[0][1], "bf16": MODES[1][1]}
FP32_BAR = 1e-3                                      # chains, as tests/test_cond_gpu.py and tests/test_learned_var_gpu.py hold them
IDS = [r["id"] for r in OR.ROWS]
K = OR.K


def model_of(row):
    m = OR.build(row)
    m.load_state_dict(OR.weights(row["id"])[0])
    return m.to(DEV).set_compute_dtype(DT[row["mode"]])


def call(m, x, t, y):
    return m(x.to(DEV), t.to(DEV)) if y is None else m(x.to(DEV), t.to(DEV), y.to(DEV))


@functools.lru_cache(maxsize=None)
def training_run(row_id):
    """One training-mode forward and backward of the row on ``OR.inputs``, and what the tests read off it: the output, every gradient,
    the engine's own dropout masks, the attention records of the tape (token count, heads, channels, pitch, path) and the ``fold`` outcome
    of every scale-shift block, recomputed with the engine's own ``_patch_copies``."""
    row = OR.ROW[row_id]
    x, t, y, gy = OR.inputs(row_id)
    m = model_of(row).train()
    eng = m.engine()
    eng.debug_keep_tape = True
    out = call(m, x, t, y)
    (out * gy.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    names = {id(mod): name for name, mod in m.named_modules()}
    attn, folds = [], []
    for rec in eng.last_tape:
        if rec[0] == "attn":
            ab, xv, qkv = rec[1], rec[2], rec[6]
            attn.append((xv.H * xv.W, ab.num_heads, ab.in_channels, qkv.ld, rec[-1]))
        elif rec[0] == "res" and rec[1].use_scale_shift_norm:
            rb, xv, a1, h1 = rec[1], rec[2], rec[4], rec[6]
            boost = xv.H * xv.W <= 4096 and any(rb is q for q in eng.res_blocks[:unet_mod._TAIL_BLOCKS])
            fold = bool(unet_mod._WGRAD3 and eng.T == torch.bfloat16 and rb.in_channels == a1.C
                        and eng._patch_copies(OR.B, xv.H, xv.W, a1.C, h1.C, bool(boost)) > 0)
            folds.append((names[id(rb)], (xv.H, xv.W), rb.in_channels, fold))
    return dict(out=out.detach().cpu().double(), grads={k: q.grad.cpu().double() for k, q in m.named_parameters()},
                masks=CA.masks_from_tape(m, row["drop"], DEV), attn=attn, folds=folds, dcode=eng.dcode)


@functools.lru_cache(maxsize=None)
def reference(row_id):
    return OR.forward_and_gradients64(row_id, masks=training_run(row_id)["masks"] or None)


# --------------------------------------------------------------------------------------------------------------- forward, gradients, paths
@pytest.mark.parametrize("row", OR.ROWS, ids=IDS)
def test_forward_and_every_gradient_against_the_composed_reference(row):
    bar, fp32 = BAR[row["mode"]], row["mode"] == "fp32"
    got, (out64, grads64) = training_run(row["id"]), reference(row["id"])
    rel = float((got["out"] - out64).abs().max() / out64.abs().max())
    scales = {k: float(v.abs().max()) for k, v in grads64.items()}
    floor = (0.02 if fp32 else 0.1) * sorted(scales.values())[len(scales) // 2]
    assert set(got["grads"]) == set(grads64)
    errs = {k: float((g - grads64[k]).abs().max()) / max(scales[k], floor) for k, g in got["grads"].items()}
    worst = sorted(((e, k) for k, e in errs.items()), reverse=True)
    print(f"\noption-rows {row['id']}: forward rel err {rel:.3e}; worst gradients " + ", ".join(f"{k} {e:.2e}" for e, k in worst[:3]))
    assert rel < bar, rel
    assert worst[0][0] < 3 * bar, worst[0]
    if row["cond"]:
        g, ref = got["grads"][CR.TABLE], grads64[CR.TABLE]
        y = OR.inputs(row["id"])[2].tolist()
        unused = [k for k in range(K + 1) if k not in y]
        assert unused == [1] and bool((g[1] == 0).all()), "a class without a sample: exactly zero"
        for what, k in (("null", K), ("used", y[0])):
            e = float((g[k] - ref[k]).abs().max()) / max(float(ref[k].abs().max()), floor)
            print(f"option-rows {row['id']}: class_embed.weight {what} row {k}: {e:.2e}")
            assert float(ref[k].abs().max()) > 0 and e < 3 * bar, (what, e)
    if row["ssn"]:
        pre = U.res_block_prefixes(OR.cfg_of(row))
        blocks = (pre[0], "middle.0.", [p for p in pre if p.startswith("upsamples")][1])          # the decoder block reads a concat input
        for blk in blocks:
            for k in ("fc.weight", "fc.bias", "conv1.bias", "norm2.weight", "norm2.bias"):
                assert errs[blk + k] < 3 * bar and scales[blk + k] > 0, (blk + k, errs[blk + k])
            print(f"option-rows {row['id']}: {blk} " + ", ".join(f"{k} {errs[blk + k]:.2e}" for k in ("fc.weight", "fc.bias", "conv1.bias", "norm2.weight", "norm2.bias")))
            cout = OR.weights(row["id"])[0][blk + "conv1.weight"].shape[0]
            assert got["grads"][blk + "fc.weight"].shape[0] == 2 * cout


@pytest.mark.parametrize("row", OR.ROWS, ids=IDS)
def test_attention_paths_are_the_ones_the_table_names(row):
    got = training_run(row["id"])
    seen = []
    for Lk, H, C, ld, path in got["attn"]:
        at_inference = ops.attention_path(H, C, C // H, got["dcode"], OR.B, Lk, ld, False)
        seen.append((Lk, H, path, at_inference))
        assert (path, at_inference) == row["paths"][Lk], (Lk, H, C, path, at_inference)
    assert {s[0] for s in seen} == set(row["paths"])
    print(f"\noption-rows {row['id']}: attention (tokens, heads, training, inference) " + " ".join(str(s) for s in sorted(set(seen), reverse=True)))
    if got["folds"]:
        print(f"option-rows {row['id']}: fold " + " ".join(f"{n}@{h}x{w}/{cin}:{int(f)}" for n, (h, w), cin, f in got["folds"]))
        if row["mode"] == "fp32":
            assert not any(f[3] for f in got["folds"])


def heads_at(row, C):
    h = OR.HEADS[row["heads"]]
    return C // h["num_head_channels"] if "num_head_channels" in h else h.get("num_heads", 1)


def test_the_rows_reach_every_attention_path():
    """Of the table's ``paths`` (which the test above holds to the tape): in training the on-chip pair, the streaming pair with one head
    and with a head index, and the materialised path; at inference the fused kernel."""
    train, infer = set(), set()
    for row in OR.ROWS:
        cfg = OR.cfg_of(row)
        Himg, Wimg = row["size"]
        L = len(cfg["ch_multipliers"])
        levels = [i for i in range(L) if cfg["apply_attn"][i]] + [L - 1]
        for i in levels:
            Lk, C = (Himg >> i) * (Wimg >> i), cfg["hid_channels"] * cfg["ch_multipliers"][i]
            tr, inf = row["paths"][Lk]
            train.add((tr, heads_at(row, C) > 1))
            infer.add(inf)
    assert {("flash", False), ("stream", False), ("stream", True), ("mat", False)} <= train, train
    assert "fused" in infer, infer


def test_both_outcomes_of_fold_occur_among_the_bf16_scale_shift_rows():
    outcomes = {}
    for row in OR.ROWS:
        if row["mode"] == "bf16" and row["ssn"]:
            for name, size, cin, fold in training_run(row["id"])["folds"]:
                outcomes.setdefault(fold, (row["id"], name, size))
    print(f"\noption-rows fold outcomes among the bf16 scale-shift rows: {outcomes}")
    assert set(outcomes) == {True, False}, outcomes


@pytest.mark.parametrize("row", [r for r in OR.ROWS if r["drop"] == 0], ids=[r["id"] for r in OR.ROWS if r["drop"] == 0])
def test_inference_equals_the_training_forward_without_dropout(row):
    x, t, y, _ = OR.inputs(row["id"])
    m = model_of(row).eval()
    with torch.no_grad():
        ev = call(m, x, t, y).cpu().double()
    same = all(a == b for a, b in row["paths"].values())
    out64 = reference(row["id"])[0]
    rel = float((ev - out64).abs().max() / out64.abs().max())
    print(f"\noption-rows {row['id']}: inference vs float64 {rel:.3e}; same attention paths as training: {same}")
    if same:
        assert torch.equal(ev, training_run(row["id"])["out"])
    else:
        assert rel < BAR[row["mode"]], rel


# --------------------------------------------------------------------------------------------------------------- Trainer
TRAINER_ROWS = ["all-on-fp32", "all-on-bf16", "cond-2heads-fixed-fp32", "2heads-ssn-range-bf16"]
TB = 4


def trainer_of(row, m, lr, **kw):
    dif = ddpm_torch.GaussianDiffusion(ddpm_torch.get_beta_schedule("linear", 1e-4, 0.02, 1000), "eps", *row["var_loss"])
    opt = torch.optim.Adam(m.parameters(), lr=lr, betas=(0.9, 0.999))
    return ddpm_torch.Trainer(m, opt, dif, epochs=1, trainloader=None, scheduler=None, use_ema=True, grad_norm=1.0, shape=(3,) + row["size"],
                              device=torch.device(DEV), ema_decay=0.9999, **kw)


def hold_to_oracle(row, lr, losses, ref, params, shadow, oracle, what):
    if row["mode"] == "fp32":
        assert torch.allclose(torch.tensor(losses, dtype=torch.float64), torch.tensor(ref, dtype=torch.float64), rtol=5e-4), (what, losses, ref)
        slack = 0.25 * lr * 3
        check_state(params, oracle.state(), 1e-3, f"{what} param", adam_slack=slack)
        check_state(shadow, oracle.shadow, 1e-3, f"{what} shadow", adam_slack=slack)
    else:
        assert all(abs(a - b) <= 1.5e-1 * abs(b) for a, b in zip(losses, ref)), (what, losses, ref)


@pytest.mark.parametrize("row_id", TRAINER_ROWS)
def test_three_trainer_steps_follow_the_composed_oracle_trainer(row_id, monkeypatch):
    from ddpm_torch.utils import train as train_mod
    row = OR.ROW[row_id]
    H, W = row["size"]
    lr = 1e-3 if row["mode"] == "fp32" else 1e-4
    g = torch.Generator().manual_seed(21)
    xs = [torch.rand(TB, 3, H, W, generator=g) * 2 - 1 for _ in range(3)]
    ys = [torch.randint(0, K, (TB,), generator=g) for _ in range(3)]
    sd0 = OR.weights(row_id)[0]
    if row["cond"]:
        # the generic autograd step (no launch plan); labels after the drop reproduced from the trainer's generator: t, noise, then B uniforms
        m = model_of(row)
        tr = trainer_of(row, m, lr, label_drop=0.5)
        m.train()
        m.engine().debug_keep_tape = True
        twin = torch.Generator(DEV).manual_seed(CA.GEN_SEED)
        oracle = OR.oracle_trainer(row, lr)
        losses, ref, dropped = [], [], 0
        for i, (x, y) in enumerate(zip(xs, ys)):
            t = torch.empty((TB,), dtype=torch.int64, device=DEV).random_(to=1000, generator=twin)
            noise = torch.empty(TB, 3, H, W, device=DEV).normal_(generator=twin)
            y_used = CR.dropped_labels(y, torch.rand((TB,), device=DEV, generator=twin).cpu(), 0.5, K)
            dropped += int((y_used != y).sum())
            tr.stats.reset()
            tr.step((x, y), global_steps=i + 1)
            losses.append(tr.current_stats["loss"])
            masks = CA.masks_from_tape(m, row["drop"], DEV)
            assert bool(masks) == (row["drop"] > 0)
            ref.append(oracle.step(x, y_used, masks=masks or None, inputs=(t.cpu(), noise.cpu()))[0])
        assert not tr._direct and tr._direct_unet() is None, "the conditional step must not take the launch plan"
        assert 0 < dropped < 3 * TB
        print(f"\noption-rows {row_id}: trainer losses {losses} vs oracle {ref}; {dropped} of {3 * TB} labels dropped")
        params, shadow = {k: v.cpu() for k, v in m.state_dict().items()}, {k: v.cpu() for k, v in tr.ema.shadow.items()}
        assert any(not torch.equal(params[k], sd0[k]) for k in params), "the steps moved nothing"
        hold_to_oracle(row, lr, losses, ref, params, shadow, oracle, row_id)
        return
    assert row["drop"] == 0
    runs = {}
    for form in ("plan", False):
        monkeypatch.setattr(train_mod, "_TRAIN_GRAPH", form)
        m = model_of(row)
        tr = trainer_of(row, m, lr)
        m.train()
        losses = []
        for i, x in enumerate(xs):
            tr.stats.reset()
            tr.step(x, global_steps=i + 1)
            losses.append(tr.current_stats["loss"])
        if form == "plan":
            ds = next(iter(tr._direct.values()))
            assert ds.plan is not None and ds.last_kind == "plan", "the third step was not replayed from the launch plan"
        runs[form] = (losses, {k: v.cpu() for k, v in m.state_dict().items()}, {k: v.cpu() for k, v in tr.ema.shadow.items()})
    (la, pa, sa), (lb, pb, sb) = runs["plan"], runs[False]
    gen = torch.Generator(DEV).manual_seed(CA.GEN_SEED)
    oracle, ref = OR.oracle_trainer(row, lr), []
    for x in xs:
        t = torch.empty((TB,), dtype=torch.int64, device=DEV).random_(to=1000, generator=gen)
        noise = torch.empty(TB, 3, H, W, device=DEV).normal_(generator=gen)
        ref.append(oracle.step(x, inputs=(t.cpu(), noise.cpu()))[0])
    print(f"\noption-rows {row_id}: trainer losses plan {la} eager {lb} oracle {ref}")
    assert any(not torch.equal(pa[k], sd0[k]) for k in pa), "the steps moved nothing"
    if row["mode"] == "fp32":
        slack = 0.25 * lr * 3
        assert torch.allclose(torch.tensor(la, dtype=torch.float64), torch.tensor(lb, dtype=torch.float64), rtol=5e-4), (la, lb)
        check_state(pa, pb, 1e-3, "plan vs eager param", adam_slack=slack)
        check_state(sa, sb, 1e-3, "plan vs eager shadow", adam_slack=slack)
    else:
        worst = max(float((pa[k] - v).abs().max()) for k, v in pb.items()) / (lr * 3)
        print(f"option-rows {row_id}: plan and eager parameters differ by at most {worst:.2f} x lr x steps")
        assert abs(la[0] - lb[0]) <= 1e-5 * abs(lb[0]), (la, lb)
        assert abs(la[1] - lb[1]) <= 7.5e-3 * abs(lb[1]) and abs(la[2] - lb[2]) <= 1.2e-1 * abs(lb[2]), (la, lb)
        assert worst <= 2.0, worst
    for what, (losses, params, shadow) in (("plan", runs["plan"]), ("eager", runs[False])):
        hold_to_oracle(row, lr, losses, ref, params, shadow, oracle, f"{row_id} {what}")


# --------------------------------------------------------------------------------------------------------------- chains
T = 8
CHAIN_Y = (2, 0, 1)
SUB = 4


@functools.lru_cache(maxsize=None)
def chain_inputs(row_id):
    shape = (OR.B, 3) + OR.ROW[row_id]["size"]
    g = torch.Generator().manual_seed(41)
    x_T, zs = torch.randn(shape, generator=g), torch.randn((T,) + shape, generator=g)
    return shape, x_T, zs, (x_T * 0.5).clamp(-1, 1), torch.tensor(CHAIN_Y)


def both_forms(monkeypatch, fn):
    """``fn()`` with the captured step replayed and eagerly: the results, equal bit for bit."""
    outs = []
    for mode in ("1", "0"):
        monkeypatch.setenv("DDPM_TORCH_AMD_GRAPH", mode)
        got = fn()
        outs.append(got if isinstance(got, (tuple, list)) else (got,))
    assert all(torch.equal(a, b) for a, b in zip(*outs)), "replayed and eager differ"
    return outs[0]


def process(row):
    return ddpm_torch.GaussianDiffusion(ddpm_torch.get_beta_schedule("linear", 1e-4, 0.02, T), "eps", *row["var_loss"])


def captured_kinds(dif):
    return {k[3][3] for k in getattr(dif, "_sample_graphs", {}) if len(k[3]) > 3}


@pytest.mark.parametrize("kind", ["p_sample", "calc_all_bpd", "guided-ddim4", "encode-decode"])
def test_all_on_chains_replayed_equal_eager_and_follow_float64(kind, monkeypatch):
    row = OR.ROW["all-on-fp32"]
    shape, x_T, zs, x_0, y = chain_inputs(row["id"])
    m, dif, yd = model_of(row).eval(), process(row), y.to(DEV)
    sub = ddim.get_selection_schedule("linear", size=SUB, timesteps=T)
    if kind == "p_sample":
        def run():
            with torch.inference_mode():
                a = dif._sample_loop(m, shape, DEV, x_T, None, z_stream=iter(zs), y=yd, guidance_scale=1.0)
            return a, dif.p_sample(m, shape=shape, device=DEV, seed=77, y=yd)
        got = both_forms(monkeypatch, run)
        assert ("cond",) in captured_kinds(dif)
        errs = {"chain": check(got[0], OR.sample_chain64(row, T, x_T, zs, y), FP32_BAR, name="conditional learned-range chain")}
        assert bool(torch.isfinite(got[1]).all())
    elif kind == "calc_all_bpd":
        got = both_forms(monkeypatch, lambda: dif.calc_all_bpd(m, x_0.to(DEV), noise_stream=iter([z.to(DEV) for z in zs]), y=yd))
        ref = OR.all_bpd64(row, T, x_0, zs, y)
        errs = {k: float((v.cpu() - ref[k]).abs().max() / ref[k].abs().max()) for v, k in zip(got, ("total", "losses", "prior", "mses"))}
        assert max(errs.values()) <= FP32_BAR, errs
    else:
        dd = ddim.DDIM.from_ddpm(dif, eta=0.0, subsequence=sub)
        if kind == "guided-ddim4":
            def run():
                with torch.inference_mode():
                    return dd._sample_loop(m, shape, DEV, x_T, None, z_stream=iter([torch.zeros(shape)] * SUB), y=yd, guidance_scale=2.0)
            got = both_forms(monkeypatch, run)
            assert ("cfg", 2.0, K) in captured_kinds(dd)
            ref = OR.guided_chain64(row, T, x_T, None, y, 2.0, sub=OR.D.selection_schedule("linear", SUB, T))
            errs = {"guided DDIM-4": check(got[0], ref, FP32_BAR, name="guided DDIM-4 on the mean half")}
        else:
            def run():
                lat = dd.encode(m, x_0.to(DEV), y=yd)
                return lat, dd.decode(m, lat, y=yd)
            got = both_forms(monkeypatch, run)
            lat64, rec64 = OR.encode_decode64(row, T, OR.D.selection_schedule("linear", SUB, T), x_0, y)
            errs = {"latent": check(got[0], lat64, FP32_BAR, name="encode"), "reconstruction": check(got[1], rec64, FP32_BAR, name="decode")}
            assert not torch.equal(got[0], dd.encode(m, x_0.to(DEV)).to(got[0].device)), "the labels changed nothing"
    print(f"\noption-rows {row['id']}: {kind} " + ", ".join(f"{k} {e:.3e}" for k, e in errs.items()))


def test_guided_ancestral_chain_on_the_conditional_fixed_variance_row(monkeypatch):
    """Scale 2: a 2B-row network call per step through two attention heads; the captured steps sit under their own keys."""
    row = OR.ROW["cond-2heads-fixed-fp32"]
    shape, x_T, zs, _, y = chain_inputs(row["id"])
    m, dif, yd = model_of(row).eval(), process(row), y.to(DEV)

    def run():
        with torch.inference_mode():
            return (dif._sample_loop(m, shape, DEV, x_T, None, z_stream=iter(zs), y=yd, guidance_scale=2.0),
                    dif._sample_loop(m, shape, DEV, x_T, None, z_stream=iter(zs), y=yd, guidance_scale=1.0))
    got = both_forms(monkeypatch, run)
    kinds = captured_kinds(dif)
    assert ("cfg", 2.0, K) in kinds and ("cond",) in kinds, kinds
    e2 = check(got[0], OR.guided_chain64(row, T, x_T, zs, y, 2.0), FP32_BAR, name="guided chain")
    e1 = check(got[1], OR.sample_chain64(row, T, x_T, zs, y), FP32_BAR, name="conditional chain")
    assert not torch.equal(got[0], got[1])
    print(f"\noption-rows {row['id']}: guided chain {e2:.3e}, conditional chain {e1:.3e}")


def test_a_bf16_chain_replayed_equals_eager(monkeypatch):
    row = OR.ROW["cond-hc32-ssn-range-bf16"]
    shape, x_T, zs, x_0, y = chain_inputs(row["id"])
    m, dif, yd = model_of(row).eval(), process(row), y.to(DEV)

    def run():
        with torch.inference_mode():
            a = dif._sample_loop(m, shape, DEV, x_T, None, z_stream=iter(zs), y=yd, guidance_scale=1.0)
        return a, dif.p_sample(m, shape=shape, device=DEV, seed=77, y=yd), dif.calc_all_bpd(m, x_0.to(DEV), seed=3, y=yd)[0]
    got = both_forms(monkeypatch, run)
    assert all(bool(torch.isfinite(v).all()) for v in got)
    rel = float((got[0].cpu().double() - OR.sample_chain64(row, T, x_T, zs, y)).abs().max())
    print(f"\noption-rows {row['id']}: replayed = eager; injected-noise chain max abs err {rel:.3e} (reported, not held: bf16)")
