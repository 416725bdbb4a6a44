"""CPU, C ABI emulated (tests/abi_emulator.py + tests/learned_var_emulator.py): the host side of the learned reverse-process variance —
``GaussianDiffusion(model_var_type="learned" | "learned-range")`` with ``loss_type`` "hybrid" / "kl": the constructor's rules, ``train_losses``
through the autograd node, three hybrid ``Trainer.step``s through the autograd-free step, ``calc_all_bpd`` and sampling chains at T = 8, DDIM
on a 2C-channel model, the ``train.py`` / ``generate.py`` round trip — and the argument validation of the four new entry points in the real
library.  The float64 reference is tests/learned_var_ref.py; the kernels themselves are held to it in tests/test_learned_var_gpu.py.

Bars: the emulator evaluates the reference's own expressions in fp32, so these tests check the wiring (which tensors, tables, weights and
flags reach which entry point), at the bars the other emulated-ABI tests use for fp32 against float64 (values and gradients 2e-4 of the
largest reference magnitude; trainer losses rtol 5e-4 and states 1e-3 with the Adam slack of tests/test_channels_accum_host.py).  Where the
T = 8 chains reach the decoder's 1e-12 floor (a model mean many sigma_0 off: cdf_upper - cdf_lower is rounding noise in fp32, see
tests/test_bpd_gpu.py) an entry is allowed 8 x the error of the reference's own fp32 evaluation instead, the margin of that file."""
import glob
import json
import os
import sys

import pytest
import torch

import ddpm_torch
import ddpm_torch.toy
from ddpm_torch import _hip
from oracle import diffusion_ref as D
from oracle import unet_ref as U
from tests import abi_emulator, ddim_emulator, learned_var_emulator
from tests import channels_accum as CA
from tests import learned_var_ref as R
from tests.golden.recipes import check, check_state, rnd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "ddpm-torch_amd")
if PKG not in sys.path:
    sys.path.insert(0, PKG)
import ddim  # noqa: E402

pytestmark = pytest.mark.skipif(not os.path.exists(_hip.LIB_PATH), reason="libddpm_hip.so not built")
CPU = torch.device("cpu")
LEARNED = ("learned", "learned-range")
NEW = ("ddpm_p_sample_step_lv", "ddpm_vlb_terms_lv", "ddpm_bpd_terms_lv", "ddpm_learned_loss")


@pytest.fixture
def emu(monkeypatch):
    return learned_var_emulator.attach(ddim_emulator.attach(abi_emulator.install(monkeypatch, _hip)))


def betas_of(T):
    return ddpm_torch.get_beta_schedule("linear", 1e-4, 0.02, T)


def net_of(w, dtype=torch.float32):
    """A closed-form 2C-channel network: mean output 0.7 x + w[t], v = 0.3 x - 0.2 (inside and outside [-1, 1])."""
    w = w.to(dtype)
    return lambda x, t: torch.cat([0.7 * x + w[int(t[0])], 0.3 * x - 0.2], dim=1)


def hold(got, ref64, ref32, name, rel=2e-4):
    """Per entry: the larger of ``rel`` x max |ref| and 8 x the error of the reference's own fp32 evaluation."""
    bar = torch.maximum(torch.full_like(ref64, rel * float(ref64.abs().max())), 8 * (ref32.double() - ref64).abs())
    err = (got.double() - ref64).abs()
    assert bool((err <= bar).all()), (name, float((err / bar).max()))


# ------------------------------------------------------------------------------------------------------------------ constructor
def test_constructor_accepts_and_rejects_the_right_combinations():
    b = betas_of(8)
    for vt in LEARNED:
        for lt in ("hybrid", "kl"):
            dif = ddpm_torch.GaussianDiffusion(b, "eps", vt, lt)
            assert dif.learned_var and dif.vlb_weight == 8 / 1000 and not hasattr(dif, "fixed_model_var") and not hasattr(dif, "fixed_model_logvar")
            assert dif.supports_direct_step() == (lt == "hybrid")
        with pytest.raises(ValueError, match="mse"):
            ddpm_torch.GaussianDiffusion(b, "eps", vt, "mse")
        with pytest.raises(NotImplementedError):
            ddpm_torch.toy.GaussianDiffusion(b, "eps", vt, "mse")
    for vt in ("fixed-small", "fixed-large"):
        with pytest.raises(ValueError, match="hybrid"):
            ddpm_torch.GaussianDiffusion(b, "eps", vt, "hybrid")
        dif = ddpm_torch.GaussianDiffusion(b, "eps", vt, "mse")
        assert not dif.learned_var and dif.supports_direct_step()
        assert not ddpm_torch.GaussianDiffusion(b, "eps", vt, "kl").supports_direct_step()
    with pytest.raises(KeyError):
        ddpm_torch.GaussianDiffusion(b, "eps", "no-such-type", "mse")
    dif = ddpm_torch.GaussianDiffusion(b, "x_0", "learned-range", "hybrid", vlb_weight=0.25)
    assert dif.vlb_weight == 0.25
    # lv_max is the "fixed-large" table, lv_min the clipped posterior log-variance: both stay attributes
    tabs = D.ddpm_tables(b, "fixed-large")
    assert torch.equal(dif.model_logvar_max, tabs["fixed_model_logvar"]) and torch.equal(dif.posterior_logvar_clipped, tabs["posterior_logvar_clipped"])
    assert torch.equal(ddpm_torch.GaussianDiffusion(b, "eps", "fixed-large", "mse").fixed_model_logvar, tabs["fixed_model_logvar"])


# ------------------------------------------------------------------------------------------------------------------ train_losses
@pytest.mark.parametrize("loss_type", ["hybrid", "kl"])
@pytest.mark.parametrize("var_type", LEARNED)
@pytest.mark.parametrize("mean_type", R.MEAN_TYPES)
def test_train_losses_values_and_gradients_match_float64_autograd(emu, mean_type, var_type, loss_type):
    T = 1000
    dif = ddpm_torch.GaussianDiffusion(betas_of(T), mean_type, var_type, loss_type, vlb_weight=0.5)
    x_0, noise = rnd(4, 2, 5, 3, seed=1).clamp(-1, 1), rnd(4, 2, 5, 3, seed=2)
    t = torch.tensor([0, 1, 500, T - 1])
    out = (rnd(4, 4, 5, 3, seed=3) * 0.5).requires_grad_(True)
    gl = torch.tensor([0.3, -1.0, 2.0, 0.5])
    loss = dif.train_losses(lambda x, tt: out, x_0, t, noise=noise)
    assert loss.shape == (4,) and loss.dtype == torch.float32
    (loss * gl).sum().backward()
    tb = R.tables(betas_of(T))
    o64 = out.detach().double().requires_grad_(True)
    x64, n64 = x_0.double(), noise.double()
    xt64 = D.q_sample(tb, x64, t, n64)
    w = (1.0, 0.5, True) if loss_type == "hybrid" else (0.0, 1.0, False)
    ref = R.weighted_loss(tb, mean_type, var_type, x64, xt64, t, o64, R.loss_target(tb, mean_type, x64, xt64, t, n64), *w)
    (ref * gl.double()).sum().backward()
    check(loss, ref.detach(), 2e-4, name="loss")
    check(out.grad[:, :2], o64.grad[:, :2], 2e-4, atol=1e-9, name="d/d mean half")
    check(out.grad[:, 2:], o64.grad[:, 2:], 2e-4, name="d/dv")
    assert emu.log.count("ddpm_learned_loss") == 2 and "ddpm_mse_fwd" not in emu.log and "ddpm_vlb_terms" not in emu.log
    if loss_type == "hybrid":                      # the mean half sees the MSE alone
        tgt = R.loss_target(tb, mean_type, x64, xt64, t, n64)
        mse_grad = 2.0 * (o64.detach()[:, :2] - tgt) / x_0[0].numel() * gl.double().reshape(4, 1, 1, 1)
        check(out.grad[:, :2], mse_grad, 2e-5, name="stop-gradient")


def test_no_grad_bound_term_returns_the_prediction_and_rejects_a_c_channel_network(emu):
    dif = ddpm_torch.GaussianDiffusion(betas_of(8), "eps", "learned-range", "kl")
    x_0, x_t, t = rnd(2, 1, 4, 4, seed=1), rnd(2, 1, 4, 4, seed=2), torch.tensor([0, 5])
    out = rnd(2, 2, 4, 4, seed=3)
    with torch.no_grad():
        loss, pred = dif._loss_term_bpd(lambda x, tt: out, x_0, x_t, t, clip_denoised=True, return_pred=True)
    tb = R.tables(betas_of(8))
    ref, rpred = R.loss_term(tb, "eps", "learned-range", x_0.double(), x_t.double(), t, out.double(), True)
    check(loss, ref, 2e-4, name="L_t")
    check(pred, rpred, 2e-5, name="pred_x0")
    assert emu.log == ["ddpm_vlb_terms_lv"]
    with pytest.raises(ValueError, match="twice the channels"):
        dif._loss_term_bpd(lambda x, tt: out[:, :1], x_0, x_t, t, clip_denoised=True, return_pred=False)
    mean, var, logvar, pred2 = dif.p_mean_var(lambda x, tt: out, x_t, t, clip_denoised=True, return_pred=True)
    assert mean.shape == var.shape == logvar.shape == x_t.shape
    check(logvar, R.model_logvar(tb, "learned-range", out.double()[:, 1:], t), 2e-5, name="logvar")
    assert torch.allclose(var.log(), logvar, atol=1e-5)
    rmean, _ = R.step(tb, "eps", "learned-range", x_t.double(), t, out.double(), torch.zeros_like(x_t).double(), True)
    check(mean, rmean, 2e-5, name="mean")


# ------------------------------------------------------------------------------------------------------------------ Trainer.step
def _make(cfg, seed=11, rand=23):
    torch.manual_seed(seed)
    m = ddpm_torch.UNet(**cfg)
    sd = U.randomize_state_dict(m.state_dict(), rand)
    m.load_state_dict(sd)
    m.set_compute_dtype(torch.float32)
    return m, sd


@pytest.mark.parametrize("var_type", LEARNED)
def test_three_hybrid_trainer_steps_match_the_float64_oracle_trainer(emu, var_type):
    lr, ch = 1e-3, 3
    cfg = CA.edge(CA.TINY, ch, 2 * ch)
    m, sd = _make(cfg)
    dif = ddpm_torch.GaussianDiffusion(betas_of(1000), "eps", var_type, "hybrid")
    assert dif.vlb_weight == 1.0
    opt = torch.optim.Adam(m.parameters(), lr=lr, betas=(0.9, 0.999))
    tr = ddpm_torch.Trainer(m, opt, dif, epochs=1, trainloader=None, scheduler=None, num_accum=1, use_ema=True, grad_norm=1.0, shape=(ch, 8, 8),
                            device=CPU, ema_decay=0.9999)
    m.train()
    oracle = R.oracle_trainer(sd, cfg, lr, "eps", var_type, 1.0)
    g = torch.Generator().manual_seed(21)
    losses, ref = [], []
    for i in range(3):
        x = torch.rand(2, ch, 8, 8, generator=g) * 2 - 1
        tr.stats.reset()
        tr.step(x, global_steps=i + 1)
        losses.append(tr.current_stats["loss"])
        ref.append(oracle.step(x)[0])
    assert tr._direct, "the hybrid loss of a learned variance takes the autograd-free step"
    assert emu.log.count("ddpm_learned_loss") == 3 and "ddpm_mse_fwd" not in emu.log and "ddpm_mse_bwd" not in emu.log
    i = emu.log.index("ddpm_learned_loss")
    assert emu.log[i + 1] == "ddpm_weighted_sum_f32"
    assert torch.allclose(torch.tensor(losses, dtype=torch.float64), torch.tensor(ref, dtype=torch.float64), rtol=5e-4), (losses, ref)
    slack = 0.25 * lr * 3
    check_state(m.state_dict(), oracle.state(), 1e-3, "param", adam_slack=slack)
    check_state(tr.ema.shadow, oracle.shadow, 1e-3, "shadow", adam_slack=slack)


def test_generic_step_with_accumulation_runs_the_autograd_node(emu):
    ch = 1
    cfg = CA.edge(CA.TINY, ch, 2 * ch)
    m, sd = _make(cfg)
    dif = ddpm_torch.GaussianDiffusion(betas_of(1000), "eps", "learned-range", "hybrid")
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    tr = ddpm_torch.Trainer(m, opt, dif, epochs=1, trainloader=None, scheduler=None, num_accum=2, use_ema=True, grad_norm=1.0, shape=(ch, 8, 8),
                            device=CPU, ema_decay=0.9999)
    m.train()
    oracle = R.oracle_trainer(sd, cfg, 1e-3, "eps", "learned-range", 1.0, num_accum=2)
    g = torch.Generator().manual_seed(5)
    for i in range(2):
        x = torch.rand(2, ch, 8, 8, generator=g) * 2 - 1
        tr.stats.reset()
        tr.step(x, global_steps=i + 1)
        lo, _ = oracle.step(x)
        assert abs(tr.current_stats["loss"] - lo) <= 5e-4 * abs(lo)
    assert not tr._direct and emu.log.count("ddpm_learned_loss") == 4          # forward (loss alone) + backward per call
    check_state(m.state_dict(), oracle.state(), 1e-3, "param", adam_slack=0.25e-3)


# ------------------------------------------------------------------------------------------------------------------ evaluation, sampling
@pytest.mark.parametrize("var_type", LEARNED)
@pytest.mark.parametrize("mean_type", R.MEAN_TYPES)
def test_calc_all_bpd_and_p_sample_chains_at_T8(emu, mean_type, var_type):
    T, shape = 8, (3, 2, 4, 5)
    dif = ddpm_torch.GaussianDiffusion(betas_of(T), mean_type, var_type, "kl")
    tb = R.tables(betas_of(T))
    w = rnd(T, *shape[1:], seed=4) * 0.3
    x_0, noise = rnd(*shape, seed=5).clamp(-1, 1), rnd(T, *shape, seed=6)
    total, losses, prior, mses = dif.calc_all_bpd(net_of(w), x_0, clip_denoised=True, noise_stream=iter(noise))
    assert emu.log == ["ddpm_q_sample", "ddpm_bpd_terms_lv", "ddpm_add_i64"] * T + ["ddpm_bpd_finish"]
    want = R.all_bpd(tb, mean_type, var_type, x_0.double(), noise.double(), net_of(w, torch.float64), True)
    want32 = R.all_bpd(R.tables(betas_of(T), torch.float32), mean_type, var_type, x_0, noise, net_of(w), True)
    for got, k in ((total, "total"), (losses, "losses"), (prior, "prior"), (mses, "mses")):
        assert got.dtype == torch.float32 and got.shape == want[k].shape
        hold(got, want[k], want32[k], k)
    emu.log.clear()
    x_T, zs = rnd(*shape, seed=7), rnd(T, *shape, seed=8)
    x = dif._sample_loop(net_of(w), shape, CPU, x_T, None, z_stream=iter(zs))
    assert emu.log == ["ddpm_p_sample_step_lv"] * T
    check(x, R.sample_chain(tb, mean_type, var_type, net_of(w, torch.float64), x_T.double(), zs.double()), 2e-4, name="p_sample")
    xp, preds = dif.p_sample_progressive(net_of(w), shape, device=CPU, noise=x_T, pred_freq=4, z_stream=iter(zs))
    assert torch.equal(xp, x) and preds.shape == (2,) + shape
    s, pred = dif.p_sample_step(net_of(w), x_T, torch.full((3,), 5), return_pred=True, generator=torch.Generator().manual_seed(0))
    assert s.shape == pred.shape == shape


def test_ddim_on_a_2c_channel_model_reads_the_mean_half_on_its_own_tables(emu):
    T, S, shape = 40, 4, (2, 2, 4, 4)
    base = ddpm_torch.GaussianDiffusion(betas_of(T), "eps", "learned-range", "hybrid")
    sub = ddim.get_selection_schedule("linear", size=S, timesteps=T)
    w = rnd(T, *shape[1:], seed=4) * 0.3
    x_T = rnd(*shape, seed=7)
    plain = ddim.DDIM(betas_of(T), "eps", "fixed-small", "mse", eta=0.0, subsequence=sub)
    want = plain._sample_loop(lambda x, t: net_of(w)(x, t)[:, :2], shape, CPU, x_T, None)
    for dd in (ddim.DDIM.from_ddpm(base, eta=0.0, subsequence=sub), ddim.DDIM(betas_of(T), "eps", "learned", "kl", eta=1.0, subsequence=sub)):
        assert dd.learned_var and dd.model_var_type == "fixed-small" and dd._var_mode() == 0
    dd = ddim.DDIM.from_ddpm(base, eta=0.0, subsequence=sub)
    emu.log.clear()
    got = dd._sample_loop(net_of(w), shape, CPU, x_T, None)
    assert emu.log.count("ddpm_p_sample_step_lv") == S and "ddpm_p_sample_step" not in emu.log
    check(got, want.double(), 1e-6, name="DDIM-4")
    # encode / reconstruct take the mean half through a slice
    x_0 = rnd(*shape, seed=9)
    lat = dd.encode(net_of(w), x_0)
    check(lat, plain.encode(lambda x, t: net_of(w)(x, t)[:, :2], x_0).double(), 1e-6, name="encode")
    rec, _ = dd.reconstruct(net_of(w), x_0)
    assert rec.shape == x_0.shape and bool(torch.isfinite(rec).all())


# ------------------------------------------------------------------------------------------------------------------ command lines
TINY_CFG = {
    "dataset": "cifar10",
    "diffusion": {"timesteps": 8, "beta_start": 1e-4, "beta_end": 0.02, "beta_schedule": "linear", "model_mean_type": "eps"},
    "model": {"in_channels": 3, "hid_channels": 32, "ch_multipliers": [1, 2], "num_res_blocks": 1, "apply_attn": [False, True], "drop_rate": 0.1},
    "train": {"lr": 2e-4, "batch_size": 4, "grad_norm": 1.0, "epochs": 1, "warmup": 10, "use_ema": True, "ema_decay": 0.9999},
}


def _import_cli(name):
    import importlib
    return importlib.import_module(name)


def test_train_then_generate_round_trip_with_a_learned_range_variance(emu, tmp_path, monkeypatch):
    """``train.py --model-var-type learned-range --loss-type hybrid --dry-run`` -> ``generate.py`` (ancestral and ``--use-ddim``) on the
    checkpoint it wrote: a 3 -> 6 UNet through the autograd-free step."""
    cfg = tmp_path / "tiny.json"
    cfg.write_text(json.dumps(TINY_CFG))
    monkeypatch.setenv("DDPM_TORCH_AMD_SYNTHETIC_DATA", "8")
    monkeypatch.chdir(tmp_path)
    train = _import_cli("train")
    tr = train.main(["--config-path", str(cfg), "--train-device", "cpu", "--dry-run", "--num-samples", "2", "--num-workers", "0", "--compute", "fp32",
                     "--model-var-type", "learned-range", "--loss-type", "hybrid", "--chkpt-dir", str(tmp_path / "chk"), "--image-dir", str(tmp_path / "img")])
    assert tr.model.out_channels == 6 and tr.diffusion.model_var_type == "learned-range" and tr.diffusion.loss_type == "hybrid"
    assert tr._direct and "ddpm_learned_loss" in emu.log and "ddpm_p_sample_step_lv" in emu.log
    chk = tmp_path / "chk" / "tiny" / "tiny_1.pt"
    assert chk.exists() and (tmp_path / "img" / "train" / "tiny" / "1.jpg").exists()
    rec = json.load(open(glob.glob(str(tmp_path / "chk" / "tiny" / "exp_*.info"))[0]))
    assert rec["diffusion"]["model_var_type"] == "learned-range" and rec["diffusion"]["loss_type"] == "hybrid" and rec["model"]["out_channels"] == 6
    assert torch.load(chk, weights_only=False)["model"]["out_conv.2.weight"].shape[0] == 6
    gcfg = tmp_path / "tiny_lr.json"
    gcfg.write_text(json.dumps(dict(TINY_CFG, diffusion=dict(TINY_CFG["diffusion"], model_var_type="learned-range", loss_type="hybrid"))))
    gen = _import_cli("generate")
    from PIL import Image
    for extra, name in ((["--use-ddim", "--subseq-size", "4"], "ddim"), ([], "ddpm")):
        emu.log.clear()
        out = gen.main(["--config-path", str(gcfg), "--device", "cpu", "--chkpt-path", str(chk), "--total-size", "3", "--batch-size", "2",
                        "--save-dir", str(tmp_path / name), "--compute", "fp32", "--seed", "7"] + extra)
        files = glob.glob(os.path.join(out, "*.png"))
        assert len(files) == 3 and Image.open(files[0]).size == (32, 32)
        assert "ddpm_p_sample_step_lv" in emu.log and "ddpm_p_sample_step" not in emu.log


def test_eval_bpd_cli_on_a_learned_variance_checkpoint(emu, tmp_path, monkeypatch):
    """``eval_bpd.py`` builds the 3 -> 6 UNet from the configuration's ``model_var_type`` and runs the bits/dim loop on the *_lv column form."""
    cfg = dict(TINY_CFG, diffusion=dict(TINY_CFG["diffusion"], timesteps=4, model_var_type="learned", loss_type="kl"), model=dict(TINY_CFG["model"], drop_rate=0.0))
    (tmp_path / "tiny.json").write_text(json.dumps(cfg))
    monkeypatch.setenv("DDPM_TORCH_AMD_SYNTHETIC_DATA", "5")
    monkeypatch.chdir(tmp_path)
    torch.manual_seed(0)
    torch.save(ddpm_torch.UNet(out_channels=6, **cfg["model"]).state_dict(), tmp_path / "bare.pt")
    cli = _import_cli("eval_bpd")
    res = cli.main(["--config-path", str(tmp_path / "tiny.json"), "--device", "cpu", "--chkpt-path", str(tmp_path / "bare.pt"), "--compute", "fp32",
                    "--batch-size", "2", "--total-size", "3", "--seed", "5", "--save-dir", str(tmp_path / "out")])
    assert res["images"] == 3 and res["bpd"] == res["bpd"]
    assert emu.log.count("ddpm_bpd_terms_lv") == 2 * 4 and emu.log.count("ddpm_bpd_finish") == 2 and "ddpm_bpd_terms" not in emu.log


# ------------------------------------------------------------------------------------------------------------------ the real library
def test_the_four_entry_points_are_declared_bound_and_known_to_the_plan_executor():
    lib = _hip.lib()
    header = open(os.path.join(ROOT, "include", "ddpm_hip.h")).read()
    for name in NEW:
        assert f"int {name}(" in header and name in _hip.PROTOTYPES
        assert lib.ddpm_plan_entry_arity(name.encode()) == len(_hip.PROTOTYPES[name])


def test_argument_validation_returns_status_codes_without_a_gpu():
    """Null pointers (5) and bad shapes / modes (1) are rejected on the host before any launch; no call here passes validation."""
    lib, p = _hip.lib(), 0x10000
    step = [p] * 12 + [2, 8, 0, 1, 2, 10, 0]
    for i in (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10):
        assert lib.ddpm_p_sample_step_lv(*(step[:i] + [0] + step[i + 1:])) == 5, i
    assert lib.ddpm_p_sample_step_lv(*(step[:16] + [3] + step[17:])) == 1 and lib.ddpm_p_sample_step_lv(*(step[:14] + [3] + step[15:])) == 1
    assert lib.ddpm_p_sample_step_lv(*(step[:12] + [0] + step[13:])) == 1
    vlb = [p] * 12 + [2, 8, 0, 1, 2, 10, 0]
    for i in (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10):
        assert lib.ddpm_vlb_terms_lv(*(vlb[:i] + [0] + vlb[i + 1:])) == 5, i
    assert lib.ddpm_vlb_terms_lv(*(vlb[:16] + [0] + vlb[17:])) == 1                       # var_mode 0 is the step's alone
    bpd = [p] * 12 + [2, 8, 10, 0, 1, 0, 2, 10, 0]
    for i in range(12):
        assert lib.ddpm_bpd_terms_lv(*(bpd[:i] + [0] + bpd[i + 1:])) == 5, i
    assert lib.ddpm_bpd_terms_lv(*(bpd[:17] + [1] + bpd[18:])) == 1                       # decoder 0 only
    assert lib.ddpm_bpd_terms_lv(*(bpd[:14] + [9] + bpd[15:])) == 1                       # ld < T
    loss = [p] * 14 + [2, 8, 0, 2, 1, 10, 1.0, 0.5, 0]
    for i in (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12):
        assert lib.ddpm_learned_loss(*(loss[:i] + [0] + loss[i + 1:])) == 5, i
    assert lib.ddpm_learned_loss(*(loss[:17] + [0] + loss[18:])) == 1 and lib.ddpm_learned_loss(*(loss[:15] + [0] + loss[16:])) == 1
    with pytest.raises(RuntimeError, match="null pointer"):
        _hip.call("ddpm_learned_loss", *(loss[:2] + [0] + loss[3:]))
