"""CPU: the bits/dim evaluation (``GaussianDiffusion.calc_all_bpd``, ``eval_bpd.py``).  Fixture G18 pins tests/bpd_ref.py — the reference
the kernels are held to on the GPU — to the live functions of upstream; the product's host logic runs on the emulated C ABI, extended here
by the two entry points of this feature; both entry points validate their arguments on the host."""
import json
import os
import sys

import numpy as np
import pytest
import torch

import ddim as ddim_mod
import ddpm_torch
from ddpm_torch import _hip, toy
from oracle import diffusion_ref as D
from tests import abi_emulator, bpd_ref
from tests.abi_emulator import f32, i64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "ddpm-torch_amd")
needs_lib = pytest.mark.skipif(not os.path.exists(_hip.LIB_PATH), reason="libddpm_hip.so not built")

MEAN_TYPES = ("eps", "x_0", "mean")
VAR_TYPES = ("fixed-small", "fixed-large")


class BpdEmulator(abi_emulator.Emulator):
    """tests/abi_emulator.py plus ddpm_bpd_terms / ddpm_bpd_finish, restated with tests/bpd_ref.py on host pointers."""

    def ddpm_bpd_terms(self, x_0, x_t, out, t, recip, recip_m1, c1, c2, lv1, lv2, losses, mses, B, n, ld, mean_type, clip, decoder, T, st):
        assert ld >= T and decoder in (0, 1)
        tt = torch.from_numpy(i64(t, B).copy())
        names = ("sqrt_recip_alphas_bar", "sqrt_recip_m1_alphas_bar", "posterior_mean_coef1", "posterior_mean_coef2", "posterior_logvar_clipped",
                 "fixed_model_logvar")
        tabs = {k: torch.from_numpy(f32(p, T).copy()) for k, p in zip(names, (recip, recip_m1, c1, c2, lv1, lv2))}
        x0, xt, o = (torch.from_numpy(f32(p, B * n).reshape(B, n).copy()) for p in (x_0, x_t, out))
        ok = (tt >= 0) & (tt < T)
        loss, mse = bpd_ref.terms(tabs, MEAN_TYPES[mean_type], x0, xt, tt.clamp(0, T - 1), o, bool(clip), decoder)
        L, M = f32(losses, B * ld).reshape(B, ld), f32(mses, B * ld).reshape(B, ld)
        for b in range(B):
            if ok[b]:                                   # a sample outside the tables writes nothing
                L[b, tt[b]], M[b, tt[b]] = float(loss[b]), float(mse[b])

    def ddpm_bpd_finish(self, x_0, losses, prior, total, B, n, T, ld, sqrt_ab_last, log_1m_ab_last, st):
        x = f32(x_0, B * n).reshape(B, n).astype(np.float64)
        m, lv = np.float32(sqrt_ab_last) * x, float(np.float32(log_1m_ab_last))
        pr = (0.5 * ((-1.0 - lv) + m * m + np.exp(lv))).mean(1) / np.log(2.0)
        f32(prior, B)[...] = pr
        f32(total, B)[...] = f32(losses, B * ld).reshape(B, ld)[:, :T].astype(np.float64).sum(1) + pr


@pytest.fixture
def emu(monkeypatch):
    _hip.lib()
    e = BpdEmulator(_hip.lib())
    monkeypatch.setattr(_hip, "_invoke", lambda name, args: e.call(name, *args))
    monkeypatch.setattr(_hip, "stream", lambda: 0)
    monkeypatch.setattr(_hip, "require_cuda", lambda *a: None)
    monkeypatch.setattr(_hip, "on_device", lambda t: True)
    return e


def close(got, want, name):
    assert torch.allclose(got.double(), want.double(), rtol=2e-5, atol=1e-6), (name, float((got.double() - want.double()).abs().max()))


# ------------------------------------------------------------------ the reference of the GPU tests against upstream's live functions
@pytest.mark.parametrize("var_type", VAR_TYPES)
@pytest.mark.parametrize("mean_type", MEAN_TYPES)
def test_float64_composition_reproduces_the_reference_fixture(golden, mean_type, var_type):
    g = golden("g18_bpd.pt")
    for kind, decoder in (("images", 0), ("toy", 1)):
        rec = g[kind]
        T = D.ddpm_tables(D.beta_schedule(*rec["schedule"]), var_type)
        w = rec["w"].double()
        net = lambda x_t, t: 0.7 * x_t + w[int(t[0])]                                      # noqa: E731
        for clip in ((True, False) if kind == "images" else (False,)):
            want = rec["records"][f"{mean_type}/{var_type}" + (f"/clip{int(clip)}" if kind == "images" else "")]
            mine = bpd_ref.all_bpd(T, mean_type, rec["x_0"].double(), rec["noise"].double(), net, clip, decoder)
            for k in ("losses", "mses", "prior", "total"):
                close(mine[k], want[k], f"{kind} {k} clip={clip}")


# ------------------------------------------------------------------ host logic on the emulated ABI
@needs_lib
@pytest.mark.parametrize("mean_type", MEAN_TYPES)
def test_calc_all_bpd_on_the_emulated_abi(emu, golden, mean_type):
    rec = golden("g18_bpd.pt")["images"]
    dif = ddpm_torch.GaussianDiffusion(ddpm_torch.get_beta_schedule(*rec["schedule"]), mean_type, "fixed-large", "mse")
    T, w = dif.timesteps, rec["w"]
    seen = []

    def net(x_t, t):
        seen.append(int(t[0]))
        assert int(t.min()) == int(t.max())
        return 0.7 * x_t + w[int(t[0])]

    total, losses, prior, mses = dif.calc_all_bpd(net, rec["x_0"], clip_denoised=True, noise_stream=iter(rec["noise"]))
    want = rec["records"][f"{mean_type}/fixed-large/clip1"]
    assert seen == list(range(T - 1, -1, -1))
    assert emu.log == ["ddpm_q_sample", "ddpm_bpd_terms", "ddpm_add_i64"] * T + ["ddpm_bpd_finish"]
    for got, k in ((total, "total"), (losses, "losses"), (prior, "prior"), (mses, "mses")):
        assert got.dtype == torch.float32 and got.shape == want[k].shape
        close(got, want[k], k)
    close(dif._prior_bpd(rec["x_0"]), want["prior"], "_prior_bpd")
    mean, var, logvar = dif.q_mean_var(rec["x_0"], torch.full((5,), T - 1))
    tabs = D.ddpm_tables(D.beta_schedule(*rec["schedule"]), "fixed-large")
    close(mean, tabs["sqrt_alphas_bar"][-1].float() * rec["x_0"], "q mean")
    assert var.shape == logvar.shape == (5, 1, 1, 1) and torch.allclose(var.log(), logvar, atol=1e-6)
    close(var.flatten(), (1 - tabs["alphas_bar"][-1]).float().expand(5), "q var")


@needs_lib
def test_rng_draw_order_and_nan_prefill(emu):
    """With a seed: T draws of x_0's shape from a generator on x_0's device, the first for t = T-1.  The tables start as NaN, so a step
    the kernel refuses shows in the total of its sample and nowhere else."""
    betas = ddpm_torch.get_beta_schedule("linear", 1e-4, 0.02, 6)
    dif = ddpm_torch.GaussianDiffusion(betas, "eps", "fixed-small", "mse")
    x_0 = torch.rand(3, 3, 4, 4, generator=torch.Generator().manual_seed(1)) * 2 - 1
    got = dif.calc_all_bpd(lambda x, t: 0.1 * x, x_0, seed=11)
    rng = torch.Generator("cpu").manual_seed(11)
    noise = [torch.empty_like(x_0).normal_(generator=rng) for _ in range(6)]
    want = dif.calc_all_bpd(lambda x, t: 0.1 * x, x_0, noise_stream=iter(noise))
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    assert all(bool(torch.isfinite(v).all()) for v in got)
    again = dif.calc_all_bpd(lambda x, t: 0.1 * x, x_0, seed=11)
    assert all(torch.equal(a, b) for a, b in zip(got, again))
    # without a seed the draws come from the default generator
    torch.manual_seed(11)
    dflt = dif.calc_all_bpd(lambda x, t: 0.1 * x, x_0)
    assert all(torch.equal(a, b) for a, b in zip(got, dflt))
    # one refused write (sample 1 at t = 2): its columns stay NaN, and so does its total
    real = emu.ddpm_bpd_terms

    def refusing(x_0_, x_t, out, t, *rest):
        tt = i64(t, 3)
        step = int(tt[0])
        if step == 2:
            tt[1] = 99
        real(x_0_, x_t, out, t, *rest)
        tt[1] = step

    emu.ddpm_bpd_terms = refusing
    total, losses, prior, mses = dif.calc_all_bpd(lambda x, t: 0.1 * x, x_0, seed=11)
    hole = torch.zeros(3, 6, dtype=torch.bool)
    hole[1, 2] = True
    assert torch.equal(torch.isnan(losses), hole) and torch.equal(torch.isnan(mses), hole)
    assert torch.equal(torch.isnan(total), torch.tensor([False, True, False])) and bool(torch.isfinite(prior).all())


@needs_lib
def test_toy_calc_all_bpd_uses_the_continuous_decoder_and_never_clips(emu, golden):
    rec = golden("g18_bpd.pt")["toy"]
    dif = toy.GaussianDiffusion(ddpm_torch.get_beta_schedule(*rec["schedule"]), "eps", "fixed-large", "mse")
    w = rec["w"]
    total, losses, prior, mses = dif.calc_all_bpd(lambda x_t, t: 0.7 * x_t + w[int(t[0])], rec["x_0"], clip_denoised=True, noise_stream=iter(rec["noise"]))
    want = rec["records"]["eps/fixed-large"]
    for got, k in ((total, "total"), (losses, "losses"), (prior, "prior"), (mses, "mses")):
        close(got, want[k], k)
    with pytest.raises(NotImplementedError):
        toy.GaussianDiffusion(ddpm_torch.get_beta_schedule(*rec["schedule"]), "eps", "fixed-large", "kl")


def test_ddim_refuses_the_bound():
    betas = ddpm_torch.get_beta_schedule("linear", 1e-4, 0.02, 100)
    dd = ddim_mod.DDIM(betas, "eps", "fixed-small", "mse", eta=0.0, subsequence=ddim_mod.get_selection_schedule("linear", 10, 100))
    with pytest.raises(NotImplementedError, match="full chain"):
        dd.calc_all_bpd(lambda x, t: x, torch.zeros(1, 3, 4, 4))


@needs_lib
def test_entry_points_validate_on_the_host():
    lib = _hip.lib()
    p = 0x10000                                                  # a non-null address that is never dereferenced: every call below is refused
    ok = [p] * 12 + [2, 8, 10, 0, 1, 0, 10, 0]                   # B, n, ld, mean_type, clip, decoder, T, stream
    for i in range(12):
        assert lib.ddpm_bpd_terms(*(ok[:i] + [0] + ok[i + 1:])) == 5, i
    bad = {12: 0, 13: 0, 14: 9, 15: 3, 17: 2, 18: 0}             # B, n, ld < T, mean_type, decoder, T
    for i, v in bad.items():
        assert lib.ddpm_bpd_terms(*(ok[:i] + [v] + ok[i + 1:])) == 1, i
    assert lib.ddpm_bpd_terms(*(ok[:15] + [-1] + ok[16:])) == 1 and lib.ddpm_bpd_terms(*(ok[:17] + [-1] + ok[18:])) == 1
    fin = [p, p, p, p, 2, 8, 10, 10, 0.5, -0.1, 0]
    for i in range(4):
        assert lib.ddpm_bpd_finish(*(fin[:i] + [0] + fin[i + 1:])) == 5, i
    for i, v in {4: 0, 5: 0, 6: 0, 7: 9}.items():
        assert lib.ddpm_bpd_finish(*(fin[:i] + [v] + fin[i + 1:])) == 1, i
    with pytest.raises(RuntimeError, match="bad shape"):
        _hip.call("ddpm_bpd_terms", *(ok[:14] + [9] + ok[15:]))


# ------------------------------------------------------------------ command line
CFG = {
    "dataset": "cifar10",
    "diffusion": {"timesteps": 4, "beta_start": 1e-4, "beta_end": 0.02, "beta_schedule": "linear", "model_mean_type": "eps",
                  "model_var_type": "fixed-large", "loss_type": "mse"},
    "model": {"in_channels": 3, "hid_channels": 32, "ch_multipliers": [1, 2], "num_res_blocks": 1, "apply_attn": [False, True], "drop_rate": 0.0},
}


@needs_lib
def test_eval_bpd_cli_on_the_emulated_abi(emu, tmp_path, monkeypatch):
    (tmp_path / "tiny.json").write_text(json.dumps(CFG))
    monkeypatch.setenv("DDPM_TORCH_AMD_SYNTHETIC_DATA", "5")
    monkeypatch.chdir(tmp_path)
    torch.manual_seed(0)
    torch.save(ddpm_torch.UNet(out_channels=3, **CFG["model"]).state_dict(), tmp_path / "bare.pt")
    if PKG not in sys.path:
        sys.path.insert(0, PKG)
    import importlib
    cli = importlib.import_module("eval_bpd")
    argv = ["--config-path", str(tmp_path / "tiny.json"), "--device", "cpu", "--chkpt-path", str(tmp_path / "bare.pt"), "--compute", "fp32",
            "--batch-size", "2", "--total-size", "3", "--seed", "5", "--save-dir", str(tmp_path / "out"), "--save-terms", str(tmp_path / "terms.npz")]
    res = cli.main(argv)
    assert res["images"] == 3 and res["split"] == "test"
    assert emu.log.count("ddpm_bpd_terms") == 2 * 4 and emu.log.count("ddpm_bpd_finish") == 2            # batches of 2 and 1, T = 4
    terms = np.load(tmp_path / "terms.npz")
    assert terms["losses"].shape == terms["mses"].shape == (4,)
    assert np.isfinite(terms["losses"]).all() and abs(float(terms["losses"][0]) - res["L_0"]) < 1e-9
    assert abs(float(terms["losses"].sum()) + res["prior_bpd"] - res["bpd"]) < 1e-4 * abs(res["bpd"])
    assert abs(float(terms["mses"].mean()) - res["mse"]) < 1e-9
    text = (tmp_path / "out" / "eval" / "tiny" / "metrics.txt").read_text()
    assert "'bpd'" in text and "'prior_bpd'" in text and "'L_0'" in text and "'mse'" in text
    res2 = cli.main(argv + ["--no-clip-denoised"])
    assert res2["prior_bpd"] == res["prior_bpd"] and res2["bpd"] != res["bpd"]
