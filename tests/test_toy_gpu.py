"""GPU: the toy pipeline (ddpm_torch.toy) on the fused decoder kernels of csrc/toymlp.hip — the upstream Decoder's fixture G8 (forward,
every gradient, the 10-step training recipe), a geometry sweep against a float64 restatement of the oracle, determinism and the launch
budget, the non-clipping sampling chain through the captured step, and train_toy.py end to end."""
import os
import re
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

from ddpm_torch import _hip
from ddpm_torch.toy import Decoder, GaussianDiffusion, Trainer, DataStreamer, get_beta_schedule
from oracle import diffusion_ref as Dref
from oracle import toy_ref
from oracle import unet_ref as U
from tests.golden.recipes import check

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORDER = ["in_fc.weight", "temp_fc.0.norm1.weight", "temp_fc.0.norm1.bias", "temp_fc.0.fc1.weight", "temp_fc.0.norm2.weight",
         "temp_fc.0.norm2.bias", "temp_fc.0.fc2.weight", "temp_fc.0.enc.weight", "temp_fc.0.enc.bias", "out_norm.weight", "out_norm.bias",
         "out_fc.weight", "out_fc.bias", "t_proj.0.weight", "t_proj.0.bias"]


def model_from(sd, D, M, L):
    m = Decoder(D, M, L)
    m.load_state_dict(sd)
    return m.to(DEV)


def ref64(sd, x, t, M, L):
    """oracle/toy_ref.decoder_forward in float64 from the fp32 sinusoidal embedding (the model computes it in fp32, functions.py:10-26)."""
    te = F.leaky_relu(F.linear(U.timestep_embedding(t, M).to(x.dtype), sd["t_proj.0.weight"], sd["t_proj.0.bias"]), 0.02)
    h = F.linear(x, sd["in_fc.weight"])
    for _ in range(L):
        h = toy_ref._temporal(sd, "temp_fc.0.", h, te, M)
    return F.linear(F.layer_norm(h, (M,), sd["out_norm.weight"], sd["out_norm.bias"]), sd["out_fc.weight"], sd["out_fc.bias"])


def grads_of(m):
    return {k: p.grad.detach().cpu() for k, p in m.named_parameters()}


def test_g8_forward_gradients_and_dx(golden):
    g = golden("g8_toy.pt")
    m = model_from(g["sd"], 2, 128, 3)
    x = g["x"].to(DEV).requires_grad_(True)
    y = m(x, g["t"].to(DEV))
    check(y, g["y"], 1e-5, name="toy.y")
    (y * g["gy"].to(DEV)).sum().backward()
    got = grads_of(m)
    for k, v in g["grads"].items():                     # the shared layer's gradients are summed over its 3 uses
        check(got[k], v, 5e-5, name="toy.grad." + k)
    xr = g["x"].clone().requires_grad_(True)
    sd = {k: v.clone() for k, v in g["sd"].items()}
    (toy_ref.decoder_forward(sd, xr, g["t"], 128, 3) * g["gy"]).sum().backward()
    check(x.grad, xr.grad, 5e-5, name="toy.dx")


CASES = [(D, M, L, B, (100, 1000)[i % 2]) for i, (D, M, L, B) in enumerate(
    [(dm + (B,)) for dm in [(2, 128, 3), (2, 64, 1), (3, 256, 2), (2, 32, 4)] for B in (1, 31, 1000, 1001, 30000)])]


@pytest.mark.parametrize("D,M,L,B,T", CASES)
def test_geometry_sweep_against_float64(D, M, L, B, T, monkeypatch):
    torch.manual_seed(B + M)
    m = Decoder(D, M, L)
    with torch.no_grad():                                # non-trivial LayerNorm affines and biases
        for k, p in m.named_parameters():
            if k.endswith("bias") or "norm" in k:
                p.add_(0.1 * torch.randn_like(p))
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    m = m.to(DEV)
    m.timesteps = T
    gen = torch.Generator().manual_seed(7)
    x = torch.randn(B, D, generator=gen)
    t = torch.randint(T, (B,), generator=gen)
    gy = torch.randn(B, D, generator=gen)
    calls = []
    real = _hip.call
    monkeypatch.setattr(_hip, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    xd = x.to(DEV).requires_grad_(True)
    y = m(xd, t.to(DEV))
    (y * gy.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    assert len(calls) <= 6 and sum(c.startswith("ddpm_toy_decoder_fwd") or c == "ddpm_toy_time_table" for c in calls) <= 2, calls
    monkeypatch.setattr(_hip, "call", real)
    g1 = grads_of(m)
    dx1 = xd.grad.clone()
    # second backward: bit-identical
    m.zero_grad(set_to_none=True)
    xd.grad = None
    y2 = m(xd, t.to(DEV))
    (y2 * gy.to(DEV)).sum().backward()
    assert torch.equal(y, y2)
    g2 = grads_of(m)
    assert all(torch.equal(g1[k], g2[k]) for k in g1) and torch.equal(dx1, xd.grad)
    # float64 oracle
    p = {k: v.double().requires_grad_(True) for k, v in sd.items() if k.startswith(("in_fc", "out", "t_proj", "temp_fc.0."))}
    xr = x.double().requires_grad_(True)
    yr = ref64(p, xr, t, M, L)
    (yr * gy.double()).sum().backward()
    # Bars.  Some of these numbers are ill-conditioned in ANY fp32 evaluation: an element whose row sits near a LeakyReLU kink can land
    # on the other side of it, and a weight gradient is a sum of ~L*B row terms with mixed signs — in_fc's most of all, since LN1 right
    # after it is scale-invariant and its row terms nearly cancel.  So each tensor is held, element-wise (max) and norm-wise, to 1e-4
    # (max) / 1e-5 (norm) of float64 or to 8x what fp32 torch itself misses there, whichever is larger (measured: equal to fp32 torch
    # at (2, 128, 3), 2.5-7.6x at (3, 256, 2) and B = 30 000, where the kernels' serial K = 256 MFMA chains round differently).  The fp32 yardstick is the worst
    # of three CPU evaluations — as given, and with every parameter moved by about one rounding unit at random — since where the kinks
    # fall depends on the rounding.
    y64, dx64 = yr.detach(), xr.grad
    refs = [(k, p[k].grad) for k in ORDER] + [("dx", dx64), ("y", y64)]
    worst = {k: [0.0, 0.0] for k, _ in refs}

    def errs(a, ref):
        d = a.double() - ref
        return float(d.abs().max()) / (float(ref.abs().max()) + 1e-30), float(d.norm()) / (float(ref.norm()) + 1e-30)

    for trial in range(3):
        gen32 = torch.Generator().manual_seed(100 + trial)
        p32 = {}
        for k, v in p.items():
            v32 = v.detach().float()
            if trial:
                v32 = v32 * (1 + (torch.rand(v32.shape, generator=gen32) - 0.5) * 2 ** -23)
            p32[k] = v32.requires_grad_(True)
        x32 = x.clone().requires_grad_(True)
        y32 = ref64(p32, x32, t, M, L)
        (y32 * gy).sum().backward()
        got = {k: p32[k].grad for k in ORDER}
        got.update(dx=x32.grad, y=y32.detach())
        for k, ref in refs:
            worst[k] = [max(a, b) for a, b in zip(worst[k], errs(got[k], ref))]
    ours = dict(g1)
    ours.update(dx=dx1.cpu(), y=y.detach().cpu())
    bad = []
    for k, ref in refs:
        e, en = errs(ours[k], ref)
        w, wn = worst[k]
        print(f"toy sweep D={D} M={M} L={L} B={B} T={T} {k}: max {e:.2e} (fp32 torch {w:.2e}) norm {en:.2e} (fp32 torch {wn:.2e})")
        if e > max(1e-5 if k == "y" else 1e-4, 8 * w) or en > max(1e-5, 8 * wn):
            bad.append((k, e, w, en, wn))
    assert not bad, bad


def _g8_data(g):
    gen = torch.Generator().manual_seed(g["data_seed"])
    ang = torch.randint(8, (10, 1000), generator=gen).double() * (3.141592653589793 / 4)
    data = (torch.stack([ang.cos(), ang.sin()], -1) * 2 + 0.1 * torch.randn(10, 1000, 2, generator=gen, dtype=torch.float64)).float()
    ts = torch.randint(100, (10, 1000), generator=gen)
    noises = torch.randn(10, 1000, 2, generator=gen)
    return data, ts, noises


def test_g8_training_recipe_on_the_gpu(golden):
    g = golden("g8_toy.pt")
    data, ts, noises = _g8_data(g)
    m = model_from(g["sd"], 2, 128, 3)
    dif = GaussianDiffusion(get_beta_schedule("linear", 1e-3, 0.2, 100), "eps", "fixed-large", "mse")
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    losses = []
    for i in range(10):
        loss = dif.train_losses(m, data[i].to(DEV), ts[i].to(DEV), noise=noises[i].to(DEV)).mean()
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    assert torch.allclose(torch.tensor(losses, dtype=torch.float64), g["losses"], rtol=2e-4), (losses, g["losses"])
    sd = {k: v.cpu() for k, v in m.state_dict().items()}
    for k, v in g["sd_after"].items():
        check(sd[k], v, 2e-3, name="toy.after." + k)


def test_sampling_chain_through_the_captured_step_matches_the_oracle(golden, monkeypatch):
    g = golden("g8_toy.pt")
    m = model_from(g["sd"], 2, 128, 3).eval()
    dif = GaussianDiffusion(get_beta_schedule("linear", 1e-3, 0.2, 100), "eps", "fixed-large", "mse")
    gen = torch.Generator().manual_seed(11)
    x_T = torch.randn(1000, 2, generator=gen) * 3
    zs = [torch.randn(1000, 2, generator=gen) for _ in range(100)]
    monkeypatch.setenv("DDPM_TORCH_AMD_GRAPH", "1")
    with torch.inference_mode():
        x = dif._sample_loop(m, (1000, 2), DEV, x_T.to(DEV), None, z_stream=iter([z.to(DEV) for z in zs]))
    assert any(k[1] == (1000, 2) and k[3][1] for k in dif._sample_graphs), "the chain did not run through the captured step"
    T = Dref.ddpm_tables(Dref.beta_schedule("linear", 1e-3, 0.2, 100), "fixed-large")
    sd = {k: v.clone() for k, v in g["sd"].items()}
    xr, big = x_T.clone(), 0.0
    with torch.no_grad():
        for i, ti in enumerate(range(99, -1, -1)):
            t = torch.full((1000,), ti, dtype=torch.int64)
            xr, pred = Dref.p_step_from_eps(T, xr, t, toy_ref.decoder_forward(sd, xr, t, 128, 3), zs[i], clip_denoised=False)
            big = max(big, float(pred.abs().max()))
    assert big > 1.0, "the oracle chain never left [-1, 1]: a clipping bug could not be seen"
    check(x, xr, 1e-3, name="toy.chain100")                       # relative to the chain's range


def test_seeded_sampling_repeats_and_sees_optimizer_updates(golden, monkeypatch):
    g = golden("g8_toy.pt")
    m = model_from(g["sd"], 2, 128, 3)
    dif = GaussianDiffusion(get_beta_schedule("linear", 1e-3, 0.2, 100), "eps", "fixed-large", "mse")
    monkeypatch.setenv("DDPM_TORCH_AMD_GRAPH", "1")
    a = dif.p_sample(m, (500, 2), device=DEV, seed=3)
    b = dif.p_sample(m, (500, 2), device=DEV, seed=3)
    assert torch.equal(a, b)
    data, ts, noises = _g8_data(g)
    opt = torch.optim.Adam(m.parameters(), lr=1e-2)
    dif.train_losses(m, data[0].to(DEV), ts[0].to(DEV), noise=noises[0].to(DEV)).mean().backward()
    opt.step()
    after = dif.p_sample(m, (500, 2), device=DEV, seed=3)          # replays the step captured before the update
    assert not torch.equal(after, a)
    monkeypatch.setenv("DDPM_TORCH_AMD_GRAPH", "0")
    eager = dif.p_sample(m, (500, 2), device=DEV, seed=3)
    assert torch.equal(after, eager), float((after - eager).abs().max())


def test_toy_trainer_step_lowers_the_loss_on_gaussian8():
    import numpy as np
    np.random.seed(0)
    torch.manual_seed(0)
    m = Decoder(2, 128, 3).to(DEV)
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    dif = GaussianDiffusion(get_beta_schedule("linear", 1e-3, 0.2, 100), "eps", "fixed-large", "mse")
    tr = Trainer(m, opt, dif, epochs=1, trainloader=DataStreamer("gaussian8", 1000, 60), device=DEV)
    assert tr._fused.eligible()
    first, last = [], []
    for i, x in enumerate(tr.trainloader):
        tr.stats.reset()
        tr.step(x.to(DEV))
        (first if i < 10 else last if i >= 50 else []).append(tr.current_stats["loss"])
    assert sum(last) / len(last) < 0.9 * sum(first) / len(first), (first, last)


def test_train_toy_command_line_end_to_end(tmp_path):
    script = os.path.join(ROOT, "ddpm-torch_amd", "train_toy.py")
    base = [sys.executable, script, "--dataset", "gaussian8", "--size", "4000", "--batch-size", "1000", "--eval-intv", "1", "--chkpt-intv", "1",
            "--chkpt-dir", str(tmp_path / "ck"), "--image-dir", str(tmp_path / "img")]
    env = dict(os.environ, PYTHONPATH=os.path.join(ROOT, "ddpm-torch_amd"))
    r = subprocess.run(base + ["--epochs", "2"], cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    ck = torch.load(str(tmp_path / "ck" / "ddpm_gaussian8.pt"), weights_only=False)
    assert {"model", "optimizer", "scheduler", "epoch", "loss", "kld"} <= set(ck) and ck["epoch"] == 2
    assert len(os.listdir(tmp_path / "img" / "gaussian8")) == 2
    r = subprocess.run(base + ["--epochs", "3", "--resume"], cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "3/3 epochs" in r.stderr and "1/3 epochs" not in r.stderr and "2/3 epochs" not in r.stderr
    assert torch.load(str(tmp_path / "ck" / "ddpm_gaussian8.pt"), weights_only=False)["epoch"] == 3
