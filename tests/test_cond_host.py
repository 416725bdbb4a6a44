"""CPU, C ABI emulated (tests/abi_emulator.py + tests/cond_emulator.py): the host side of class conditioning and classifier-free guidance —
``UNet(num_classes=)`` and its ``forward(x, t, y)``, ``train_losses(..., y=)``, the labelled loaders, the conditional ``Trainer``, the guided
``p_sample`` / ``DDIM.p_sample``, the ``train.py --num-classes`` / ``generate.py --labels --guidance-scale`` round trip — and the argument
validation of the three new entry points in the real library.  The float64 reference is tests/cond_ref.py; the kernels themselves are held
to it in tests/test_cond_gpu.py.

Bars: the emulator evaluates the reference's own expressions in fp32, so these tests check the wiring, at the bars the other emulated-ABI
tests use for fp32 against float64 (values 2e-4 of the largest reference magnitude; trainer losses rtol 5e-4 and states 1e-3 with the Adam
slack of tests/test_channels_accum_host.py)."""
import glob
import json
import os
import sys

import pytest
import torch

import ddpm_torch
import ddpm_torch.toy
from ddpm_torch import _hip
from ddpm_torch import datasets as DS
from oracle import diffusion_ref as D
from oracle import unet_ref as U
from tests import abi_emulator, batch_emulator, cond_emulator, ddim_emulator, learned_var_emulator
from tests import channels_accum as CA
from tests import cond_ref as R
from tests.golden.recipes import check, check_state, noise_driven, rnd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "ddpm-torch_amd")
if PKG not in sys.path:
    sys.path.insert(0, PKG)
import ddim  # noqa: E402

pytestmark = pytest.mark.skipif(not os.path.exists(_hip.LIB_PATH), reason="libddpm_hip.so not built")
CPU = torch.device("cpu")
NEW = ("ddpm_class_embed_fwd", "ddpm_class_embed_bwd", "ddpm_p_sample_step_cfg")
K = 3                                                           # classes of the test networks; class K is the null class


@pytest.fixture
def emu(monkeypatch):
    return cond_emulator.attach(batch_emulator.attach(learned_var_emulator.attach(ddim_emulator.attach(abi_emulator.install(monkeypatch, _hip)))))


def betas_of(T):
    return ddpm_torch.get_beta_schedule("linear", 1e-4, 0.02, T)


def _make(cfg, seed=11, rand=23, **kw):
    torch.manual_seed(seed)
    m = ddpm_torch.UNet(**cfg, **kw)
    sd = U.randomize_state_dict(m.state_dict(), rand)
    m.load_state_dict(sd)
    m.set_compute_dtype(torch.float32)
    return m, sd


class ClosedFormNet:
    """out = 0.7 x + w[t] + c[y]: a conditional network in closed form (``num_classes`` names its null class)."""

    def __init__(self, w, c, dtype=torch.float32):
        self.w, self.c, self.num_classes, self.calls = w.to(dtype), c.to(dtype), len(c) - 1, []

    def __call__(self, x, t, y):
        self.calls.append((tuple(x.shape), y.clone()))
        return 0.7 * x + self.w[t.long()].to(x) + self.c[y.long()].reshape((-1,) + (1,) * (x.ndim - 1)).to(x)


# ------------------------------------------------------------------------------------------------------------------ the model
def test_an_unconditional_unet_is_what_it_was_and_the_class_table_comes_last():
    cfg = CA.TINY
    torch.manual_seed(5)
    plain = ddpm_torch.UNet(**cfg)
    torch.manual_seed(5)
    want = U.init_state_dict(cfg)
    assert plain.num_classes is None and list(plain.state_dict()) == [k for k, _, _ in U.param_spec(cfg)] == list(want)
    assert all(torch.equal(v, want[k]) for k, v in plain.state_dict().items())
    torch.manual_seed(5)
    cond = ddpm_torch.UNet(**cfg, num_classes=K)
    sd = cond.state_dict()
    assert list(sd) == list(want) + ["class_embed.weight"] and [k for k, _ in cond.named_parameters()][-1] == "class_embed.weight"
    assert all(torch.equal(sd[k], want[k]) for k in want), "the class table is drawn after every other parameter"
    assert sd["class_embed.weight"].shape == (K + 1, cond.time_embedding_dim) and 0.5 < float(sd["class_embed.weight"].std()) < 1.5
    for bad in (0, -2, 2.5, True):
        with pytest.raises(ValueError, match="num_classes"):
            ddpm_torch.UNet(**cfg, num_classes=bad)


def test_forward_rules_values_and_gradients(emu):
    cfg = CA.TINY
    m, sd = _make(cfg, num_classes=K)
    plain, _ = _make(cfg)
    x, t = rnd(4, 3, 8, 8, seed=1), torch.tensor([0, 17, 500, 999])
    y = torch.tensor([0, 2, K, 0])
    with pytest.raises(ValueError, match="unconditional"):
        plain(x, t, y)
    with pytest.raises(ValueError, match="shape"):
        m(x, t, y[:3])
    with pytest.raises(ValueError, match="int64"):
        m(x, t, y.float())
    sd64 = {k: v.double() for k, v in sd.items()}
    with torch.no_grad():
        out = m(x, t, y)
        assert emu.log.count("ddpm_class_embed_fwd") == 1 and emu.log.count("ddpm_silu_fwd") == 1          # it took the second SiLU's place
        check(out, R.unet_forward(sd64, cfg, x.double(), t, y), 2e-4, name="forward")
        check(m(x, t), R.unet_forward(sd64, cfg, x.double(), t, torch.full((4,), K)), 2e-4, name="y=None is the null class")
        emu.log.clear()
        plain(x, t)
        assert "ddpm_class_embed_fwd" not in emu.log and emu.log.count("ddpm_silu_fwd") == 2
    # a sampler's time table is not for a conditional engine
    eng = m.engine()
    eng.enable_time_table(1000)
    assert eng.cond and eng.tt is None and not plain.engine().cond
    # gradients, class_embed.weight included: a row with two samples, rows with one, a row with none
    m.train()
    gout = rnd(4, 3, 8, 8, seed=2)
    (m(x, t, y) * gout).sum().backward()
    assert emu.log.count("ddpm_class_embed_bwd") == 1
    leaves = {k: v.clone().requires_grad_(True) for k, v in sd64.items()}
    (R.unet_forward(leaves, cfg, x.double(), t, y) * gout.double()).sum().backward()
    for k, p in m.named_parameters():
        if not noise_driven(k):                                  # (gradients that are analytically zero in this network: rounding noise)
            check(p.grad, leaves[k].grad, 2e-4, atol=1e-9, name=f"d {k}")
    assert bool((m.class_embed.weight.grad[1] == 0).all()) and float(m.class_embed.weight.grad[0].abs().max()) > 0


def test_train_losses_hands_the_labels_to_the_network(emu):
    T = 1000
    dif = ddpm_torch.GaussianDiffusion(betas_of(T), "eps", "fixed-large", "mse")
    net = ClosedFormNet(rnd(T, 2, 4, 4, seed=3) * 0.3, torch.tensor([0.5, -1.0, 0.25, 0.0]))
    x_0, noise, t, y = rnd(4, 2, 4, 4, seed=1), rnd(4, 2, 4, 4, seed=2), torch.tensor([0, 1, 500, 999]), torch.tensor([0, 2, 3, 1])
    loss = dif.train_losses(net, x_0, t, noise=noise, y=y)
    assert torch.equal(net.calls[0][1], y)
    tb = D.ddpm_tables(betas_of(T), "fixed-large")
    x_t = D.q_sample(tb, x_0.double(), t, noise.double())
    ref = D.mse_eps_loss(ClosedFormNet(net.w, net.c, torch.float64)(x_t, t, y), noise.double())
    check(loss, ref, 2e-4, name="loss")


# ------------------------------------------------------------------------------------------------------------------ data
def test_labelled_loaders_and_device_loader_pairs(emu, tmp_path, monkeypatch):
    import numpy as np
    import pickle
    # CIFAR-10's own files
    folder = tmp_path / "cifar-10-batches-py"
    folder.mkdir()
    rng = np.random.RandomState(0)
    want = []
    for i in range(1, 6):
        lab = [int(v) for v in rng.randint(0, 10, 2)]
        want += lab
        with open(folder / f"data_batch_{i}", "wb") as f:
            pickle.dump({"data": rng.randint(0, 256, (2, 3072), dtype=np.uint8), "labels": lab}, f)
    ds = DS.CIFAR10(root=str(tmp_path), labels=True)
    assert [ds[i][1] for i in range(10)] == want and ds[0][0].shape == (3, 32, 32)
    assert torch.is_tensor(DS.CIFAR10(root=str(tmp_path))[0])                  # without the flag: one image per item
    host, _ = ddpm_torch.get_dataloader("cifar10", 4, "train", root=str(tmp_path), labels=True, random_seed=3)
    torch.manual_seed(7)
    pairs = [(xb, yb) for xb, yb in host]
    assert all(yb.dtype == torch.int64 and len(xb) == len(yb) for xb, yb in pairs) and sorted(int(v) for _, yb in pairs for v in yb) == sorted(want)
    with pytest.raises(ValueError, match="classes"):
        ddpm_torch.get_dataloader("cifar10", 4, "train", root=str(tmp_path), labels=True, num_classes=K)        # labels up to 9
    # MNIST's idx files
    import struct
    raw = tmp_path / "MNIST" / "raw"
    raw.mkdir(parents=True)
    (raw / "train-images-idx3-ubyte").write_bytes(struct.pack(">IIII", 2051, 3, 28, 28) + rng.randint(0, 256, (3, 28, 28), dtype=np.uint8).tobytes())
    (raw / "train-labels-idx1-ubyte").write_bytes(struct.pack(">II", 2049, 3) + bytes([7, 0, 9]))
    assert [DS.MNIST(root=str(tmp_path), labels=True)[i][1] for i in range(3)] == [7, 0, 9]
    # a data set without classes, a tensor file with and without labels, the synthetic stand-in
    for name in ("celeba", "celeba_hq"):
        with pytest.raises(ValueError, match="no class labels"):
            ddpm_torch.get_dataloader(name, 2, "train", root=str(tmp_path), labels=True)
    files = tmp_path / "files"
    files.mkdir()
    imgs = torch.randint(0, 256, (6, 1, 32, 32), dtype=torch.uint8)
    torch.save(imgs, files / "mnist.pt")
    with pytest.raises(ValueError, match="labels"):
        ddpm_torch.get_dataloader("mnist", 2, "test", root=str(files), labels=True)
    torch.save({"images": imgs, "labels": torch.tensor([1, 3, 5, 7, 9, 0])}, files / "mnist.pt")
    lab, _ = ddpm_torch.get_dataloader("mnist", 4, "test", root=str(files), labels=True)
    assert [yb.tolist() for _, yb in lab] == [[1, 3, 5, 7], [9, 0]]
    assert torch.is_tensor(next(iter(ddpm_torch.get_dataloader("mnist", 4, "test", root=str(files))[0])))
    monkeypatch.setenv("DDPM_TORCH_AMD_SYNTHETIC_DATA", "7")
    syn, _ = ddpm_torch.get_dataloader("cifar10", 7, "test", root=str(tmp_path / "none"), labels=True, num_classes=K)
    assert next(iter(syn))[1].tolist() == [i % K for i in range(7)]
    syn, _ = ddpm_torch.get_dataloader("cifar10", 7, "test", root=str(tmp_path / "none"), labels=True)
    assert next(iter(syn))[1].tolist() == [i % 10 for i in range(7)]
    # DeviceLoader: the host loader's batches and labels, in its order
    data = DS.TensorImages(torch.rand(10, 3, 4, 4) * 2 - 1, labels=torch.arange(10) % 4)
    torch.manual_seed(11)
    want_pairs = list(torch.utils.data.DataLoader(data, batch_size=4, shuffle=True))
    torch.manual_seed(11)
    got_pairs = list(DS.DeviceLoader(data, 4, CPU, shuffle=True, flip=False))
    assert len(got_pairs) == len(want_pairs) == 3
    for (xa, ya), (xb, yb) in zip(got_pairs, want_pairs):
        assert torch.equal(xa, xb) and torch.equal(ya, yb) and ya.dtype == torch.int64
    assert torch.is_tensor(next(iter(DS.DeviceLoader(DS.TensorImages(torch.rand(4, 3, 4, 4)), 2, CPU))))


# ------------------------------------------------------------------------------------------------------------------ Trainer
def _trainer(m, label_drop, **kw):
    dif = ddpm_torch.GaussianDiffusion(betas_of(1000), "eps", "fixed-large", "mse")
    opt = torch.optim.Adam(m.parameters(), lr=1e-3, betas=(0.9, 0.999))
    return ddpm_torch.Trainer(m, opt, dif, epochs=1, trainloader=None, scheduler=None, num_accum=1, use_ema=True, grad_norm=1.0, shape=(3, 8, 8),
                              device=CPU, ema_decay=0.9999, label_drop=label_drop, **kw)


def test_get_input_draws_what_the_unconditional_trainer_draws_then_the_label_drop(emu):
    cond, _ = _make(CA.TINY, num_classes=K)
    plain, _ = _make(CA.TINY)
    a, b = _trainer(cond, 0.5), _trainer(plain, 0.5)
    x, y = rnd(6, 3, 8, 8, seed=1), torch.tensor([0, 1, 2, 0, 1, 2])
    for _ in range(2):
        ia, ib = a.get_input((x, y)), b.get_input(x)
        assert torch.equal(ia["t"], ib["t"]) and torch.equal(ia["noise"], ib["noise"]) and "y" not in ib
        u = torch.rand((6,), generator=b.generator)              # the conditional trainer's third draw, taken here from the other generator
        assert torch.equal(ia["y"], R.dropped_labels(y, u, 0.5, K)) and ia["y"].dtype == torch.int64
    assert torch.equal(_trainer(cond, 0.0).get_input((x, y))["y"], y)
    assert torch.equal(_trainer(cond, 1.0).get_input((x, y))["y"], torch.full((6,), K))
    with pytest.raises(ValueError, match="pairs"):
        a.step(x)
    with pytest.raises(ValueError, match="unconditional"):
        b.get_input((x, y))
    with pytest.raises(ValueError, match="probability"):
        _trainer(cond, 1.5)


def test_three_conditional_trainer_steps_match_the_float64_oracle_trainer(emu):
    cfg, lr = CA.TINY, 1e-3
    m, sd = _make(cfg, num_classes=K)
    tr = _trainer(m, 0.5)
    m.train()
    oracle = R.oracle_trainer(sd, cfg, lr, K)
    gen = torch.Generator().manual_seed(CA.GEN_SEED)
    g = torch.Generator().manual_seed(21)
    losses, ref = [], []
    for i in range(3):
        x = torch.rand(4, 3, 8, 8, generator=g) * 2 - 1
        y = torch.randint(0, K, (4,), generator=g)
        t = torch.empty((4,), dtype=torch.int64).random_(to=1000, generator=gen)
        noise = torch.empty(4, 3, 8, 8).normal_(generator=gen)
        y_used = R.dropped_labels(y, torch.rand((4,), generator=gen), 0.5, K)
        tr.stats.reset()
        tr.step((x, y), global_steps=i + 1)
        losses.append(tr.current_stats["loss"])
        ref.append(oracle.step(x, y_used, inputs=(t, noise))[0])
    assert not tr._direct, "the conditional step is the generic autograd step"
    assert tr._direct_unet() is None
    assert emu.log.count("ddpm_class_embed_fwd") == 3 and emu.log.count("ddpm_class_embed_bwd") == 3
    assert "ddpm_mt_adam_ema" in emu.log or "ddpm_adam_ema_step" in emu.log, "the fused clip + Adam + EMA update"
    assert torch.allclose(torch.tensor(losses, dtype=torch.float64), torch.tensor(ref, dtype=torch.float64), rtol=5e-4), (losses, ref)
    slack = 0.25 * lr * 3
    check_state(m.state_dict(), oracle.state(), 1e-3, "param", adam_slack=slack)
    check_state(tr.ema.shadow, oracle.shadow, 1e-3, "shadow", adam_slack=slack)
    # the per-epoch grid: classes in turn, unguided
    m.eval()
    emu.log.clear()
    tr.diffusion = ddpm_torch.GaussianDiffusion(betas_of(4), "eps", "fixed-large", "mse")
    grid = tr.sample_fn(sample_size=4, sample_seed=1)
    assert grid.shape == (4, 3, 8, 8) and emu.log.count("ddpm_class_embed_fwd") == 4 and "ddpm_p_sample_step_cfg" not in emu.log


# ------------------------------------------------------------------------------------------------------------------ samplers
@pytest.mark.parametrize("mean_type", R.MEAN_TYPES)
def test_guided_p_sample_runs_one_doubled_network_call_per_step(emu, mean_type):
    T, shape, scale = 8, (3, 2, 4, 5), 2.0
    dif = ddpm_torch.GaussianDiffusion(betas_of(T), mean_type, "fixed-large", "mse")
    tb = D.ddpm_tables(betas_of(T), "fixed-large")
    w, c = rnd(T, *shape[1:], seed=4) * 0.3, torch.tensor([0.5, -1.0, 0.25, 0.0])
    net, net64 = ClosedFormNet(w, c), ClosedFormNet(w, c, torch.float64)
    x_T, zs, y = rnd(*shape, seed=7), rnd(T, *shape, seed=8), torch.tensor([0, 2, 1])
    x = dif._sample_loop(net, shape, CPU, x_T, None, z_stream=iter(zs), y=y, guidance_scale=scale)
    assert emu.log == ["ddpm_p_sample_step_cfg"] * T
    assert all(s == (6,) + shape[1:] and lab.tolist() == [0, 2, 1, K, K, K] for s, lab in net.calls)
    check(x, R.guided_chain(tb, mean_type, net64, x_T.double(), zs.double(), y, K, scale), 2e-4, name="guided chain")
    # scale 1 with labels: the plain conditional chain on B rows and the existing step kernel
    emu.log.clear()
    net.calls.clear()
    x1 = dif._sample_loop(net, shape, CPU, x_T, None, z_stream=iter(zs), y=y, guidance_scale=1.0)
    assert emu.log == ["ddpm_p_sample_step"] * T and all(s == shape for s, _ in net.calls)
    check(x1, R.guided_chain(tb, mean_type, net64, x_T.double(), zs.double(), y, K, 1.0), 2e-4, name="conditional chain")
    # RNG consumption is the unguided loop's: x_T of [B], then one z of [B] per step
    torch.manual_seed(3)
    a = dif.p_sample(net, shape, device=CPU, y=y, guidance_scale=scale)
    torch.manual_seed(3)
    x_T2 = torch.randn(shape)
    zs2 = [torch.randn(shape) for _ in range(T)]
    assert torch.equal(a, dif._sample_loop(net, shape, CPU, x_T2, None, z_stream=iter(zs2), y=y, guidance_scale=scale))
    xp, preds = dif.p_sample_progressive(net, shape, device=CPU, noise=x_T, pred_freq=4, z_stream=iter(zs), y=y, guidance_scale=scale)
    assert torch.equal(xp, x) and preds.shape == (2,) + shape


def test_guided_ddim_and_the_stated_limits(emu):
    T, S, shape, scale = 40, 4, (2, 2, 4, 4), 3.0
    sub = ddim.get_selection_schedule("linear", size=S, timesteps=T)
    dd = ddim.DDIM(betas_of(T), "eps", "fixed-small", "mse", eta=0.0, subsequence=sub)
    w, c = rnd(T, *shape[1:], seed=4) * 0.3, torch.tensor([0.5, -1.0, 0.25, 0.0])
    net, net64 = ClosedFormNet(w, c), ClosedFormNet(w, c, torch.float64)
    x_T, y = rnd(*shape, seed=7), torch.tensor([1, 0])
    got = dd.p_sample(net, shape, device=CPU, noise=x_T, y=y, guidance_scale=scale)
    assert emu.log.count("ddpm_p_sample_step_cfg") == S and "ddpm_p_sample_step" not in emu.log
    tb = D.ddim_tables(betas_of(T), "fixed-small", 0.0, sub)
    want = R.guided_chain(tb, "eps", net64, x_T.double(), torch.zeros(S, *shape, dtype=torch.float64), y, K, scale, timestep_map=sub)
    check(got, want, 2e-4, name="guided DDIM-4")
    # learned variance: unguided only
    lv = ddpm_torch.GaussianDiffusion(betas_of(8), "eps", "learned-range", "hybrid")
    two = lambda x, t, yy: torch.cat([net(x, t, yy), 0.3 * x - 0.2], dim=1)                # noqa: E731
    two.num_classes = K
    with pytest.raises(NotImplementedError, match="learned-variance"):
        lv.p_sample(two, shape, device=CPU, y=y, guidance_scale=2.0)
    assert lv.p_sample(two, shape, device=CPU, y=y, guidance_scale=1.0).shape == shape
    # guidance needs a network that names its null class; the toy decoder takes no labels
    with pytest.raises(ValueError, match="num_classes"):
        dd.p_sample(lambda x, t, yy: x, shape, device=CPU, noise=x_T, y=y, guidance_scale=2.0)
    with pytest.raises(ValueError, match="shape"):
        dd.p_sample(net, shape, device=CPU, noise=x_T, y=torch.tensor([1, 0, 2]), guidance_scale=2.0)
    with pytest.raises(NotImplementedError, match="unconditional"):
        ddpm_torch.toy.GaussianDiffusion(betas_of(8), "eps", "fixed-small", "mse").p_sample(net, (2, 2), device=CPU, y=y)


def test_loops_without_a_label_input_of_their_own_run_conditionally(emu):
    """``calc_all_bpd`` and ``DDIM.encode`` / ``decode`` / ``reconstruct`` with ``y``: the network with its labels bound, no guidance."""
    T, shape = 8, (3, 2, 4, 5)
    w, c = rnd(40, *shape[1:], seed=4) * 0.3, torch.tensor([0.5, -1.0, 0.25, 0.0])
    net = ClosedFormNet(w, c)
    x_0, noise, y = rnd(*shape, seed=5).clamp(-1, 1), rnd(T, *shape, seed=6), torch.tensor([0, 2, 1])
    bound = lambda x, t: 0.7 * x + w[t.long()] + c[y].reshape(-1, 1, 1, 1)                # noqa: E731
    # (the bits/dim kernels the emulator restates are the learned-variance ones: a 2C-channel network, mean output | v)
    dif = ddpm_torch.GaussianDiffusion(betas_of(T), "eps", "learned-range", "kl")
    got = dif.calc_all_bpd(lambda x, t, yy: torch.cat([net(x, t, yy), 0.3 * x - 0.2], dim=1), x_0, noise_stream=iter(noise), y=y)
    want = dif.calc_all_bpd(lambda x, t: torch.cat([bound(x, t), 0.3 * x - 0.2], dim=1), x_0, noise_stream=iter(noise))
    assert all(torch.equal(a, b) for a, b in zip(got, want)) and len(net.calls) == T and all(torch.equal(lab, y) for _, lab in net.calls)
    assert "ddpm_bpd_terms_lv" in emu.log
    dd = ddim.DDIM(betas_of(40), "eps", "fixed-small", "mse", eta=0.0, subsequence=ddim.get_selection_schedule("linear", size=4, timesteps=40))
    assert torch.equal(dd.encode(net, x_0, y=y), dd.encode(bound, x_0))
    rec, lat = dd.reconstruct(net, x_0, y=y)
    rec2, lat2 = dd.reconstruct(bound, x_0)
    assert torch.equal(rec, rec2) and torch.equal(lat, lat2)


def test_a_conditional_unet_under_the_guided_sampler(emu):
    m, sd = _make(CA.TINY, num_classes=K)
    m.eval()
    T, shape = 4, (2, 3, 8, 8)
    dif = ddpm_torch.GaussianDiffusion(betas_of(T), "eps", "fixed-large", "mse")
    x_T, zs, y = rnd(*shape, seed=7), rnd(T, *shape, seed=8), torch.tensor([2, 0])
    got = dif._sample_loop(m, shape, CPU, x_T, None, z_stream=iter(zs), y=y, guidance_scale=2.0)
    assert emu.log.count("ddpm_class_embed_fwd") == T and emu.log.count("ddpm_p_sample_step_cfg") == T and "ddpm_gather_rows_f32" not in emu.log
    sd64 = {k: v.double() for k, v in sd.items()}
    net64 = lambda x, t, yy: R.unet_forward(sd64, CA.TINY, x, t, yy)                        # noqa: E731
    check(got, R.guided_chain(D.ddpm_tables(betas_of(T), "fixed-large"), "eps", net64, x_T.double(), zs.double(), y, K, 2.0), 2e-4, name="UNet chain")


# ------------------------------------------------------------------------------------------------------------------ command lines
TINY_CFG = {
    "dataset": "cifar10",
    "diffusion": {"timesteps": 8, "beta_start": 1e-4, "beta_end": 0.02, "beta_schedule": "linear", "model_mean_type": "eps"},
    "model": {"in_channels": 3, "hid_channels": 32, "ch_multipliers": [1, 2], "num_res_blocks": 1, "apply_attn": [False, True], "drop_rate": 0.1},
    "train": {"lr": 2e-4, "batch_size": 4, "grad_norm": 1.0, "epochs": 1, "warmup": 10, "use_ema": True, "ema_decay": 0.9999},
}


def test_train_then_generate_round_trip_with_class_labels_and_guidance(emu, tmp_path, monkeypatch):
    import importlib
    cfg = tmp_path / "tiny.json"
    cfg.write_text(json.dumps(TINY_CFG))
    monkeypatch.setenv("DDPM_TORCH_AMD_SYNTHETIC_DATA", "8")
    monkeypatch.chdir(tmp_path)
    train = importlib.import_module("train")
    tr = train.main(["--config-path", str(cfg), "--train-device", "cpu", "--dry-run", "--num-samples", "2", "--num-workers", "0", "--compute", "fp32",
                     "--num-classes", "3", "--label-drop", "0.25", "--chkpt-dir", str(tmp_path / "chk"), "--image-dir", str(tmp_path / "img")])
    assert tr.model.num_classes == 3 and tr.label_drop == 0.25 and not tr._direct
    assert "ddpm_class_embed_fwd" in emu.log and "ddpm_class_embed_bwd" in emu.log
    chk = tmp_path / "chk" / "tiny" / "tiny_1.pt"
    assert chk.exists() and (tmp_path / "img" / "train" / "tiny" / "1.jpg").exists()
    rec = json.load(open(glob.glob(str(tmp_path / "chk" / "tiny" / "exp_*.info"))[0]))
    assert rec["model"]["num_classes"] == 3
    assert torch.load(chk, weights_only=False)["model"]["class_embed.weight"].shape == (4, 128)
    gen = importlib.import_module("generate")
    cfg = tmp_path / "tiny_gen.json"                              # generate.py reads the variance and loss types from the configuration
    cfg.write_text(json.dumps(dict(TINY_CFG, diffusion=dict(TINY_CFG["diffusion"], model_var_type="fixed-large", loss_type="mse"))))
    from PIL import Image
    for extra, name, step in ((["--use-ddim", "--subseq-size", "4"], "ddim", "ddpm_p_sample_step_cfg"), ([], "ddpm", "ddpm_p_sample_step_cfg")):
        emu.log.clear()
        out = gen.main(["--config-path", str(cfg), "--device", "cpu", "--chkpt-path", str(chk), "--total-size", "3", "--batch-size", "2",
                        "--save-dir", str(tmp_path / name), "--compute", "fp32", "--seed", "7", "--labels", "cycle", "--guidance-scale", "2"] + extra)
        files = glob.glob(os.path.join(out, "*.png"))
        assert len(files) == 3 and Image.open(files[0]).size == (32, 32)
        assert step in emu.log and "ddpm_p_sample_step" not in emu.log and "ddpm_class_embed_fwd" in emu.log
    assert gen.labels_of("cycle", 3, 2, 5, CPU).tolist() == [2, 0, 1, 2, 0] and gen.labels_of("1, 2", 3, 1, 3, CPU).tolist() == [2, 1, 2]
    with pytest.raises(ValueError, match="classes in"):
        gen.labels_of("0,3", 3, 0, 2, CPU)
    with pytest.raises(SystemExit):
        gen.parse_args(["--guidance-scale", "2"])
    # without --labels a conditional checkpoint samples the null class on the plain step
    emu.log.clear()
    gen.main(["--config-path", str(cfg), "--device", "cpu", "--chkpt-path", str(chk), "--total-size", "1", "--batch-size", "1",
              "--save-dir", str(tmp_path / "null"), "--compute", "fp32", "--seed", "7"])
    assert "ddpm_class_embed_fwd" in emu.log and "ddpm_p_sample_step_cfg" not in emu.log


# ------------------------------------------------------------------------------------------------------------------ the real library
def test_the_three_entry_points_are_declared_bound_and_known_to_the_plan_executor():
    lib = _hip.lib()
    header = open(os.path.join(ROOT, "include", "ddpm_hip.h")).read()
    for name in NEW:
        assert f"int {name}(" in header and name in _hip.PROTOTYPES
        assert lib.ddpm_plan_entry_arity(name.encode()) == len(_hip.PROTOTYPES[name])


def test_argument_validation_returns_status_codes_without_a_gpu():
    """Null pointers (5), bad shapes (1) and misaligned pointers (3) are rejected on the host before any launch; no call here passes."""
    lib, p = _hip.lib(), 0x10000
    fwd = [p] * 5 + [2, 8, 4, 0]
    for i in range(5):
        assert lib.ddpm_class_embed_fwd(*(fwd[:i] + [0] + fwd[i + 1:])) == 5, i
    for i in (5, 6, 7):
        assert lib.ddpm_class_embed_fwd(*(fwd[:i] + [0] + fwd[i + 1:])) == 1, i
    assert lib.ddpm_class_embed_fwd(*(fwd[:2] + [p + 4] + fwd[3:])) == 3
    bwd = [p] * 3 + [2, 8, 4, 0]
    for i in range(3):
        assert lib.ddpm_class_embed_bwd(*(bwd[:i] + [0] + bwd[i + 1:])) == 5, i
    assert lib.ddpm_class_embed_bwd(*(bwd[:5] + [70000] + bwd[6:])) == 1 and lib.ddpm_class_embed_bwd(*(bwd[:3] + [0] + bwd[4:])) == 1
    step = [p] * 9 + [2.0, p, p] + [2, 8, 0, 1, 1, 10, 0]
    for i in (0, 1, 2, 3, 4, 5, 6, 7, 8, 10):
        assert lib.ddpm_p_sample_step_cfg(*(step[:i] + [0] + step[i + 1:])) == 5, i
    assert lib.ddpm_p_sample_step_cfg(*(step[:14] + [3] + step[15:])) == 1 and lib.ddpm_p_sample_step_cfg(*(step[:12] + [70000] + step[13:])) == 1
    assert lib.ddpm_p_sample_step_cfg(*(step[:17] + [0] + step[18:])) == 1 and lib.ddpm_p_sample_step_cfg(*(step[:10] + [p + 2] + step[11:])) == 3
    with pytest.raises(RuntimeError, match="null pointer"):
        _hip.call("ddpm_class_embed_bwd", 0, p, p, 2, 8, 4, 0)
