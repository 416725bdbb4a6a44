"""CPU, C ABI emulated (tests/abi_emulator.py + tests/ddim_emulator.py): the host side of DDIM inversion and latent interpolation —
``DDIM.encode / decode / reconstruct / interpolate``, ``ddim.slerp``, the three ``generate.py`` flags — and the argument validation of the
two new entry points in the real library.  The kernels themselves are held to float64 in tests/test_ddim_inverse_gpu.py."""
import glob
import json
import os
import sys

import pytest
import torch

import ddpm_torch
from ddpm_torch import _hip
from tests import abi_emulator, ddim_emulator
from tests import ddim_inverse_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "ddpm-torch_amd")
if PKG not in sys.path:
    sys.path.insert(0, PKG)
import ddim  # noqa: E402

pytestmark = pytest.mark.skipif(not os.path.exists(_hip.LIB_PATH), reason="libddpm_hip.so not built")
T = 1000


@pytest.fixture
def emu(monkeypatch):
    return ddim_emulator.attach(abi_emulator.install(monkeypatch, _hip))


def make(size, eta=0.0, mean_type="eps", schedule="linear"):
    betas = ddpm_torch.get_beta_schedule("linear", 1e-4, 0.02, T)
    sub = ddim.get_selection_schedule(schedule, size=size, timesteps=T)
    return ddim.DDIM(betas, mean_type, "fixed-small", "mse", eta=eta, subsequence=sub), betas, sub


def table_denoiser(betas, dtype=torch.float32):
    """eps = sqrt(1 - alphas_bar[t]) * x for the MODEL timestep t it is handed: the chain is then a product of known per-step gains."""
    s = torch.sqrt(1.0 - torch.cumprod(1.0 - betas, 0)).to(dtype)
    return lambda x, t: s[t].reshape((-1,) + (1,) * (x.ndim - 1)) * x


@pytest.mark.parametrize("size", [8, 50])
def test_encode_and_reconstruct_are_the_float64_products_of_the_step_gains(emu, size):
    """Bar 1e-5 relative: the emulator is fp32, S steps of a few roundings each (S * 2^-23 = 6e-6 at S = 50)."""
    dif, betas, sub = make(size)
    tb = R.tables(betas, sub)
    s = torch.sqrt(1.0 - tb["ab"])
    gain = torch.prod(tb["cx"] + tb["ce"] * s)
    back = torch.prod(tb["coef1"] * (tb["recip"] - tb["recip_m1"] * s) + tb["coef2"])
    x_0 = torch.randn(3, 1, 4, 5, generator=torch.Generator().manual_seed(size))
    state = torch.get_rng_state()
    latent = dif.encode(table_denoiser(betas), x_0)
    assert torch.equal(torch.get_rng_state(), state), "encode consumed RNG"
    assert latent.shape == x_0.shape and latent.dtype == torch.float32
    rel = float((latent.double() - gain * x_0.double()).abs().max() / (gain * x_0.double()).abs().max())
    x_rec, latent2 = dif.reconstruct(table_denoiser(betas), x_0)
    rel_rt = float((x_rec.double() - gain * back * x_0.double()).abs().max() / x_0.double().abs().max())
    print(f"\nS = {size}: encode gain {float(gain):.5f} (rel err {rel:.2e}), round-trip gain {float(gain * back):.6f} (rel err {rel_rt:.2e})")
    assert rel <= 1e-5 and rel_rt <= 1e-5
    assert torch.equal(latent, latent2)
    # the float64 restatement's own loop agrees with the closed form, and its decode inverts its encode step by step
    ref = R.encode(tb, table_denoiser(betas, torch.float64), x_0)
    assert float((ref - gain * x_0.double()).abs().max()) < 1e-12
    assert emu.log.count("ddpm_ddim_encode_step") == 2 * size and "ddpm_gather_i64" in emu.log


def test_encode_step_and_sampling_step_share_one_index_convention():
    """float64, linear 50-step schedule: the decode update on the encode step's output and the same eps returns x at i = 0, 1, 25, 49 —
    to a few 1e-16 from i = 1 on; at i = 0 to 1e-13, because 1 - ab[0] = 1e-4 carries a relative rounding error of 1e-12 that sqrt(1 - ab)
    (in ce) and sqrt(1 / ab - 1) (in the decode) see differently.  And the planted identity step of the quadratic schedule (timestep 0
    twice: cx = 1, ce = 0 at i = 1)."""
    g = torch.Generator().manual_seed(0)
    x, eps = torch.randn(4, 7, generator=g, dtype=torch.float64), torch.randn(4, 7, generator=g, dtype=torch.float64)
    _, betas, sub = make(50)
    tb = R.tables(betas, sub)
    t = torch.tensor([0, 1, 25, 49])
    nxt, _ = R.encode_step(tb, x, eps, t)
    err = (R.decode_step(tb, nxt, eps, t) - x).abs().max(1).values
    assert float(err[0]) <= 1e-13 and float(err[1:].max()) <= 2e-15, err
    tq = R.tables(betas, ddim.get_selection_schedule("quadratic", size=50, timesteps=T))
    assert float(tq["cx"][1]) == 1.0 and float(tq["ce"][1]) == 0.0


def test_return_pred_collects_the_x0_estimate_of_every_step(emu):
    dif, betas, sub = make(8)
    tb = R.tables(betas, sub)
    x_0 = torch.randn(2, 3, 4, 4, generator=torch.Generator().manual_seed(1))
    latent, preds = dif.encode(table_denoiser(betas), x_0, return_pred=True)
    assert preds.shape == (8,) + x_0.shape and torch.equal(latent, dif.encode(table_denoiser(betas), x_0))
    s = torch.sqrt(1.0 - tb["ab"])
    want0 = (tb["recip_prev"][0] - tb["recip_m1_prev"][0] * s[0]) * x_0.double()              # step 0: ab_prev = 1, the estimate is x itself
    assert float((preds[0].double() - want0).abs().max()) <= 1e-6 and torch.equal(preds[0], x_0)


def test_refusals_shapes_and_interpolation_ends(emu):
    _, betas, _ = make(8)
    net = table_denoiser(betas)
    x = torch.randn(2, 3, 4, 4, generator=torch.Generator().manual_seed(2))
    with pytest.raises(ValueError, match="eta"):
        make(8, eta=0.5)[0].encode(net, x)
    with pytest.raises(NotImplementedError, match="0 / 0"):
        make(8, mean_type="x_0")[0].encode(net, x)
    dif = make(8)[0]
    x_rec, latent = dif.reconstruct(net, x)
    assert x_rec.shape == latent.shape == x.shape
    y = torch.randn(2, 3, 4, 4, generator=torch.Generator().manual_seed(3))
    out = dif.interpolate(net, x, y, num=5, batch_size=4)
    assert out.shape == (2, 5, 3, 4, 4) and out.dtype == torch.float32
    assert torch.equal(out, dif.interpolate(net, x, y, num=5))                              # the decode batch size changes nothing
    ends = dif.interpolate(net, x, y, num=2, encoded=True)
    assert ends.shape == (2, 2, 3, 4, 4)
    assert torch.equal(ends[:, 0], dif.decode(net, x)) and torch.equal(ends[:, 1], dif.decode(net, y))
    assert not torch.equal(dif.decode(net, 3 * x, clip_denoised=True), dif.decode(net, 3 * x, clip_denoised=False))


def test_slerp_function_against_float64(emu):
    g = torch.Generator().manual_seed(4)
    a, b = torch.randn(3, 2, 5, 7, generator=g), torch.randn(3, 2, 5, 7, generator=g)
    b[1] = a[1]                                                                            # parallel pair: the linear branch
    al = [0.0, 0.3, 1.0]
    out = ddim.slerp(a, b, al)
    ref = R.slerp(a, b, al)
    assert out.shape == (3, 3, 2, 5, 7)
    assert float((out.double() - ref).abs().max()) <= 1e-5 * float(torch.maximum(a.abs().max(), b.abs().max()))
    assert torch.allclose(out[1, 1], a[1], rtol=3e-7, atol=0) and torch.equal(out[:, 0], a) and torch.equal(out[:, 2], b)
    assert ddim.slerp(a[:0], b[:0], al).shape == (0, 3, 2, 5, 7)
    with pytest.raises(ValueError):
        ddim.slerp(a, b[:2], al)


# ------------------------------------------------------------------------------------------------------------------ generate.py
TINY_CFG = {
    "dataset": "cifar10",
    "diffusion": {"timesteps": 40, "beta_start": 1e-4, "beta_end": 0.02, "beta_schedule": "linear", "model_mean_type": "eps",
                  "model_var_type": "fixed-large", "loss_type": "mse"},
    "model": {"in_channels": 3, "hid_channels": 32, "ch_multipliers": [1, 2], "num_res_blocks": 1, "apply_attn": [False, True], "drop_rate": 0.1},
    "train": {"lr": 2e-4, "batch_size": 4, "grad_norm": 1.0, "epochs": 1, "warmup": 10, "use_ema": True, "ema_decay": 0.9999},
}


def _import_cli(name):
    import importlib
    return importlib.import_module(name)


def _files(folder):
    return {os.path.basename(f): open(f, "rb").read() for f in sorted(glob.glob(os.path.join(folder, "*.png")))}


def test_generate_interpolate_and_reconstruct_end_to_end(emu, tmp_path, monkeypatch, capsys):
    cfg = tmp_path / "tiny.json"
    cfg.write_text(json.dumps(TINY_CFG))
    monkeypatch.setenv("DDPM_TORCH_AMD_SYNTHETIC_DATA", "8")
    monkeypatch.chdir(tmp_path)
    train = _import_cli("train")
    train.main(["--config-path", str(cfg), "--train-device", "cpu", "--dry-run", "--num-samples", "0", "--num-workers", "0", "--compute", "fp32",
                "--chkpt-dir", str(tmp_path / "chk"), "--image-dir", str(tmp_path / "img")])
    chk = str(tmp_path / "chk" / "tiny" / "tiny_1.pt")
    gen = _import_cli("generate")
    common = ["--config-path", str(cfg), "--device", "cpu", "--chkpt-path", chk, "--use-ddim", "--subseq-size", "4", "--compute", "fp32"]
    from PIL import Image
    # drawn latents: 3 pairs, 5 columns, --batch-size 10 -> two pairs per chain
    runs = []
    for name in ("a", "b"):
        out = gen.main(common + ["--interpolate", "5", "--total-size", "3", "--batch-size", "10", "--seed", "7", "--save-dir", str(tmp_path / name)])
        runs.append(_files(out))
    assert sorted(runs[0]) == ["interp_00000.png", "interp_00001.png", "interp_00002.png"] and runs[0] == runs[1]
    assert Image.open(os.path.join(out, "interp_00000.png")).size == (5 * 34 + 2, 36)
    other = _files(gen.main(common + ["--interpolate", "5", "--total-size", "1", "--batch-size", "10", "--seed", "8", "--save-dir", str(tmp_path / "c")]))
    assert other["interp_00000.png"] != runs[0]["interp_00000.png"]
    # images: a uint8 tensor file of 4 -> 2 pairs encoded, and each reconstructed
    src = tmp_path / "src.pt"
    torch.save(torch.randint(0, 256, (4, 3, 32, 32), dtype=torch.uint8, generator=torch.Generator().manual_seed(0)), src)
    out = gen.main(common + ["--interpolate", "3", "--source", str(src), "--batch-size", "4", "--save-dir", str(tmp_path / "d")])
    assert sorted(_files(out)) == ["interp_00000.png", "interp_00001.png"]
    assert "ddpm_ddim_encode_step" in emu.log and "ddpm_slerp" in emu.log
    capsys.readouterr()
    recs = []
    for name in ("e", "f"):
        out = gen.main(common + ["--reconstruct", "--source", str(src), "--batch-size", "3", "--save-dir", str(tmp_path / name)])
        recs.append(_files(out))
    assert sorted(recs[0]) == [f"recon_{i:05d}.png" for i in range(4)] and recs[0] == recs[1]
    assert Image.open(os.path.join(out, "recon_00000.png")).size == (2 * 34 + 2, 36)
    printed = capsys.readouterr().out
    assert "mean squared error per dimension" in printed and float(printed.strip().split()[-1]) >= 0.0
    # a folder of pictures reads like the tensor file
    folder = tmp_path / "pics"
    folder.mkdir()
    data = torch.load(src)
    for i in range(2):
        Image.fromarray(data[i].permute(1, 2, 0).numpy()).save(folder / f"{i}.png")
    assert torch.equal(gen.load_source(str(folder), (3, 32, 32)), data[:2].float() / 127.5 - 1.0)
    # refusals go through parser.error
    for bad in (["--interpolate", "5"],                                                    # no --use-ddim
                ["--use-ddim", "--eta", "0.5", "--interpolate", "5"],
                ["--use-ddim", "--reconstruct"],                                            # no --source
                ["--use-ddim", "--source", str(src)]):
        with pytest.raises(SystemExit) as e:
            gen.main(["--config-path", str(cfg), "--device", "cpu", "--chkpt-path", chk] + bad)
        assert e.value.code == 2


# ------------------------------------------------------------------------------------------------------------------ the real library
def test_argument_validation_of_the_two_entries_without_a_gpu():
    """Only refused calls: a call that passes validation would launch on these fake addresses wherever a GPU is present."""
    lib = _hip.lib()
    f = 0x10000
    enc = lambda *a: lib.ddpm_ddim_encode_step(*a)                                          # noqa: E731
    assert enc(0, f, f, f, f, f, f, f, 0, 2, 8, 50, 0) == 5 and enc(f, f, f, f, f, f, f, 0, 0, 2, 8, 50, 0) == 5
    assert enc(f, f, 0, f, f, f, f, f, 0, 2, 8, 50, 0) == 5 and enc(f, f, f, 0, f, f, f, f, 0, 2, 8, 50, 0) == 5
    for B, n, S in ((0, 8, 50), (2, 0, 50), (2, 8, 0), (-1, 8, 50), (65536, 8, 50)):
        assert enc(f, f, f, f, f, f, f, f, 0, B, n, S, 0) == 1
    assert enc(f + 2, f, f, f, f, f, f, f, 0, 2, 8, 50, 0) == 3 and enc(f, f, f, f, f, f, f, f + 1, 0, 2, 8, 50, 0) == 3
    assert enc(f, f, f, f, f, f, f, f, f + 2, 2, 8, 50, 0) == 3 and enc(f, f, f + 4, f, f, f, f, f, 0, 2, 8, 50, 0) == 3
    assert lib.ddpm_slerp(0, f, f, f, f, 1, 1, 8, 0) == 5 and lib.ddpm_slerp(f, f, f, f, 0, 1, 1, 8, 0) == 5
    for P, K, n in ((0, 1, 8), (1, 0, 8), (1, 1, 0), (65536, 1, 8)):
        assert lib.ddpm_slerp(f, f, f, f, f, P, K, n, 0) == 1
    assert lib.ddpm_slerp(f, f + 2, f, f, f, 1, 1, 8, 0) == 3 and lib.ddpm_slerp(f, f, f, f + 1, f, 1, 1, 8, 0) == 3
    ws = lib.ddpm_slerp_workspace_floats
    assert ws(0, 100) == 0 and ws(3, 0) == 0 and ws(-1, 5) == -1 and ws(5, -1) == -1
    assert ws(1, 1) == 6 and ws(1, 2048) == 6 and ws(1, 2049) == 12 and ws(64, 12288) == 6 * 64 * 6 and ws(3, 196607) == 6 * 3 * 96
    for P, n in ((0, 100), (1, 2048), (1, 2049), (3, 196607)):
        assert ws(P, n) == ddim_emulator.slerp_workspace_floats(P, n)
    # the plan executor knows the launching entries by their declared arity, and refuses to record the size query
    assert lib.ddpm_plan_entry_arity(b"ddpm_ddim_encode_step") == 13 and lib.ddpm_plan_entry_arity(b"ddpm_slerp") == 9
    import ctypes
    h = ctypes.c_void_p(lib.ddpm_plan_create())
    words = (ctypes.c_ulonglong * 2)(1, 1)
    assert lib.ddpm_plan_append(h, b"ddpm_slerp_workspace_floats", ctypes.cast(words, ctypes.c_void_p), 2) == -1
    assert lib.ddpm_plan_destroy(h) == 0
