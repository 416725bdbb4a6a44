"""-m gpu: the command-line counterparts (reference train.py:141-144, generate.py:72-93,128) end to end ON THE
DEVICE through the real C ABI: `train.py --dry-run` -> checkpoint -> resume -> `generate.py` -> PNG files, and the forward of the
re-loaded EMA weights against the oracle."""
import glob
import importlib
import json
import os
import sys

import pytest
import torch

from oracle import unet_ref as U

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "ddpm-torch_amd")
DEV = "cuda:0"

CFG = {
    "dataset": "cifar10",
    "diffusion": {"timesteps": 40, "beta_start": 1e-4, "beta_end": 0.02, "beta_schedule": "linear", "model_mean_type": "eps",
                  "model_var_type": "fixed-large", "loss_type": "mse"},
    "model": {"in_channels": 3, "hid_channels": 32, "ch_multipliers": [1, 2], "num_res_blocks": 1, "apply_attn": [False, True], "drop_rate": 0.1},
    "train": {"lr": 2e-4, "batch_size": 4, "grad_norm": 1.0, "epochs": 1, "warmup": 10, "use_ema": True, "ema_decay": 0.9999},
}


def _cli(name):
    if PKG not in sys.path:
        sys.path.insert(0, PKG)
    return importlib.import_module(name)


@pytest.mark.parametrize("compute", ["fp32", "bf16"])
def test_train_dry_run_checkpoint_generate_on_device(tmp_path, monkeypatch, compute):
    cfg = tmp_path / "tiny.json"
    cfg.write_text(json.dumps(CFG))
    monkeypatch.setenv("DDPM_TORCH_AMD_SYNTHETIC_DATA", "8")
    monkeypatch.chdir(tmp_path)
    train, gen = _cli("train"), _cli("generate")
    tr = train.main(["--config-path", str(cfg), "--train-device", DEV, "--dry-run", "--num-samples", "4", "--num-workers", "0",
                     "--compute", compute, "--chkpt-dir", str(tmp_path / "chk"), "--image-dir", str(tmp_path / "img")])
    assert tr.ema.num_updates == 0 and int(next(iter(tr.optimizer.state.values()))["step"]) == 1          # exactly one update
    assert next(tr.model.parameters()).is_cuda and tr._direct, "the dry run must have gone through the direct (C-ABI) step"
    chk = tmp_path / "chk" / "tiny" / "tiny_1.pt"
    assert chk.exists() and (tmp_path / "img" / "train" / "tiny" / "1.jpg").exists()
    saved = torch.load(chk, map_location="cpu", weights_only=False)
    assert set(saved) >= {"model", "optimizer", "ema", "scheduler", "epoch"} and saved["epoch"] == 1
    assert list(saved["model"]) == list(U.init_state_dict(dict(CFG["model"], out_channels=3)))             # reference key order (Appendix B)
    moved = max(float((saved["model"][k] - saved["ema"]["shadow"][k]).abs().max()) for k in saved["ema"]["shadow"])
    assert 0 < moved < 1e-2                                      # one Adam step at lr 2e-5 (warm-up) away from the shadow's initial copy
    # resume on the device: epoch counter, EMA counter and Adam state come back, and the next step runs
    tr2 = train.main(["--config-path", str(cfg), "--train-device", DEV, "--dry-run", "--num-samples", "0", "--resume", "--num-workers", "0",
                      "--compute", compute, "--chkpt-path", str(chk), "--chkpt-dir", str(tmp_path / "chk2"), "--image-dir", str(tmp_path / "img2")])
    assert tr2.ema.num_updates == 1 and int(next(iter(tr2.optimizer.state.values()))["step"]) == 2
    # generate.py: EMA shadow preferred, frozen model, PNG files; --seed makes whole chains repeat
    outs = []
    for rep in range(2):
        out = gen.main(["--config-path", str(cfg), "--device", DEV, "--chkpt-path", str(chk), "--total-size", "5", "--batch-size", "4",
                        "--save-dir", str(tmp_path / f"gen{rep}"), "--compute", compute, "--seed", "7"])
        files = sorted(glob.glob(os.path.join(out, "*.png")))
        assert len(files) == 5
        from PIL import Image
        import numpy as np
        imgs = np.stack([np.asarray(Image.open(f)) for f in files])
        assert imgs.shape == (5, 32, 32, 3) and imgs.std() > 0
        outs.append(np.sort(imgs.reshape(5, -1).astype(np.int64).sum(1)))        # file names are random uuids: compare as a multiset
    assert (outs[0] == outs[1]).all()
    # the re-loaded EMA weights, forward on the device vs the oracle on the host
    process, model, device, shape, _ = gen.build(gen.parse_args(["--config-path", str(cfg), "--device", DEV, "--chkpt-path", str(chk), "--compute", compute]))
    assert not any(p.requires_grad for p in model.parameters()) and not model.training
    sd = {k: v.cpu() for k, v in saved["ema"]["shadow"].items()}
    g = torch.Generator().manual_seed(3)
    x, t = torch.randn(2, 3, 32, 32, generator=g), torch.tensor([1, 38])
    with torch.no_grad():
        y = model(x.to(DEV), t.to(DEV)).cpu()
        ref = U.unet_forward(sd, dict(CFG["model"], out_channels=3), x, t, training=False)
    rel = float((y - ref).abs().max() / ref.abs().max())
    assert rel < (1e-3 if compute == "fp32" else 6e-2), rel


def test_block_size_and_accumulation_round_trip_on_device(tmp_path, monkeypatch):
    """``train.py --block-size 2 --num-accum 2 --dry-run`` -> resume -> ``generate.py`` in the bf16 compute mode: the 12 -> 12 UNet between
    PixelUnshuffle(2) and PixelShuffle(2), two micro-batches of batch_size // 2 per update through the generic step with the fused
    update, the sampler over the wrapped model (tests/test_cli_host.py holds the same round trip on the emulated ABI)."""
    cfg = tmp_path / "tiny.json"
    cfg.write_text(json.dumps(CFG))
    monkeypatch.setenv("DDPM_TORCH_AMD_SYNTHETIC_DATA", "8")
    monkeypatch.chdir(tmp_path)
    train, gen = _cli("train"), _cli("generate")
    common = ["--config-path", str(cfg), "--train-device", DEV, "--dry-run", "--block-size", "2", "--num-accum", "2", "--num-workers", "0",
              "--compute", "bf16"]
    tr = train.main(common + ["--num-samples", "4", "--chkpt-dir", str(tmp_path / "chk"), "--image-dir", str(tmp_path / "img")])
    unet = tr.model._model
    assert type(tr.model).__name__ == "ModelWrapper" and unet.in_channels == 12 and unet.out_channels == 12
    assert unet.compute_dtype == torch.bfloat16 and next(unet.parameters()).is_cuda
    assert tr.num_accum == 2 and not tr._direct, "a wrapped model accumulating gradients takes the generic step"
    assert tr.trainloader.batch_size == CFG["train"]["batch_size"] // 2
    assert tr.ema.num_updates == 0 and int(next(iter(tr.optimizer.state.values()))["step"]) == 1          # two calls, exactly one update
    rec = json.load(open(glob.glob(str(tmp_path / "chk" / "tiny" / "exp_*.info"))[0]))
    assert rec["model"]["block_size"] == 2 and rec["model"]["in_channels"] == 12 and rec["model"]["out_channels"] == 12
    chk = tmp_path / "chk" / "tiny" / "tiny_1.pt"
    assert chk.exists() and (tmp_path / "img" / "train" / "tiny" / "1.jpg").exists()
    saved = torch.load(chk, map_location="cpu", weights_only=False)
    assert all(k.startswith("_model.") for k in saved["model"]) and saved["model"]["_model.in_conv.weight"].shape == (32, 12, 3, 3)
    assert all(bool(torch.isfinite(v).all()) for v in saved["model"].values())
    moved = max(float((saved["model"][k] - saved["ema"]["shadow"][k]).abs().max()) for k in saved["ema"]["shadow"])
    assert 0 < moved < 1e-2                                      # one Adam step at lr 2e-5 (warm-up) away from the shadow's initial copy
    tr2 = train.main(common + ["--num-samples", "0", "--resume", "--chkpt-path", str(chk), "--chkpt-dir", str(tmp_path / "chk2"),
                               "--image-dir", str(tmp_path / "img2")])
    assert tr2.ema.num_updates == 1 and int(next(iter(tr2.optimizer.state.values()))["step"]) == 2
    gcfg = tmp_path / "tiny_block2.json"                         # generate.py takes the block size from the configuration
    gcfg.write_text(json.dumps(dict(CFG, model=dict(CFG["model"], block_size=2))))
    out = gen.main(["--config-path", str(gcfg), "--device", DEV, "--chkpt-path", str(chk), "--total-size", "5", "--batch-size", "4",
                    "--save-dir", str(tmp_path / "gen"), "--compute", "bf16", "--seed", "7"])
    files = sorted(glob.glob(os.path.join(out, "*.png")))
    assert len(files) == 5
    from PIL import Image
    import numpy as np
    imgs = np.stack([np.asarray(Image.open(f)) for f in files])
    assert imgs.shape == (5, 32, 32, 3) and imgs.std() > 0
    # the re-loaded EMA weights behind the wrapper, forward on the device vs the oracle between pixel-unshuffle and pixel-shuffle
    process, model, device, shape, _ = gen.build(gen.parse_args(["--config-path", str(gcfg), "--device", DEV, "--chkpt-path", str(chk), "--compute", "bf16"]))
    sd = {k[len("_model."):]: v.cpu() for k, v in saved["ema"]["shadow"].items()}
    g = torch.Generator().manual_seed(3)
    x, t = torch.randn(2, 3, 32, 32, generator=g), torch.tensor([1, 38])
    with torch.no_grad():
        y = model(x.to(DEV), t.to(DEV)).cpu()
        inner = U.unet_forward(sd, dict(CFG["model"], in_channels=12, out_channels=12), torch.nn.functional.pixel_unshuffle(x, 2), t, training=False)
        ref = torch.nn.functional.pixel_shuffle(inner, 2)
    rel = float((y - ref).abs().max() / ref.abs().max())
    assert rel < 6e-2, rel                                       # the bf16 bar of the 3-channel round trip above
