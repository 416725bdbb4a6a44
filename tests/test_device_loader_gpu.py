"""-m gpu: the device-resident data path end to end on the real C ABI — ``get_dataloader(device=)`` yields device batches that equal the
numpy restatement (tests/batch_emulator.py) bit for bit, in torch's order, with other orders and flips in the next epoch;
``train.py --device-data --dry-run`` reaches the direct step; and a Trainer fed by the device loader sees the batches and computes the
first loss of one fed by the host loader, bit for bit (flip-free data: the host path draws its flips from the global generator, the
device path from a hash)."""
import json

import numpy as np
import torch
import pytest
from torch.utils.data import DataLoader

import ddpm_torch
from ddpm_torch import datasets as D
from tests import batch_emulator as BE
from tests.test_cli_gpu import CFG, _cli
from tests.test_odd_geometry_gpu import REDUCED
from tests.test_unet_gpu import DEV, make

pytestmark = pytest.mark.gpu


def test_get_dataloader_on_the_device_equals_the_restatement(tmp_path):
    n, batch = 37, 8
    data = torch.randint(0, 256, (n, 3, 32, 32), dtype=torch.uint8, generator=torch.Generator().manual_seed(0))
    torch.save(data, tmp_path / "cifar10.pt")
    loader, sampler = ddpm_torch.get_dataloader("cifar10", batch, "train", root=str(tmp_path), random_seed=1234, device=DEV)
    assert isinstance(loader, ddpm_torch.DeviceLoader) and sampler is None and len(loader) == 5
    assert loader.data.is_cuda and loader.data.dtype == torch.uint8
    lut = D.TensorImages(torch.arange(256, dtype=torch.uint8).view(1, 1, 1, 256))[0].reshape(256).numpy()
    orders, flips = [], []
    for epoch in range(2):
        torch.manual_seed(50 + epoch)
        want_order = [b.tolist() for b in DataLoader(range(n), batch_size=batch, shuffle=True)]
        torch.manual_seed(50 + epoch)
        got = list(loader)
        assert [len(b) for b in got] == [8, 8, 8, 8, 5]
        seed = BE.epoch_seed(1234, epoch)
        for x, idx in zip(got, want_order):
            assert x.is_cuda and x.dtype == torch.float32 and x.is_contiguous()
            assert np.array_equal(x.cpu().numpy(), BE.gather(data.numpy(), idx, lut, 1, seed)), (epoch, idx)
        orders.append(want_order)
        flips.append(BE.flip_bits(seed, np.arange(n)))
        assert flips[-1].any() and not flips[-1].all()
    assert orders[0] != orders[1] and (flips[0] != flips[1]).any()


def test_train_cli_with_device_data_takes_the_direct_step(tmp_path, monkeypatch):
    cfg = tmp_path / "tiny.json"
    cfg.write_text(json.dumps(CFG))
    monkeypatch.setenv("DDPM_TORCH_AMD_SYNTHETIC_DATA", "8")
    monkeypatch.chdir(tmp_path)
    tr = _cli("train").main(["--config-path", str(cfg), "--train-device", DEV, "--device-data", "--dry-run", "--num-samples", "0",
                             "--num-workers", "0", "--compute", "fp32", "--chkpt-dir", str(tmp_path / "chk"), "--image-dir", str(tmp_path / "img")])
    assert isinstance(tr.trainloader, ddpm_torch.DeviceLoader) and tr.trainloader.data.is_cuda
    assert int(next(iter(tr.optimizer.state.values()))["step"]) == 1
    assert tr._direct, "the dry run must have gone through the direct (C-ABI) step"
    assert (tmp_path / "chk" / "tiny" / "tiny_1.pt").exists()


def test_trainer_losses_do_not_depend_on_which_loader_feeds_it():
    """Two Trainers from the same seeds, one fed by the host loader and one by the device loader.  What is a pure function of the seeds
    is bit-equal: the batches of both steps, and the loss of step 1 (same parameters, same batch, same t and noise draws, a forward
    without atomics).  The loss of step 2 is held to rel 2e-3, the bound tests/test_configs_gpu.py holds two runs of one Trainer to:
    Trainer.step is not bit-reproducible — weight-gradient split-K slices, GroupNorm's dgamma / dbeta, the bias column sums and the
    accumulating GEMM epilogue add with fp32 atomics (profiles/knob_retirement.txt: also with DDPM_WGRAD_SLABS=1) — so the parameters after
    step 1 differ in their last bits from run to run whatever feeds the step, and the next loss with them (observed: 1.8319735527038574
    against 1.8319733142852783, 1.3e-7 relative, on bit-equal batches)."""
    data = torch.randint(0, 256, (12, 3, 16, 48), dtype=torch.uint8, generator=torch.Generator().manual_seed(2))
    images = D.TensorImages(data, flip=False)
    loaders = {"host": lambda: DataLoader(images, batch_size=4, shuffle=True, drop_last=True),
               "device": lambda: ddpm_torch.DeviceLoader(images, 4, DEV, shuffle=True, drop_last=True)}
    losses, batches = {}, {}
    for name, build in loaders.items():
        m, _ = make(REDUCED)
        m.train()
        dif = ddpm_torch.GaussianDiffusion(ddpm_torch.get_beta_schedule("linear", 1e-4, 0.02, 1000), "eps", "fixed-large", "mse")
        tr = ddpm_torch.Trainer(m, torch.optim.Adam(m.parameters(), lr=2e-4), dif, epochs=1, trainloader=build(), use_ema=True, grad_norm=1.0,
                                shape=(3, 16, 48), device=torch.device(DEV))
        torch.manual_seed(7)
        losses[name], batches[name] = [], []
        for step, x in zip(range(2), tr.trainloader):
            batches[name].append(x.cpu())
            tr.stats.reset()
            tr.step(x, global_steps=step + 1)
            losses[name].append(tr.current_stats["loss"])
        assert tr._direct
    print(f"\nlosses host {losses['host']} device {losses['device']}")
    assert len(batches["host"]) == len(batches["device"]) == 2
    assert all(torch.equal(a, b) for a, b in zip(batches["host"], batches["device"]))
    assert not torch.equal(batches["host"][0], batches["host"][1])
    assert all(np.isfinite(losses["host"])) and losses["host"][0] == losses["device"][0]
    assert losses["device"][1] == pytest.approx(losses["host"][1], rel=2e-3)
