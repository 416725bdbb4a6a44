"""CPU: ``ddpm_torch.datasets.DeviceLoader`` / ``get_dataloader(device=)`` on the emulated C ABI (tests/abi_emulator.py +
tests/batch_emulator.py): the order of the batches is the host ``DataLoader``'s, the values are the host transform's bit for bit, the
flips are the counter hash's and depend on (seed, epoch, data-set index) alone, and a batch costs exactly one ``ddpm_batch_gather``.
The kernel itself is held to the same restatement on the GPU (tests/test_batch_gpu.py, tests/test_device_loader_gpu.py).

The flip-hash bounds are conditions fixed in advance, [0.45, 0.55] for a share over 4096 indices (binomial sd 0.008); measured for the
seeds below: flipped share 0.487 to 0.507, agreement between consecutive epochs 0.497."""
import os
import struct

import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader, Dataset
from torch.utils.data.distributed import DistributedSampler

import ddpm_torch
from ddpm_torch import _hip
from ddpm_torch import datasets as D
from tests import abi_emulator
from tests import batch_emulator as BE
from tests.test_datasets import _write_cifar

pytestmark = pytest.mark.skipif(not os.path.exists(_hip.LIB_PATH), reason="libddpm_hip.so not built")
N, B = 37, 8                                         # a ragged tail of 5


@pytest.fixture
def emu(monkeypatch):
    monkeypatch.delenv("DDPM_TORCH_AMD_SYNTHETIC_DATA", raising=False)
    return BE.attach(abi_emulator.install(monkeypatch, _hip))


def images(n=N, shape=(3, 32, 32), seed=0):
    """Random uint8 images whose first row of channel 0 is the image's own index in every column: a flip leaves it alone, so a yielded
    sample names the image it came from (``ids``)."""
    t = torch.randint(0, 256, (n,) + shape, dtype=torch.uint8, generator=torch.Generator().manual_seed(seed))
    t[:, 0, 0, :] = torch.arange(n, dtype=torch.uint8)[:, None]
    return t


def ids(batch):
    return ((batch[:, 0, 0, 0].double() + 1) * 127.5).round().long().tolist()


def host(x):
    """The host loader's value of a uint8 image (TensorImages' own rounding chain, flip off)."""
    return D.TensorImages(x[None])[0]


def index_batches(n, batch_size, seed, shuffle=False, sampler=None, drop_last=False):
    """What torch yields for these arguments: the definition of the order."""
    torch.manual_seed(seed)
    return [b.tolist() for b in DataLoader(range(n), batch_size=batch_size, shuffle=shuffle, sampler=sampler, drop_last=drop_last)]


def both(tmp_path, data, name="cifar10", **kw):
    torch.save(data, tmp_path / f"{name}.pt")
    h, hs = D.get_dataloader(name, root=str(tmp_path), **kw)
    d, ds = D.get_dataloader(name, root=str(tmp_path), device="cpu", **kw)
    assert isinstance(d, ddpm_torch.DeviceLoader) and type(h) is DataLoader
    return h, hs, d, ds


def epoch_of(loader, seed):
    torch.manual_seed(seed)
    return list(loader)


@pytest.mark.parametrize("drop_last", [False, True])
@pytest.mark.parametrize("split", ["train", "test"])                   # shuffled / in order
def test_order_is_the_host_loaders(emu, tmp_path, split, drop_last):
    data = images()
    h, _, d, sampler = both(tmp_path, data, batch_size=B, split=split, drop_last=drop_last, random_seed=3)
    assert sampler is None and len(d) == len(h) == (4 if drop_last else 5)
    for epoch in range(2):
        want = index_batches(N, B, 100 + epoch, shuffle=split == "train", drop_last=drop_last)
        got_h = [ids(b) for b in epoch_of(h, 100 + epoch)]
        got_d = [ids(b) for b in epoch_of(d, 100 + epoch)]
        assert got_d == got_h == want
        assert [len(b) for b in got_d] == [8, 8, 8, 8] + ([] if drop_last else [5])
    if split == "train":
        assert got_d != sorted(got_d) and want != index_batches(N, B, 100, shuffle=True, drop_last=drop_last)    # shuffled, anew per epoch


@pytest.mark.parametrize("split", ["train", "valid"])
def test_order_with_a_validation_split(emu, tmp_path, split):
    data = images()
    h, _, d, _ = both(tmp_path, data, batch_size=B, split=split, val_size=10, random_seed=11)
    perm = torch.randperm(N, generator=torch.Generator().manual_seed(11))
    part = perm[10:] if split == "train" else perm[:10]
    assert len(d) == len(h) == -(-len(part) // B)
    want = [part[torch.tensor(b)].tolist() for b in index_batches(len(part), B, 5, shuffle=split == "train")]
    assert [ids(b) for b in epoch_of(d, 5)] == [ids(b) for b in epoch_of(h, 5)] == want
    flat = sorted(i for b in want for i in b)
    assert flat == sorted(part.tolist())


def _as_rank(monkeypatch, rank, world=2):
    monkeypatch.setenv("WORLD_SIZE", str(world))
    monkeypatch.setattr(torch.distributed, "get_world_size", lambda *a, **k: world)
    monkeypatch.setattr(torch.distributed, "get_rank", lambda *a, **k: rank)


@pytest.mark.parametrize("rank", [0, 1])
def test_order_with_a_distributed_sampler(emu, tmp_path, monkeypatch, rank):
    _as_rank(monkeypatch, rank)
    data = images()
    h, hs, d, ds = both(tmp_path, data, batch_size=B, split="train", distributed=True, random_seed=21)
    assert isinstance(ds, DistributedSampler) and d.batch_size == B // 2 and len(d) == len(h) == 5          # 19 per rank in batches of 4
    seen = []
    for epoch in (0, 3):                                                   # before and after set_epoch
        if epoch:
            hs.set_epoch(epoch), ds.set_epoch(epoch)
        ref = DistributedSampler(range(N), num_replicas=2, rank=rank, shuffle=True, seed=21)
        ref.set_epoch(epoch)
        want = index_batches(N, B // 2, 0, sampler=ref)
        assert [ids(b) for b in epoch_of(d, 0)] == [ids(b) for b in epoch_of(h, 0)] == want
        seen.append(want)
    assert seen[0] != seen[1]


def _check_values(data, batches, order, seed_word, flip, expect_both):
    """Every sample is the host value of its image, mirrored exactly where the hash says."""
    assert [len(b) for b in batches] == [len(o) for o in order]
    for batch, idx in zip(batches, order):
        assert batch.dtype == torch.float32 and tuple(batch.shape[1:]) == tuple(data.shape[1:])
        bits = BE.flip_bits(seed_word, np.asarray(idx)) if flip else np.zeros(len(idx), dtype=bool)
        if expect_both:
            assert bits.any() and not bits.all(), (idx, bits)
        for x, i, f in zip(batch, idx, bits):
            want = host(data[i])
            assert torch.equal(x, want.flip(-1) if f else want), (i, f)
            assert not torch.equal(want, want.flip(-1))


def test_values_and_flips_follow_the_hash(emu, tmp_path):
    data = images(seed=1)
    _, _, d, _ = both(tmp_path, data, batch_size=B, split="train", drop_last=True, random_seed=1234)
    flips = []
    for epoch in range(2):                                                 # no sampler: the epoch is the number of earlier iter() calls
        order = index_batches(N, B, 40 + epoch, shuffle=True, drop_last=True)
        batches = epoch_of(d, 40 + epoch)
        _check_values(data, batches, order, BE.epoch_seed(1234, epoch), True, expect_both=True)
        flips.append(BE.flip_bits(BE.epoch_seed(1234, epoch), np.arange(N)))
    assert (flips[0] != flips[1]).any()
    assert emu.log == ["ddpm_batch_gather"] * (2 * len(d))               # one launch per batch and nothing else


def test_without_flips_the_batches_are_the_host_loaders_bit_for_bit(emu, tmp_path):
    data = images(seed=2)
    h, _, d, _ = both(tmp_path, data, batch_size=B, split="test", random_seed=9)            # cifar10 flips, but not its test split
    for a, b in zip(epoch_of(h, 0), epoch_of(d, 0), strict=True):
        assert torch.equal(a, b)
    grey = images(shape=(1, 32, 32), seed=3)
    for stored in (grey, grey.float().div(127.5).sub(1.0)):                                 # mnist never flips; uint8 and float32 sources
        h, _, d, _ = both(tmp_path, stored, name="mnist", batch_size=B, split="train")
        for a, b in zip(epoch_of(h, 6), epoch_of(d, 6), strict=True):
            assert torch.equal(a, b)
    assert set(emu.log) == {"ddpm_batch_gather"}


SEEDS = [0, 1, 1234 << 32, 1234 << 32 | 1, 1234 << 32 | 7, 0x9E3779B97F4A7C15]


def test_flip_hash_is_balanced_and_independent_between_epochs():
    index = np.arange(4096)
    for seed in SEEDS:
        share = float(BE.flip_bits(seed, index).mean())
        print(f"seed {seed:#x}: flipped share {share:.3f}")
        assert 0.45 <= share <= 0.55, (seed, share)
    for epoch in (0, 1, 7):
        a, b = (BE.flip_bits(BE.epoch_seed(1234, e), index) for e in (epoch, epoch + 1))
        agree = float((a == b).mean())
        print(f"epochs {epoch}, {epoch + 1}: agreement {agree:.3f}")
        assert 0.45 <= agree <= 0.55, (epoch, agree)
    assert BE.epoch_seed(1234, 7) == 1234 << 32 | 7 and BE.epoch_seed(None, 2) == 2


def test_flips_do_not_depend_on_the_world_size(emu, tmp_path, monkeypatch):
    data = images(seed=4)

    def flipped(loader, seed):
        out = {}
        for batch in epoch_of(loader, seed):
            for x, i in zip(batch, ids(batch)):
                f = not torch.equal(x, host(data[i]))
                assert torch.equal(x, host(data[i]).flip(-1) if f else host(data[i]))
                assert out.setdefault(i, f) == f                          # (the sampler pads 37 to 38: one image comes twice)
        return out

    _, _, single, _ = both(tmp_path, data, batch_size=B, split="train", random_seed=77)
    one = [flipped(single, 1), flipped(single, 2)]                        # epochs 0 and 1
    two = [{}, {}]
    for rank in (0, 1):
        _as_rank(monkeypatch, rank)
        _, _, d, ds = both(tmp_path, data, batch_size=B, split="train", distributed=True, random_seed=77)
        for epoch in (0, 1):
            ds.set_epoch(epoch)
            two[epoch].update(flipped(d, 5))
    for epoch in (0, 1):
        assert sorted(one[epoch]) == sorted(two[epoch]) == list(range(N))
        assert one[epoch] == two[epoch]
        assert [one[epoch][i] for i in range(N)] == BE.flip_bits(BE.epoch_seed(77, epoch), np.arange(N)).tolist()
    assert one[0] != one[1]


def test_cifar10_from_its_pickle_directory(emu, tmp_path):
    _write_cifar(tmp_path / "cifar-10-batches-py", np.random.RandomState(6))
    raw = D.CIFAR10(root=str(tmp_path), split="train", transform=None)
    d, _ = D.get_dataloader("cifar10", 4, "train", root=str(tmp_path), device="cpu", random_seed=5)
    assert d.data.dtype == torch.uint8 and tuple(d.data.shape) == (20, 3, 32, 32) and d.flip and len(d) == 5
    order = index_batches(20, 4, 8, shuffle=True)
    seen = 0
    for batch, idx in zip(epoch_of(d, 8), order, strict=True):
        bits = BE.flip_bits(BE.epoch_seed(5, 0), np.asarray(idx))
        seen += int(bits.sum())
        for x, i, f in zip(batch, idx, bits):
            want = D._to_unit(raw[i])                                      # ToTensor + Normalize(0.5, 0.5), this class's chain
            assert torch.equal(x, want.flip(-1) if f else want)
    assert 0 < seen < 20
    t, _ = D.get_dataloader("cifar10", 4, "test", root=str(tmp_path), device="cpu")
    assert not t.flip and len(t.data) == 4


def test_mnist_from_its_idx_file(emu, tmp_path):
    rng = np.random.RandomState(0)
    folder = tmp_path / "MNIST" / "raw"
    folder.mkdir(parents=True)
    (folder / "train-images-idx3-ubyte").write_bytes(struct.pack(">IIII", 2051, 11, 28, 28) + rng.randint(0, 256, (11, 28, 28), dtype=np.uint8).tobytes())
    h, _ = D.get_dataloader("mnist", 4, "train", root=str(tmp_path))
    d, _ = D.get_dataloader("mnist", 4, "train", root=str(tmp_path), device="cpu")
    assert d.data.dtype == torch.uint8 and tuple(d.data.shape) == (11, 1, 32, 32) and not d.flip        # resized once, at construction
    for a, b in zip(epoch_of(h, 2), epoch_of(d, 2), strict=True):
        assert torch.equal(a, b)
    assert [len(b) for b in epoch_of(d, 2)] == [4, 4, 3]


def test_two_live_iterators_are_two_epochs(emu, tmp_path):
    """As with a DataLoader: a second iter() does not disturb the first (Trainer.__init__ peeks at one batch when it is given no shape)."""
    data = images(seed=5)
    _, _, d, _ = both(tmp_path, data, batch_size=B, split="train", random_seed=6)
    torch.manual_seed(1)
    first = iter(d)
    head = next(first)
    torch.manual_seed(2)
    second = list(d)
    rest = list(first)
    want = [index_batches(N, B, 1, shuffle=True), index_batches(N, B, 2, shuffle=True)]
    _check_values(data, [head] + rest, want[0], BE.epoch_seed(6, 0), True, expect_both=False)
    _check_values(data, second, want[1], BE.epoch_seed(6, 1), True, expect_both=False)


def test_refusals(emu, tmp_path):
    torch.save(images(), tmp_path / "cifar10.pt")
    with pytest.raises(ValueError, match="raw"):
        D.get_dataloader("cifar10", B, "train", root=str(tmp_path), raw=True, device="cpu")

    class Other(Dataset):
        def __len__(self):
            return 3

        def __getitem__(self, i):
            return torch.zeros(3, 8, 8)

    with pytest.raises(TypeError, match="Other"):
        ddpm_torch.DeviceLoader(Other(), 2, "cpu")
    with pytest.raises(TypeError):
        ddpm_torch.DeviceLoader(D.TensorImages(torch.zeros(3, 1, 8, 8, dtype=torch.float64)), 2, "cpu")
    with pytest.raises(TypeError):
        ddpm_torch.DeviceLoader(D.TensorImages(images(), raw=True), 2, "cpu")


def test_without_the_emulator_a_host_tensor_is_refused(tmp_path):
    """No fallback: the loader is for a GPU, and says so at construction."""
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ddpm_torch.DeviceLoader(D.TensorImages(images()), 2, "cpu")
