"""Data path behind the reference's names (``ddpm_torch/datasets.py:13-266`` of tqch/ddpm-torch).

The reference builds its loaders on torchvision dataset classes; torchvision is not part of this image and image decoding is outside
the accelerated hot path, so the four datasets are read from their ON-DISK FORMATS directly (numpy + PIL):

* ``MNIST``      ``<root>/MNIST/raw/{train,t10k}-images-idx3-ubyte[.gz]``, 28×28 → 32×32 bilinear (datasets.py:28-45);
* ``CIFAR10``    ``<root>/cifar-10-batches-py/{data_batch_1..5,test_batch}`` (pickled dicts, opened with a whitelist unpickler),
                 random horizontal flip in training form (:48-66);
* ``CelebA``     ``<root>/celeba/list_eval_partition.txt`` + ``img_align_celeba/``, crop (top 40, left 15, 148×148) → 64×64 bilinear,
                 flip (:69-153); splits train / valid / test / all;
* ``CelebA_HQ``  ``<root>/celeba_hq/img_celeba_hq/*.png`` in ProGAN's legacy order (numeric sort, ``RandomState(123).shuffle``), flip
                 (:156-198).

Every class yields one image per item and, by default, no label: a float ``[C, H, W]`` tensor in [-1, 1] (``ToTensor`` + ``Normalize(0.5, 0.5)``),
or — ``transform=None`` / ``raw=True``, what the evaluation code reads — the uint8 ``[C, H, W]`` tensor.  ``DATASET_INFO`` carries the
class constants (resolution, channels, split sizes) the CLIs size their models and sample grids from.  ``labels=True`` (class-conditional
training; not in the reference, whose loaders drop them) makes the readers whose format carries a class — MNIST's idx1 label files,
CIFAR-10's ``labels`` lists, a tensor file saved as ``{"images": ..., "labels": ...}``, the synthetic stand-in (``index % num_classes``) —
yield ``(image, label)`` pairs; a data set without classes raises ``ValueError``.

Two more sources exist for boxes without the datasets (this build container and the GPU box have neither the files nor a network):
a **tensor file** ``<root>/<dataset>[_<split>].pt`` (uint8 or [-1, 1] float ``[N, C, H, W]``; tried FIRST, it is also the fastest way to
feed a 10 ms training step) and, when ``DDPM_TORCH_AMD_SYNTHETIC_DATA=N`` is set, N seeded uniform images (smoke / dry runs).

``get_dataloader(dataset, batch_size, split, ...) -> (loader, sampler)`` keeps the reference's contract (:225-266): per-rank batch =
``batch_size // WORLD_SIZE`` when ``distributed``, ``DistributedSampler`` with per-epoch reshuffling, no shuffling for raw / test reads.
With ``device=`` it returns a ``DeviceLoader`` instead: the whole data set is put on the GPU once and every batch is assembled there by
one kernel (``ddpm_batch_gather``, csrc/batch.hip) in the order a host ``DataLoader`` would have drawn.
"""
import copy
import gzip
import io
import os
import pickle
import struct

import numpy as np
import torch
from torch.utils.data import DataLoader, Dataset, Subset
from torch.utils.data.distributed import DistributedSampler

from . import _hip

__all__ = ["DATASET_INFO", "DATASET_DICT", "get_dataloader", "DeviceLoader", "TensorImages", "MNIST", "CIFAR10", "CelebA", "CelebA_HQ", "ImageFolder"]

ROOT = os.path.expanduser("~/datasets")
DATASET_DICT, DATASET_INFO = {}, {}


def _register(cls):
    """``DATASET_DICT[name] = cls`` and the class's plain constants into ``DATASET_INFO[name]`` (datasets.py:17-26)."""
    name = cls.__name__.lower()
    DATASET_DICT[name] = cls
    DATASET_INFO[name] = {k: v for k, v in vars(cls).items() if not k.startswith("_") and not callable(v) and not isinstance(v, (staticmethod, classmethod, property))}
    return cls


def _pil():
    try:
        from PIL import Image
    except ImportError as e:                                                         # pragma: no cover
        raise RuntimeError("reading image files needs Pillow; use a tensor file (<root>/<dataset>.pt) instead") from e
    return Image


def _to_unit(x):
    """uint8 [C, H, W] -> float in [-1, 1] exactly as ToTensor + Normalize(0.5, 0.5) round: (x / 255 - 0.5) / 0.5."""
    return x.to(torch.float32).div_(255).sub_(0.5).div_(0.5)


class _Images(Dataset):
    """Common part: ``_load(i)`` -> uint8 [C, H, W]; ``transform=None`` (the reference's raw form) returns it, the default training form
    flips (where the reference's transform does) and normalises.  ``transform`` may also be any callable on the uint8 tensor."""
    flip = False
    num_classes = None                                         # classes of the on-disk labels; None: the format carries none

    def __init__(self, root=ROOT, split="train", transform="train", labels=False):
        self.root, self.split, self.transform = os.path.expanduser(root), split, transform
        if labels and self.num_classes is None:
            raise ValueError(f"{type(self).__name__} carries no class labels")
        self.labels = None                                     # int64 [N] when asked for (filled by the subclass): items are (image, label)

    def _load(self, index):
        raise NotImplementedError

    def _image(self, index):
        x = self._load(index)
        if self.transform is None:
            return x
        if callable(self.transform):
            return self.transform(x)
        if self.flip and torch.rand(1) < 0.5:                  # RandomHorizontalFlip: one uniform draw per image
            x = x.flip(-1)
        return _to_unit(x)

    def __getitem__(self, index):
        x = self._image(index)
        return x if self.labels is None else (x, int(self.labels[index]))


def _read_idx_images(path):
    opener = gzip.open if path.endswith(".gz") else open
    with opener(path, "rb") as f:
        magic, n, h, w = struct.unpack(">IIII", f.read(16))
        if magic != 2051:
            raise ValueError(f"{path}: not an idx3-ubyte image file (magic {magic})")
        data = np.frombuffer(f.read(n * h * w), dtype=np.uint8)
    if data.size != n * h * w:
        raise ValueError(f"{path}: truncated ({data.size} of {n * h * w} bytes)")
    return data.reshape(n, h, w)


def _read_idx_labels(path):
    opener = gzip.open if path.endswith(".gz") else open
    with opener(path, "rb") as f:
        magic, n = struct.unpack(">II", f.read(8))
        if magic != 2049:
            raise ValueError(f"{path}: not an idx1-ubyte label file (magic {magic})")
        data = np.frombuffer(f.read(n), dtype=np.uint8)
    if data.size != n:
        raise ValueError(f"{path}: truncated ({data.size} of {n} bytes)")
    return torch.from_numpy(data.astype(np.int64))


@_register
class MNIST(_Images):
    resolution = (32, 32)
    channels = 1
    train_size = 60000
    test_size = 10000
    num_classes = 10

    def __init__(self, root=ROOT, split="train", transform="train", labels=False):
        super().__init__(root, split, transform, labels)
        stem = "t10k" if split == "test" else "train"
        base = os.path.join(self.root, "MNIST", "raw", f"{stem}-images-idx3-ubyte")
        path = next((p for p in (base, base + ".gz") if os.path.exists(p)), None)
        if path is None:
            raise FileNotFoundError(base)
        self.data = _read_idx_images(path)
        if labels:
            base = os.path.join(self.root, "MNIST", "raw", f"{stem}-labels-idx1-ubyte")
            path = next((p for p in (base, base + ".gz") if os.path.exists(p)), None)
            if path is None:
                raise FileNotFoundError(base)
            self.labels = _read_idx_labels(path)
            if len(self.labels) != len(self.data):
                raise ValueError(f"{path}: {len(self.labels)} labels for {len(self.data)} images")

    def __len__(self):
        return len(self.data)

    def _load(self, index):
        Image = _pil()
        im = Image.fromarray(self.data[index]).resize(self.resolution[::-1], Image.BILINEAR)
        return torch.from_numpy(np.asarray(im, dtype=np.uint8).copy()).unsqueeze(0)


class _ArraysOnly(pickle.Unpickler):
    """The CIFAR batches are pickled dicts of lists, strings and one numpy array: nothing else is allowed to be constructed."""
    ALLOWED = {("numpy.core.multiarray", "_reconstruct"), ("numpy._core.multiarray", "_reconstruct"), ("numpy", "ndarray"), ("numpy", "dtype"),
               ("_codecs", "encode")}

    def find_class(self, module, name):
        if (module, name) not in self.ALLOWED:
            raise pickle.UnpicklingError(f"refusing to load {module}.{name} from a dataset file")
        return super().find_class(module, name)


@_register
class CIFAR10(_Images):
    resolution = (32, 32)
    channels = 3
    train_size = 50000
    test_size = 10000
    flip = True
    num_classes = 10

    def __init__(self, root=ROOT, split="train", transform="train", labels=False):
        super().__init__(root, split, transform, labels)
        folder = os.path.join(self.root, "cifar-10-batches-py")
        names = ["test_batch"] if split == "test" else [f"data_batch_{i}" for i in range(1, 6)]
        parts, classes = [], []
        for fn in names:
            path = os.path.join(folder, fn)
            if not os.path.exists(path):
                raise FileNotFoundError(path)
            with open(path, "rb") as f:
                entry = _ArraysOnly(io.BytesIO(f.read()), encoding="latin1").load()
            parts.append(np.asarray(entry["data"], dtype=np.uint8).reshape(-1, 3, 32, 32))
            if labels:
                classes.append(np.asarray(entry["labels"], dtype=np.int64))
        self.data = np.concatenate(parts)
        if labels:
            self.labels = torch.from_numpy(np.concatenate(classes))

    def __len__(self):
        return len(self.data)

    def _load(self, index):
        return torch.from_numpy(self.data[index].copy())


def _open_rgb(path):
    with _pil().open(path) as im:
        return im.convert("RGB") if im.mode != "RGB" else im.copy()


def _chw(im):
    return torch.from_numpy(np.asarray(im, dtype=np.uint8).copy()).permute(2, 0, 1).contiguous()


@_register
class CelebA(_Images):
    base_folder = "celeba"
    resolution = (64, 64)
    channels = 3
    all_size = 202599
    train_size = 162770
    val_size = 19867
    test_size = 19962
    flip = True

    def __init__(self, root=ROOT, split="train", transform="train", labels=False):
        super().__init__(root, split, transform, labels)
        want = {"train": 0, "valid": 1, "test": 2, "all": None}[split.lower()]
        part = os.path.join(self.root, self.base_folder, "list_eval_partition.txt")
        if not os.path.exists(part):
            raise FileNotFoundError(part)
        self.filename = []
        with open(part) as f:
            for line in f:
                fields = line.split()
                if len(fields) >= 2 and (want is None or int(fields[1]) == want):
                    self.filename.append(fields[0])

    def __len__(self):
        return len(self.filename)

    def _load(self, index):
        Image = _pil()
        im = _open_rgb(os.path.join(self.root, self.base_folder, "img_align_celeba", self.filename[index]))
        im = im.crop((15, 40, 15 + 148, 40 + 148)).resize(self.resolution[::-1], Image.BILINEAR)      # (left, top, right, bottom)
        return _chw(im)


@_register
class CelebA_HQ(_Images):
    base_folder = "celeba_hq"
    resolution = (256, 256)
    channels = 3
    all_size = 30000
    train_size = 24000                       # (this package's CLI reports progress against it; the reference trains on all 30000)
    flip = True

    def __init__(self, root=ROOT, split="train", transform="train", labels=False):
        super().__init__(root, split, transform, labels)     # split is unused, as in the reference
        folder = os.path.join(self.root, self.base_folder, "img_celeba_hq")
        if not os.path.isdir(folder):
            raise FileNotFoundError(folder)
        self.filename = sorted((fn for fn in os.listdir(folder) if fn.endswith(".png")), key=lambda fn: int(fn[:-4]))
        np.random.RandomState(123).shuffle(self.filename)      # legacy ProGAN order

    def __len__(self):
        return len(self.filename)

    def _load(self, index):
        return _chw(_open_rgb(os.path.join(self.root, self.base_folder, "img_celeba_hq", self.filename[index])))


class ImageFolder(Dataset):
    """Every image file of one folder as a uint8 [C, H, W] tensor — the generated samples ``eval.py`` scores (eval.py:56-70)."""
    EXT = {"jpg", "jpeg", "png", "bmp", "webp", "tiff"}

    def __init__(self, img_dir, transform=None):
        self.img_dir = img_dir
        self.img_list = sorted(fn for fn in os.listdir(img_dir) if fn.rsplit(".", 1)[-1].lower() in self.EXT)
        self.transform = transform

    def __len__(self):
        return len(self.img_list)

    def __getitem__(self, index):
        with _pil().open(os.path.join(self.img_dir, self.img_list[index])) as im:
            x = np.asarray(im, dtype=np.uint8)
        x = torch.from_numpy(x.copy())
        x = x.unsqueeze(0) if x.ndim == 2 else x.permute(2, 0, 1).contiguous()
        return x if self.transform is None else self.transform(x)


class TensorImages(Dataset):
    """Images held in one tensor; ``__getitem__`` returns a float image in [-1, 1], or the stored uint8 image when ``raw`` — and, with
    ``labels`` (int64 ``[N]``), the pair (image, label)."""

    def __init__(self, data, flip=False, raw=False, labels=None):
        assert data.ndim == 4, "expected [N, C, H, W]"
        self.data, self.flip, self.raw = data, flip, raw
        if labels is not None:
            labels = torch.as_tensor(labels).to(torch.int64)
            assert labels.shape == (data.shape[0],), "expected one label per image"
        self.labels = labels

    def __len__(self):
        return self.data.shape[0]

    def __getitem__(self, i):
        x = self._image(i)
        return x if self.labels is None else (x, int(self.labels[i]))

    def _image(self, i):
        x = self.data[i]
        if self.raw:
            return x if x.dtype == torch.uint8 else (x * 127.5 + 128).clamp(0, 255).to(torch.uint8)
        if x.dtype == torch.uint8:
            x = x.float().div_(127.5).sub_(1.0)
        if self.flip and torch.rand(()) < 0.5:          # RandomHorizontalFlip of the reference's training transforms
            x = x.flip(-1)
        return x


class _OwnIndex(Dataset):
    """item i is i: a ``DataLoader`` over it yields the batches of indices a ``DataLoader`` over the images would have fetched."""

    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        return i


def _resident(data, num_workers):
    """(images [N, C, H, W] uint8 or float32 on the host, positions in them or None, table of the 256 byte values' floats or None)
    of a data set this module can hold on the device."""
    if isinstance(data, Subset):
        images, inner, lut = _resident(data.dataset, num_workers)
        picked = torch.as_tensor(data.indices, dtype=torch.int64)
        return images, picked if inner is None else inner[picked], lut
    every_byte = torch.arange(256, dtype=torch.uint8)
    if isinstance(data, TensorImages) and not data.raw and data.data.dtype in (torch.uint8, torch.float32):
        if data.data.dtype == torch.float32:
            return data.data, None, None
        return data.data, None, TensorImages(every_byte.view(1, 1, 1, 256))[0].reshape(256)       # its own rounding chain, whatever it is
    if isinstance(data, _Images) and data.transform == "train":
        if isinstance(data, CIFAR10):
            images = torch.from_numpy(data.data)
        else:                                                    # decode (and resize) every image once, in the caller's worker processes
            raw = copy.copy(data)
            raw.transform, raw.labels = None, None
            images, at = None, 0                                 # filled chunk by chunk: the data set is held once (CelebA-HQ is 5.9 GB)
            for chunk in DataLoader(raw, batch_size=256, num_workers=num_workers):
                if images is None:
                    images = torch.empty((len(raw),) + tuple(chunk.shape[1:]), dtype=torch.uint8)
                images[at:at + len(chunk)] = chunk
                at += len(chunk)
        return images, None, _to_unit(every_byte)
    raise TypeError(f"{type(data).__name__}: not a data set DeviceLoader can hold on the device (TensorImages of uint8 / float32 in its "
                    f"training form, the dataset classes of this module in theirs, or a Subset of one)")


def _resident_labels(data):
    """int64 labels aligned with the images ``_resident`` returns (before its positions are applied), None for an unlabelled data set."""
    while isinstance(data, Subset):
        data = data.dataset
    labels = getattr(data, "labels", None)
    return None if labels is None else torch.as_tensor(labels).to(torch.int64)


class _Epoch:
    """Iterator over one epoch of a ``DeviceLoader``: the epoch's indices on the device and where each batch ends."""

    def __init__(self, loader, index, ends, seed):
        self.loader, self.index, self.ends, self.seed, self.at = loader, index, ends, seed, 0

    def __iter__(self):
        return self

    def __next__(self):
        if self.at >= len(self.ends):
            raise StopIteration
        lo, hi = self.ends[self.at - 1] if self.at else 0, self.ends[self.at]
        self.at += 1
        data, lut = self.loader.data, self.loader.lut
        n, c, h, w = data.shape
        out = torch.empty((hi - lo, c, h, w), dtype=torch.float32, device=data.device)
        _hip.call("ddpm_batch_gather", data.data_ptr(), 0 if data.dtype == torch.uint8 else 1, self.index.data_ptr() + 8 * lo, _hip.ptr(lut),
                  out.data_ptr(), hi - lo, n, c, h, w, int(self.loader.flip), self.seed, _hip.stream())
        if self.loader.labels is None:
            return out
        return out, self.loader.labels.index_select(0, self.index[lo:hi])      # the labels of the same images, by the same indices


class DeviceLoader:
    """The training batches of ``DataLoader(data, batch_size, shuffle / sampler, drop_last)`` with the images resident on ``device``.

    Construction copies the data set to the device once (uint8 stays uint8: CIFAR-10 is 150 MB, CelebA-HQ 5.9 GB).  ``iter()`` draws the
    epoch's index batches exactly as the host loader would — a ``DataLoader`` over a data set that returns its own index, so the same
    ``RandomSampler`` / ``DistributedSampler`` / ``Subset`` composition and the same draws from the global generator — and uploads them
    as one int64 tensor; ``next()`` on the iterator it returns then allocates the batch and enqueues one ``ddpm_batch_gather`` on the
    current stream: no copy from the host, no synchronisation.  (The upload is ordered on the stream that is current at ``iter()``;
    consume the batches on it.)  Each ``iter()`` is an epoch of its own, as with a ``DataLoader``: iterators do not disturb each other.

    Flips do not consume the global generator: image i is mirrored iff the top bit of the library's counter hash of
    ``((random_seed or 0) << 32 | epoch, i)`` is set, ``epoch`` = ``sampler.epoch`` where the sampler has one, else the number of
    earlier ``iter()`` calls — the same for any batch size and any number of ranks.

    A labelled data set (``TensorImages(..., labels=)``, a dataset class opened with ``labels=True``) also keeps its int64 labels on the
    device, and every batch is the pair ``(images, labels)``: the labels gathered by the indices the images were."""

    def __init__(self, data, batch_size, device, shuffle=False, sampler=None, drop_last=False, flip=None, random_seed=None, num_workers=0):
        images, self._positions, lut = _resident(data, num_workers)
        if flip is None:
            base = data
            while isinstance(base, Subset):
                base = base.dataset
            flip = base.flip
        self.device = torch.device(device)
        self.data = images.contiguous().to(self.device)
        self.lut = None if lut is None else lut.to(self.device)
        labels = _resident_labels(data)
        self.labels = None if labels is None else labels.contiguous().to(self.device)
        _hip.require_cuda(self.data)
        self.flip, self.sampler, self.random_seed = bool(flip), sampler, random_seed or 0
        self.batch_size = batch_size
        self._order = DataLoader(_OwnIndex(len(data)), batch_size=batch_size, shuffle=shuffle, sampler=sampler, drop_last=drop_last)
        self._epochs = 0

    def __len__(self):
        return len(self._order)

    def __iter__(self):
        epoch = self.sampler.epoch if hasattr(self.sampler, "epoch") else self._epochs
        self._epochs += 1
        seed = ((self.random_seed << 32) | (epoch & 0xFFFFFFFF)) & 0xFFFFFFFFFFFFFFFF
        batches = list(self._order)
        index = torch.cat(batches) if batches else torch.zeros(0, dtype=torch.int64)
        if self._positions is not None:
            index = self._positions[index]
        if self.device.type == "cuda":
            index = index.pin_memory()
        ends = torch.tensor([len(b) for b in batches], dtype=torch.int64).cumsum(0).tolist()
        return _Epoch(self, index.to(self.device, non_blocking=True), ends, seed)


def _open(name, root, split, raw=False, labels=False, num_classes=None):
    """Tensor file, then the dataset's own files, then (if asked for) synthetic images.  ``labels``: items are (image, label) pairs;
    ``num_classes`` (default: the data set's own count) is what the synthetic labels are taken modulo and what every label must be below."""
    info = DATASET_INFO[name]
    if labels and info.get("num_classes") is None:
        raise ValueError(f"{name} carries no class labels")
    data = _open_source(name, info, root, split, raw, labels, num_classes or info.get("num_classes"))
    if labels and num_classes is not None and len(data) and not 0 <= int(data.labels.min()) <= int(data.labels.max()) < num_classes:
        raise ValueError(f"{name}: labels span [{int(data.labels.min())}, {int(data.labels.max())}], the model has {num_classes} classes")
    return data


def _open_source(name, info, root, split, raw, labels, modulus):
    shape = (info["channels"],) + tuple(info["resolution"])
    root = os.path.expanduser(root)
    for fn in (f"{name}_{split}.pt", f"{name}.pt"):
        path = os.path.join(root, fn)
        if os.path.exists(path):
            data, classes = torch.load(path, map_location="cpu"), None
            if isinstance(data, dict):                          # {"images": [N, C, H, W], "labels": [N]}
                data, classes = data["images"], data.get("labels")
            assert tuple(data.shape[1:]) == shape, f"{path}: images of shape {tuple(data.shape[1:])}, expected {shape}"
            if labels and classes is None:
                raise ValueError(f"{path} has no 'labels' entry next to its images")
            return TensorImages(data, flip=(DATASET_DICT[name].flip and split != "test"), raw=raw, labels=classes if labels else None)
    try:
        return DATASET_DICT[name](root=root, split=split, transform=None if raw else "train", **({"labels": True} if labels else {}))
    except FileNotFoundError as e:
        missing = e
    n = int(os.environ.get("DDPM_TORCH_AMD_SYNTHETIC_DATA", "0"))
    if n > 0:
        g = torch.Generator().manual_seed(1234)
        return TensorImages(torch.rand((n,) + shape, generator=g) * 2 - 1, raw=raw,
                            labels=torch.arange(n) % modulus if labels else None)
    raise FileNotFoundError(
        f"{name}: neither a tensor file {name}.pt under {root} ([N, C, H, W] uint8 or float) nor the dataset's own files ({missing}).  "
        f"Set DDPM_TORCH_AMD_SYNTHETIC_DATA=<N> for N synthetic images of shape {shape}.")


def get_dataloader(dataset, batch_size, split, val_size=0., random_seed=None, root=ROOT, pin_memory=False, drop_last=False,
                   num_workers=0, distributed=False, raw=False, device=None, labels=False, num_classes=None, **kwargs):
    """(DataLoader, sampler) with the reference's batch / shard semantics (datasets.py:225-266).  ``device``: the same batches, in the same
    order, from a ``DeviceLoader`` that holds the data set on that GPU (training form only; ``num_workers`` then only serves the one-off
    decode of a dataset read from image files).  ``labels``: batches are ``(images, int64 labels)`` pairs (class-conditional training);
    ``ValueError`` for a data set without classes, or one whose labels do not all lie below ``num_classes`` (the model's class count, when
    given; the synthetic stand-in takes its labels modulo it)."""
    if device is not None and raw:
        raise ValueError("device= serves the training form only: the evaluation readers (raw=True) stay on the host path")
    data = _open(dataset, root, split, raw=raw, labels=labels, num_classes=num_classes)
    flip = data.flip and split != "test"
    if distributed:
        batch_size = batch_size // int(os.environ.get("WORLD_SIZE", "1"))
    if split != "test" and val_size > 0.:
        n = len(data)
        g = torch.Generator().manual_seed(random_seed or 0)
        perm = torch.randperm(n, generator=g)
        n_val = int(n * val_size) if val_size < 1 else int(val_size)
        idx = perm[n_val:] if split == "train" else perm[:n_val]
        data = torch.utils.data.Subset(data, idx.tolist())
    sampler = DistributedSampler(data, shuffle=True, seed=random_seed or 0, drop_last=drop_last) if distributed else None
    shuffle = sampler is None and split in ("train", "all") and not raw
    if device is not None:
        return DeviceLoader(data, batch_size, device, shuffle=shuffle, sampler=sampler, drop_last=drop_last, flip=flip, random_seed=random_seed,
                            num_workers=num_workers), sampler
    loader = DataLoader(data, batch_size=batch_size, shuffle=shuffle, sampler=sampler, drop_last=drop_last,
                        pin_memory=pin_memory and torch.cuda.is_available(), num_workers=num_workers)
    return loader, sampler
