"""TEST INFRASTRUCTURE for the device-resident data path (csrc/batch.hip, ddpm_torch.datasets.DeviceLoader): a numpy restatement of
``ddpm_batch_gather`` as include/ddpm_hip.h states it — ``gather`` on arrays, which tests/test_batch_gpu.py holds the kernel to with
tolerance 0, and the same thing over raw host pointers for the host emulator (tests/abi_emulator.py; ``attach`` hangs it on the Emulator
instance ``install`` returns).  ``dropout_word`` restates the counter hash of csrc/common.h (abi_emulator._keep_mask has the same mixer
for the dropout masks)."""
import ctypes

import numpy as np

from tests.abi_emulator import f32, i64

U32 = np.uint32


def _mix32(x):
    x = x.astype(U32)
    x ^= x >> U32(16); x = (x * U32(0x7FEB352D)).astype(U32)
    x ^= x >> U32(15); x = (x * U32(0x846CA68B)).astype(U32)
    x ^= x >> U32(16)
    return x


def dropout_word(seed, counter):
    """csrc/common.h dropout_word(seed, counter) for an array of 64-bit counters: mix32(lo ^ mix32(hi + seed_lo) ^ seed_hi * 0x9E3779B9)."""
    counter = np.asarray(counter).astype(np.uint64)
    lo, hi = (counter & np.uint64(0xFFFFFFFF)).astype(U32), (counter >> np.uint64(32)).astype(U32)
    s_lo, s_hi = U32(seed & 0xFFFFFFFF), (seed >> 32) & 0xFFFFFFFF
    with np.errstate(over="ignore"):
        return _mix32(lo ^ _mix32((hi + s_lo).astype(U32)) ^ U32((s_hi * 0x9E3779B9) & 0xFFFFFFFF))


def flip_bits(seed, index):
    """True where ddpm_batch_gather (flip = 1) mirrors the image with that data-set index."""
    return (dropout_word(seed, index) >> U32(31)).astype(bool)


def epoch_seed(random_seed, epoch):
    """The seed word DeviceLoader passes: (random_seed or 0) << 32 | epoch."""
    return (((random_seed or 0) << 32) | epoch) & 0xFFFFFFFFFFFFFFFF


def gather(data, index, lut, flip, seed):
    """out [B, C, H, W] float32 of data [N, C, H, W] (uint8 through lut [256] float32, or float32 copied); a sample whose index is
    outside [0, N) is NaN."""
    data, index = np.asarray(data), np.asarray(index, dtype=np.int64)
    out = np.full((len(index),) + data.shape[1:], np.nan, dtype=np.float32)
    ok = (index >= 0) & (index < data.shape[0])
    picked = data[index[ok]]
    picked = np.asarray(lut, dtype=np.float32)[picked] if data.dtype == np.uint8 else picked.astype(np.float32)
    if flip:
        mirror = flip_bits(seed, index[ok])
        picked[mirror] = picked[mirror][..., ::-1]
    out[ok] = picked
    return out


def ddpm_batch_gather(data, src_dtype, index, lut, out, B, n_images, C, H, W, flip, seed, st):
    assert src_dtype in (0, 1) and data and index and out and (lut or src_dtype == 1)
    assert B > 0 and n_images > 0 and C > 0 and H > 0 and W > 0 and C * H * W < 2 ** 31
    n = n_images * C * H * W
    if src_dtype == 0:
        images = np.frombuffer((ctypes.c_uint8 * n).from_address(data), dtype=np.uint8)
    else:
        images = f32(data, n)
    f32(out, B * C * H * W).reshape(B, C, H, W)[...] = gather(images.reshape(n_images, C, H, W), i64(index, B), f32(lut, 256) if lut else None,
                                                           flip, seed)


def attach(emu):
    """Add the entry point to an ``abi_emulator.Emulator`` instance (its ``call`` is ``getattr(self, name)``)."""
    emu.ddpm_batch_gather = ddpm_batch_gather
    return emu
