"""-m gpu: ``ddpm_batch_gather`` (csrc/batch.hip) against its numpy restatement (tests/batch_emulator.py), tolerance 0 — the kernel only
moves values and looks them up.  Geometries: 32 x 32 in 3 and 1 channels (the 16-byte path), 8 x 16 (one group per row: its own mirror),
16 x 48 (three groups: the middle one maps to itself, the outer two swap), 24 x 20 (no whole groups: the element path); every one with
uint8 through a RANDOM table (a kernel that computes x / 127.5 - 1 instead of looking up fails) and with float32, flip off and on, the
output inside a larger buffer whose guard elements must keep their sentinel, and once more each at an output address and at a data-set
address that is not 16-byte aligned (the element path on a geometry that has whole groups).  Then the NaN contract of an index outside the data set, the status
codes, and images that straddle byte offsets 2^31 and 2^32 of a 4.3 GB data set."""
import numpy as np
import pytest
import torch

from ddpm_torch import _hip
from tests import batch_emulator as BE

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GEOMETRIES = [(3, 32, 32), (1, 32, 32), (3, 8, 16), (3, 16, 48), (3, 24, 20)]
N_IMAGES, INDEX = 7, [4, 0, 6, 4, 2]                 # not monotonic, one repeat
SEED = 1234 << 32 | 4                               # the seed word of random_seed 1234, epoch 4: both kinds of flip bit in every index list below
SENTINEL = -12345.0


def _inputs(geom, dtype, seed=0):
    g = torch.Generator().manual_seed(seed)
    if dtype == torch.uint8:
        data = torch.randint(0, 256, (N_IMAGES,) + geom, dtype=torch.uint8, generator=g)
    else:
        data = torch.randn((N_IMAGES,) + geom, generator=g)
    return data, torch.randn(256, generator=g)


def _run(data, lut, index, flip, seed=SEED, guard=64, shift=0):
    """The kernel's output for host tensors, after checking the guard elements around it.  ``shift``: the data set starts that many
    elements into its allocation (1: one byte / four bytes off a 16-byte boundary, and with it every image's base)."""
    B, per = len(index), data[0].numel()
    raw = torch.empty(shift + data.numel(), dtype=data.dtype, device=DEV)
    d = raw[shift:].view(data.shape)
    d.copy_(data)
    assert d.data_ptr() % 16 == (shift * data.element_size()) % 16
    idx = torch.tensor(index, dtype=torch.int64, device=DEV)
    table = lut.to(DEV) if data.dtype == torch.uint8 else None
    buf = torch.full((guard + B * per + guard,), SENTINEL, device=DEV)
    out = buf[guard:guard + B * per]
    _hip.call("ddpm_batch_gather", d.data_ptr(), 0 if data.dtype == torch.uint8 else 1, idx.data_ptr(), _hip.ptr(table), out.data_ptr(),
              B, data.shape[0], *data.shape[1:], flip, seed, _hip.stream())
    torch.cuda.synchronize()
    host = buf.cpu()
    assert bool((host[:guard] == SENTINEL).all()) and bool((host[-guard:] == SENTINEL).all()), "a guard element was overwritten"
    return host[guard:-guard].reshape((B,) + tuple(data.shape[1:])).numpy()


@pytest.mark.parametrize("dtype", [torch.uint8, torch.float32], ids=["uint8", "float32"])
@pytest.mark.parametrize("geom", GEOMETRIES, ids=lambda g: "x".join(map(str, g)))
def test_kernel_equals_the_restatement(geom, dtype):
    data, lut = _inputs(geom, dtype)
    bits = BE.flip_bits(SEED, np.asarray(INDEX))
    assert bits.any() and not bits.all()                               # the flip = 1 cases see both kinds
    for flip in (0, 1):
        want = BE.gather(data.numpy(), INDEX, lut.numpy(), flip, SEED)
        assert np.isfinite(want).all()
        for guard, shift in ((64, 0), (3, 0), (64, 1)):                # guard 3: the output, shift 1: the data set is not 16-byte aligned
            got = _run(data, lut, INDEX, flip, guard=guard, shift=shift)
            assert np.array_equal(got.view(np.int32), want.view(np.int32)), (geom, dtype, flip, guard, shift, float(np.abs(got - want).max()))
    mirrored = BE.gather(data.numpy(), INDEX, lut.numpy(), 1, SEED)
    plain = BE.gather(data.numpy(), INDEX, lut.numpy(), 0, SEED)
    for b, f in enumerate(bits):                                       # (what the restatement itself means by a flip)
        assert np.array_equal(mirrored[b], plain[b][..., ::-1] if f else plain[b])


@pytest.mark.parametrize("dtype", [torch.uint8, torch.float32], ids=["uint8", "float32"])
@pytest.mark.parametrize("geom", [(3, 32, 32), (3, 24, 20)], ids=["wide", "scalar"])
def test_an_index_outside_the_data_set_poisons_its_sample_only(geom, dtype):
    data, lut = _inputs(geom, dtype, seed=1)
    index = [-1, 3, N_IMAGES, 1, 5]
    for flip in (0, 1):
        got = _run(data, lut, index, flip)
        want = BE.gather(data.numpy(), index, lut.numpy(), flip, SEED)
        assert np.isnan(got[0]).all() and np.isnan(got[2]).all()
        for b in (1, 3, 4):
            assert np.isfinite(got[b]).all() and np.array_equal(got[b], want[b])


def test_status_codes_without_a_launch():
    """Only refused argument sets go through the launching entry point: one that passes would launch on these fake addresses."""
    lib = _hip.lib()
    a = 0x10000
    ok = dict(data=a, src_dtype=0, index=a, lut=a, out=a, B=5, n_images=7, C=3, H=32, W=32, flip=1, seed=9, st=0)
    call = lambda **k: lib.ddpm_batch_gather(*{**ok, **k}.values())                # noqa: E731
    for name in ("data", "index", "out", "lut"):
        assert call(**{name: 0}) == 5, name
    assert call(src_dtype=2) == 2 and call(src_dtype=-1) == 2
    for name in ("B", "n_images", "C", "H", "W"):
        assert call(**{name: 0}) == 1 and call(**{name: -3}) == 1, name
    assert call(C=2048, H=1024, W=1024) == 1                                       # one image of 2^31 elements
    assert call(C=2 ** 31 - 1, H=2 ** 31 - 1, W=2 ** 31 - 1) == 1                  # (a product that does not fit 64 bits either)
    with pytest.raises(RuntimeError, match="null pointer"):
        _hip.call("ddpm_batch_gather", 0, 0, a, a, a, 5, 7, 3, 32, 32, 0, 0, 0)
    with pytest.raises(RuntimeError, match="unsupported dtype"):
        _hip.call("ddpm_batch_gather", a, 7, a, a, a, 5, 7, 3, 32, 32, 0, 0, 0)


def test_images_beyond_byte_offsets_2_31_and_2_32():
    """21 846 images of 3 x 256 x 256 bytes = 4.295e9 bytes, left uninitialised except four images: 0, 10 922 (straddles byte offset
    2^31), 10 923 and 21 845 (straddles 2^32).  A 32-bit image base reads one of the others."""
    free = torch.cuda.mem_get_info()[0]
    if free < 6 * 2 ** 30:
        pytest.skip(f"{free / 2 ** 30:.1f} GiB of device memory free, 6 GiB needed")
    n, geom = 21846, (3, 256, 256)
    per = 3 * 256 * 256
    assert 10922 * per < 2 ** 31 < 10923 * per and 21845 * per < 2 ** 32 < 21846 * per
    data = torch.empty((n,) + geom, dtype=torch.uint8, device=DEV)
    g = torch.Generator().manual_seed(5)
    known = {i: torch.randint(0, 256, geom, dtype=torch.uint8, generator=g) for i in (0, 10922, 10923, 21845)}
    for i, img in known.items():
        data[i] = img.to(DEV)
    lut = torch.randn(256, generator=g)
    index = [21845, 0, 10923, 10922]
    bits = BE.flip_bits(SEED, np.asarray(index))
    assert bits.any() and not bits.all()
    idx, out = torch.tensor(index, dtype=torch.int64, device=DEV), torch.empty((4,) + geom, device=DEV)
    _hip.call("ddpm_batch_gather", data.data_ptr(), 0, idx.data_ptr(), lut.to(DEV).data_ptr(), out.data_ptr(), 4, n, *geom, 1, SEED, _hip.stream())
    got = out.cpu()
    for b, (i, f) in enumerate(zip(index, bits)):
        want = lut[known[i].long()]
        assert torch.equal(got[b], want.flip(-1) if f else want), i
