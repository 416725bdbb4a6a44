"""CPU: the host side of the fused precision / recall kernels (csrc/manifold.hip) — argument validation of the two entry points in the
built library, and the dispatch of ``ddpm_torch.metrics.precision_recall`` under the host emulator (tests/abi_emulator.py +
tests/manifold_emulator.py).  The kernels themselves are checked on the GPU (tests/test_manifold_gpu.py).

Acceptance criteria (tests/manifold_emulator.py): float64 yardstick, window w = 8 * e_ref with e_ref the block path's own fp32 error on the
inputs; measured on the 1000 x 777 x 264 clouds used here: e_ref between 4.2e-6 and 6.2e-6, w between 3.3e-5 and 5.0e-5 (each check prints its own)."""
import contextlib
import os

import pytest
import torch

from ddpm_torch import _hip
from ddpm_torch.metrics import precision_recall as M
from tests import abi_emulator
from tests import manifold_emulator as ME

needs_lib = pytest.mark.skipif(not os.path.exists(_hip.LIB_PATH), reason="libddpm_hip.so not built")
GPU = torch.device("cuda:0")


@needs_lib
def test_manifold_entry_points_validate_on_the_host_without_a_gpu():
    """Only refused argument sets go through the launching entry points: one that passes would launch on these fake addresses."""
    lib = _hip.lib()
    a = 0x10000
    nr, nc, d = 300, 200, 264
    ws = ME.kth_workspace_bytes(nr, nc)
    kth = lambda **k: lib.ddpm_manifold_kth_f16(*[{**dict(rows=a, rows_ld=d, nr=nr, cols=a, cols_ld=d, nc=nc, d=d, rank=4, out=a, ws=a, ws_bytes=ws, st=0), **k}[n]  # noqa: E731
                                                  for n in ("rows", "rows_ld", "nr", "cols", "cols_ld", "nc", "d", "rank", "out", "ws", "ws_bytes", "st")])
    for name in ("rows", "cols", "out", "ws"):
        assert kth(**{name: 0}) == 5, name
    assert kth(d=12, rows_ld=16, cols_ld=16) == 1                      # D not a multiple of 8
    assert kth(rank=17) == 1 and kth(rank=0) == 1
    assert kth(nc=3, rank=4) == 1                                      # rank > Nc
    assert kth(nr=0) == 1 and kth(rows_ld=d - 8) == 1
    assert kth(ws_bytes=ws - 1) == 1                                   # one byte short
    assert kth(rows_ld=d + 4) == 3 and kth(cols_ld=d + 4) == 3         # pitch not a multiple of 16 bytes
    assert kth(rows=a + 2) == 3 and kth(ws=a + 4) == 3
    assert kth(nr=2 ** 20, rows_ld=1024, d=1024, cols_ld=1024, ws_bytes=2 ** 40) == 1           # a 2 GiB operand
    cws = ME.cover_workspace_bytes(nr, nc)
    cov = lambda **k: lib.ddpm_manifold_cover_f16(*[{**dict(p=a, p_ld=d, np=nr, s=a, s_ld=d, ns=nc, d=d, kth=a, hit=a, ws=a, ws_bytes=cws, st=0), **k}[n]  # noqa: E731
                                                    for n in ("p", "p_ld", "np", "s", "s_ld", "ns", "d", "kth", "hit", "ws", "ws_bytes", "st")])
    for name in ("p", "s", "kth", "hit", "ws"):
        assert cov(**{name: 0}) == 5, name
    assert cov(d=12, p_ld=16, s_ld=16) == 1
    assert cov(ns=0) == 1 and cov(ws_bytes=cws - 1) == 1
    assert cov(s_ld=d + 4) == 3 and cov(p=a + 8) == 3
    # the ctypes table raises on a refusal like every other entry point
    with pytest.raises(RuntimeError, match="bad shape"):
        _hip.call("ddpm_manifold_kth_f16", a, d, nr, a, d, nc, d, 17, a, a, ws, 0)


def test_workspace_formula_of_the_python_side_matches_the_emulators():
    for nr, nc in [(1, 16), (129, 1000), (1000, 1000), (5000, 5000), (50000, 50000), (3000, 2500), (100000, 7)]:
        assert M._column_splits(nr, nc) == ME.column_splits(nr, nc) >= 1
    assert ME.column_splits(1000, 1000) == 8 and ME.column_splits(50000, 50000) == 11 and ME.column_splits(5000, 5000) == 20


@pytest.fixture
def emu(monkeypatch):
    monkeypatch.delenv("DDPM_TORCH_AMD_FUSED_PR", raising=False)
    return ME.attach(abi_emulator.install(monkeypatch, _hip))


@pytest.fixture
def as_gpu(monkeypatch):
    """Let the builder's GPU branch run on host tensors: nothing is uploaded, there is no device to select, and the block loop (when it
    is the one that runs) computes on the CPU."""
    block_loop = M.compute_distance
    monkeypatch.setattr(M, "_upload", lambda t, device: t)
    monkeypatch.setattr(M.torch.cuda, "device", lambda d: contextlib.nullcontext())
    monkeypatch.setattr(M, "compute_distance", lambda r, c, rb, cb, device: block_loop(r, c, rb, cb, torch.device("cpu")))


@needs_lib
@pytest.mark.parametrize("nhood", [3, 5])
def test_fused_functions_meet_the_float64_criteria_under_emulation(emu, nhood):
    real, gen = ME.cloud("real", 1000, 264), ME.cloud("gen", 777, 264)
    radii = {}
    for name, x in (("real", real), ("gen", gen)):
        d64 = ME.dist64(x, x)
        w = ME.WINDOW_FACTOR * ME.e_ref(x, x, d64)
        radii[name] = M.kth_radii(x, x, nhood + 1)
        ME.check_radii(radii[name], ME.kth64(d64, nhood + 1), w, f"{name} radii nhood {nhood}")
    d64 = ME.dist64(gen, real)
    w = ME.WINDOW_FACTOR * ME.e_ref(gen, real, d64)
    cross = M.kth_radii(ME.pitched(gen), real, nhood + 1)               # rows != columns, pitched rows
    ME.check_radii(cross, ME.kth64(d64, nhood + 1), w, "gen against real")
    for label, probe, support, dd in (("precision", gen, real, d64), ("recall", real, gen, d64.t())):
        key = "real" if support is real else "gen"
        hit = M.coverage_hits(probe, ME.pitched(support), radii[key])
        ME.check_coverage(hit, ME.coverage64(dd, radii[key]), w, f"{label} nhood {nhood}")
    assert emu.log == ["ddpm_manifold_kth_f16"] * 3 + ["ddpm_manifold_cover_f16"] * 2


@needs_lib
def test_builder_and_calc_pr_dispatch(emu, as_gpu, monkeypatch):
    real, gen = ME.cloud("real", 1000, 264), ME.cloud("gen", 777, 264)
    cpu = torch.device("cpu")
    # the CPU device: the block loop, no ABI call
    b_real, b_gen = M.ManifoldBuilder(features=real, device=cpu), M.ManifoldBuilder(features=gen, device=cpu)
    want = M.calc_pr(b_gen.manifold, b_real.manifold, 10000, 10000, cpu)
    assert emu.log == []
    # a GPU device: one call per radius set and per coverage direction, results with the dtypes of the block loop
    f_real, f_gen = M.ManifoldBuilder(features=real, device=GPU), M.ManifoldBuilder(features=gen, device=[GPU])
    assert emu.log == ["ddpm_manifold_kth_f16"] * 2
    for f, b in ((f_real, b_real), (f_gen, b_gen)):
        assert f.kth.dtype == torch.float16 and f.kth.device.type == "cpu" and f.kth.shape == b.kth.shape
        assert int((f.kth != b.kth).sum()) <= 0.01 * len(b.kth)
    got = M.calc_pr(f_gen.manifold, f_real.manifold, 10000, 10000, GPU)
    assert emu.log[2:] == ["ddpm_manifold_cover_f16"] * 2
    assert all(g.dtype == torch.float32 and g.dim() == 0 for g in got)
    assert all(abs(float(g) - float(t)) <= 0.02 for g, t in zip(got, want)) and 0.5 < float(got[0]) < 0.9
    radii = f_real.compute_kth(gen, real)
    assert radii.shape == (777,) and emu.log[-1] == "ddpm_manifold_kth_f16"
    # what the kernels do not serve keeps the block loop, without a call: fp32 features, rank 17, D % 8 != 0
    del emu.log[:]
    small, other = real[:64, :12].contiguous(), gen[:48, :12].contiguous()
    assert torch.equal(f_real.compute_kth(real.float()), b_real.compute_kth(real.float()))
    wide = M.ManifoldBuilder(features=real, nhood_size=16, device=GPU)
    assert torch.equal(wide.kth, M.ManifoldBuilder(features=real, nhood_size=16, device=cpu).kth)
    odd, odd_cpu = M.ManifoldBuilder(features=small, device=GPU), M.ManifoldBuilder(features=small, device=cpu)
    assert torch.equal(odd.kth, odd_cpu.kth)
    m_other = M.ManifoldBuilder(features=other, device=GPU).manifold
    assert M.calc_pr(m_other, odd.manifold, 10000, 10000, GPU) == M.calc_pr(m_other, odd.manifold, 10000, 10000, cpu)
    f32_manifold = M.Manifold(features=real.float(), kth=b_real.kth.float())
    assert M.calc_pr(f32_manifold, f32_manifold, 10000, 10000, GPU) == M.calc_pr(f32_manifold, f32_manifold, 10000, 10000, cpu)
    assert emu.log == []
    assert not M._fused(GPU, real, real, 17) and not M._fused(GPU, real.float(), real.float(), 4) and not M._fused(GPU, small, small, 4)
    assert not M._fused(GPU, real[:3], real[:3], 4) and not M._fused(cpu, real, real, 4) and M._fused(GPU, real, real, 16)
    # the A/B switch is read at call time
    monkeypatch.setenv("DDPM_TORCH_AMD_FUSED_PR", "0")
    forced = M.ManifoldBuilder(features=real, device=GPU)
    assert torch.equal(forced.kth, b_real.kth)
    assert M.calc_pr(f_gen.manifold, f_real.manifold, 10000, 10000, GPU) == M.calc_pr(f_gen.manifold, f_real.manifold, 10000, 10000, cpu)
    assert emu.log == []
    monkeypatch.setenv("DDPM_TORCH_AMD_FUSED_PR", "1")
    M.ManifoldBuilder(features=real, device=GPU)
    assert emu.log == ["ddpm_manifold_kth_f16"]
