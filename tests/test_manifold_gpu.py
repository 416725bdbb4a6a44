"""GPU: the fused precision / recall kernels (csrc/manifold.hip) against float64.

Yardstick and criteria: tests/manifold_emulator.py.  The window is w = 8 * e_ref, e_ref being the block path's own fp32 deviation from float64
on each case's inputs, computed here on the CPU (and asserted below 1e-5).  Measured: e_ref = 4.8e-6, w = 3.8e-5 on the 3000 x 2500 x 4096
clouds (2.7e-6 ... 4.1e-6, w = 2.2e-5 ... 3.3e-5 with the cdist of the GPU host's CPU); e_ref between 3.3e-6 and 6.2e-6 on the
1000 x 777 x 264 clouds; at most 5.2e-6 on the ragged cases.  The kernels' radii that are not fp16(kth64) lie within 1.7e-6 of the rounding
boundary (2 to 6 per set of 2500 / 3000), and no coverage bit differed from the float64 decision.  Every check prints its figures
(pytest -s) before it asserts."""
import functools
import importlib.util
import os
import pickle

import numpy as np
import pytest
import torch

import ddpm_torch
from ddpm_torch.metrics import precision_recall as M
from tests import manifold_emulator as ME

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
TABLE = [(3000, 2500, 4096), (1000, 777, 264)]


@functools.lru_cache(maxsize=None)
def _yardstick(kind_a, n_a, kind_b, n_b, D):
    """(float64 distances, w) of one pair of clouds, shared by the tests that use it."""
    a, b = ME.cloud(kind_a, n_a, D), ME.cloud(kind_b, n_b, D)
    d64 = ME.dist64(a, b)
    e = ME.e_ref(a, b, d64)
    print(f"{kind_a}{n_a} x {kind_b}{n_b} x {D}: e_ref {e:.3e}, w {ME.WINDOW_FACTOR * e:.3e}")
    return d64, ME.WINDOW_FACTOR * e


@pytest.mark.parametrize("nhood", [3, 5])
@pytest.mark.parametrize("n_real,n_gen,D", TABLE)
def test_both_entry_points_against_float64(n_real, n_gen, D, nhood):
    real, gen = ME.cloud("real", n_real, D), ME.cloud("gen", n_gen, D)
    real_d, gen_d = real.to(DEV), gen.to(DEV)
    radii = {}
    for name, n, x in (("real", n_real, real_d), ("gen", n_gen, gen_d)):
        d64, w = _yardstick(name, n, name, n, D)
        radii[name] = M.kth_radii(x, x, nhood + 1)
        ME.check_radii(radii[name], ME.kth64(d64, nhood + 1), w, f"{name} radii {n} x {D} nhood {nhood}")
    d64, w = _yardstick("gen", n_gen, "real", n_real, D)
    cross = M.kth_radii(gen_d, real_d, nhood + 1)                               # rows != columns: compute_kth(gen, real)
    ME.check_radii(cross, ME.kth64(d64, nhood + 1), w, f"gen against real {D} nhood {nhood}")
    for label, probe, support, key, dd in (("precision", gen_d, real_d, "real", d64), ("recall", real_d, gen_d, "gen", d64.t())):
        hit = M.coverage_hits(probe, support, radii[key])
        ME.check_coverage(hit, ME.coverage64(dd, radii[key]), w, f"{label} {D} nhood {nhood}")


RAGGED = [(1, 16), (5, 31), (33, 129), (129, 1000), (1000, 1000), (1000, 16)]
RAGGED_CASES = [(nr, nc, D) for D in (24, 264, 2048, 4096) for nr, nc in RAGGED] + [(1, 16, 8), (5, 31, 8)]


@pytest.mark.parametrize("rank", [1, 4, 16])
@pytest.mark.parametrize("nr,nc,D", RAGGED_CASES)
def test_ragged_geometry_against_float64(nr, nc, D, rank):
    """Rows from the generated recipe, columns from the real one (distinct sets: rank 1 means something).  Nc = 16 with rank = 16 is the
    Nc == rank edge; one size per D runs on pitched operands (ld = D + 8)."""
    rows, cols = ME.cloud("gen", nr, D), ME.cloud("real", nc, D)
    d64, w = _yardstick("gen", nr, "real", nc, D)
    want = ME.kth64(d64, rank)
    floor = ME.cancellation_floor(rows, cols)
    print(f"{nr} x {nc} x {D} rank {rank}: smallest radius {float(want.min()):.3f}, floor {floor:.3f}")
    assert float(want.min()) > floor                                            # a miss here is a mistake in the inputs, not in the kernel
    r_d, c_d = rows.to(DEV), cols.to(DEV)
    if (nr, nc) in ((33, 129), (5, 31)):
        r_d, c_d = ME.pitched(r_d), ME.pitched(c_d)
        assert r_d.stride(0) == D + 8
    out = M.kth_radii(r_d, c_d, rank)
    ME.check_radii(out, want, w, f"ragged radii {nr} x {nc} x {D} rank {rank}")
    # coverage against radii that put a mix of rows inside and outside: a little above / below each column's distance to its
    # min(rank, Nr)-th nearest row, alternating
    nearest = d64.t().kthvalue(min(rank, nr), dim=1).values
    kth = (nearest * torch.where(torch.arange(nc) % 2 == 0, 1.05, 0.97)).half()
    hit = M.coverage_hits(r_d, c_d, kth.to(DEV))
    ME.check_coverage(hit, ME.coverage64(d64, kth), w, f"ragged coverage {nr} x {nc} x {D} rank {rank}")


def test_results_are_bit_identical_across_runs_and_streams():
    real, gen = ME.cloud("real", 3000, 4096).to(DEV), ME.cloud("gen", 2500, 4096).to(DEV)
    radii = M.kth_radii(real, real, 4)
    hits = M.coverage_hits(gen, real, radii)
    torch.cuda.synchronize()
    assert torch.equal(M.kth_radii(real, real, 4), radii) and torch.equal(M.coverage_hits(gen, real, radii), hits)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        radii_side = M.kth_radii(real, real, 4)
        hits_side = M.coverage_hits(gen, real, radii)
    side.synchronize()
    assert torch.equal(radii_side, radii) and torch.equal(hits_side, hits)
    assert 0 < int(hits.sum()) < hits.numel()


def test_public_interface_fused_against_forced_block_loop_and_cpu(tmp_path, monkeypatch):
    n_real, n_gen, D, nhood = 1000, 777, 264, 3
    real, gen = ME.cloud("real", n_real, D), ME.cloud("gen", n_gen, D)
    cpu = torch.device("cpu")

    def run(device):
        br, bg = M.ManifoldBuilder(features=real, nhood_size=nhood, device=device), M.ManifoldBuilder(features=gen, nhood_size=nhood, device=device)
        return br, bg, M.calc_pr(bg.manifold, br.manifold, 10000, 10000, device)

    monkeypatch.delenv("DDPM_TORCH_AMD_FUSED_PR", raising=False)
    fused = run(DEV)
    monkeypatch.setenv("DDPM_TORCH_AMD_FUSED_PR", "0")
    block = run(DEV)                                                            # the parent commit's GPU path
    monkeypatch.delenv("DDPM_TORCH_AMD_FUSED_PR")
    host = run(cpu)
    d_cross, w = _yardstick("gen", n_gen, "real", n_real, D)
    slack = {}
    for name, (br, bg, (p, r)) in (("fused", fused), ("block", block), ("cpu", host)):
        off = 0
        for kind, n, b in (("real", n_real, br), ("gen", n_gen, bg)):
            d64, w_self = _yardstick(kind, n, kind, n, D)
            assert b.kth.dtype == torch.float16 and b.kth.device.type == "cpu" and b.features.device.type == "cpu"
            off += ME.check_radii(b.kth, ME.kth64(d64, nhood + 1), w_self, f"{name} {kind} radii")
        # precision / recall against the float64 decision on this path's own radii
        m_p, m_r = ME.coverage64(d_cross, br.kth), ME.coverage64(d_cross.t(), bg.kth)
        amb = [int(((m >= 1 - w) & (m <= 1 + w)).sum()) for m in (m_p, m_r)]
        print(f"{name}: precision {float(p):.4f} recall {float(r):.4f}, ambiguous rows {amb}, radii one ulp off {off}")
        assert p.dtype == torch.float32 and r.dtype == torch.float32 and p.device.type == "cpu"
        assert abs(float(p) - float((m_p <= 1).double().mean())) <= amb[0] / n_gen + 1e-6
        assert abs(float(r) - float((m_r <= 1).double().mean())) <= amb[1] / n_real + 1e-6
        assert amb[0] <= ME.AMBIGUOUS_CAP * n_gen and amb[1] <= ME.AMBIGUOUS_CAP * n_real
        slack[name] = (off, amb)
    # fused and forced-block differ in at most the rows float64 cannot decide (a radius one ulp off can move the rows it decides)
    radii_off = slack["fused"][0] + slack["block"][0]
    assert int((fused[0].kth != block[0].kth).sum()) + int((fused[1].kth != block[1].kth).sum()) <= radii_off
    if radii_off == 0:
        assert abs(float(fused[2][0]) - float(block[2][0])) <= max(slack["fused"][1][0], slack["block"][1][0]) / n_gen + 1e-6
        assert abs(float(fused[2][1]) - float(block[2][1])) <= max(slack["fused"][1][1], slack["block"][1][1]) / n_real + 1e-6
    # a set against itself; a set against a far copy of itself
    mr = fused[0].manifold
    assert tuple(float(v) for v in M.calc_pr(mr, mr, 10000, 10000, DEV)) == (1.0, 1.0)
    far = M.ManifoldBuilder(features=real.float() + 100.0, nhood_size=nhood, device=DEV).manifold
    assert tuple(float(v) for v in M.calc_pr(far, mr, 10000, 10000, DEV)) == (0.0, 0.0)
    # the manifold file is the reference's format
    fused[0].save(str(tmp_path / "m" / "manifold.pt"))
    loaded = M.load_manifold(str(tmp_path / "m" / "manifold.pt"))
    assert torch.equal(loaded.features, real) and torch.equal(loaded.kth, fused[0].kth) and loaded.kth.dtype == torch.float16


def test_eval_cli_prints_the_same_pr_on_the_gpu_as_on_the_cpu(tmp_path):
    """``eval.py --metrics pr`` with the stand-in extractor of tests/test_metrics.py, on inputs for which float64 decides every radius and
    every row (verified first, on the CPU): ``--device cuda:0`` (fused kernels) prints what ``--device cpu`` (block loop) prints."""
    from PIL import Image
    spec = importlib.util.spec_from_file_location("eval_cli", os.path.join(os.path.dirname(ddpm_torch.__file__), "..", "eval.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    rng = np.random.RandomState(0)
    folder = tmp_path / "data" / "cifar-10-batches-py"
    folder.mkdir(parents=True)
    real = []
    for fn in [f"data_batch_{i}" for i in range(1, 6)]:
        arr = rng.randint(0, 256, (12, 3072), dtype=np.uint8)
        real.append(arr.reshape(-1, 3, 32, 32))
        with open(folder / fn, "wb") as f:
            pickle.dump({"data": arr, "labels": [0] * 12}, f, protocol=2)
    real = torch.from_numpy(np.concatenate(real))
    gen = torch.from_numpy(np.concatenate([rng.randint(0, 256, (20, 32, 32, 3), dtype=np.uint8), rng.randint(0, 160, (20, 32, 32, 3), dtype=np.uint8)]))
    run = tmp_path / "images" / "run1"
    run.mkdir(parents=True)
    for i, g in enumerate(gen):
        Image.fromarray(g.numpy()).save(run / f"{i:03d}.png")
    # the stand-in of tests/test_metrics.py, centred: 8 x 8 block means of uint8 pixels sit near 8 with a spread of 0.6, where the fp32 norm
    # expansion of BOTH paths loses five digits of the distance (e_ref 5e-5) and no window can separate them.  Every value is a multiple of
    # 2^-11 below 16: exact in fp32 in any summation order, so both devices extract the same features.
    pr_net = lambda x: (x.float() - 127.5).reshape(x.shape[0], 3, 4, 8, 4, 8).mean(dim=(3, 5)).reshape(x.shape[0], -1) / 16      # noqa: E731  (uint8 in, D = 48)
    nhood = 2
    # float64 decides every row on these inputs, whichever admissible radii a path produces: a radius is fp16(kth64), or its neighbour when
    # kth64 lies within w of the rounding boundary between the two; a row must be inside some sphere of the SMALLEST admissible radii with
    # the window to spare, or outside every sphere of the LARGEST.  (The darker half of the samples sits far from the origin, so this
    # set's own fp32 error is 1.4e-5: above the ceiling that guards the cloud recipe, and the window is accordingly wider here.)
    ft, fg = pr_net(real).half(), pr_net(gen.permute(0, 3, 1, 2)).half()
    lo, hi, k64, w_self = {}, {}, {}, {}
    for name, x in (("real", ft), ("gen", fg)):
        d64 = ME.dist64(x, x)
        w_self[name] = w = ME.WINDOW_FACTOR * ME.e_ref(x, x, d64, ceiling=None)
        k64[name] = k = ME.kth64(d64, nhood + 1)
        near = k.half()
        up, down = (near.double() + ME._next_up(near).double()) / 2, (near.double() + ME._next_down(near).double()) / 2
        hi[name] = torch.where((k - up).abs() <= w * up, ME._next_up(near), near)
        lo[name] = torch.where((k - down).abs() <= w * down, ME._next_down(near), near)
    d64 = ME.dist64(fg, ft)
    w = ME.WINDOW_FACTOR * ME.e_ref(fg, ft, d64, ceiling=None)
    for dd, key in ((d64, "real"), (d64.t(), "gen")):
        inside, outside = ME.coverage64(dd, lo[key]) <= 1 - w, ME.coverage64(dd, hi[key]) >= 1 + w
        print(f"probe against {key}: {int(inside.sum())} rows inside, {int(outside.sum())} outside, of {len(inside)}; "
              f"{int((lo[key] != hi[key]).sum())} radii with two admissible values")
        assert bool((inside | outside).all())
    out = {}
    for device in ("cpu", "cuda:0"):
        argv = ["--root", str(tmp_path / "data"), "--dataset", "cifar10", "--sample-folder", str(run) + "/", "--device", device, "--num-workers", "0",
                "--eval-batch-size", "16", "--eval-total-size", "1000", "--precomputed-dir", str(tmp_path / ("pre_" + device[:3])), "--nhood-size", str(nhood),
                "--metrics", "pr"]
        out[device] = cli.main(argv, extractors={"pr": pr_net})
        loaded = M.load_manifold(tmp_path / ("pre_" + device[:3]) / "pr_manifold_cifar10.pt")
        assert torch.equal(loaded.features, ft), device
        ME.check_radii(loaded.kth, k64["real"], w_self["real"], f"saved radii ({device})")
    assert out["cuda:0"]["pr"] == out["cpu"]["pr"] and 0.0 < float(out["cpu"]["pr"].split("/")[0]) < 1.0
