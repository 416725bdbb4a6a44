"""Time precision / recall on the GPU: the fused manifold kernels (csrc/manifold.hip) against the block loop they replace
(DDPM_TORCH_AMD_FUSED_PR=0: torch.cdist per 10 000 x 10 000 block, every block copied to the host, kthvalue / any on the CPU), in the same
process on the same device.

    python scripts/pr_bench.py [--sizes 5000,50000] [--pairs 3] [--dim 4096] [--nhood 3] [--no-block-loop] [--kernels-only]

End to end: ManifoldBuilder(features=...) for both sets plus calc_pr, host clock around work that ends in a device synchronise (the block
loop includes host work by construction); the two paths alternate, --pairs times, after a warm-up of each at a small size; every time is
reported.  Kernels: each entry point alone on features already on the device, device events, with 2 Nr Nc D / duration as a share of the
nominal 2.5 PFLOP/s and of what ddpm_mfma_probe sustains on this device.  --kernels-only runs just that part (the shape to put behind
``rocprofv3 --kernel-trace --stats --``).  Features: the seeded low-intrinsic-dimension clouds of tests/manifold_emulator.py.  One JSON line
per measurement."""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "ddpm-torch_amd")]

import torch  # noqa: E402

from ddpm_torch import _hip  # noqa: E402
from ddpm_torch.metrics import precision_recall as M  # noqa: E402

DEV = torch.device("cuda:0")
NOMINAL_TFLOPS = 2500.0


def cloud(kind, n, D):
    """relu(z W + 0.05 noise).half(), z in R^8: the recipe of tests/manifold_emulator.cloud, generated in slices to bound the host memory."""
    w = torch.randn(8, D, generator=torch.Generator().manual_seed(99)) / math.sqrt(8.0)
    g = torch.Generator().manual_seed({"real": 1, "gen": 2}[kind])
    z = torch.randn(n, 8, generator=g)
    if kind == "gen":
        z = 1.25 * z + 0.3
    out = torch.empty(n, D, dtype=torch.float16)
    for i in range(0, n, 5000):                              # (the noise of a slice is drawn per slice: not the test clouds bit for bit)
        out[i:i + 5000] = torch.relu(z[i:i + 5000] @ w + 0.05 * torch.randn(min(5000, n - i), D, generator=g)).half()
    return out


def end_to_end(real, gen, nhood, fused):
    os.environ["DDPM_TORCH_AMD_FUSED_PR"] = "1" if fused else "0"
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    mr = M.ManifoldBuilder(features=real, nhood_size=nhood, device=DEV).manifold
    mg = M.ManifoldBuilder(features=gen, nhood_size=nhood, device=DEV).manifold
    p, r = M.calc_pr(mg, mr, 10000, 10000, DEV)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, float(p), float(r)


def practical_peak():
    sink = torch.zeros(256, device=DEV)
    iters, st = 200000, torch.cuda.current_stream().cuda_stream
    for _ in range(3):
        _hip.call("ddpm_mfma_probe", sink.data_ptr(), iters, 0, st)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(6):
        _hip.call("ddpm_mfma_probe", sink.data_ptr(), iters, 0, st)
    b.record()
    torch.cuda.synchronize()
    return 6 * iters * 16 * 32768.0 * 1024 / (a.elapsed_time(b) * 1e-3) / 1e12


def kernels(real, gen, nhood, peak, reps=3):
    r, g = real.to(DEV), gen.to(DEV)
    radii = M.kth_radii(r, r, nhood + 1)
    M.coverage_hits(g, r, radii)
    torch.cuda.synchronize()
    for what, fn, nr, nc in (("ddpm_manifold_kth_f16", lambda: M.kth_radii(r, r, nhood + 1), len(r), len(r)),
                             ("ddpm_manifold_cover_f16", lambda: M.coverage_hits(g, r, radii), len(g), len(r))):
        ms = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
        tf = 2.0 * nr * nc * r.shape[1] / (min(ms) * 1e-3) / 1e12
        print(json.dumps({"what": what, "Nr": nr, "Nc": nc, "D": r.shape[1], "ms": [round(v, 3) for v in ms], "tflops_best": round(tf, 1),
                          "share_of_2500tf": round(tf / NOMINAL_TFLOPS, 3), "share_of_practical_peak": round(tf / peak, 3)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="5000,50000")
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--dim", type=int, default=4096)
    ap.add_argument("--nhood", type=int, default=3)
    ap.add_argument("--no-block-loop", action="store_true", help="time the fused path alone")
    ap.add_argument("--kernels-only", action="store_true")
    args = ap.parse_args()
    peak = practical_peak()
    print(json.dumps({"what": "practical_peak (ddpm_mfma_probe, bf16)", "tflops": round(peak, 1)}), flush=True)
    warm_r, warm_g = cloud("real", 1500, args.dim), cloud("gen", 1200, args.dim)
    for fused in (True, False):
        end_to_end(warm_r, warm_g, args.nhood, fused)
    for n in (int(v) for v in args.sizes.split(",")):
        real, gen = cloud("real", n, args.dim), cloud("gen", n, args.dim)
        kernels(real, gen, args.nhood, peak)
        if args.kernels_only:
            continue
        for pair in range(args.pairs):
            for fused in (True,) if args.no_block_loop else (True, False):
                s, p, r = end_to_end(real, gen, args.nhood, fused)
                print(json.dumps({"what": "end_to_end", "N": n, "D": args.dim, "nhood": args.nhood, "pair": pair,
                                  "path": "fused" if fused else "block_loop", "seconds": round(s, 3), "precision": round(p, 5), "recall": round(r, 5)}), flush=True)


if __name__ == "__main__":
    main()
