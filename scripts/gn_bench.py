"""Isolated timing of the GroupNorm(+SiLU+dropout) forward / backward launches on the CIFAR UNet's tensor shapes (B = 128, bf16).

``--mod``: the scale-shift norm's entry points (ddpm_groupnorm_mod_silu_fwd / _bwd) next to the plain ones at the same shape in the same
process — alternating (plain, modulated) pairs, the median of each and the spread (min .. max) of the pair ratios — on the B = 128
shapes and on the CelebA-HQ streaming shapes at B = 2.  The yardstick is the plain entry point of the same run."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "ddpm-torch_amd")]
import torch
from ddpm_torch import _hip, _ops as ops
from ddpm_torch._ops import View
B = 128
ACC = int(os.environ.get('GN_ACC', '0'))          # 1: the backward adds into dx ("+=")
DROP = float(os.environ.get('GN_DROP', '0.1')); SILU = os.environ.get('GN_SILU', '1') == '1'
SHAPES = [(32, 128, 8), (32, 256, 2), (32, 384, 1), (16, 256, 11), (16, 512, 2), (16, 384, 1), (16, 128, 1), (8, 256, 7), (8, 512, 3), (4, 256, 12), (4, 512, 3)]


def timeit(fn, n=20):
    fn(); torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) / n * 1e3


def mod_column():
    """plain vs modulated, alternating pairs (measuring-on-mi355x: one process, interleaved, spread reported)"""
    import statistics
    PAIRS = 7
    hq = [(256, 128), (128, 128), (64, 256)]                       # CelebA-HQ at B = 2: the streaming family
    print("shape                 fwd plain / mod us   ratio (min .. max)      bwd plain / mod us   ratio (min .. max)")
    for Bq, H, C in [(B, h, c) for h, c, _ in SHAPES] + [(2, h, c) for h, c in hq]:
        x = View(torch.randn(Bq, H, H, C, device="cuda").bfloat16(), Bq, H, H, C)
        y, dy, dx = (View(torch.randn(Bq, H, H, C, device="cuda").bfloat16(), Bq, H, H, C) for _ in range(3))
        g, bt = torch.ones(C, device="cuda"), torch.zeros(C, device="cuda")
        dg, db = torch.zeros(C, device="cuda"), torch.zeros(C, device="cuda")
        stats = torch.zeros(Bq, 32, 2, device="cuda")
        ld = 2 * C + 12                                            # an engine-like pitch: the block's columns of a wider buffer
        mod, dmod = 0.5 * torch.randn(Bq, ld, device="cuda"), torch.zeros(Bq, ld, device="cuda")
        ws = torch.zeros(ops.gn_workspace_floats(Bq, H * H, C, x.dtype), device="cuda")
        m = dict(mod_ptr=mod.data_ptr(), mod_ld=ld)
        fw = {0: lambda: ops.gn_fwd(x, y, g, bt, stats, ws, silu=SILU, drop_p=DROP, seed=123),
              1: lambda: ops.gn_fwd(x, y, g, bt, stats, ws, silu=SILU, drop_p=DROP, seed=123, **m)}
        bw = {0: lambda: ops.gn_bwd(x, dy, dx, g, bt, stats, dg.data_ptr(), db.data_ptr(), ws, silu=SILU, drop_p=DROP, seed=123, accumulate=ACC),
              1: lambda: ops.gn_bwd(x, dy, dx, g, bt, stats, dg.data_ptr(), db.data_ptr(), ws, silu=SILU, drop_p=DROP, seed=123, accumulate=ACC,
                                    dmod_ptr=dmod.data_ptr(), dmod_ld=ld, **m)}
        cols = []
        for pair in (fw, bw):
            t = {0: [], 1: []}
            for _ in range(PAIRS):
                for k in (0, 1):
                    t[k].append(timeit(pair[k], n=10))
            r = [b / a for a, b in zip(t[0], t[1])]
            cols.append(f"{statistics.median(t[0]):7.1f} / {statistics.median(t[1]):7.1f}   {statistics.median(r):5.3f} ({min(r):5.3f} .. {max(r):5.3f})")
        print(f"B{Bq:3d} {H:3d}^2 x {C:3d}:   {cols[0]}      {cols[1]}", flush=True)


if "--mod" in sys.argv:
    mod_column()
    sys.exit(0)
tot_f = tot_b = 0.0
if os.environ.get('GN_ONLY'):
    SHAPES = SHAPES[:int(os.environ['GN_ONLY'])]
for H, C, cnt in SHAPES:
    x = View(torch.randn(B, H, H, C, device="cuda").bfloat16(), B, H, H, C)
    y, dy, dx = (View(torch.randn(B, H, H, C, device="cuda").bfloat16(), B, H, H, C) for _ in range(3))
    g, bt = torch.ones(C, device="cuda"), torch.zeros(C, device="cuda")
    dg, db = torch.zeros(C, device="cuda"), torch.zeros(C, device="cuda")
    stats = torch.zeros(B, 32, 2, device="cuda")
    cs = torch.zeros(B, C, device="cuda")
    ws = torch.zeros(ops.gn_workspace_floats(B, H * H, C, x.dtype), device="cuda")
    tf = timeit(lambda: ops.gn_fwd(x, y, g, bt, stats, ws, silu=SILU, drop_p=DROP, seed=123))
    tb = timeit(lambda: ops.gn_bwd(x, dy, dx, g, bt, stats, dg.data_ptr(), db.data_ptr(), ws, silu=SILU, drop_p=DROP, seed=123, colsum_ptr=cs.data_ptr(), colsum_ld=C, accumulate=ACC))
    mb = B * H * H * C * 2 / 1e6
    tc = timeit(lambda: y.base.copy_(x.base))
    print(f"{H:2d}^2 x {C:3d} x{cnt:2d}: fwd {tf:6.1f} us ({2 * mb / tf:5.2f} TB/s)  bwd {tb:6.1f} us ({3 * mb / tb:5.2f} TB/s)   [copy_ {tc:5.1f} us {2 * mb / tc:5.2f} TB/s]", flush=True)
    tot_f += tf * cnt; tot_b += tb * cnt
print(f"network totals: fwd {tot_f / 1e3:.3f} ms  bwd {tot_b / 1e3:.3f} ms")
