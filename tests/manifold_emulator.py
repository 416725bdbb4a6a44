"""TEST INFRASTRUCTURE for the precision / recall kernels (csrc/manifold.hip): a numpy restatement of the two ABI contracts for the host
emulator (tests/abi_emulator.py; ``attach`` hangs them on the Emulator instance ``install`` returns), the seeded feature clouds the tests
run on and the float64 acceptance criteria shared by tests/test_manifold_host.py (emulated) and tests/test_manifold_gpu.py (the kernels).

The yardstick is float64 — ``torch.cdist(x.double(), y.double(), compute_mode="donot_use_mm_for_euclid_dist")`` on the fp16 features — not the
code under test and not torch's fp32 bits (no kernel can reproduce torch's rounding order).  ``e_ref`` is the largest relative deviation of
the block path's own fp32 distances (``torch.cdist`` on the widened features) from float64 over the pairs at a non-zero float64 distance
(a set against itself has an exactly zero diagonal, where a relative deviation means nothing and the fp32 norm expansion returns up to
0.054); the window is ``w = 8 * e_ref``.  The factor 8 is the margin DESIGN.md section 7 measured between serial MFMA accumulation over a long
K and a blocked CPU GEMM (2.5 to 7.6 x); it was fixed before the kernels existed."""
import ctypes
import functools
import math

import numpy as np
import torch

WINDOW_FACTOR = 8.0
E_REF_CEILING = 1e-5            # a changed recipe is noticed: 4.8e-6 on the 3000 x 2500 x 4096 clouds, at most 5.2e-6 on the ragged cases
RADII_SECOND_BRANCH_CAP = 0.01
AMBIGUOUS_CAP = 0.02


# ------------------------------------------------------------------ inputs
@functools.lru_cache(maxsize=None)
def _mixing(D):
    return torch.randn(8, D, generator=torch.Generator().manual_seed(99)) / math.sqrt(8.0)


@functools.lru_cache(maxsize=None)
def cloud(kind, n, D):
    """fp16 [n, D] features of intrinsic dimension 8: relu(z W + 0.05 noise); "real": z ~ N(0, I), seed 1; "gen": z ~ 1.25 N(0, I) + 0.3, seed 2.
    z is drawn first, then the noise, from the set's own generator."""
    g = torch.Generator().manual_seed({"real": 1, "gen": 2}[kind])
    z = torch.randn(n, 8, generator=g)
    if kind == "gen":
        z = 1.25 * z + 0.3
    noise = torch.randn(n, D, generator=g)
    return torch.relu(z @ _mixing(D) + 0.05 * noise).half()


def pitched(x, extra=8):
    """The same values in a buffer with row pitch D + extra."""
    buf = torch.zeros(x.shape[0], x.shape[1] + extra, dtype=x.dtype, device=x.device)
    buf[:, :x.shape[1]] = x
    return buf[:, :x.shape[1]]


# ------------------------------------------------------------------ float64 yardstick and criteria
def dist64(a, b):
    return torch.cdist(a.double().cpu(), b.double().cpu(), compute_mode="donot_use_mm_for_euclid_dist")


def e_ref(a, b, d64, ceiling=E_REF_CEILING):
    """Largest relative deviation of the block path's fp32 distances from float64 (pairs at float64 distance 0 excluded, see the module text).
    ``ceiling`` guards the cloud recipe; inputs from elsewhere pass None and live with the window their conditioning gives them."""
    d32 = torch.cdist(a.float().cpu().unsqueeze(0), b.float().cpu().unsqueeze(0)).squeeze(0).double()
    ok = d64 > 0
    e = float(((d32 - d64).abs()[ok] / d64[ok]).max())
    assert ceiling is None or e < ceiling, e
    return e


def _next_up(h):
    """The next fp16 value above each (positive, finite) fp16 value."""
    return (h.contiguous().view(torch.int16) + 1).view(torch.float16)


def _next_down(h):
    return (h.contiguous().view(torch.int16) - 1).view(torch.float16)


def kth64(d64, rank):
    return d64.kthvalue(rank, dim=1).values


def check_radii(out, want64, w, label=""):
    """out[i] == fp16(kth64[i]), or exactly one fp16 ulp from it with kth64[i] within w (relative) of the midpoint of the two; at most 1 % of the
    set may take the second branch.  Returns the number that did."""
    out = out.detach().cpu()
    assert out.dtype == torch.float16 and out.shape == want64.shape and bool(torch.isfinite(out).all()), label
    near = want64.half()
    off = out != near
    if bool(off.any()):
        o, n, t = out[off], near[off], want64[off]
        one_ulp = (o == _next_up(n)) | (o == _next_down(n))
        mid = (o.double() + n.double()) / 2
        close = (t - mid).abs() <= w * mid
        print(f"{label}: {int(off.sum())} of {out.numel()} radii one ulp off, worst midpoint distance {float(((t - mid).abs() / mid).max()):.3e} (w = {w:.3e})")
        assert bool(one_ulp.all()), (label, o[~one_ulp][:4], n[~one_ulp][:4])
        assert bool(close.all()), (label, float(((t - mid).abs() / mid).max()), w)
    n_off = int(off.sum())
    assert n_off <= RADII_SECOND_BRANCH_CAP * out.numel(), (label, n_off, out.numel())
    return n_off


def coverage64(d64, support_kth):
    """m[i] = min_j d64(i, j) / b_j with b_j the midpoint between kth[j] and the next fp16 value above it — where fp16(d) <= kth[j] flips.
    The float64 decision is m <= 1."""
    k = support_kth.detach().cpu()
    b = (k.double() + _next_up(k).double()) / 2
    return (d64 / b.unsqueeze(0)).min(dim=1).values


def check_coverage(hit, m, w, label=""):
    """A reported hit needs m <= 1 + w, a reported miss m >= 1 - w; rows with m inside the window are ambiguous, at most 2 % of the probe rows.
    Returns (ambiguous rows, float64 share)."""
    hit = hit.detach().cpu()
    assert hit.dtype == torch.bool and hit.shape == m.shape, label
    ambiguous = int(((m >= 1 - w) & (m <= 1 + w)).sum())
    print(f"{label}: {int(hit.sum())} of {hit.numel()} rows hit, {ambiguous} ambiguous (w = {w:.3e}), {int((hit != (m <= 1)).sum())} differ from float64")
    assert bool((m[hit] <= 1 + w).all()), (label, float(m[hit].max()))
    assert bool((m[~hit] >= 1 - w).all()), (label, float(m[~hit].min()) if bool((~hit).any()) else None)
    assert ambiguous <= AMBIGUOUS_CAP * hit.numel(), (label, ambiguous)
    share64 = float((m <= 1).double().mean())
    assert abs(float(hit.double().mean()) - share64) <= ambiguous / hit.numel() + 1e-12, label
    return ambiguous, share64


def cancellation_floor(a, b):
    """100 * sqrt(2^-24 * max |x|^2): radii above it are far from where the fp32 norm expansion loses the distance."""
    biggest = max(float((a.double() ** 2).sum(1).max()), float((b.double() ** 2).sum(1).max()))
    return 100.0 * math.sqrt(2.0 ** -24 * biggest)


# ------------------------------------------------------------------ the ABI contracts in numpy
def column_splits(nr, nc):
    rt, ct = -(-nr // 128), -(-nc // 128)
    s0, half = min(ct, 64, -(-4096 // rt)), -(-ct // 2)
    if rt * half >= 512:
        s0 = min(s0, half)
    return -(-ct // -(-ct // s0))


def kth_workspace_bytes(nr, nc):
    return 4 * (nr + nc) + 64 * column_splits(nr, nc) * nr


def cover_workspace_bytes(n_p, ns):
    return 4 * (n_p + ns)


def _halves(ptr, n, d, ld):
    raw = np.frombuffer((ctypes.c_uint16 * ((n - 1) * ld + d)).from_address(ptr), dtype=np.float16)
    return np.lib.stride_tricks.as_strided(raw, (n, d), (2 * ld, 2), writeable=True)


def _distances(r, c):
    """d = fp16(sqrt(max(|r|^2 + |c|^2 - 2 r.c, 0))) with fp32 arithmetic."""
    r, c = r.astype(np.float32), c.astype(np.float32)
    d2 = (r * r).sum(1, dtype=np.float32)[:, None] + (c * c).sum(1, dtype=np.float32)[None, :] - np.float32(2) * (r @ c.T)
    with np.errstate(over="ignore"):
        return np.sqrt(np.maximum(d2, np.float32(0))).astype(np.float16)


def _served(r, r_ld, nr, c, c_ld, nc, d, ws, ws_bytes, need):
    assert r and c and ws and nr >= 1 and nc >= 1 and d >= 8 and d % 8 == 0 and r_ld >= d and c_ld >= d
    assert r_ld % 8 == 0 and c_ld % 8 == 0 and r % 16 == 0 and c % 16 == 0 and ws % 16 == 0
    assert nr * r_ld * 2 < 2 ** 31 and nc * c_ld * 2 < 2 ** 31 and ws_bytes >= need, (ws_bytes, need)


def ddpm_manifold_kth_f16(rows, rows_ld, nr, cols, cols_ld, nc, d, rank, out, ws, ws_bytes, st):
    _served(rows, rows_ld, nr, cols, cols_ld, nc, d, ws, ws_bytes, kth_workspace_bytes(nr, nc))
    assert out and 1 <= rank <= min(16, nc)
    dist = _distances(_halves(rows, nr, d, rows_ld), _halves(cols, nc, d, cols_ld)).astype(np.float32)
    _halves(out, 1, nr, nr)[0, :] = np.partition(dist, rank - 1, axis=1)[:, rank - 1].astype(np.float16)


def ddpm_manifold_cover_f16(probe, probe_ld, n_p, support, support_ld, ns, d, kth, hit, ws, ws_bytes, st):
    _served(probe, probe_ld, n_p, support, support_ld, ns, d, ws, ws_bytes, cover_workspace_bytes(n_p, ns))
    assert kth and hit
    dist = _distances(_halves(probe, n_p, d, probe_ld), _halves(support, ns, d, support_ld))
    radii = _halves(kth, 1, ns, ns)[0]
    np.frombuffer((ctypes.c_uint8 * n_p).from_address(hit), dtype=np.uint8)[:] = (dist <= radii[None, :]).any(axis=1)


def attach(emu):
    """Add the two entry points to an ``abi_emulator.Emulator`` instance (its ``call`` is ``getattr(self, name)``)."""
    emu.ddpm_manifold_kth_f16 = ddpm_manifold_kth_f16
    emu.ddpm_manifold_cover_f16 = ddpm_manifold_cover_f16
    return emu
