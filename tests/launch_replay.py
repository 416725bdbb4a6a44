"""Launch recording and replay against float64 references (TEST INFRASTRUCTURE).

record()   wraps ddpm_torch._hip._invoke while a workload runs and keeps one SIGNATURE per distinct launch: the entry name, every
           scalar argument, and for every pointer argument whether it is NULL and its address modulo 256 (the hipStream_t is dropped).
replay()   re-issues one recorded signature on fresh random inputs at that geometry — same pitches, same pointer offsets modulo 256,
           the same optional operands present or absent, the same accumulate / output mode / splits — and compares every output with a
           float64 torch restatement of include/ddpm_hip.h written here (tests/abi_emulator.py is not used as a reference).

The float64 work runs in torch on the device that holds the buffers: the MI355X in the -m gpu test, the host in the CPU test.  Every
image of every output is compared.

Memory safety: every buffer's extent is computed from the contract (a pitched [rows][cols] operand spans (rows - 1) * ld + cols
elements), and sits between two 64 KiB guard bands filled with a sentinel byte.  After each launch the guards, and every element of the
buffer the contract does not let the call write (pitch gaps, read-only operands), must hold what they held before.

Hostile inputs (opt-in keywords of replay(); tests/test_hostile_inputs_gpu.py and _host.py): poison=True overwrites, before the launch,
everything the contract does not let the call read — both guard bands, pitch gaps and channel-slice neighbours of inputs, the prior
content of overwritten outputs, unspecified workspaces — with 0xFF bytes (NaN); profile= transforms the data operands after the draw
(PROFILES); yardstick=True also puts a plain fp32 torch composition through the same bars.  Without keywords the draws are unchanged.

Table-driven entries (the optimizer tail: ddpm_wgrad_unpack(_sumsq), ddpm_mt_grad_sumsq, ddpm_mt_adam_ema, ddpm_pack_weight_multi,
ddpm_mt_gather_f32) read their geometry from a table in device memory.  record() keeps the table's address and, once the workload has
ended, replaces the pointer word of the signature by the normalised table (resolve_tables / normalise_table: per row the element counts,
for every pointer column null / address modulo 16 / byte gap to the next row's tensor); the replay rebuilds that packing out of guarded
buffers.  Their references and bars are stated where they are defined ("the optimizer tail").

Error model: each output element i gets its own bar
    |got_i - ref_i| <= c * (u_out * M_i + u_acc * sqrt(K) * S_i)
M_i is the sum of the magnitudes of the terms added into element i (the product sum, bias, row bias, residual, prior content), S_i is
sqrt(sum_k (a_k b_k)^2) over the K products of a reduction (the same operation on squared operands), u_out is the unit roundoff of the
stored type (2^-8 bf16, 2^-24 fp32) and u_acc = 2^-24 that of the fp32 accumulator.  Families whose error has another shape state their
model where they are defined.  A bar is never a fraction of the tensor-wide maximum.
"""
import ctypes
import math

import numpy as np
import torch
import torch.nn.functional as F

from ddpm_torch import _hip

F32, BF16 = 0, 1
U_BF16, U_F32 = 2.0 ** -8, 2.0 ** -24
U_ACC = 2.0 ** -24
GUARD = 64 * 1024                   # bytes of sentinel on each side of every buffer
SENTINEL = 0xA5
POISON = 0xFF                       # poison mode: NaN in fp32 and bf16, -1 in int64
C_GEMM = 4                          # c of the GEMM-shaped families (conv, dgrad, wgrad, gemm, atb, colsum, upsample backward)
C_NORM = 4                          # GroupNorm forward / backward
C_ATTN = 4                          # attention forward / backward
C_ELEM = 8                          # fp32 diffusion elementwise kernels (expf / sqrtf of the tables are a few ulp)
TINY = 1e-30                        # floor of a bar: an element whose every term is exactly zero must come out exactly zero
# fp32 operands on the matrix cores (v_mfma_f32_32x32x2_f32, csrc/gemm.hip Mma<float>) fold two products into the fp32 accumulator per
# step, and the ISA does not specify that step as a correctly rounded addition; a faithful one (error below one ulp of the accumulated
# value, 2 u_acc) is what bounds it.  Measured on the MI355X (W5-W8): the fp32 convs miss a float64 sum by 1.6x what a round-to-nearest
# sequential fp32 sum of the same products misses (1.19 of the u_acc bar at 16 M outputs, where round-to-nearest sums reach 0.72).
# The accumulation term of fp32 GEMM-shaped replays therefore uses 2 u_acc; bf16 products keep u_acc (their bars are set by the store).
U_ACC_MFMA_F32 = 2 * U_ACC


# ----------------------------------------------------------------------------------------------------------------- recording
def _is_ptr(t):
    return t is ctypes.c_void_p


def signature(name, args):
    types = _hip.PROTOTYPES[name]
    n = len(args) if name == "ddpm_stream_order" else len(args) - 1          # the last argument is the hipStream_t
    sig = []
    for a, t in zip(args[:n], types[:n]):
        if _is_ptr(t):
            a = int(a or 0)
            sig.append(("p", a == 0, a % 256))
        elif t is ctypes.c_float:
            sig.append(float(a))
        else:
            sig.append(int(a))
    return (name, tuple(sig))


class Recorder:
    """Callable that stands in for _hip._invoke: keeps the distinct signatures (in first-seen order) and calls through."""

    def __init__(self, inner):
        self.inner = inner
        self.sigs = {}
        self.tables = {}                    # signature of a table-driven launch -> the address of the table it read (resolve_tables)

    def __call__(self, name, args):
        sig = signature(name, args)
        self.sigs.setdefault(sig, None)
        if name in TABLE_ARG:
            self.tables.setdefault(sig, int(args[TABLE_ARG[name][0]] or 0))
        return self.inner(name, args)

    @property
    def names(self):
        return sorted({s[0] for s in self.sigs})


# ----------------------------------------------------------------------------------------------------------------- guarded buffers
_TD = {F32: torch.float32, BF16: torch.bfloat16, "i64": torch.int64, "u64": torch.int64}
_INT = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.int64: torch.int64}


class Arena:
    """All buffers of one replay, each between sentinel guard bands, allocated on `device`."""

    def __init__(self, device, seed, poison=False, profile=None, yardstick=False):
        self.device = device
        self.gen = torch.Generator().manual_seed(seed)                   # host draws (time steps)
        self.dgen = torch.Generator(device=device).manual_seed(seed)    # buffer contents, drawn where they live
        self.pgen = torch.Generator(device=device).manual_seed(seed + 7919)   # draws of a profile (masks): never the buffers' stream
        self.poison, self.profile, self.yardstick = poison, profile, yardstick
        self.amplify, self.rows_per_image = None, None      # replay(amplify=): see amplify_images
        assert profile is None or profile in PROFILES, profile
        self.bufs = []

    def buf(self, name, n, dtype, mod=0):
        b = Buf(name, n, _TD[dtype], mod, self.device)
        self.bufs.append(b)
        return b

    def randn(self, n, mean=0.0, scale=1.0):
        return torch.randn(n, generator=self.dgen, device=self.device) * scale + mean

    def shape(self, role, view, **kw):
        """Apply the active profile's transform for `role` (PROFILES) to a strided view of a buffer, in place; the values are formed
        in fp32 and stored in the buffer's type, and the references read the stored values.  No profile, or a profile without that
        role: nothing happens and nothing is drawn."""
        fn = PROFILES[self.profile][1].get(role) if self.profile else None
        if fn is not None and view.numel():
            view.copy_(fn(self, view.to(torch.float32), **kw))

    def shaped(self, role, values, **kw):
        """shape() for values that are not in a buffer yet."""
        fn = PROFILES[self.profile][1].get(role) if self.profile else None
        return values if fn is None else fn(self, values, **kw)

    def snapshot(self):
        if self.poison:
            for b in self.bufs:
                b.poison()
        for b in self.bufs:
            b.before = b.raw.clone()

    def check(self):
        """Guards intact, and nothing outside the declared outputs changed."""
        for b in self.bufs:
            lo, hi = b.start, b.start + b.nbytes
            assert torch.equal(b.raw[:lo], b.before[:lo]) and torch.equal(b.raw[hi:], b.before[hi:]), f"{b.name}: guard band overwritten"
            keep = ~b.written
            if bool(keep.any()):
                now, was = b.t.view(_INT[b.t.dtype]), b.before[lo:hi].view(_INT[b.t.dtype])
                bad = (now != was) & keep
                assert not bool(bad.any()), f"{b.name}: {int(bad.sum())} element(s) outside the contract's output changed"


class Buf:
    def __init__(self, name, n, dtype, mod, device):
        es = torch.empty(0, dtype=dtype).element_size()
        self.name, self.n = name, max(int(n), 1)
        self.nbytes = self.n * es
        self.raw = torch.full((GUARD + 256 + self.nbytes + GUARD,), SENTINEL, dtype=torch.uint8, device=device)
        self.start = GUARD + (mod - self.raw.data_ptr() - GUARD) % 256          # address of the first element = mod (modulo 256)
        self.t = self.raw[self.start:self.start + self.nbytes].view(dtype)
        self.written = torch.zeros(self.n, dtype=torch.bool, device=device)
        self.ptr = self.raw.data_ptr() + self.start
        # poison mode: the elements the contract lets the call READ (inp / all_in); every other element, and both guard bands, are
        # overwritten with POISON before the first snapshot.  A buffer that declares nothing is poisoned whole.
        self.readable = torch.zeros(self.n, dtype=torch.bool, device=device)
        self.poisoned = False
        self.atomic = False             # an fp32-atomic accumulation target: its bits depend on the order of arrival
        self.scratch = False            # a workspace whose final content the contract does not state
        self.result = None              # mask of the written elements whose content the contract states (None: all of them)

    def inp(self, rows, cols, ld, off=0):
        """The call may read the [rows][cols] elements with pitch ld starting `off` elements in."""
        if rows > 0 and cols > 0:
            self.readable.as_strided((rows, cols), (ld, 1), off).fill_(True)
        return self

    def all_in(self):
        self.readable.fill_(True)
        return self

    def poison(self):
        if self.poisoned:
            return
        self.poisoned = True
        self.raw[:self.start] = POISON
        self.raw[self.start + self.nbytes:] = POISON
        self.t.view(_INT[self.t.dtype])[~self.readable] = -1

    def fill(self, values):
        self.t.copy_(values.to(self.t.dtype).reshape(-1)[:self.n])
        return self

    def mat(self, rows, cols, ld, off=0):
        """[rows][cols] view with pitch ld starting `off` elements in."""
        return self.t.as_strided((rows, cols), (ld, 1), self.t.storage_offset() + off)

    def out(self, rows, cols, ld, off=0):
        self.written.as_strided((rows, cols), (ld, 1), off).fill_(True)
        return self.mat(rows, cols, ld, off)

    def all_out(self):
        self.written.fill_(True)
        return self.t


def pitched(rows, cols, ld):
    return (rows - 1) * ld + cols if rows > 0 else 0


def _d(t):
    return t.to(torch.float64)


F64_SLICE = 8 << 30                 # bytes of float64 working set per slice of images in the largest references (W13: B = 2048)


def image_slices(B, per_image):
    """[(b0, b1)] covering the B images so that a slice's float64 working set (per_image elements an image) stays near F64_SLICE:
    the references of operands >= 1 GiB run in several passes instead of one pass that would need tens of GB of device memory."""
    n = max(1, int(F64_SLICE // (8 * max(per_image, 1))))
    return [(b0, min(B, b0 + n)) for b0 in range(0, B, n)]


class Result:
    def __init__(self, sig, nonfinite=False):
        self.sig, self.worst, self.where, self.max_bytes = sig, 0.0, "", 0
        self.nonfinite = nonfinite          # the `nonfinite_*` profiles: cmp_nonfinite stands in for cmp
        self.yard, self.yard_where = None, ""
        self.planted = {}                   # what -> number of elements the float64 reference makes non-finite
        self.outputs = {}                   # buffer name -> the stored output elements (replay() fills it)
        self.tensors = {}                   # table-driven entries: (row, column name) -> that row's output, whatever the packing
        self.depth, self.clip = None, None  # reductions: the chain length of the bound; the update: the float64 clip coefficient
        self.sensitivity = {}               # (output, image) -> fraction of elements the loss of that image moves by > 8 bars (amplify=)

    def cmp(self, what, got, ref, bar, yard=None):
        """yard (optional): the yardstick's value of the same output, put through the same bar; it never decides a replay."""
        if self.nonfinite:
            return self.cmp_nonfinite(what, got, ref, bar)
        got, ref, bar = _d(got), ref.to(got.device), bar.to(got.device)
        assert bool(torch.isfinite(got).all()), f"{what}: non-finite output"
        r = float(((got - ref).abs() / (bar + TINY)).max()) if got.numel() else 0.0
        if r >= self.worst:
            self.worst, self.where = r, what
        if yard is not None and got.numel():
            ry = float(((_d(yard).to(got.device) - ref).abs() / (bar + TINY)).max())
            if self.yard is None or ry >= self.yard:
                self.yard, self.yard_where = ry, what
        return r

    def cmp_nonfinite(self, what, got, ref, bar):
        """cmp for inputs that hold a NaN or an inf: wherever the float64 reference is non-finite the output must be non-finite, and
        everywhere else it must be finite and within its bar."""
        got, ref, bar = _d(got), ref.to(got.device), bar.to(got.device)
        nf = ~torch.isfinite(ref)
        self.planted[what] = self.planted.get(what, 0) + int(nf.sum())
        swallowed = nf & torch.isfinite(got)
        assert not bool(swallowed.any()), f"{what}: {int(swallowed.sum())} of {int(nf.sum())} element(s) finite where the reference is not"
        ok = ~nf
        assert bool(torch.isfinite(got[ok]).all()), f"{what}: {int((~torch.isfinite(got) & ok).sum())} non-finite element(s) where the reference is finite"
        assert bool(torch.isfinite(bar[ok]).all()), f"{what}: the bar is non-finite where the reference is finite"
        r = float(((got[ok] - ref[ok]).abs() / (bar[ok] + TINY)).max()) if bool(ok.any()) else 0.0
        if r >= self.worst:
            self.worst, self.where = r, what
        return r


# ----------------------------------------------------------------------------------------------------------------- fp64 convolution
def canvas(x, Ho, Wo, R, S, stride, pad_t, pad_l, upsample, dilate):
    """x [B,H,W,C] (NHWC) -> zero canvas [B, (Ho-1)*stride+R, (Wo-1)*stride+S, C] on which a VALID correlation with stride `stride`
    gathers exactly the contract's  x[b, f(oy*stride + r - pad_t), f(ox*stride + s - pad_l), c]  (zero outside the virtual grid)."""
    B, H, W, C = x.shape
    if upsample:
        xv = x.repeat_interleave(2, 1).repeat_interleave(2, 2)
    elif dilate:
        xv = x.new_zeros(B, 2 * H - 1, 2 * W - 1, C)
        xv[:, ::2, ::2] = x
    else:
        xv = x
    nh, nw = (Ho - 1) * stride + R, (Wo - 1) * stride + S
    can = x.new_zeros(B, nh, nw, C)
    hv, wv = xv.shape[1], xv.shape[2]
    ys, xs = max(0, -pad_t), max(0, -pad_l)
    ye, xe = min(hv, nh - pad_t), min(wv, nw - pad_l)
    if ye > ys and xe > xs:
        can[:, pad_t + ys:pad_t + ye, pad_l + xs:pad_l + xe] = xv[:, ys:ye, xs:xe]
    return can


def _tap(can, r, s, Ho, Wo, stride):
    return can[:, r:r + (Ho - 1) * stride + 1:stride, s:s + (Wo - 1) * stride + 1:stride]


def conv_fp64(can, w, Ho, Wo, stride):
    """y[b,oy,ox,n] = sum_{r,s,c} can[b, oy*stride+r, ox*stride+s, c] * w[n,r,s,c]  (w: [N,R,S,C], all float64) by R*S matmuls."""
    N, R, S, C = w.shape
    y = can.new_zeros(can.shape[0], Ho, Wo, N)
    for r in range(R):
        for s in range(S):
            y += _tap(can, r, s, Ho, Wo, stride) @ w[:, r, s, :].T
    return y


def wgrad_fp64(can, dy, R, S, Ho, Wo, stride):
    """dw[n,r,s,c] = sum_{b,oy,ox} dy[b,oy,ox,n] * can[b, oy*stride+r, ox*stride+s, c]  ->  [N,R,S,C]."""
    N, C = dy.shape[-1], can.shape[-1]
    P = dy.numel() // N
    out = can.new_zeros(N, R, S, C)
    if P >= 1 << 18 and P % 1024 == 0:
        # millions of pixels into one N x C tile: a single matmul keeps a few compute units busy for tens of seconds; partial sums over
        # runs of 1024 pixels as one batched product, added up afterwards (float64 either way)
        g = dy.reshape(-1, 1024, N).transpose(1, 2)
        for r in range(R):
            for s in range(S):
                out[:, r, s] = torch.bmm(g, _tap(can, r, s, Ho, Wo, stride).reshape(-1, 1024, C)).sum(0)
        return out
    g = dy.reshape(-1, N).T
    for r in range(R):
        for s in range(S):
            out[:, r, s] = g @ _tap(can, r, s, Ho, Wo, stride).reshape(-1, C)
    return out


# ----------------------------------------------------------------------------------------------------------------- replay builders
def _launch(name, args):
    _hip._invoke(name, list(args) + [_hip.stream() if torch.device(_DEVICE[0]).type == "cuda" else 0])


_DEVICE = ["cpu"]


def _ptr(b):
    return 0 if b is None else b.ptr


def _opt(sig_entry):
    return not sig_entry[1]            # pointer present


def _mod(sig_entry):
    return sig_entry[2]


def rep_conv2d(A, sig, res):
    (px, x_ld, pw, py, y_ld, pb, prb, rb_ld, pres, res_ld, B, H, W, C, Ho, Wo, N, R, S, stride, pad_t, pad_l, ups, dil, acc, mode,
     splits, pws, pcnt, dt) = sig
    M = B * Ho * Wo
    odt = dt if mode == 0 else F32
    x = A.buf("x", pitched(B * H * W, C, x_ld), dt, _mod(px))
    w = A.buf("w", N * R * S * C, dt, _mod(pw))
    ny = B * N * Ho * Wo if mode == 3 else pitched(M, N, y_ld)
    y = A.buf("y", ny, odt, _mod(py))
    bias = A.buf("bias", N, F32, _mod(pb)) if _opt(pb) else None
    rb = A.buf("rowbias", pitched(B, N, rb_ld), F32, _mod(prb)) if _opt(prb) else None
    r_ = A.buf("residual", pitched(M, N, res_ld), dt, _mod(pres)) if _opt(pres) else None
    ws = cnt = None
    if _opt(pws):
        tiles = max(-(-M // 128) * -(-N // 128) * 16384, -(-M // 64) * -(-N // 64) * 4096) * max(splits, 1)
        if splits == 2:
            tiles = max(tiles, 256 * 4096)
        ws = A.buf("splitk_ws", tiles, F32, _mod(pws))
        ws.fill(torch.full((ws.n,), float("nan"))).all_out()
    if _opt(pcnt):
        cnt = A.buf("splitk_cnt", -(-M // 64) * -(-N // 64), F32, _mod(pcnt))
        cnt.fill(torch.zeros(cnt.n))
        cnt.all_out()
    K = R * S * C
    x.fill(A.randn(x.n))
    w.fill(A.randn(w.n, scale=1.0 / math.sqrt(K)))       # products O(1): bias, row bias and residual weigh as much as the sum
    y.fill(A.randn(y.n))
    for b in (bias, rb, r_):
        if b is not None:
            b.fill(A.randn(b.n))
    x.inp(B * H * W, C, x_ld)
    w.all_in()
    A.shape("data", x.mat(B * H * W, C, x_ld))
    for b, v in ((bias, (1, N, N)), (rb, (B, N, rb_ld)), (r_, (M, N, res_ld))):
        if b is not None:
            A.shape("additive", b.inp(*v).mat(*v))
    if acc:                                                 # the prior content is an operand; otherwise it is overwritten
        A.shape("additive", y.all_in().t if mode == 3 else y.inp(M, N, y_ld).mat(M, N, y_ld))
    if ws is not None:
        ws.scratch = True
    if cnt is not None:
        cnt.all_in()                                        # zero on entry (contract)
    prior = _d(y.t).clone()
    if mode == 3:
        y.all_out()
    else:
        y.out(M, N, y_ld)
    A.snapshot()
    _launch("ddpm_conv2d_nhwc", [x.ptr, x_ld, w.ptr, y.ptr, y_ld, _ptr(bias), _ptr(rb), rb_ld, _ptr(r_), res_ld, B, H, W, C, Ho, Wo, N,
                                 R, S, stride, pad_t, pad_l, ups, dil, acc, mode, splits, _ptr(ws), _ptr(cnt), dt])
    sync()
    A.check()
    if cnt is not None:
        assert not bool(cnt.t.view(torch.int32).any()), "split-K counters not left zero"
    wt = _d(w.t).reshape(N, R, S, C)
    HWo = Ho * Wo
    nh, nw = (Ho - 1) * stride + R, (Wo - 1) * stride + S
    u = U_BF16 if odt == BF16 else U_F32
    ua = U_ACC_MFMA_F32 if dt == F32 else U_ACC
    for b0, b1 in image_slices(B, 3 * nh * nw * C + 8 * HWo * N):
        r0, r1 = b0 * HWo, b1 * HWo
        xs = _d(x.mat(B * H * W, C, x_ld)[b0 * H * W:b1 * H * W]).reshape(b1 - b0, H, W, C)
        can = canvas(xs, Ho, Wo, R, S, stride, pad_t, pad_l, ups, dil)
        ref = conv_fp64(can, wt, Ho, Wo, stride).reshape(-1, N)
        mag = ref.abs()
        sq = conv_fp64(can * can, wt * wt, Ho, Wo, stride).reshape(-1, N).sqrt()
        del can
        if bias is not None:
            ref = ref + _d(bias.t)[None]
            mag = mag + _d(bias.t).abs()[None]
        if rb is not None:
            v = _d(rb.mat(B, N, rb_ld)[b0:b1]).repeat_interleave(HWo, 0)
            ref, mag = ref + v, mag + v.abs()
        if r_ is not None:
            v = _d(r_.mat(M, N, res_ld)[r0:r1])
            ref, mag = ref + v, mag + v.abs()
        if mode == 3:
            got = _d(y.mat(B * N, HWo, HWo)[b0 * N:b1 * N]).reshape(b1 - b0, N, HWo).permute(0, 2, 1).reshape(-1, N)
            pv = prior.reshape(B, N, HWo)[b0:b1].permute(0, 2, 1).reshape(-1, N)
        else:
            got = _d(y.mat(M, N, y_ld)[r0:r1])
            pv = prior.as_strided((M, N), (y_ld, 1))[r0:r1]
        if acc:
            ref, mag = ref + pv, mag + pv.abs()
        bar = C_GEMM * (u * mag + ua * math.sqrt(K) * sq)
        res.cmp("y", got, ref, bar)


def _slab_setup(A, name, n_one, copies, stride, mod):
    b = A.buf(name, (copies - 1) * stride + n_one if copies > 1 else n_one, F32, mod)
    b.fill(torch.full((b.n,), float("nan")))
    for s in range(copies):
        b.written[s * stride:s * stride + n_one] = True
    return b


def _reduce_slabs(A, slab, n_one, copies, stride):
    """ddpm_wgrad_reduce over the copies, as the step runs it; returns the reduced [n_one] floats."""
    dst = A.buf(slab.name + "_reduced", n_one, F32)
    dst.all_out()
    tab = torch.tensor([slab.ptr, dst.ptr, n_one, copies, stride], dtype=torch.int64, device=A.device)
    A.snapshot()
    _launch("ddpm_wgrad_reduce", [tab.data_ptr(), 1])
    sync()
    A.check()
    return dst.t


def amplify_images(A, view, rows_per_image, ld, es):
    """Reductions over millions of pixels (LARGE_OPERANDS): one lost image would move the sum by a few bars only, so the rows of three
    images of `view` ([rows][cols], pitch ld, elements of es bytes) — the first, the last and the one whose bytes straddle offset 2^30
    of the operand — are multiplied by A.amplify (a power of two: exact in either type).  Returns the three image indices; nothing
    happens (and () comes back) when the replay was not asked to amplify."""
    if not A.amplify:
        return ()
    B = view.shape[0] // rows_per_image
    picked = sorted({0, min(B - 1, (1 << 30) // (rows_per_image * ld * es)), B - 1})
    for b in picked:
        view[b * rows_per_image:(b + 1) * rows_per_image] *= A.amplify
    return tuple(picked)


def _sensitivity(res, what, contributions, bar):
    """Result.sensitivity[(what, image)]: the fraction of the output elements that dropping that image alone would move by more than
    8 bars, measured on the float64 reference (contributions: image -> its float64 share of the sum)."""
    for b, c in contributions.items():
        res.sensitivity[(what, b)] = float((c.abs() > 8 * bar).double().mean())


def _wgrad_common(A, res, dy_b, x_b, pieces, R, S, Ho, Wo, stride, Nreal, Creal, dw, slab_stride, copies, prior, dbias=None,
                  bias_stride=0, bprior=None, amplified=()):
    """pieces: iterable of (can, dy, b0) — the float64 canvas and output gradient of the images b0 .. of one slice (image_slices):
    the sums over all slices are the reference, so that operands of 2 GiB never need their float64 copy whole."""
    n_one = Nreal * R * S * Creal
    full = sq = g1 = g2 = None
    K, share = 0, {}
    cut = lambda t: t[:Nreal, :, :, :Creal].reshape(-1)
    for can, dy, b0 in pieces:
        f = cut(wgrad_fp64(can, dy, R, S, Ho, Wo, stride))
        q = cut(wgrad_fp64(can * can, dy * dy, R, S, Ho, Wo, stride))
        g = dy.reshape(-1, dy.shape[-1])[:, :Nreal]
        full, sq = (f, q) if full is None else (full + f, sq + q)
        g1, g2 = (g.sum(0), (g * g).sum(0)) if g1 is None else (g1 + g.sum(0), g2 + (g * g).sum(0))
        K += dy.shape[0] * Ho * Wo
        for b in amplified:
            if b0 <= b < b0 + dy.shape[0]:
                share[b] = cut(wgrad_fp64(can[b - b0:b - b0 + 1], dy[b - b0:b - b0 + 1], R, S, Ho, Wo, stride))
        del can, dy, f, q, g
    mag, sq = full.abs(), sq.sqrt()
    ua = U_ACC_MFMA_F32 if dy_b.t.dtype == torch.float32 else U_ACC
    if slab_stride == 0:
        got = dw.t[:n_one]
        full, mag = full + prior, mag + prior.abs()
    else:
        got = _reduce_slabs(A, dw, n_one, copies, slab_stride)
    bar = C_GEMM * (U_F32 * mag + ua * math.sqrt(K) * sq)
    res.cmp("dw", got, full, bar)
    _sensitivity(res, "dw", share, bar)
    if dbias is not None:
        ref, sq = g1, g2.sqrt()
        mag = ref.abs()
        if bias_stride == 0 and slab_stride == 0:
            got = dbias.t[:Nreal]
            ref, mag = ref + bprior, mag + bprior.abs()
        else:
            got = _reduce_slabs(A, dbias, Nreal, copies, bias_stride)
        res.cmp("dbias", got, ref, C_GEMM * (U_F32 * mag + U_ACC * math.sqrt(K) * sq))


def _wgrad_launch(A, name, args):
    A.snapshot()
    _launch(name, args)
    sync()
    A.check()


def rep_conv3x3_wgrad(A, sig, res, up=False):
    pdy, dy_ld, px, x_ld, pdw, slab_stride, pdb, bias_stride, B, H, W, C, N, Nreal, splits, dt = sig
    Hs, Ws = (H // 2, W // 2) if up else (H, W)
    copies = _hip.lib().ddpm_conv3x3_wgrad_splits(B, H, W, C, N, splits) if slab_stride else 1
    assert copies > 0
    dy = A.buf("dy", pitched(B * H * W, N, dy_ld), dt, _mod(pdy)).fill(A.randn(pitched(B * H * W, N, dy_ld)))
    x = A.buf("x", pitched(B * Hs * Ws, C, x_ld), dt, _mod(px)).fill(A.randn(pitched(B * Hs * Ws, C, x_ld)))
    A.shape("data", dy.inp(B * H * W, N, dy_ld).mat(B * H * W, N, dy_ld))
    amplified = amplify_images(A, dy.mat(B * H * W, N, dy_ld), H * W, dy_ld, 2)
    x.inp(B * Hs * Ws, C, x_ld)
    n_one = Nreal * 9 * C
    if slab_stride:
        dw = _slab_setup(A, "dw", n_one, copies, slab_stride, _mod(pdw))
        db = _slab_setup(A, "dbias", Nreal, copies, bias_stride, _mod(pdb)) if _opt(pdb) else None
        prior = bprior = None
    else:
        dw = A.buf("dw", n_one, F32, _mod(pdw)).fill(A.randn(n_one))
        dw.all_out()
        A.shape("additive", dw.all_in().t)
        dw.atomic = True
        prior = _d(dw.t).clone()
        db = A.buf("dbias", Nreal, F32, _mod(pdb)).fill(A.randn(Nreal)) if _opt(pdb) else None
        if db is not None:
            db.all_out()
            A.shape("additive", db.all_in().t)
            db.atomic = True
        bprior = None if db is None else _d(db.t).clone()
    _wgrad_launch(A, "ddpm_conv3x3_wgrad_up_nhwc" if up else "ddpm_conv3x3_wgrad_nhwc",
                  [dy.ptr, dy_ld, x.ptr, x_ld, dw.ptr, slab_stride, _ptr(db), bias_stride, B, H, W, C, N, Nreal, splits, dt])
    def pieces():
        for b0, b1 in image_slices(B, 5 * (H + 2) * (W + 2) * C + 4 * H * W * N):
            xs = _d(x.mat(B * Hs * Ws, C, x_ld)[b0 * Hs * Ws:b1 * Hs * Ws]).reshape(b1 - b0, Hs, Ws, C)
            g = _d(dy.mat(B * H * W, N, dy_ld)[b0 * H * W:b1 * H * W]).reshape(b1 - b0, H, W, N)
            yield canvas(xs, H, W, 3, 3, 1, 1, 1, int(up), 0), g, b0
    _wgrad_common(A, res, dy, x, pieces(), 3, 3, H, W, 1, Nreal, C, dw, slab_stride, copies, prior, db, bias_stride, bprior, amplified)


def rep_conv3x3_wgrad_up(A, sig, res):
    rep_conv3x3_wgrad(A, sig, res, up=True)


def rep_conv1x1_wgrad(A, sig, res):
    pdy, dy_ld, px, x_ld, pdw, slab_stride, pdb, bias_stride, P, C, N, splits, dt = sig
    if splits <= 0:                    # a hand-written signature (ODD_GEOMETRY): the slab count the library plans for this geometry
        splits = int(_hip.lib().ddpm_conv1x1_wgrad_splits(P, C, N))
    assert slab_stride > 0 and splits >= 1
    dy = A.buf("dy", pitched(P, N, dy_ld), dt, _mod(pdy)).fill(A.randn(pitched(P, N, dy_ld)))
    x = A.buf("x", pitched(P, C, x_ld), dt, _mod(px)).fill(A.randn(pitched(P, C, x_ld)))
    A.shape("data", dy.inp(P, N, dy_ld).mat(P, N, dy_ld))
    rpi = A.rows_per_image or P                           # a 1x1 weight gradient has no images of its own: the table row names them
    amplified = amplify_images(A, dy.mat(P, N, dy_ld), rpi, dy_ld, 2)
    x.inp(P, C, x_ld)
    dw = _slab_setup(A, "dw", N * C, splits, slab_stride, _mod(pdw))
    db = _slab_setup(A, "dbias", N, splits, bias_stride, _mod(pdb)) if _opt(pdb) else None
    _wgrad_launch(A, "ddpm_conv1x1_wgrad_nhwc", [dy.ptr, dy_ld, x.ptr, x_ld, dw.ptr, slab_stride, _ptr(db), bias_stride, P, C, N, splits, dt])
    def pieces():
        for b0, b1 in image_slices(P // rpi, 3 * rpi * (C + N)):
            yield (_d(x.mat(P, C, x_ld)[b0 * rpi:b1 * rpi]).reshape(b1 - b0, rpi, 1, C),
                   _d(dy.mat(P, N, dy_ld)[b0 * rpi:b1 * rpi]).reshape(b1 - b0, rpi, 1, N), b0)
    _wgrad_common(A, res, dy, x, pieces(), 1, 1, rpi, 1, 1, N, C, dw, slab_stride, splits, None, db, bias_stride, None, amplified)


def rep_conv2d_wgrad(A, sig, res):
    (pdy, dy_ld, px, x_ld, pdw, slab_stride, B, H, W, C, Creal, Ho, Wo, N, Nreal, R, S, stride, pad_t, pad_l, ups, splits, dt) = sig
    dy = A.buf("dy", pitched(B * Ho * Wo, N, dy_ld), dt, _mod(pdy)).fill(A.randn(pitched(B * Ho * Wo, N, dy_ld)))
    x = A.buf("x", pitched(B * H * W, C, x_ld), dt, _mod(px)).fill(A.randn(pitched(B * H * W, C, x_ld)))
    A.shape("data", dy.inp(B * Ho * Wo, N, dy_ld).mat(B * Ho * Wo, N, dy_ld))
    amplified = amplify_images(A, dy.mat(B * Ho * Wo, N, dy_ld), Ho * Wo, dy_ld, 2 if dt == BF16 else 4)
    x.inp(B * H * W, C, x_ld)
    n_one = Nreal * R * S * Creal
    if slab_stride:
        copies = splits
        dw = _slab_setup(A, "dw", n_one, copies, slab_stride, _mod(pdw))
        prior = None
    else:
        copies = 1
        dw = A.buf("dw", n_one, F32, _mod(pdw)).fill(A.randn(n_one))
        dw.all_out()
        A.shape("additive", dw.all_in().t)
        dw.atomic = True
        prior = _d(dw.t).clone()
    _wgrad_launch(A, "ddpm_conv2d_wgrad_nhwc", [dy.ptr, dy_ld, x.ptr, x_ld, dw.ptr, slab_stride, B, H, W, C, Creal, Ho, Wo, N, Nreal,
                                               R, S, stride, pad_t, pad_l, ups, splits, dt])
    def pieces():
        nh, nw = (Ho - 1) * stride + R, (Wo - 1) * stride + S
        for b0, b1 in image_slices(B, 5 * nh * nw * C + 4 * Ho * Wo * N):
            xs = _d(x.mat(B * H * W, C, x_ld)[b0 * H * W:b1 * H * W]).reshape(b1 - b0, H, W, C)
            g = _d(dy.mat(B * Ho * Wo, N, dy_ld)[b0 * Ho * Wo:b1 * Ho * Wo]).reshape(b1 - b0, Ho, Wo, N)
            yield canvas(xs, Ho, Wo, R, S, stride, pad_t, pad_l, ups, 0), g, b0
    _wgrad_common(A, res, dy, x, pieces(), R, S, Ho, Wo, stride, Nreal, Creal, dw, slab_stride, copies, prior, amplified=amplified)


def rep_wgrad_reduce(A, sig, res):
    """Stand-alone check of the fixed-order slab sum (the slab replays above also run it): copies of random partials.  A hand-written
    signature may name (floats, copies, stride) behind the two recorded words."""
    n_one, copies, stride = sig[2:5] if len(sig) >= 5 else (1000, 3, 1024)
    slab = A.buf("slabs", (copies - 1) * stride + n_one, F32).fill(A.randn((copies - 1) * stride + n_one))
    for c in range(copies):
        A.shape("data", slab.inp(1, n_one, n_one, c * stride).mat(1, n_one, n_one, c * stride))
    got = _reduce_slabs(A, slab, n_one, copies, stride)
    parts = torch.stack([_d(slab.t[s * stride:s * stride + n_one]) for s in range(copies)])
    # a short fixed-order fp32 sum: the worst-case bound u * sum |partials| (M of every added term)
    res.cmp("sum", got, parts.sum(0), C_GEMM * U_F32 * parts.abs().sum(0))


def rep_gemm(A, sig, res):
    (pa, a_ld, a_bs, a_tr, pb, b_ld, b_bs, b_tr, pc, c_ld, c_bs, pbias, pres, res_ld, res_bs, M, N, K, batch, alpha, acc, mode, splits,
     dt) = sig
    odt = dt if mode == 0 else F32
    na = (batch - 1) * a_bs + (pitched(K, M, a_ld) if a_tr else pitched(M, K, a_ld))
    nb = (batch - 1) * b_bs + (pitched(K, N, b_ld) if b_tr else pitched(N, K, b_ld))
    nc = (batch - 1) * c_bs + pitched(M, N, c_ld)
    a = A.buf("a", na, dt, _mod(pa)).fill(A.randn(na))
    b = A.buf("b", nb, dt, _mod(pb)).fill(A.randn(nb, scale=1.0 / math.sqrt(K)))
    c = A.buf("c", nc, odt, _mod(pc)).fill(A.randn(nc))
    bias = A.buf("bias", N, F32, _mod(pbias)).fill(A.randn(N)) if _opt(pbias) else None
    r_ = None
    if _opt(pres):
        nr = (batch - 1) * res_bs + pitched(M, N, res_ld)
        r_ = A.buf("residual", nr, dt, _mod(pres)).fill(A.randn(nr))
    for i in range(batch):
        av = (K, M, a_ld, i * a_bs) if a_tr else (M, K, a_ld, i * a_bs)
        A.shape("data", a.inp(*av).mat(*av), k_axis=0 if a_tr else 1)
        b.inp(*((K, N, b_ld, i * b_bs) if b_tr else (N, K, b_ld, i * b_bs)))
        if r_ is not None:
            A.shape("additive", r_.inp(M, N, res_ld, i * res_bs).mat(M, N, res_ld, i * res_bs))
        if acc or mode == 2:
            A.shape("additive", c.inp(M, N, c_ld, i * c_bs).mat(M, N, c_ld, i * c_bs))
    if bias is not None:
        A.shape("additive", bias.all_in().t)
    c.atomic = mode == 2
    prior = _d(c.t).clone()
    A.snapshot()
    _launch("ddpm_gemm", [a.ptr, a_ld, a_bs, a_tr, b.ptr, b_ld, b_bs, b_tr, c.ptr, c_ld, c_bs, _ptr(bias), _ptr(r_), res_ld, res_bs,
                          M, N, K, batch, alpha, acc, mode, splits, dt])
    sync()
    for i in range(batch):
        c.out(M, N, c_ld, i * c_bs)
    A.check()
    u = U_BF16 if odt == BF16 else U_F32
    ua = U_ACC_MFMA_F32 if dt == F32 else U_ACC
    for i in range(batch):
        Am = _d(a.mat(K, M, a_ld, i * a_bs)).T if a_tr else _d(a.mat(M, K, a_ld, i * a_bs))
        Bm = _d(b.mat(K, N, b_ld, i * b_bs)).T if b_tr else _d(b.mat(N, K, b_ld, i * b_bs))
        ref = alpha * Am @ Bm.T
        mag = ref.abs()
        sq = abs(alpha) * ((Am * Am) @ (Bm * Bm).T).sqrt()
        if bias is not None:
            ref, mag = ref + _d(bias.t)[None], mag + _d(bias.t).abs()[None]
        if r_ is not None:
            v = _d(r_.mat(M, N, res_ld, i * res_bs))
            ref, mag = ref + v, mag + v.abs()
        if acc or mode == 2:
            v = prior.as_strided((M, N), (c_ld, 1), i * c_bs)
            ref, mag = ref + v, mag + v.abs()
        res.cmp(f"c[{i}]", c.mat(M, N, c_ld, i * c_bs), ref, C_GEMM * (u * mag + ua * math.sqrt(K) * sq))


def rep_atb(A, sig, res):
    pa, lda, pb, ldb, pc, ldc, M, N, K = sig
    a = A.buf("a", pitched(K, M, lda), F32, _mod(pa)).fill(A.randn(pitched(K, M, lda)))
    b = A.buf("b", pitched(K, N, ldb), F32, _mod(pb)).fill(A.randn(pitched(K, N, ldb)))
    c = A.buf("c", pitched(M, N, ldc), F32, _mod(pc)).fill(A.randn(pitched(M, N, ldc)))
    A.shape("data", a.inp(K, M, lda).mat(K, M, lda))
    b.inp(K, N, ldb)
    A.snapshot()
    _launch("ddpm_atb_f32", [a.ptr, lda, b.ptr, ldb, c.ptr, ldc, M, N, K])
    sync()
    got = c.out(M, N, ldc)
    A.check()
    Am, Bm = _d(a.mat(K, M, lda)), _d(b.mat(K, N, ldb))
    # K = the batch: a short fixed-order fp32 reduction, held to the worst-case bound of such a sum (M = sum_k |a_k b_k|)
    ref, sq = Am.T @ Bm, ((Am * Am).T @ (Bm * Bm)).sqrt()
    mag = Am.abs().T @ Bm.abs()
    res.cmp("c", got, ref, C_GEMM * (U_F32 * mag + U_ACC * math.sqrt(K) * sq))


# GroupNorm ---------------------------------------------------------------------------------------------------------------------------
_M32 = 0xFFFFFFFF


def _mul32(x, c):
    """(x * c) mod 2^32 for int64 tensors holding uint32 values (split so no product leaves int64)."""
    return (x * (c & 0xFFFF) + (((x * (c >> 16)) & 0xFFFF) << 16)) & _M32


def _mix32(x):
    x = x ^ (x >> 16)
    x = _mul32(x, 0x7FEB352D)
    x = x ^ (x >> 15)
    x = _mul32(x, 0x846CA68B)
    return x ^ (x >> 16)


def keep_mask(seed, idx, p):
    """Dropout keep mask for linear element indices idx (int64 tensor): a torch restatement of abi_emulator._keep_mask (the hash of
    dropout_keep() in csrc/common.h) that runs where idx lives; the host check holds the two bit-equal."""
    th = p * 65536.0
    thresh = 0 if th <= 0 else (65536 if th >= 65536.0 else int(th + 0.5))
    pair = idx >> 1
    lo, hi = pair & _M32, (pair >> 32) & _M32
    s_lo, s_hi = seed & _M32, (seed >> 32) & _M32
    w = _mix32(lo ^ _mix32((hi + s_lo) & _M32) ^ ((s_hi * 0x9E3779B9) & _M32))
    field = torch.where((idx & 1) == 1, w >> 16, w & 0xFFFF)
    return field >= thresh


def _keep(A, B, HW, C, drop_p, seed, b0=0):
    """Keep mask of the dropout after the GroupNorm for images b0 .. b0 + B - 1, linear NHWC index b*HW*C + p*C + c (not the
    library's mask hook)."""
    idx = torch.arange(b0 * HW * C, (b0 + B) * HW * C, dtype=torch.int64, device=A.device)
    return keep_mask(seed & ((1 << 64) - 1), idx, drop_p).to(torch.float64).reshape(B, HW, C)


def _gn_stats(x, G, eps):
    B, HW, C = x.shape
    xg = x.reshape(B, HW, G, C // G).permute(0, 2, 1, 3).reshape(B, G, -1)
    mean, var = xg.mean(-1), xg.var(-1, unbiased=False)
    return mean, 1.0 / torch.sqrt(var + eps)


def _per_c(v, B, HW, C, G):
    """[B,G] -> [B,HW,C]"""
    return v.repeat_interleave(C // G, 1)[:, None, :].expand(B, HW, C)


def _seed(A, pseed, seed, drop_p):
    if not _opt(pseed):
        return None, seed
    word = A.buf("seed_dev", 1, "u64", _mod(pseed))
    w = 0x5DEECE66D
    word.t.fill_(w)
    word.all_in()
    return word, (seed + w) & ((1 << 64) - 1)


def rep_gn_fwd(A, sig, res):
    """GroupNorm(G) -> SiLU -> dropout.  t = gamma * xh + beta with xh = (x - mean) * rstd; y = drop(silu(t)).
    Model: M_i = |y_i| (the bf16 / fp32 store) and the fp32 statistics term  sqrt(n) * (|gamma| (|x| + |mean|) rstd + |beta|) * |y'(t)|
    with y' = silu'(t) * keep / (1 - p)  (n = (C/G) * HW, the statistics are sums of n terms; |x| + |mean| bounds the magnitude of the
    centred value the kernel forms about its pivot).  Statistics: mean to u_acc * sqrt(n) * (|mean| + std), rstd to u_acc * sqrt(n).
    fp32 stores add the fp32 evaluation of silu(t) and of the dropout scale, relative to |y|:  e_silu = _sigmoid_err(t) - 1 (the fast exp
    and 1 + e, see rep_silu_fwd) + 2 (the hardware reciprocal of silu_fast_, 1 ulp) + 1 (t * s) + 1 (* keep / (1 - p)), in units of
    u_acc.  Where silu'(t) = 0 (t = -1.28) the statistics term vanishes and this is the whole error; a bf16 store is 2^16 times coarser
    and its bar is left as it was."""
    px, x_ld, py, y_ld, pg, pb, pst, pws, B, HW, C, G, eps, silu, drop_p, seed, pseed, dt = sig
    x = A.buf("x", pitched(B * HW, C, x_ld), dt, _mod(px)).fill(A.randn(pitched(B * HW, C, x_ld), mean=1.5))
    y = A.buf("y", pitched(B * HW, C, y_ld), dt, _mod(py)).fill(A.randn(pitched(B * HW, C, y_ld)))
    g = A.buf("gamma", C, F32, _mod(pg)).fill(1.0 + 0.3 * A.randn(C))
    b = A.buf("beta", C, F32, _mod(pb)).fill(0.5 * A.randn(C))
    st = A.buf("stats", B * G * 2, F32, _mod(pst)) if _opt(pst) else None
    nws = int(_hip.lib().ddpm_gn_workspace_floats(B, HW, C, G, dt))
    ws = A.buf("workspace", nws, F32, _mod(pws)).fill(torch.zeros(nws))
    ws.all_out()
    ws.scratch = True                                     # the header does not state its initial content: poisoned
    if st is not None:
        st.all_out()
    A.shape("gn_x", x.inp(B * HW, C, x_ld).mat(B * HW, C, x_ld), B=B, HW=HW, C=C, G=G)
    A.shape("gn_gamma", g.all_in().t, silu=silu)
    b.all_in()
    word, eff = _seed(A, pseed, seed, drop_p)
    A.snapshot()
    _launch("ddpm_groupnorm_silu_fwd", [x.ptr, x_ld, y.ptr, y_ld, g.ptr, b.ptr, _ptr(st), ws.ptr, B, HW, C, G, eps, silu, drop_p, seed,
                                        _ptr(word), dt])
    sync()
    got = y.out(B * HW, C, y_ld)
    A.check()
    n = (C // G) * HW
    u = U_BF16 if dt == BF16 else U_F32
    gm, bt = _d(g.t), _d(b.t)
    for b0, b1 in image_slices(B, 14 * HW * C):
        nb = b1 - b0
        xs = _d(x.mat(B * HW, C, x_ld)[b0 * HW:b1 * HW]).reshape(nb, HW, C)
        mean, rstd = _gn_stats(xs, G, eps)
        mu, rs = _per_c(mean, nb, HW, C, G), _per_c(rstd, nb, HW, C, G)
        xh = (xs - mu) * rs
        t = gm * xh + bt
        sg = torch.sigmoid(t)
        yv, dyv = (t * sg, sg * (1 + t * (1 - sg))) if silu else (t, torch.ones_like(t))
        del xh, sg
        dropped = None
        if drop_p > 0:
            k = _keep(A, nb, HW, C, drop_p, eff, b0) / (1.0 - drop_p)
            dropped = k == 0
            # a dropped element is exactly zero whatever its value (the contract's dropout is a select: a NaN group stays NaN only
            # where it is kept); for finite values this is the product it always was
            yv, dyv = torch.where(k > 0, yv * k, torch.zeros_like(yv)), torch.where(k > 0, dyv * k, torch.zeros_like(dyv))
            del k
        bar = C_NORM * (u * yv.abs() + U_ACC * math.sqrt(n) * (gm.abs() * (xs.abs() + mu.abs()) * rs + bt.abs()) * dyv.abs())
        if dt == F32:
            bar = bar + C_NORM * U_ACC * ((_sigmoid_err(t) + 3) if silu else 1.0) * yv.abs()
        if dropped is not None:
            bar = torch.where(dropped, torch.zeros_like(bar), bar)       # exactly zero (it was: every term of the bar carries y or y')
        yard = None
        if A.yardstick:                                   # F.group_norm -> F.silu -> the same mask, in fp32, rounded to the stored type
            yard = F.group_norm(x.mat(B * HW, C, x_ld)[b0 * HW:b1 * HW].float().reshape(nb, HW, C).permute(0, 2, 1), G, g.t, b.t, eps)
            yard = (F.silu(yard) if silu else yard).permute(0, 2, 1)
            if drop_p > 0:
                yard = yard * (_keep(A, nb, HW, C, drop_p, eff, b0) / (1.0 - drop_p)).float()
            yard = yard.to(_TD[dt])
        res.cmp("y", got[b0 * HW:b1 * HW].reshape(nb, HW, C), yv, bar, yard)
        del xs, t, yv, dyv, bar
        if st is not None:
            s_ = _d(st.t).reshape(B, G, 2)[b0:b1]
            std = 1.0 / rstd
            res.cmp("mean", s_[..., 0], mean, C_NORM * U_ACC * math.sqrt(n) * (mean.abs() + std))
            res.cmp("rstd", s_[..., 1], rstd, C_NORM * U_ACC * math.sqrt(n) * rstd)


def rep_gn_bwd(A, sig, res):
    """Backward of rep_gn_fwd with (mean, rstd) given:  dz = dy * keep / (1 - p) * silu'(t),
        dx = rstd * (dz*gamma - xh*c1 - c2) + add (+ prior),  c1 = mean_g(dz*gamma*xh),  c2 = mean_g(dz*gamma)
        dgamma += sum dz*xh,  dbeta += sum dz,  dx_colsum[b,c] += sum_p dx.
    Model: M_i = rstd (|dz*gamma| + |xh*c1| + |c2|) + |add| + |prior| for the store; the fp32 part adds u_acc * sqrt(n) * (that bracket
    without the store + rstd*|c1| (|x| + |mean|) rstd + rstd |gamma| |dy| e_t), which covers the group sums, the recomputed xh and the
    fp32 error of t (e_t = |gamma| (|x| + |mean|) rstd + |beta|, in units of u_acc) carried through silu'.  dgamma / dbeta add that
    error of every term linearly.  The pixel sums are GEMM-shaped
    (M = sum of |terms|, S = root of the sum of squared terms, K = the pixel count), with the per-element error of the summed dx as M."""
    (px, x_ld, pdy, dy_ld, pdx, dx_ld, pg, pb, pst, pdg, pdb, pws, B, HW, C, G, silu, drop_p, seed, pseed, acc, pcs, cs_ld, padd, add_ld,
     dt) = sig
    rows = B * HW
    x = A.buf("x", pitched(rows, C, x_ld), dt, _mod(px)).fill(A.randn(pitched(rows, C, x_ld), mean=1.5))
    dy = A.buf("dy", pitched(rows, C, dy_ld), dt, _mod(pdy)).fill(A.randn(pitched(rows, C, dy_ld), mean=0.3))
    dx = A.buf("dx", pitched(rows, C, dx_ld), dt, _mod(pdx)).fill(A.randn(pitched(rows, C, dx_ld)))
    g = A.buf("gamma", C, F32, _mod(pg)).fill(1.0 + 0.3 * A.randn(C))
    b = A.buf("beta", C, F32, _mod(pb)).fill(0.5 * A.randn(C))
    A.shape("gn_x", x.inp(rows, C, x_ld).mat(rows, C, x_ld), B=B, HW=HW, C=C, G=G)
    A.shape("gn_dy", dy.inp(rows, C, dy_ld).mat(rows, C, dy_ld))
    A.shape("gn_gamma", g.all_in().t, silu=silu)
    b.all_in()
    xs = _d(x.mat(rows, C, x_ld)).reshape(B, HW, C)
    mean, rstd = _gn_stats(xs, G, 1e-6)
    st = A.buf("stats", B * G * 2, F32, _mod(pst)).fill(torch.stack([mean, rstd], -1)).all_in()
    dg = A.buf("dgamma", C, F32, _mod(pdg)).fill(A.randn(C)) if _opt(pdg) else None
    db = A.buf("dbeta", C, F32, _mod(pdb)).fill(A.randn(C)) if _opt(pdb) else None
    nws = int(_hip.lib().ddpm_gn_workspace_floats(B, HW, C, G, dt))
    ws = A.buf("workspace", nws, F32, _mod(pws)).fill(torch.zeros(nws))
    ws.all_out()
    ws.scratch = True
    cs = None
    if _opt(pcs):
        cs = A.buf("dx_colsum", pitched(B, C, cs_ld), F32, _mod(pcs)).fill(A.randn(pitched(B, C, cs_ld)))
        cs.mat(B, C, cs_ld).zero_()                        # zero on entry (contract)
        cs.inp(B, C, cs_ld).atomic = True
    ad = A.buf("add", pitched(rows, C, add_ld), dt, _mod(padd)).fill(A.randn(pitched(rows, C, add_ld))) if _opt(padd) else None
    if ad is not None:
        ad.inp(rows, C, add_ld)
    if acc:
        dx.inp(rows, C, dx_ld)
    for o in (dg, db):
        if o is not None:
            o.all_out()
            o.all_in().atomic = True
    word, eff = _seed(A, pseed, seed, drop_p)
    prior = _d(dx.mat(rows, C, dx_ld)).reshape(B, HW, C).clone()
    pdg_v = None if dg is None else _d(dg.t).clone()
    pdb_v = None if db is None else _d(db.t).clone()
    A.snapshot()
    _launch("ddpm_groupnorm_silu_bwd", [x.ptr, x_ld, dy.ptr, dy_ld, dx.ptr, dx_ld, g.ptr, b.ptr, st.ptr, _ptr(dg), _ptr(db), ws.ptr,
                                        B, HW, C, G, silu, drop_p, seed, _ptr(word), acc, _ptr(cs), cs_ld, _ptr(ad), add_ld, dt])
    sync()
    got = dx.out(rows, C, dx_ld)
    if cs is not None:
        cs.out(B, C, cs_ld)
    A.check()
    s = _d(st.t).reshape(B, G, 2)                        # the fp32 statistics the kernel was given
    mu, rs = _per_c(s[..., 0], B, HW, C, G), _per_c(s[..., 1], B, HW, C, G)
    gm, bt = _d(g.t), _d(b.t)
    xh = (xs - mu) * rs
    t = gm * xh + bt
    sg = torch.sigmoid(t)
    dz = _d(dy.mat(rows, C, dy_ld)).reshape(B, HW, C)
    if silu:
        dz = dz * sg * (1 + t * (1 - sg))
    if drop_p > 0:
        dz = dz * _keep(A, B, HW, C, drop_p, eff) / (1.0 - drop_p)
    dyk = _d(dy.mat(rows, C, dy_ld)).reshape(B, HW, C).abs()
    if drop_p > 0:
        dyk = dyk * _keep(A, B, HW, C, drop_p, eff) / (1.0 - drop_p)
    dt_err = dyk * (gm.abs() * (xs.abs() + mu.abs()) * rs + bt.abs()) if silu else 0.0 * dyk   # |dy| * (what bounds t's fp32 error) / u
    a = dz * gm
    grp = lambda v: _per_c(v.reshape(B, HW, G, C // G).mean((1, 3)), B, HW, C, G)
    c1, c2 = grp(a * xh), grp(a)
    ref = rs * (a - xh * c1 - c2)
    inner = rs * (a.abs() + (xh * c1).abs() + c2.abs())
    mag = inner.clone()
    if ad is not None:
        v = _d(ad.mat(rows, C, add_ld)).reshape(B, HW, C)
        ref, mag = ref + v, mag + v.abs()
    if acc:
        ref, mag = ref + prior, mag + prior.abs()
    n = (C // G) * HW
    u = U_BF16 if dt == BF16 else U_F32
    fp32_part = U_ACC * math.sqrt(n) * (inner + rs * c1.abs() * (xs.abs() + mu.abs()) * rs + rs * gm.abs() * dt_err)
    yard = None
    if A.yardstick:                                       # the same formula on the given statistics, every step in fp32
        x32, st32 = x.mat(rows, C, x_ld).float().reshape(B, HW, C), st.t.reshape(B, G, 2)
        mu32, rs32 = _per_c(st32[..., 0], B, HW, C, G), _per_c(st32[..., 1], B, HW, C, G)
        xh32 = (x32 - mu32) * rs32
        dz32 = dy.mat(rows, C, dy_ld).float().reshape(B, HW, C)
        if silu:
            t32 = g.t * xh32 + b.t
            sg32 = torch.sigmoid(t32)
            dz32 = dz32 * (sg32 * (1 + t32 * (1 - sg32)))
        if drop_p > 0:
            dz32 = dz32 * (_keep(A, B, HW, C, drop_p, eff) / (1.0 - drop_p)).float()
        a32 = dz32 * g.t
        grp32 = lambda v: _per_c(v.reshape(B, HW, G, C // G).mean((1, 3)), B, HW, C, G)
        yard = rs32 * (a32 - xh32 * grp32(a32 * xh32) - grp32(a32))
        if ad is not None:
            yard = yard + ad.mat(rows, C, add_ld).float().reshape(B, HW, C)
        if acc:
            yard = yard + prior.float()
        yard = yard.to(_TD[dt])
    res.cmp("dx", got.reshape(B, HW, C), ref, C_NORM * (u * mag + fp32_part), yard)
    if cs is not None:
        # the colsum adds the dx values the kernel forms (before or after the store): their per-element error is part of M
        dxm = mag * u + fp32_part
        res.cmp("dx_colsum", cs.mat(B, C, cs_ld), ref.sum(1),
                C_NORM * (dxm.sum(1) + U_F32 * ref.abs().sum(1) + U_ACC * math.sqrt(HW) * (ref * ref).sum(1).sqrt()))
    K = B * HW
    flat = lambda v: v.reshape(K, C)
    for o, terms, p0, nm in ((dg, dz * xh, pdg_v, "dgamma"), (db, dz, pdb_v, "dbeta")):
        if o is None:
            continue
        tm = flat(terms)
        ref_c, sq_c = tm.sum(0) + p0, (tm * tm).sum(0).sqrt()
        mag_c = tm.sum(0).abs() + p0.abs()
        lin = flat(dt_err * (xh.abs() if nm == "dgamma" else 1.0) + (dz.abs() * (xs.abs() + mu.abs()) * rs if nm == "dgamma" else 0.0)).sum(0)
        res.cmp(nm, o.t, ref_c, C_NORM * (U_F32 * mag_c + U_ACC * (math.sqrt(K) * sq_c + lin)))


# attention ----------------------------------------------------------------------------------------------------------------------------
def _qkv(A, sig_p, ld, B, L, C, dt):
    qkv = A.buf("qkv", pitched(B * L, 3 * C, ld), dt, _mod(sig_p)).fill(A.randn(pitched(B * L, 3 * C, ld), scale=1.5))
    A.shape("qkv", qkv.inp(B * L, 3 * C, ld).mat(B * L, 3 * C, ld), B=B, L=L, C=C)
    v = _d(qkv.mat(B * L, 3 * C, ld)).reshape(B, L, 3 * C)
    return qkv, v[..., :C], v[..., C:2 * C], v[..., 2 * C:]


def _logit_err(q, k, scale):
    """per (i, j) fp32 error bound of the logits q_i . k_j * scale: u_acc sqrt(C) sqrt(sum_c (q k)^2) * scale"""
    C = q.shape[-1]
    return U_ACC * math.sqrt(C) * ((q * q) @ (k * k).transpose(1, 2)).sqrt() * scale


def _heads(t, heads):
    """[B, L, heads * d] -> [B * heads, L, d]: head h of a packed third is its channels [h d, (h + 1) d) (include/ddpm_hip.h)."""
    B, L, C = t.shape
    return t if heads == 1 else t.reshape(B, L, heads, C // heads).permute(0, 2, 1, 3).reshape(B * heads, L, C // heads)


def _unheads(t, B, heads):
    """inverse of _heads"""
    _, L, d = t.shape
    return t if heads == 1 else t.reshape(B, heads, L, d).permute(0, 2, 1, 3).reshape(B, L, heads * d)


def rep_attn_fwd(A, sig, res, lse_entry=False, mh=False):
    """out = softmax(q k^T * scale) v, lse = log sum exp.  Model (csrc/attention.hip rounds P to bf16 in front of the PV product):
    M_ic = |out_ic| + sum_j P_ij |v_jc| (the bf16 store, and the rounding of P: 2^-8 sum_j P_ij |v_jc|), plus the logit error e_ij
    carried through exp: 2 max_j e_ij * sum_j P_ij |v_jc|, and the fp32 PV sum u_acc sqrt(L) S.  lse: u_acc (|lse| + log L) + max_j e_ij."""
    heads = 1
    if mh:                              # ddpm_attention_mh_fwd: the same product per head of width C / heads, lse [B][heads][L]
        pq, ld, po, o_ld, plse, B, L, C, heads, scale, dt = sig
    elif lse_entry:
        pq, ld, po, o_ld, plse, B, L, C, scale, dt = sig
    else:
        pq, ld, po, o_ld, B, L, C, scale, dt = sig
        plse = ("p", True, 0)
    qkv, q, k, v = _qkv(A, pq, ld, B, L, C, dt)
    q, k, v = (_heads(t, heads) for t in (q, k, v))
    o = A.buf("out", pitched(B * L, C, o_ld), dt, _mod(po)).fill(A.randn(pitched(B * L, C, o_ld)))
    lse = A.buf("lse", B * heads * L, F32, _mod(plse)) if _opt(plse) else None
    if lse is not None:
        lse.all_out()
    A.snapshot()
    if mh:
        _launch("ddpm_attention_mh_fwd", [qkv.ptr, ld, o.ptr, o_ld, _ptr(lse), B, L, C, heads, scale, dt])
    elif lse_entry:
        _launch("ddpm_attention_fwd_lse", [qkv.ptr, ld, o.ptr, o_ld, _ptr(lse), B, L, C, scale, dt])
    else:
        _launch("ddpm_attention_fwd", [qkv.ptr, ld, o.ptr, o_ld, B, L, C, scale, dt])
    sync()
    got = o.out(B * L, C, o_ld)
    A.check()
    s = q @ k.transpose(1, 2) * scale
    ls = torch.logsumexp(s, -1)
    P = torch.exp(s - ls[..., None])
    ref = P @ v
    pv = P @ v.abs()
    e = _logit_err(q, k, scale).amax(-1, keepdim=True)
    sq = ((P * P) @ (v * v)).sqrt()
    bar = C_ATTN * (U_BF16 * (ref.abs() + pv) + 2 * e * pv + U_ACC * math.sqrt(L) * sq)
    yard = ylse = None
    if A.yardstick:                                       # matmul -> softmax -> matmul in fp32
        s32 = q.float() @ k.float().transpose(1, 2) * scale
        yard, ylse = (torch.softmax(s32, -1) @ v.float()).to(_TD[dt]), torch.logsumexp(s32, -1)
    res.cmp("out", _heads(got.reshape(B, L, C), heads), ref, bar, yard)
    if lse is not None:
        res.cmp("lse", lse.t.reshape(B * heads, L), ls, C_ATTN * (U_ACC * (ls.abs() + math.log(L)) + e[..., 0]), ylse)


def rep_attn_fwd_lse(A, sig, res):
    rep_attn_fwd(A, sig, res, lse_entry=True)


def rep_attn_mh_fwd(A, sig, res):
    rep_attn_fwd(A, sig, res, mh=True)


def rep_attn_mh_bwd(A, sig, res):
    rep_attn_bwd(A, sig, res, mh=True)


def rep_attn_bwd(A, sig, res, mh=False):
    """dV = P^T dO, dS = P o (dO V^T - D), D_i = dO_i . O_i, dQ = dS K scale, dK = dS^T Q scale, with P from q, k and the given lse and
    O the given (bf16) forward output.  Model: the bf16 store (2^-8 |ref|); P rounded to bf16 before dV (2^-8 sum_i P_ij |dO_ic|); dS
    rounded to bf16 before dQ / dK — independent roundings of the L terms, so 2^-8 sqrt(sum_j (dS_ij k_jc)^2); the fp32 error of
    dP - D (u_acc sqrt(C) (root of the squared dO V^T terms) + u_acc |D|) and of the logits carried through P and dS; the fp32 sums
    u_acc sqrt(L) S.  D: GEMM-shaped over C."""
    heads = 1
    if mh:                              # ddpm_attention_mh_bwd: per head of width C / heads; lse, dvec [B][heads][L]
        pq, ld, po, o_ld, pdo, do_ld, plse, pdv, pdq, dq_ld, B, L, C, heads, scale, dt = sig
    else:
        pq, ld, po, o_ld, pdo, do_ld, plse, pdv, pdq, dq_ld, B, L, C, scale, dt = sig
    qkv, q, k, v = _qkv(A, pq, ld, B, L, C, dt)
    q, k, v = (_heads(t, heads) for t in (q, k, v))
    BH, Cf, C = B * heads, C, C // heads           # from here on C is the head's width, Cf a third of the packed row
    s = q @ k.transpose(1, 2) * scale
    ls = torch.logsumexp(s, -1)
    o = A.buf("o", pitched(B * L, Cf, o_ld), dt, _mod(po)).fill(A.randn(pitched(B * L, Cf, o_ld)))
    o.inp(B * L, Cf, o_ld).mat(B * L, Cf, o_ld).copy_(_unheads(torch.exp(s - ls[..., None]) @ v, B, heads).reshape(B * L, Cf))
    d_o = A.buf("d_o", pitched(B * L, Cf, do_ld), dt, _mod(pdo)).fill(A.randn(pitched(B * L, Cf, do_ld)))
    A.shape("attn_do", d_o.inp(B * L, Cf, do_ld).mat(B * L, Cf, do_ld))
    lse = A.buf("lse", BH * L, F32, _mod(plse)).fill(ls).all_in()
    dvec = A.buf("dvec", BH * L, F32, _mod(pdv)).fill(torch.full((BH * L,), float("nan")))
    dvec.all_out()
    dq = A.buf("dqkv", pitched(B * L, 3 * Cf, dq_ld), dt, _mod(pdq)).fill(A.randn(pitched(B * L, 3 * Cf, dq_ld)))
    A.snapshot()
    if mh:
        _launch("ddpm_attention_mh_bwd", [qkv.ptr, ld, o.ptr, o_ld, d_o.ptr, do_ld, lse.ptr, dvec.ptr, dq.ptr, dq_ld, B, L, Cf, heads, scale, dt])
    else:
        _launch("ddpm_attention_bwd", [qkv.ptr, ld, o.ptr, o_ld, d_o.ptr, do_ld, lse.ptr, dvec.ptr, dq.ptr, dq_ld, B, L, Cf, scale, dt])
    sync()
    got = _d(dq.out(B * L, 3 * Cf, dq_ld)).reshape(B, L, 3 * Cf)
    A.check()
    O = _heads(_d(o.mat(B * L, Cf, o_ld)).reshape(B, L, Cf), heads)
    dO = _heads(_d(d_o.mat(B * L, Cf, do_ld)).reshape(B, L, Cf), heads)
    B = BH                                          # one problem per (image, head)
    P = torch.exp(s - _d(lse.t).reshape(B, L, 1))
    D = (dO * O).sum(-1)
    dP = dO @ v.transpose(1, 2)
    dS = P * (dP - D[..., None])
    kT = lambda t: t.transpose(1, 2)
    e_s = _logit_err(q, k, scale)                                                  # logit error -> relative error of P
    e_dp = U_ACC * math.sqrt(C) * ((dO * dO) @ kT(v * v)).sqrt() + U_ACC * D.abs()[..., None]
    dS_err = e_s * dS.abs() + P * e_dp                                              # fp32 error of each dS_ij before its rounding
    res.cmp("dvec", dvec.t.reshape(B, L), D, C_ATTN * (U_F32 * (dO * O).abs().sum(-1) + U_ACC * math.sqrt(C) * ((dO * O) ** 2).sum(-1).sqrt()))
    outs = (
        ("dq", dS @ k * scale, (dS * dS) @ (k * k), dS_err @ k.abs() * scale, 0),
        ("dk", kT(dS) @ q * scale, kT(dS * dS) @ (q * q), kT(dS_err) @ q.abs() * scale, Cf),
        ("dv", kT(P) @ dO, kT(P * P) @ (dO * dO), kT(e_s * P) @ dO.abs(), 2 * Cf),
    )
    yard = {}
    if A.yardstick:                                       # the same products on the given o and lse, every step in fp32, stores in bf16
        q32, k32, v32, O32, dO32 = (t.float() for t in (q, k, v, O, dO))
        P32 = torch.exp(q32 @ kT(k32) * scale - lse.t.reshape(B, L, 1))
        dS32 = P32 * (dO32 @ kT(v32) - (dO32 * O32).sum(-1, keepdim=True))
        yard = {"dq": (dS32 @ k32 * scale).to(_TD[dt]), "dk": (kT(dS32) @ q32 * scale).to(_TD[dt]), "dv": (kT(P32) @ dO32).to(_TD[dt])}
    for nm, ref, sq, prop, c0 in outs:
        sq = sq.sqrt() * (scale if nm != "dv" else 1.0)
        rounding = (U_BF16 * (kT(P) @ dO.abs())) if nm == "dv" else U_BF16 * sq
        bar = C_ATTN * (U_BF16 * ref.abs() + rounding + prop + U_ACC * math.sqrt(L) * sq)
        res.cmp(nm, _heads(got[..., c0:c0 + Cf], heads), ref, bar, yard.get(nm))


# elementwise, reductions and diffusion -----------------------------------------------------------------------------------------------
def rep_colsum(A, sig, res):
    pdy, ld, pps, ps_ld, ptot, B, HW, C, dt = sig
    dy = A.buf("dy", pitched(B * HW, C, ld), dt, _mod(pdy)).fill(A.randn(pitched(B * HW, C, ld)))
    ps = A.buf("per_sample", pitched(B, C, ps_ld), F32, _mod(pps)).fill(A.randn(pitched(B, C, ps_ld))) if _opt(pps) else None
    tot = A.buf("total", C, F32, _mod(ptot)).fill(A.randn(C)) if _opt(ptot) else None
    A.shape("data", dy.inp(B * HW, C, ld).mat(B * HW, C, ld))
    amplified = amplify_images(A, dy.mat(B * HW, C, ld), HW, ld, 2 if dt == BF16 else 4)
    if ps is not None:
        A.shape("additive", ps.inp(B, C, ps_ld).mat(B, C, ps_ld))
        ps.atomic = True
    if tot is not None:
        A.shape("additive", tot.all_in().t)
        tot.atomic = True
    p_ps = None if ps is None else _d(ps.mat(B, C, ps_ld)).clone()
    p_tot = None if tot is None else _d(tot.t).clone()
    A.snapshot()
    _launch("ddpm_colsum", [dy.ptr, ld, _ptr(ps), ps_ld, _ptr(tot), B, HW, C, dt])
    sync()
    if ps is not None:
        ps.out(B, C, ps_ld)
    if tot is not None:
        tot.all_out()
    A.check()
    g = _d(dy.mat(B * HW, C, ld)).reshape(B, HW, C)
    if ps is not None:
        res.cmp("per_sample", ps.mat(B, C, ps_ld), g.sum(1) + p_ps,
                C_GEMM * (U_F32 * (g.sum(1).abs() + p_ps.abs()) + U_ACC * math.sqrt(HW) * (g * g).sum(1).sqrt()))
    if tot is not None:
        gg = g.reshape(-1, C)
        bar = C_GEMM * (U_F32 * (gg.sum(0).abs() + p_tot.abs()) + U_ACC * math.sqrt(B * HW) * (gg * gg).sum(0).sqrt())
        res.cmp("total", tot.t, gg.sum(0) + p_tot, bar)
        _sensitivity(res, "total", {b: g[b].sum(0) for b in amplified}, bar)


def rep_upsample2x_bwd(A, sig, res):
    pdy, pdx, dx_ld, B, H, W, C, acc, dt = sig
    dyu = A.buf("dy_up", B * 4 * H * W * C, dt, _mod(pdy)).fill(A.randn(B * 4 * H * W * C))
    dx = A.buf("dx", pitched(B * H * W, C, dx_ld), dt, _mod(pdx)).fill(A.randn(pitched(B * H * W, C, dx_ld)))
    A.shape("data", dyu.all_in().t)
    if acc:
        A.shape("additive", dx.inp(B * H * W, C, dx_ld).mat(B * H * W, C, dx_ld))
    prior = _d(dx.mat(B * H * W, C, dx_ld)).clone()
    A.snapshot()
    _launch("ddpm_upsample2x_bwd", [dyu.ptr, dx.ptr, dx_ld, B, H, W, C, acc, dt])
    sync()
    got = dx.out(B * H * W, C, dx_ld)
    A.check()
    blk = _d(dyu.t).reshape(B, H, 2, W, 2, C)
    ref = blk.sum((2, 4)).reshape(-1, C)
    mag = ref.abs()
    sq = (blk * blk).sum((2, 4)).reshape(-1, C).sqrt()
    if acc:
        ref, mag = ref + prior, mag + prior.abs()
    u = U_BF16 if dt == BF16 else U_F32
    res.cmp("dx", got, ref, C_GEMM * (u * mag + U_ACC * 2 * sq))


def _tables(A, T):
    return torch.linspace(0.05, 1.5, T, dtype=torch.float64)


def _t(A, B, T, p):
    tb = A.buf("t", B, "i64", _mod(p))
    tv = torch.randint(0, T, (B,), generator=A.gen)
    tv[0], tv[-1] = 0, T - 1
    tb.t.copy_(tv)
    tb.all_in()
    return tb, tv


def rep_q_sample(A, sig, res):
    px0, pn, pt, pa, pb, pxt, B, n, T = sig
    x0 = A.buf("x0", B * n, F32, _mod(px0)).fill(A.randn(B * n))
    nz = A.buf("noise", B * n, F32, _mod(pn)).fill(A.randn(B * n))
    tb, tv = _t(A, B, T, pt)
    ta = A.buf("sqrt_ab", T, F32, _mod(pa)).fill(A.randn(T).abs())
    tbb = A.buf("sqrt_1mab", T, F32, _mod(pb)).fill(A.randn(T).abs())
    xt = A.buf("xt", B * n, F32, _mod(pxt)).fill(A.randn(B * n))
    for b in (x0, nz, ta, tbb):
        b.all_in()
    A.shape("elem", x0.t.view(B, n))
    A.snapshot()
    _launch("ddpm_q_sample", [x0.ptr, nz.ptr, tb.ptr, ta.ptr, tbb.ptr, xt.ptr, B, n, T])
    sync()
    xt.all_out()
    A.check()
    tv = tv.to(A.device)
    a, b = _d(ta.t)[tv][:, None], _d(tbb.t)[tv][:, None]
    X, N_ = _d(x0.t).reshape(B, n), _d(nz.t).reshape(B, n)
    res.cmp("xt", xt.t.reshape(B, n), a * X + b * N_, C_ELEM * U_F32 * ((a * X).abs() + (b * N_).abs()))


def rep_mse_fwd(A, sig, res):
    pp, pt, pl, B, n = sig
    p = A.buf("pred", B * n, F32, _mod(pp)).fill(A.randn(B * n))
    tg = A.buf("target", B * n, F32, _mod(pt)).fill(A.randn(B * n))
    loss = A.buf("loss", B, F32, _mod(pl)).fill(A.randn(B))
    A.shape("elem", p.all_in().t.view(B, n))
    tg.all_in()
    A.snapshot()
    _launch("ddpm_mse_fwd", [p.ptr, tg.ptr, loss.ptr, B, n])
    sync()
    loss.all_out()
    A.check()
    P_, T_ = _d(p.t).reshape(B, n), _d(tg.t).reshape(B, n)
    d = T_ - P_
    mag = (d * d + 2 * d.abs() * (P_.abs() + T_.abs())).sum(1) / n
    res.cmp("loss", loss.t, (d * d).mean(1), C_GEMM * (U_F32 * mag + U_ACC * math.sqrt(n) * (d ** 4).sum(1).sqrt() / n))


def rep_mse_bwd(A, sig, res):
    pp, pt, pg, pgp, B, n = sig
    p = A.buf("pred", B * n, F32, _mod(pp)).fill(A.randn(B * n))
    tg = A.buf("target", B * n, F32, _mod(pt)).fill(A.randn(B * n))
    gl = A.buf("gloss", B, F32, _mod(pg)).fill(A.randn(B))
    gp = A.buf("gpred", B * n, F32, _mod(pgp)).fill(A.randn(B * n))
    for b in (p, tg, gl):
        b.all_in()
    A.snapshot()
    _launch("ddpm_mse_bwd", [p.ptr, tg.ptr, gl.ptr, gp.ptr, B, n])
    sync()
    gp.all_out()
    A.check()
    P_, T_, G_ = _d(p.t).reshape(B, n), _d(tg.t).reshape(B, n), _d(gl.t)[:, None]
    ref = (P_ - T_) * (2.0 / n) * G_
    res.cmp("gpred", gp.t.reshape(B, n), ref, C_ELEM * U_F32 * ((P_.abs() + T_.abs()) * (2.0 / n) * G_.abs()))


def rep_p_sample_step(A, sig, res):
    """x0 = clamp(recip[t] x_t - recip_m1[t] out); x_prev = c1[t] x0 + c2[t] x_t + [t > 0] exp(logvar[t] / 2) z.  Model: u_f32 times
    the magnitudes of every term (x0's terms scaled by |c1|; the clamp is 1-Lipschitz), c = C_ELEM for the fp32 exp."""
    pxt, po, pz, pt, pr, prm1, pc1, pc2, plv, pxp, ppred, B, n, mean_type, clip, T = sig
    xt = A.buf("x_t", B * n, F32, _mod(pxt)).fill(A.randn(B * n))
    out = A.buf("model_out", B * n, F32, _mod(po)).fill(A.randn(B * n))
    z = A.buf("z", B * n, F32, _mod(pz)).fill(A.randn(B * n))
    tb, tv = _t(A, B, T, pt)
    tabs = [A.buf(nm, T, F32, _mod(p)).fill(_tables(A, T) * f) for nm, p, f in
            (("recip", pr, 1.0), ("recip_m1", prm1, 0.5), ("coef1", pc1, 0.3), ("coef2", pc2, 0.7), ("logvar", plv, -2.0))]
    xp = A.buf("x_prev", B * n, F32, _mod(pxp)).fill(A.randn(B * n))
    pred = A.buf("pred_x0", B * n, F32, _mod(ppred)).fill(A.randn(B * n)) if _opt(ppred) else None
    for b in [xt, out, z] + tabs:
        b.all_in()
    A.snapshot()
    _launch("ddpm_p_sample_step", [xt.ptr, out.ptr, z.ptr, tb.ptr] + [tb_.ptr for tb_ in tabs] + [xp.ptr, _ptr(pred), B, n, mean_type,
                                                                                                  clip, T])
    sync()
    xp.all_out()
    if pred is not None:
        pred.all_out()
    A.check()
    tv = tv.to(A.device)
    rc, rm, c1, c2, lv = (_d(tb_.t)[tv][:, None] for tb_ in tabs)
    X, O, Z = (_d(b.t).reshape(B, n) for b in (xt, out, z))
    assert mean_type == 0, "the recorded workloads predict eps"
    x0 = rc * X - rm * O
    x0m = (rc * X).abs() + (rm * O).abs()
    if clip:
        x0 = x0.clamp(-1.0, 1.0)
    sig_ = torch.exp(0.5 * lv) * (tv > 0).to(X.dtype)[:, None]
    ref = c1 * x0 + c2 * X + sig_ * Z
    mag = (c1 * x0).abs() + c1.abs() * x0m + (c2 * X).abs() + (sig_ * Z).abs()
    res.cmp("x_prev", xp.t.reshape(B, n), ref, C_ELEM * U_F32 * mag)
    if pred is not None:
        res.cmp("pred_x0", pred.t.reshape(B, n), x0, C_ELEM * U_F32 * x0m)


def rep_softmax_fwd(A, sig, res):
    """P = softmax(s) over rows of L (s fp32 [rows][L], P [rows][L] of dtype).  The kernel forms m = max_j s_j, e_i = expf(s_i - m),
    Z = sum_j e_j (lane-strided fp32 sums, then a wave tree) and stores e_i * (1 / Z).  Model, relative to each p_i:
        e_i:  the fp32 rounding of s_i - m is u_acc |s_i - m| in the exponent, the fast exp (exp2 of (s_i - m) log2 e) another
              u_acc |s_i - m| from that product and ~2 ulp of its own:  r_i = u_acc (2 |s_i - m| + 4);
        Z:    sum_j p_j r_j from its terms, u_acc sqrt(L) sqrt(sum_j p_j^2) from the fp32 sum, u_acc for the reciprocal;
        p_i:  u_acc for the product and u_out for the store.
    |got_i - p_i| <= c * p_i * (u_out + r_i + sum_j p_j r_j + u_acc (sqrt(L) sqrt(sum_j p_j^2) + 2)), never relative to the row maximum.
    The logits are N(0, 3^2): the smallest p_i stay far above the fp32 normal range, so no term flushes."""
    ps, pp, rows, L, dt = sig
    s_ = A.buf("s", rows * L, F32, _mod(ps)).fill(A.randn(rows * L, scale=3.0))
    p = A.buf("p", rows * L, dt, _mod(pp)).fill(A.randn(rows * L))
    A.shape("logits", s_.all_in().t.view(rows, L))
    A.snapshot()
    _launch("ddpm_softmax_fwd", [s_.ptr, p.ptr, rows, L, dt])
    sync()
    got = p.all_out()
    A.check()
    S = _d(s_.t).reshape(rows, L)
    d = S - S.amax(-1, keepdim=True)
    P = torch.softmax(d, -1)
    r = U_ACC * (2 * d.abs() + 4)
    zr = (P * r).sum(-1, keepdim=True) + U_ACC * (math.sqrt(L) * (P * P).sum(-1, keepdim=True).sqrt() + 2)
    u = U_BF16 if dt == BF16 else U_F32
    yard = torch.softmax(s_.t.view(rows, L), -1).to(_TD[dt]) if A.yardstick else None
    res.cmp("p", got.reshape(rows, L), P, C_ATTN * P * (u + r + zr), yard)


def rep_softmax_bwd(A, sig, res):
    """dS_i = p_i (dp_i - D), D = sum_j p_j dp_j, with P (dtype) and dP (fp32) as given.  Model: D is an fp32 sum of L products
    (u_acc (sum_j |p_j dp_j| + sqrt(L) sqrt(sum_j (p_j dp_j)^2))), the difference adds u_acc (|dp_i| + |D|) <= u_acc (|dp_i| +
    sum_j |p_j dp_j|), and both scale with p_i through the product; the product and the store add u_acc |dS_i| and u_out |dS_i|:
        |got_i - dS_i| <= c * ((u_out + u_acc) |dS_i| + u_acc p_i (|dp_i| + 2 sum_j |p_j dp_j| + sqrt(L) sqrt(sum_j (p_j dp_j)^2)))."""
    pp, pdp, pds, rows, L, dt = sig
    p = A.buf("p", rows * L, dt, _mod(pp)).fill(torch.softmax(A.shaped("logits", A.randn(rows * L, scale=3.0).reshape(rows, L)), -1))
    dp = A.buf("dp", rows * L, F32, _mod(pdp)).fill(A.randn(rows * L))
    ds = A.buf("ds", rows * L, dt, _mod(pds)).fill(A.randn(rows * L))
    p.all_in()
    dp.all_in()
    A.snapshot()
    _launch("ddpm_softmax_bwd", [p.ptr, dp.ptr, ds.ptr, rows, L, dt])
    sync()
    got = ds.all_out()
    A.check()
    P, G = _d(p.t).reshape(rows, L), _d(dp.t).reshape(rows, L)
    pg = P * G
    ref = P * (G - pg.sum(-1, keepdim=True))
    dot_err = 2 * pg.abs().sum(-1, keepdim=True) + math.sqrt(L) * (pg * pg).sum(-1, keepdim=True).sqrt()
    u = U_BF16 if dt == BF16 else U_F32
    yard = None
    if A.yardstick:
        p32, g32 = p.t.float().view(rows, L), dp.t.view(rows, L)
        yard = (p32 * (g32 - (p32 * g32).sum(-1, keepdim=True))).to(_TD[dt])
    res.cmp("ds", got.reshape(rows, L), ref, C_ATTN * ((u + U_ACC) * ref.abs() + U_ACC * P * (G.abs() + dot_err)), yard)


def _sigmoid_err(x):
    """relative fp32 error of sigmoidf_ (csrc/common.h: 1 / (1 + expf(-x)), fast exp) in units of u: the exp's r = |x| + 2 (argument
    product and the exp itself) damped by 1 - s in 1 + e, one rounding for the sum and one for the division"""
    return 2 + (x.abs() + 2) * (1 - torch.sigmoid(x))


def rep_silu_fwd(A, sig, res):
    """y = x sigmoid(x) (fp32).  Model: |got - y| <= c u (1 + e_s) |y| with e_s = _sigmoid_err(x): relative to each element."""
    px, py, n = sig
    x = A.buf("x", n, F32, _mod(px)).fill(A.randn(n, scale=4.0))
    y = A.buf("y", n, F32, _mod(py)).fill(A.randn(n))
    A.shape("silu_x", x.all_in().t)
    A.snapshot()
    _launch("ddpm_silu_fwd", [x.ptr, y.ptr, n])
    sync()
    got = y.all_out()
    A.check()
    X = _d(x.t)
    ref = X * torch.sigmoid(X)
    res.cmp("y", got, ref, C_ELEM * U_F32 * (1 + _sigmoid_err(X)) * ref.abs(), F.silu(x.t) if A.yardstick else None)


def rep_silu_bwd(A, sig, res):
    """dx (+)= dy silu'(x), silu'(x) = s (1 + x (1 - s)), s = sigmoid(x) (fp32, csrc/common.h silu_gradf_).  Model: s carries
    e_s = _sigmoid_err(x) (relative, units of u); 1 - s then carries s e_s + (1 - s) absolutely, x (1 - s) |x| times that plus its own
    rounding, and the bracket and the product one rounding each:
        E' = |silu'| (e_s + 2) + s |x| (s e_s + 2 (1 - s))     (units of u, absolute)
        |got - ref| <= c u (|dy| E' + 2 |dy silu'| + |prior|)   (prior only with accumulate)."""
    px, pdy, pdx, n, acc = sig
    x = A.buf("x", n, F32, _mod(px)).fill(A.randn(n, scale=4.0))
    dy = A.buf("dy", n, F32, _mod(pdy)).fill(A.randn(n))
    dx = A.buf("dx", n, F32, _mod(pdx)).fill(A.randn(n))
    A.shape("silu_x", x.all_in().t)
    dy.all_in()
    if acc:
        dx.all_in()
    prior = _d(dx.t).clone()
    A.snapshot()
    _launch("ddpm_silu_bwd", [x.ptr, dy.ptr, dx.ptr, n, acc])
    sync()
    got = dx.all_out()
    A.check()
    X, G = _d(x.t), _d(dy.t)
    sg = torch.sigmoid(X)
    d1 = sg * (1 + X * (1 - sg))
    es = _sigmoid_err(X)
    e1 = d1.abs() * (es + 2) + sg * X.abs() * (sg * es + 2 * (1 - sg))
    ref = G * d1
    mag = G.abs() * e1 + 2 * ref.abs()
    if acc:
        ref, mag = ref + prior, mag + prior.abs() + ref.abs()
    yard = None
    if A.yardstick:
        with torch.enable_grad():
            x32 = x.t.clone().requires_grad_(True)
            F.silu(x32).backward(dy.t.clone())
        yard = x32.grad + prior.float() if acc else x32.grad
    res.cmp("dx", got, ref, C_ELEM * U_F32 * mag, yard)


def rep_add_rows(A, sig, res):
    """y (+)= x over [rows][C] with pitches.  A copy (accumulate = 0) is exact: bar 0.  With accumulate the fp32 sum and the store
    round once each: c u_out (|x| + |prior|)."""
    px, x_ld, py, y_ld, rows, C, acc, dt = sig
    x = A.buf("x", pitched(rows, C, x_ld), dt, _mod(px)).fill(A.randn(pitched(rows, C, x_ld)))
    y = A.buf("y", pitched(rows, C, y_ld), dt, _mod(py)).fill(A.randn(pitched(rows, C, y_ld)))
    A.shape("data", x.inp(rows, C, x_ld).mat(rows, C, x_ld))
    if acc:
        A.shape("additive", y.inp(rows, C, y_ld).mat(rows, C, y_ld))
    prior = _d(y.mat(rows, C, y_ld)).clone()
    A.snapshot()
    _launch("ddpm_add_rows", [x.ptr, x_ld, y.ptr, y_ld, rows, C, acc, dt])
    sync()
    got = y.out(rows, C, y_ld)
    A.check()
    X = _d(x.mat(rows, C, x_ld))
    if acc:
        u = U_BF16 if dt == BF16 else U_F32
        res.cmp("y", got, X + prior, C_GEMM * u * (X.abs() + prior.abs()))
    else:
        res.cmp("y", got, X, torch.zeros_like(X))


def rep_nchw_to_nhwc(A, sig, res):
    """y[b][p][c] = x[b][c][p] for c < C, zero for C <= c < Cp (x fp32 NCHW, y the compute type, NHWC with Cp channels).  A copy: exact
    in fp32 (bar 0); a bf16 store rounds once, u_out |x|; a pad channel must be exactly zero."""
    px, py, B, C, HW, Cp, dt = sig
    x = A.buf("x", B * C * HW, F32, _mod(px)).fill(A.randn(B * C * HW)).all_in()
    y = A.buf("y", B * HW * Cp, dt, _mod(py)).fill(A.randn(B * HW * Cp))
    A.shape("data", x.t)
    y.all_out()
    A.snapshot()
    _launch("ddpm_nchw_to_nhwc", [x.ptr, y.ptr, B, C, HW, Cp, dt])
    sync()
    A.check()
    u = U_BF16 if dt == BF16 else 0.0
    for b0, b1 in image_slices(B, 6 * HW * Cp):
        ref = torch.zeros(b1 - b0, HW, Cp, dtype=torch.float64, device=A.device)
        ref[..., :C] = _d(x.t[b0 * C * HW:b1 * C * HW]).reshape(b1 - b0, C, HW).transpose(1, 2)
        res.cmp("y", y.t[b0 * HW * Cp:b1 * HW * Cp].reshape(b1 - b0, HW, Cp), ref, u * ref.abs())


def rep_timestep_embedding(A, sig, res):
    """out[b] = [sin(a_b), cos(a_b)] (+ a zero column when dim is odd) with a_bi = fl32(t_b * f_i): the kernel's fp32 product is part of
    the contract (functions.py's torch.outer), so the reference rounds it exactly as fp32 does (t_b * f_i is exact in float64) and
    evaluates sin / cos of that argument in float64.  Model: the fp32 sinf / cosf with full range reduction, a few ulp of the result:
    c u |ref|; the pad column must be exactly zero.  freqs is the host's table exp(-i ln(1e4) / (half - 1)) in fp32."""
    pt, pf, po, B, dim = sig
    half = dim // 2
    tb = A.buf("t", B, "i64", _mod(pt))
    tv = torch.randint(0, 1000, (B,), generator=A.gen)
    tv[0] = 0
    tv[-1] = 999
    tb.t.copy_(tv)
    f = torch.exp(-torch.arange(half, dtype=torch.float64) * math.log(1e4) / (half - 1)).to(torch.float32)
    fr = A.buf("freqs", half, F32, _mod(pf)).fill(f).all_in()
    tb.all_in()
    out = A.buf("out", B * dim, F32, _mod(po)).fill(A.randn(B * dim))
    A.snapshot()
    _launch("ddpm_timestep_embedding", [tb.ptr, fr.ptr, out.ptr, B, dim])
    sync()
    got = out.all_out()
    A.check()
    arg = (_d(tb.t)[:, None] * _d(fr.t)[None, :]).to(torch.float32).to(torch.float64)
    ref = torch.zeros(B, dim, dtype=torch.float64, device=arg.device)
    ref[:, :half], ref[:, half:2 * half] = torch.sin(arg), torch.cos(arg)
    res.cmp("out", got.reshape(B, dim), ref, C_ELEM * U_F32 * ref.abs())


def rep_gather_rows(A, sig, res):
    """out[r] = table[idx[r]], bit-exact (bar 0); an index outside [0, table_rows) must give a NaN row.  Two launches: every index
    valid (first and last table row included), then every even row's index out of range (-1, table_rows, 2^40 in turn)."""
    ptab, pidx, pout, rows, row_len, table_rows = sig
    tab = A.buf("table", table_rows * row_len, F32, _mod(ptab)).fill(A.randn(table_rows * row_len)).all_in()
    ib = A.buf("idx", rows, "i64", _mod(pidx)).all_in()
    out = A.buf("out", rows * row_len, F32, _mod(pout))
    T = _d(tab.t).reshape(table_rows, row_len)
    for bad in (False, True):
        iv = torch.randint(0, table_rows, (rows,), generator=A.gen)
        iv[0], iv[-1] = (0, table_rows - 1) if rows > 1 else (iv[0], iv[0])
        poison = torch.zeros(rows, dtype=torch.bool)
        if bad:
            poison[::2] = True
            oob = torch.tensor([-1, table_rows, 1 << 40], dtype=torch.int64)
            iv[::2] = oob[torch.arange(0, rows, 2) // 2 % 3]
        ib.t.copy_(iv)
        out.fill(A.randn(out.n))
        out.poisoned = False                              # overwritten by each launch: poisoned before each
        A.snapshot()
        _launch("ddpm_gather_rows_f32", [tab.ptr, ib.ptr, out.ptr, rows, row_len, table_rows])
        sync()
        got = out.all_out().reshape(rows, row_len)
        A.check()
        poison = poison.to(got.device)
        assert bool(torch.isnan(got[poison]).all()), "an index outside the table did not give a NaN row"
        keep = ~poison
        ref = T[iv.clamp(0, table_rows - 1).to(T.device)][keep]
        res.cmp("out" if not bad else "out(oob)", got[keep], ref, torch.zeros_like(ref))


def rep_weighted_sum(A, sig, res):
    """out = sum_i x_i w_i, one block in a fixed order: a short fp32 sum held, like ddpm_atb_f32, to
    c (u sum_i |x_i w_i| + u_acc sqrt(n) sqrt(sum_i (x_i w_i)^2))."""
    px, pw, po, n = sig
    x = A.buf("x", n, F32, _mod(px)).fill(A.randn(n))
    w = A.buf("w", n, F32, _mod(pw)).fill(A.randn(n))
    out = A.buf("out", 1, F32, _mod(po)).fill(A.randn(1))
    x.all_in()
    w.all_in()
    A.snapshot()
    _launch("ddpm_weighted_sum_f32", [x.ptr, w.ptr, out.ptr, n])
    sync()
    got = out.all_out()
    A.check()
    pr = _d(x.t) * _d(w.t)
    res.cmp("out", got, pr.sum().reshape(1), (C_GEMM * (U_F32 * pr.abs().sum() + U_ACC * math.sqrt(n) * (pr * pr).sum().sqrt())).reshape(1))


# ----------------------------------------------------------------------------------------------------------------- the optimizer tail
# What a step runs after its last weight gradient: ddpm_wgrad_unpack(_sumsq) -> ddpm_mt_adam_ema -> ddpm_pack_weight_multi ->
# ddpm_mt_gather_f32 (and ddpm_mt_grad_sumsq / the single-tensor pair on the autograd path).  All but the single-tensor pair read their
# geometry from a TABLE in device memory, so the signature of such a launch carries, in place of the table pointer, a table word
#     ("t", rows, opts)
# rows: the normalised table (normalise_table: per row the element counts / descriptor fields and, for every pointer column, whether it
# is null, its address modulo 16 and the byte gap to the next row's tensor when the two share a buffer); opts: ((key, value), ...) that
# only hand-written rows set (the draw of the gradient, the optimizer step, the scalars behind hyper_dev).  The replay rebuilds that
# packing out of guarded buffers (_carve): every float between two tensors of a buffer is outside the contract's output.
TABLE_ARG = {            # entry -> (index of the table argument, index of n_tensors, int64 words per row)
    "ddpm_mt_adam_ema": (0, 1, 6), "ddpm_mt_grad_sumsq": (0, 1, 6), "ddpm_mt_gather_f32": (0, 1, 4),
    "ddpm_pack_weight_multi": (0, 1, 8), "ddpm_wgrad_unpack": (2, 3, 5), "ddpm_wgrad_unpack_sumsq": (2, 3, 5),
}
SEPARATE = -1                       # gap of a tensor whose successor in the column lives in another buffer (or is null / the last row)
GAP_SHARED = 4096                   # recorded addresses: a successor that starts within this many bytes of a tensor's end shares its buffer
GAP_CAP = 256                       # ... and gaps beyond this are shortened to it (keeping the successor's address modulo 16)
DENORM = 2.0 ** -149                # absolute rounding step below the fp32 normal range
BETA1, BETA2, ADAM_EPS = 0.9, 0.999, 1e-8
SUMSQ_SLOT_BLOCKS = 64              # ddpm_mt_sumsq_slots(n) = 64 + 64 n


def _f(x):
    """the value a C float argument takes"""
    return float(np.float32(x))


def is_table(w):
    return isinstance(w, tuple) and len(w) == 3 and w[0] == "t"


def _columns(ptrs, nbytes):
    """ptrs[r][c] (addresses), nbytes[r][c] -> per row a tuple of (null, address % 16, gap) per pointer column."""
    out = []
    for r, row in enumerate(ptrs):
        cols = []
        for c, a in enumerate(row):
            if not a:
                cols.append((True, 0, SEPARATE))
                continue
            gap = SEPARATE
            if r + 1 < len(ptrs) and ptrs[r + 1][c]:
                g = ptrs[r + 1][c] - (a + nbytes[r][c])
                if 0 <= g < GAP_SHARED:
                    gap = g if g <= GAP_CAP else GAP_CAP + g % 16
            cols.append((False, a % 16, gap))
        out.append(tuple(cols))
    return out


def _pack_extents(N, C, Rf, Cp, Np, es):
    R, up = Rf & 0xff, bool(Rf & 0x100)
    return 4 * N * C * R * R, es * N * R * R * Cp, es * C * (16 if up else R * R) * Np


def normalise_table(name, rows, dtype=None):
    """rows: the int64 table a launch of `name` read, as lists of ints -> the table word of its signature (no pointer values)."""
    if name in ("ddpm_wgrad_unpack", "ddpm_wgrad_unpack_sumsq"):       # offsets into gpack / gflat, not addresses: kept as they are
        return ("t", tuple(tuple(int(v) for v in r) for r in rows), ())
    if name == "ddpm_pack_weight_multi":
        es = 2 if dtype == BF16 else 4
        cols = _columns([r[:3] for r in rows], [_pack_extents(*r[3:8], es) for r in rows])
        return ("t", tuple((tuple(int(v) for v in r[3:8]), c) for r, c in zip(rows, cols)), ())
    k = TABLE_ARG[name][2] - 1                                           # pointer columns; the last word is numel
    cols = _columns([r[:k] for r in rows], [[4 * r[k]] * k for r in rows])
    return ("t", tuple((int(r[k]), c) for r, c in zip(rows, cols)), ())


def _carve(A, name, col, sizes, dtype):
    """One pointer column of a table out of guarded buffers.  col[r] = (null, address % 16, gap), sizes[r] in elements.  Consecutive
    rows with a gap share a Buf, `gap` bytes apart; returns per row None (null) or (Buf, offset in elements)."""
    es = 2 if dtype == BF16 else 4
    out, run = [None] * len(col), []

    def flush():
        if not run:
            return
        offs, o = [], 0
        for r in run:
            offs.append(o)
            o += sizes[r] + (col[r][2] // es if r != run[-1] else 0)
        b = A.buf(f"{name}[{run[0]}]", o, dtype, col[run[0]][1])
        for r, off in zip(run, offs):
            assert (b.ptr + off * es) % 16 == col[r][1], f"{name}[{r}]: the packing does not give the recorded address modulo 16"
            out[r] = (b, off)
        run.clear()

    for r, (null, _, gap) in enumerate(col):
        if null:
            flush()
            continue
        assert gap == SEPARATE or gap % es == 0
        run.append(r)
        if gap == SEPARATE:
            flush()
    flush()
    return out


def _sl(slot, n):
    b, off = slot
    return b.t[off:off + n]


def _addr(slot, es=4):
    return 0 if slot is None else slot[0].ptr + slot[1] * es


def _mark(slot, n, read=False, write=False):
    b, off = slot
    if read:
        b.readable[off:off + n] = True
    if write:
        b.written[off:off + n] = True


def _table_buf(A, rows):
    t = A.buf("table", max(len(rows) * len(rows[0]) if rows else 1, 1), "i64")
    if rows:
        t.t.copy_(torch.tensor(rows, dtype=torch.int64).reshape(-1))
    return t.all_in()


def bias_corrections(k):
    """(bias_corr1, bias_corr2) of optimizer step k as torch.optim.Adam forms them from the betas the kernel is handed (0.9f, 0.999f)"""
    return 1.0 - _f(BETA1) ** k, 1.0 - _f(BETA2) ** k


def _step_of(bc2):
    """optimizer step behind a recorded bias_corr2"""
    if not 0.0 < bc2 < 1.0:
        return 10 ** 6
    return max(1, min(10 ** 6, round(math.log1p(-bc2) / math.log(BETA2))))


def _planted(numels, sweep, store):
    """The exact coverage draw: zero everywhere except up to 12 positions of the first and the last non-empty row, which hold distinct
    powers of two 2^0 .. 2^11 — index 0, n - 2, n - 1, the first scalar-tail index 4 (n >> 2) and either side of one grid sweep
    (sweep(row) elements).  Every partial sum of squares is then exact in fp32: a missed position clears its bit of the total, a
    doubled one sets an odd bit.  store(row, i, value) plants element i of the row.  Returns the sum of the squares planted."""
    live = [r for r, n in enumerate(numels) if n > 0]
    k, total = 0, 0.0
    for r in dict.fromkeys(live[:1] + live[-1:]):
        n = numels[r]
        for i in sorted({0, n - 2, n - 1, 4 * (n >> 2), sweep(r) - 1, sweep(r)} & set(range(n))):
            store(r, i, 2.0 ** k)
            total += 4.0 ** k
            k += 1
    assert 0 < k <= 12
    return total


def _mt_setup(A, rows, opts):
    """Buffers and draws of a {p, g, m, v, shadow, numel} table.  The values of a row do not depend on how the table is packed (the same
    seed gives the same numbers at every alignment): p = N(0, 1) 10^U(-4, 0), shadow = p (1 + 0.01 N), g by opts["g"] — "normal" N(0, 0.5),
    "loguniform" +-10^U(-9, 0) so that eps matters on part of the tensor, "planted" (_planted) — times opts["gscale"]; m = |g| N(0, 1)
    and v = g^2 U(0.5, 2): non-zero state of the gradient's own magnitude."""
    numels = [n for n, _ in rows]
    names = ("p", "g", "m", "v", "shadow")
    slots = [_carve(A, nm, [c[i] for _, c in rows], numels, F32) for i, nm in enumerate(names)]
    kind, gscale = opts.get("g", "normal"), opts.get("gscale", 1.0)
    for r, n in enumerate(numels):
        if n == 0:
            continue
        p = A.randn(n) * 10.0 ** (-4.0 * torch.rand(n, generator=A.dgen, device=A.device))
        s = p * (1.0 + 0.01 * A.randn(n))
        if kind == "loguniform":
            g = torch.sign(A.randn(n)) * 10.0 ** (-9.0 * torch.rand(n, generator=A.dgen, device=A.device))
        else:
            g = A.randn(n, scale=0.5)
        g = g * gscale
        m = g.abs() * A.randn(n)
        v = g * g * (0.5 + 1.5 * torch.rand(n, generator=A.dgen, device=A.device))
        if kind == "planted":
            g = torch.zeros_like(g)
        else:
            g = A.shaped("grad", g.reshape(-1, 1)).reshape(-1)
        for slot, val in zip((slots[0][r], slots[1][r], slots[2][r], slots[3][r], slots[4][r]), (p, g, m, v, s)):
            if slot is not None:
                _sl(slot, n).copy_(val)
    return numels, slots


def _mt_rows_table(rows, slots):
    return [[_addr(slots[c][r]) for c in range(5)] + [n] for r, (n, _) in enumerate(rows)]


def _sumsq_depth(numel_its, n_slots):
    """Longest chain of fp32 additions (and the product) one squared term passes through: the thread's own chain (numel_its, from the
    launch geometry), 6 levels of the wave reduction, 2 of the 4-way block sum, the finish kernel's per-thread chain over n_slots slots
    in 1024 threads and its 10-level tree."""
    return numel_its + 6 + 2 + -(-n_slots // 1024) + 10


def _check_bank(res, what, bank, ref, bar, planted_sum=None):
    """bank: the 64 floats at total_sq after a producing launch.  Lane 0 against the float64 sum, lanes 1..63 exactly zero; after a
    planted draw lane 0 must hold the planted sum bit for bit."""
    assert not bool(bank[1:].view(torch.int32).any()), f"{what}: lanes 1..63 of the bank are not zero"
    if planted_sum is not None:
        assert float(bank[0]) == planted_sum, f"{what}: planted sum of squares {float(bank[0]):.1f}, exactly {planted_sum:.1f} expected " \
                                              f"(difference {float(bank[0]) - planted_sum:+.1f})"
    res.cmp(what, bank[:1], ref.reshape(1), bar.reshape(1))


def rep_mt_grad_sumsq(A, sig, res):
    """total_sq[0] = sum_i ||g_i||^2 in a fixed order, lanes 1..63 zero.  Bound (first order): d u sum g^2 with d the longest chain
    of operations a term passes through (_sumsq_depth) — csrc/optim.hip mt_sumsq_kernel: 16 blocks of 256 threads a row, a float4
    body (two in-vector levels and the thread's running sum) when g is 16-byte aligned, then the scalar tail — plus one denormal step
    a term for squares below the normal range."""
    table, n, ptot, total_floats = sig
    rows, opts = table[1], dict(table[2])
    assert n == len(rows) and total_floats >= 64 + SUMSQ_SLOT_BLOCKS * n
    numels, slots = _mt_setup(A, rows, opts)
    tot = A.buf("total_sq", total_floats, F32, _mod(ptot)).fill(A.randn(total_floats))
    tot.written[:64 + SUMSQ_SLOT_BLOCKS * n] = True
    tot.result = torch.zeros_like(tot.written)
    tot.result[:64] = True
    planted = None
    if opts.get("g") == "planted":
        def store(r, i, value):
            _sl(slots[1][r], numels[r])[i] = value
        planted = _planted(numels, lambda r: 16 * 256 * 4, store)
    for r, nn in enumerate(numels):
        _mark(slots[1][r], nn, read=True)
    tb = _table_buf(A, _mt_rows_table(rows, slots))
    A.snapshot()
    _launch("ddpm_mt_grad_sumsq", [tb.ptr, n, tot.ptr, total_floats])
    sync()
    A.check()
    S = sum((_d(_sl(slots[1][r], nn)) ** 2).sum() for r, nn in enumerate(numels) if nn) + torch.zeros((), dtype=torch.float64, device=A.device)
    its = 0
    for (nn, cols) in rows:
        nv = nn >> 2 if cols[1][1] == 0 else 0
        its = max(its, 1 + (2 + -(-nv // 4096) if nv else 0) + -(-(nn - 4 * nv) // 4096))
    d = _sumsq_depth(its, 16 * n)
    res.depth = d
    _check_bank(res, "total_sq", tot.t[:64], S, d * U_F32 * S + sum(numels) * DENORM, planted)


def _adam_bars(P, G, M, V, S, ref, clip_on, lr, bc1, bc2, eps, w):
    """Per-element bars of one row (float64 tensors; ref = (p', m', v', shadow') of the float64 chain) — the first-order propagation of
    the operation list of `upd` in csrc/optim.hip, one u per fp32 operation weighted by the magnitude of its result (u = U_F32; an
    operation on values below the normal range adds DENORM instead), the whole multiplied by C_ELEM:
        clip   c = max_norm / (sqrtf(tot) + 1e-6):  sqrtf, +, /  ->  3 u relative (0 when nothing clips: the bank's sum is exact by the draw)
        g'     g c                                   e_g = |g'| (e_c + u)
        m'     b1 m + (1 - b1) g'                    e_m = u |b1 m| + (1 - b1) (e_g + 2 u |g'|) + u |m'|          (1 - b1 and the product round)
        v'     b2 v + (1 - b2) g' g'                 e_v = u |b2 v| + (1 - b2) (2 |g'| e_g + 3 u g'^2) + u |v'|
        s      sqrtf(v')                             e_s = e_v / (2 s) + u s
        q      s / sqrtf(bc2)                        e_q = e_s / sqrt(bc2) + 2.5 u q       (bc2 is handed in fp32: u / 2; sqrtf; the division)
        d      q + eps                               e_d = e_q + u d
        r      m' / d                                e_r = e_m / d + |r| e_d / d + u |r|
        t      (lr / bc1) r                          e_t = step e_r + 3 u |t|              (bc1 handed in fp32, the division, the product)
        p'     p - t                                 e_p = e_t + u |p'|
        sh'    sh + w (p' - sh)                      e_sh = w (e_p + u |p' - sh|) + u |w (p' - sh)| + u |sh'|
    Returns (bar_p, bar_m, bar_v, bar_shadow)."""
    b1, b2 = _f(BETA1), _f(BETA2)
    p1, m1, v1, s1 = ref
    u = U_F32
    g = G.abs()
    e_g = g * ((3 * u if clip_on else 0.0) + u) + DENORM
    e_m = u * (b1 * M).abs() + (1 - b1) * (e_g + 2 * u * g) + u * m1.abs() + DENORM
    e_v = u * (b2 * V).abs() + (1 - b2) * (2 * g * e_g + 3 * u * g * g) + u * v1.abs() + 4 * DENORM
    s = v1.sqrt()
    e_s = torch.minimum(e_v / (2 * s).clamp_min(1e-300), e_v.sqrt()) + u * s            # (sqrt(0 + e) = sqrt(e))
    q = s / math.sqrt(bc2)
    e_q = e_s / math.sqrt(bc2) + 2.5 * u * q
    d = q + eps
    e_d = e_q + u * d
    r = m1 / d
    e_r = e_m / d + r.abs() * e_d / d + u * r.abs()
    step = lr / bc1
    e_t = step * e_r + 3 * u * (step * r).abs()
    e_p = e_t + u * p1.abs()
    bars = [C_ELEM * e_p, C_ELEM * e_m, C_ELEM * e_v]
    if S is not None:
        diff = (p1 - S).abs()
        bars.append(C_ELEM * (w * (e_p + u * diff) + u * w * diff + u * s1.abs()))
    else:
        bars.append(None)
    return bars


ADAM_CHUNK = 32 << 20               # elements of a table that go through one torch.optim.Adam in float64 (the CIFAR table: two passes)


def _adam_chunks(numels):
    out, cur, tot = [], [], 0
    for r, n in enumerate(numels):
        if n == 0:
            continue
        if cur and tot + n > ADAM_CHUNK:
            out.append(cur)
            cur, tot = [], 0
        cur.append(r)
        tot += n
    return out + ([cur] if cur else [])


def adam_reference(P, G, M, V, S, clip, k, lr, bc1, bc2, eps, w):
    """One optimizer step of torch.optim.Adam in float64 on lists of float64 tensors (state handed in), on gradients scaled by `clip`
    the way clip_grad_norm_ scales them, then the EMA recurrence shadow += w (p - shadow).  Returns [(p', m', v', shadow')].
    The kernel is HANDED its bias corrections (bc1, bc2: C floats); torch.optim.Adam forms its own, t1 = 1 - b1^k and t2 = 1 - b2^k.
    Its update (lr' / t1) m / (sqrt(v) / sqrt(t2) + eps') is the handed one, (lr / bc1) m / (sqrt(v) / sqrt(bc2) + eps), exactly when
    eps' = rho eps and lr' = lr rho t1 / bc1 with rho = sqrt(bc2 / t2): torch runs with those (any step k serves)."""
    t1, t2 = bias_corrections(k)
    rho = math.sqrt(bc2 / t2)
    params = [torch.nn.Parameter(p.clone()) for p in P]
    for q, g in zip(params, G):
        q.grad = g * clip
    opt = torch.optim.Adam(params, lr=lr * rho * t1 / bc1, betas=(_f(BETA1), _f(BETA2)), eps=eps * rho)
    for q, m, v in zip(params, M, V):
        opt.state[q] = {"step": torch.tensor(float(k - 1)), "exp_avg": m.clone(), "exp_avg_sq": v.clone()}
    opt.step()
    out = []
    for q, s in zip(params, S):
        p1 = q.detach()
        out.append((p1, opt.state[q]["exp_avg"], opt.state[q]["exp_avg_sq"], None if s is None else s + w * (p1 - s)))
    return out


def clip_coefficient(bank, max_norm):
    """min(1, max_norm / (norm + 1e-6)) in float64 from the bank the update is handed (clip_grad_norm_'s coefficient; a NaN norm gives
    NaN).  Returns (coefficient, whether it clips)."""
    c = max_norm / (math.sqrt(float(_d(bank).sum())) + 1e-6) if float(_d(bank).sum()) >= 0 else float("nan")
    return (1.0, False) if c >= 1.0 else (c, True)


def _adam_yardstick(p, g, m, v, s, bank, max_norm, lr, bc1, bc2, eps, w):
    """the same update as a plain fp32 torch composition (torch.optim.Adam's own operation order)"""
    f = lambda x: torch.tensor(x, dtype=torch.float32, device=p.device)
    b1, b2 = f(BETA1), f(BETA2)
    bc1, bc2 = f(bc1), f(bc2)
    if bank is not None:
        c = f(max_norm) / (bank.sum().sqrt() + f(1e-6))
        g = g * torch.where(c >= 1, torch.ones_like(c), c)
    m1 = b1 * m + (1 - b1) * g
    v1 = b2 * v + (1 - b2) * g * g
    p1 = p - (f(lr) / bc1) * (m1 / (v1.sqrt() / bc2.sqrt() + f(eps)))
    return p1, m1, v1, None if s is None else s + f(w) * (p1 - s)


def _adam_check(A, res, before, after, bank, max_norm, lr, bc1, bc2, eps, w):
    """before[r] = (p, g, m, v, shadow or None) as stored before the launch (fp32 clones; None for an empty row), after[r] = (p, m, v,
    shadow or None) as they are now.  bank: the 64 floats the update read (None: no clipping).  Scalars: what the kernel was handed."""
    lr, bc1, bc2, eps, w, max_norm = (_f(x) for x in (lr, bc1, bc2, eps, w, max_norm))
    k = _step_of(bc2)
    if max_norm <= 0:
        bank = None
    clip, clip_on = (1.0, False) if bank is None else clip_coefficient(bank, max_norm)
    res.clip = clip
    if clip_on and math.isfinite(clip) and clip > 0 and not res.nonfinite:
        # the coefficient torch's own clip_grad_norm_ derives from these gradients: the bank the update is handed must agree with it
        gs = [torch.nn.Parameter(torch.zeros(1, dtype=torch.float64, device=A.device)) for b in before if b is not None]
        for q, b in zip(gs, [b for b in before if b is not None]):
            q.grad = (_d(b[1]) ** 2).sum().sqrt().reshape(1)
        norm = float(torch.nn.utils.clip_grad_norm_(gs, max_norm))
        assert abs(max_norm / (norm + 1e-6) / clip - 1) < 2.0 ** -16, "the bank handed to the update is not the gradients' squared norm"
    for chunk in _adam_chunks([0 if b is None else b[0].numel() for b in before]):
        B = [before[r] for r in chunk]
        D = [[_d(t) if t is not None else None for t in b] for b in B]
        refs = adam_reference([d[0] for d in D], [d[1] for d in D], [d[2] for d in D], [d[3] for d in D], [d[4] for d in D], clip, k, lr, bc1, bc2, eps, w)
        for r, b, d, ref in zip(chunk, B, D, refs):
            bars = _adam_bars(d[0], d[1] * clip, d[2], d[3], d[4], ref, clip_on, lr, bc1, bc2, eps, w)
            yard = _adam_yardstick(*b, bank, max_norm, lr, bc1, bc2, eps, w) if A.yardstick else (None,) * 4
            for j, nm in enumerate(("p", "m", "v", "shadow")):
                if after[r][j] is not None:
                    res.tensors[(r, nm)] = after[r][j].clone()
                    res.cmp(f"{nm}[{r}]", after[r][j], ref[j], bars[j], yard[j])


def _after(numels, slots):
    return [tuple(None if slots[c][r] is None or n == 0 else _sl(slots[c][r], n) for c in (0, 2, 3, 4)) for r, n in enumerate(numels)]


def _before(numels, slots):
    return [None if n == 0 else tuple(None if slots[c][r] is None else _sl(slots[c][r], n).clone() for c in range(5)) for r, n in enumerate(numels)]


def _bank_for(A, numels, slots, tot, spread=True):
    """Fill the 64-float bank with the squared norm of the drawn gradients: 64 equal lanes whose low six mantissa bits are zero, so
    that the kernel's fp32 sum of the lanes is exact whatever its order (a kernel that reads lane 0 alone is off by sqrt(64) in the
    coefficient).  The reference reads the bank back."""
    S = sum(float((_d(_sl(slots[1][r], n)) ** 2).sum()) for r, n in enumerate(numels) if n)
    lane = np.float32(S / 64 if spread else S)
    if spread and np.isfinite(lane):
        lane = (lane.view(np.uint32) & np.uint32(0xFFFFFFC0)).view(np.float32)
    tot.t[:64] = float(lane) if spread else 0.0
    if not spread:
        tot.t[0] = float(lane)


def rep_mt_adam_ema(A, sig, res):
    """clip_grad_norm_ -> torch.optim.Adam -> EMA over every row of the table, in place.  Reference: adam_reference (torch's own Adam in
    float64 on the stored values, the betas, lr and eps as the C floats the kernel is handed), with the clip coefficient taken in
    float64 from the bank the kernel reads; bars: _adam_bars.  The scalars of a signature recorded with hyper_dev are not in it: the
    replay hands over those of step 1000 (lr 2e-4, ema_w 1e-4, where training spends its life) unless opts say otherwise."""
    table, n, ptot, max_norm, lr, b1, b2, eps, bc1, bc2, ema_w, phyper = sig
    rows, opts = table[1], dict(table[2])
    assert n == len(rows) and _f(b1) == _f(BETA1) and _f(b2) == _f(BETA2)
    numels, slots = _mt_setup(A, rows, opts)
    by_value = [lr, b1, b2, eps, bc1, bc2, ema_w]
    hyper = None
    if _opt(phyper):
        bcs = bias_corrections(opts.get("step", 1000))
        hyper = A.buf("hyper", 4, F32, _mod(phyper)).fill(torch.tensor([opts.get("lr", 2e-4), bcs[0], bcs[1], opts.get("ema_w", 1e-4)],
                                                                       dtype=torch.float64)).all_in()
        lr, bc1, bc2, ema_w = (float(x) for x in hyper.t)              # what the kernel reads
    tot = None
    if _opt(ptot):
        tot = A.buf("total_sq", 64, F32, _mod(ptot)).all_in()
        _bank_for(A, numels, slots, tot)
    for r, nn in enumerate(numels):
        for c in range(5):
            if slots[c][r] is not None:
                _mark(slots[c][r], nn, read=True, write=c != 1)
    before = _before(numels, slots)
    tb = _table_buf(A, _mt_rows_table(rows, slots))
    A.snapshot()
    _launch("ddpm_mt_adam_ema", [tb.ptr, n, _ptr(tot), max_norm] + by_value + [_ptr(hyper)])
    sync()
    A.check()
    _adam_check(A, res, before, _after(numels, slots), None if tot is None else tot.t.clone(), max_norm, lr, bc1, bc2, eps, ema_w)


def rep_adam_ema_step(A, sig, res):
    """The single-tensor form of the same update (total_sq[0] is the squared norm): the same reference and bars."""
    pp, pg, pm, pv, psh, n, ptot, max_norm, lr, b1, b2, eps, bc1, bc2, ema_w = sig
    cols = tuple((not _opt(p), _mod(p) % 16, SEPARATE) for p in (pp, pg, pm, pv, psh))
    rows = ((n, cols),)
    numels, slots = _mt_setup(A, rows, {"g": "loguniform"})
    tot = None
    if _opt(ptot):
        tot = A.buf("total_sq", 1, F32, _mod(ptot)).all_in()
        tot.t[0] = float((_d(_sl(slots[1][0], n)) ** 2).sum())
    for c in range(5):
        if slots[c][0] is not None:
            _mark(slots[c][0], n, read=True, write=c != 1)
    before = _before(numels, slots)
    A.snapshot()
    _launch("ddpm_adam_ema_step", [_addr(slots[c][0]) for c in range(5)] + [n, _ptr(tot), max_norm, lr, b1, b2, eps, bc1, bc2, ema_w])
    sync()
    A.check()
    bank = None
    if tot is not None:
        bank = torch.zeros(64, dtype=torch.float32, device=A.device)
        bank[0] = tot.t[0]
    _adam_check(A, res, before, _after(numels, slots), bank, max_norm, lr, bc1, bc2, eps, ema_w)


def rep_sumsq_accumulate(A, sig, res):
    """total_sq[0] += ||g||^2 (csrc/optim.hip sumsq_kernel + sum_partials_kernel: min(1024, ceil(n / 256)) blocks of 256 threads, one
    running sum a thread, 6 wave levels, a 3-step block sum; then one block over the partials and the add into the prior content).
    Bound: d u (sum g^2 + |prior|)."""
    pg, n, ptot, pws = sig
    g = A.buf("g", n, F32, _mod(pg)).fill(A.randn(n, scale=0.5)).all_in()
    A.shape("grad", g.t.view(-1, 1))
    tot = A.buf("total_sq", 1, F32, _mod(ptot)).fill(A.randn(1).abs()).all_in()
    ws = A.buf("workspace", 1024, F32, _mod(pws))
    ws.all_out()
    ws.scratch = True
    tot.all_out()
    prior = _d(tot.t).clone()
    A.snapshot()
    _launch("ddpm_sumsq_accumulate", [g.ptr, n, tot.ptr, ws.ptr])
    sync()
    A.check()
    nblk = min(1024, -(-n // 256))
    d = (1 + -(-n // (nblk * 256)) + 6 + 3) + (-(-nblk // 256) + 6 + 3 + 1)
    S = (_d(g.t) ** 2).sum().reshape(1)
    res.cmp("total_sq", tot.t, S + prior, d * U_F32 * (S + prior.abs()) + n * DENORM)


# ---- layout entries: bit-exact against an indexing reference rounded once to the stored type (bar 0)
def _unpack_common(A, sig, res, fused):
    pgp, pgf, table, n, scale = sig[:5]
    rows, opts = table[1], dict(table[2])
    assert n == len(rows)
    cnt = [N * C * RS for _, _, N, C, RS in rows]
    gp = A.buf("gpack", max(r[0] + c for r, c in zip(rows, cnt)), F32, _mod(pgp))
    gf = A.buf("gflat", max(r[1] + c for r, c in zip(rows, cnt)), F32, _mod(pgf))
    gp.fill(A.randn(gp.n))
    gf.fill(A.randn(gf.n))
    planted = None
    if opts.get("g") == "planted":
        gp.t.zero_()

        def store(r, i, value):                       # element i of the row's destination comes from (n, tap, c) of its source
            src, _, N, C, RS = rows[r]
            nc, tap = divmod(i, RS)
            nn, c = divmod(nc, C)
            gp.t[src + (nn * RS + tap) * C + c] = value
        # one sweep of the 64 blocks: 64 * 256 elements, or 64 * 4 wave items of 64 channels x 9 taps in the slab form
        planted = _planted(cnt, lambda r: 64 * 4 * 64 * 9 if rows[r][4] == 9 and rows[r][3] % 64 == 0 else 64 * 256, store)
        planted *= _f(scale) ** 2
    else:
        for src, c in dict.fromkeys((r[0], c) for r, c in zip(rows, cnt) if c):       # (rows may share a source: transformed once)
            A.shape("data", gp.t[src:src + c].view(-1, 1))
    for (src, dst, _, _, _), c in zip(rows, cnt):
        gp.readable[src:src + c] = True
        gf.written[dst:dst + c] = True
    tot = None
    if fused:
        ptot, total_floats = sig[5:7]
        assert total_floats >= 64 + SUMSQ_SLOT_BLOCKS * n
        tot = A.buf("total_sq", total_floats, F32, _mod(ptot)).fill(A.randn(total_floats))
        tot.written[:64 + SUMSQ_SLOT_BLOCKS * n] = True
        tot.result = torch.zeros_like(tot.written)
        tot.result[:64] = True
    tb = _table_buf(A, [list(r) for r in rows])
    A.snapshot()
    if fused:
        _launch("ddpm_wgrad_unpack_sumsq", [gp.ptr, gf.ptr, tb.ptr, n, scale, tot.ptr, total_floats])
    else:
        _launch("ddpm_wgrad_unpack", [gp.ptr, gf.ptr, tb.ptr, n, scale])
    sync()
    A.check()
    S = torch.zeros((), dtype=torch.float64, device=A.device)
    its = 0
    for r, ((src, dst, N, C, RS), c) in enumerate(zip(rows, cnt)):
        if c == 0:
            continue
        ref = (_d(gp.t[src:src + c]).reshape(N, RS, C).transpose(1, 2) * _f(scale)).to(torch.float32).reshape(-1)
        got = gf.t[dst:dst + c]
        res.tensors[(r, "gflat")] = got.clone()
        res.cmp(f"gflat[{r}]", got, _d(ref), torch.zeros(c, dtype=torch.float64, device=A.device))
        S = S + (_d(got) ** 2).sum()
        if RS == 9 and C % 64 == 0:
            its = max(its, 1 + 9 * -(-(N * (C // 64)) // 256))
        else:
            its = max(its, 1 + -(-c // (64 * 256)))
    if fused:
        d = _sumsq_depth(its, 64 * n)
        res.depth = d
        _check_bank(res, "total_sq", tot.t[:64], S, d * U_F32 * S + sum(cnt) * DENORM, planted)


def rep_wgrad_unpack(A, sig, res):
    """gflat[dst + (n C + c) RS + tap] = fl32(scale gpack[src + (n RS + tap) C + c]) for every row {src, dst, N, C, RS} of the table:
    one fp32 product an element, bit-exact against the float64 product rounded once; nothing outside the rows' destinations changes."""
    _unpack_common(A, sig, res, False)


def rep_wgrad_unpack_sumsq(A, sig, res):
    """The same pass, and total_sq[0] = the sum of squares of what it wrote (csrc/elementwise.hip wgrad_unpack_kernel: 64 blocks a row;
    a thread's running sum over ceil(count / (64 * 256)) elements, or in the wave-slab form of the 3x3 rows with C % 64 == 0 nine taps
    an item over ceil(N (C / 64) / 256) items).  Bound: d u sum g^2 against the float64 sum of the values read back from gflat."""
    _unpack_common(A, sig, res, True)


def rep_pack_weight_multi(A, sig, res):
    """Both derived layouts of every row {w, w_fwd, w_dgrad, N, C, R | flags, Cp, Np}: w_fwd[n][tap][c] and w_dgrad[c][flipped tap][n],
    channel pads zero — copies rounded once to the stored type, bit-exact.  Flag 0x100: w_dgrad is the 4 x 4 effective kernel of the
    Upsample convs, E[P][Q] = sum of up to four flipped taps in fp32, held to c (u_f32 sum |taps| + u_out |E|)."""
    table, n, dt = sig
    rows = table[1]
    assert n == len(rows)
    es, T = (2 if dt == BF16 else 4), _TD[dt]
    ext = [_pack_extents(*g, es) for g, _ in rows]
    ws = _carve(A, "w", [c[0] for _, c in rows], [e[0] // 4 for e in ext], F32)
    wf = _carve(A, "w_fwd", [c[1] for _, c in rows], [e[1] // es for e in ext], dt)
    wd = _carve(A, "w_dgrad", [c[2] for _, c in rows], [e[2] // es for e in ext], dt)
    tab = []
    for r, ((N, C, Rf, Cp, Np), _) in enumerate(rows):
        R = Rf & 0xff
        _sl(ws[r], ext[r][0] // 4).copy_(A.randn(ext[r][0] // 4, scale=1.0 / math.sqrt(C * R * R)))
        _mark(ws[r], ext[r][0] // 4, read=True)
        for slot, e in ((wf[r], ext[r][1] // es), (wd[r], ext[r][2] // es)):
            if slot is not None:
                _sl(slot, e).copy_(A.randn(e).to(T))
                _mark(slot, e, write=True)
        tab.append([_addr(ws[r]), _addr(wf[r], es), _addr(wd[r], es), N, C, Rf, Cp, Np])
    tb = _table_buf(A, tab)
    A.snapshot()
    _launch("ddpm_pack_weight_multi", [tb.ptr, n, dt])
    sync()
    A.check()
    u = U_BF16 if dt == BF16 else U_F32
    for r, ((N, C, Rf, Cp, Np), _) in enumerate(rows):
        R, up = Rf & 0xff, bool(Rf & 0x100)
        w = _d(_sl(ws[r], N * C * R * R)).reshape(N, C, R, R)
        if wf[r] is not None:
            ref = w.new_zeros(N, R, R, Cp)
            ref[..., :C] = w.permute(0, 2, 3, 1)
            got = _sl(wf[r], ext[r][1] // es)
            res.tensors[(r, "w_fwd")] = got.clone()
            res.cmp(f"w_fwd[{r}]", got, _d(ref.reshape(-1).to(T)), torch.zeros(got.numel(), dtype=torch.float64, device=A.device))
        if wd[r] is None:
            continue
        got = _sl(wd[r], ext[r][2] // es)
        res.tensors[(r, "w_dgrad")] = got.clone()
        D = w.flip(2, 3)
        if up:
            E, mag = w.new_zeros(N, C, 4, 4), w.new_zeros(N, C, 4, 4)
            for a in range(2):
                for b in range(2):
                    E[:, :, a:a + 3, b:b + 3] += D
                    mag[:, :, a:a + 3, b:b + 3] += D.abs()
            ref, bar = w.new_zeros(C, 4, 4, Np), w.new_zeros(C, 4, 4, Np)
            ref[..., :N], bar[..., :N] = E.permute(1, 2, 3, 0), C_GEMM * (U_F32 * mag + u * E.abs()).permute(1, 2, 3, 0)
            res.cmp(f"w_dgrad4x4[{r}]", got, ref.reshape(-1), bar.reshape(-1))
        else:
            ref = w.new_zeros(C, R, R, Np)
            ref[..., :N] = D.permute(1, 2, 3, 0)
            res.cmp(f"w_dgrad[{r}]", got, _d(ref.reshape(-1).to(T)), torch.zeros(got.numel(), dtype=torch.float64, device=A.device))


def rep_mt_gather(A, sig, res):
    """dst_i = a_i (+ b_i) for every row {a, b (0 = none), dst, numel}: a copy, or one fp32 addition — the float64 sum rounded once."""
    table, n = sig
    rows = table[1]
    assert n == len(rows)
    numels = [nn for nn, _ in rows]
    slots = [_carve(A, nm, [c[i] for _, c in rows], numels, F32) for i, nm in enumerate(("a", "b", "dst"))]
    for r, nn in enumerate(numels):
        for c in range(3):
            if slots[c][r] is not None:
                _sl(slots[c][r], nn).copy_(A.randn(nn))
                _mark(slots[c][r], nn, read=c < 2, write=c == 2)
    tb = _table_buf(A, [[_addr(slots[c][r]) for c in range(3)] + [nn] for r, nn in enumerate(numels)])
    A.snapshot()
    _launch("ddpm_mt_gather_f32", [tb.ptr, n])
    sync()
    A.check()
    for r, nn in enumerate(numels):
        ref = _d(_sl(slots[0][r], nn))
        if slots[1][r] is not None:
            ref = ref + _d(_sl(slots[1][r], nn))
        got = _sl(slots[2][r], nn)
        res.tensors[(r, "dst")] = got.clone()
        res.cmp(f"dst[{r}]", got, _d(ref.to(torch.float32)), torch.zeros(nn, dtype=torch.float64, device=A.device))


REPLAY = {
    "ddpm_mt_grad_sumsq": rep_mt_grad_sumsq,
    "ddpm_mt_adam_ema": rep_mt_adam_ema,
    "ddpm_sumsq_accumulate": rep_sumsq_accumulate,
    "ddpm_adam_ema_step": rep_adam_ema_step,
    "ddpm_wgrad_unpack": rep_wgrad_unpack,
    "ddpm_wgrad_unpack_sumsq": rep_wgrad_unpack_sumsq,
    "ddpm_pack_weight_multi": rep_pack_weight_multi,
    "ddpm_mt_gather_f32": rep_mt_gather,
    "ddpm_conv2d_nhwc": rep_conv2d,
    "ddpm_conv3x3_wgrad_nhwc": rep_conv3x3_wgrad,
    "ddpm_conv3x3_wgrad_up_nhwc": rep_conv3x3_wgrad_up,
    "ddpm_conv1x1_wgrad_nhwc": rep_conv1x1_wgrad,
    "ddpm_conv2d_wgrad_nhwc": rep_conv2d_wgrad,
    "ddpm_wgrad_reduce": rep_wgrad_reduce,
    "ddpm_gemm": rep_gemm,
    "ddpm_atb_f32": rep_atb,
    "ddpm_groupnorm_silu_fwd": rep_gn_fwd,
    "ddpm_groupnorm_silu_bwd": rep_gn_bwd,
    "ddpm_attention_fwd": rep_attn_fwd,
    "ddpm_attention_fwd_lse": rep_attn_fwd_lse,
    "ddpm_attention_bwd": rep_attn_bwd,
    "ddpm_attention_mh_fwd": rep_attn_mh_fwd,
    "ddpm_attention_mh_bwd": rep_attn_mh_bwd,
    "ddpm_colsum": rep_colsum,
    "ddpm_upsample2x_bwd": rep_upsample2x_bwd,
    "ddpm_q_sample": rep_q_sample,
    "ddpm_mse_fwd": rep_mse_fwd,
    "ddpm_mse_bwd": rep_mse_bwd,
    "ddpm_p_sample_step": rep_p_sample_step,
    "ddpm_softmax_fwd": rep_softmax_fwd,
    "ddpm_softmax_bwd": rep_softmax_bwd,
    "ddpm_silu_fwd": rep_silu_fwd,
    "ddpm_silu_bwd": rep_silu_bwd,
    "ddpm_add_rows": rep_add_rows,
    "ddpm_nchw_to_nhwc": rep_nchw_to_nhwc,
    "ddpm_timestep_embedding": rep_timestep_embedding,
    "ddpm_gather_rows_f32": rep_gather_rows,
    "ddpm_weighted_sum_f32": rep_weighted_sum,
}

def _p(mod=0, null=False):
    return ("p", null, mod)


# Signatures of the replayed elementwise / softmax entries at edge geometries of their own (both dtypes, accumulate on and off, pitched
# rows, odd lengths, a single row), replayed next to the recorded ones: ddpm_gather_rows_f32 (the graph-captured sampler's time table)
# and ddpm_add_rows (gradient fan-in) are launched by no recorded workload.
SYNTHETIC = [
    ("ddpm_softmax_fwd", (_p(), _p(16), 1000, 256, F32)),
    ("ddpm_softmax_fwd", (_p(), _p(), 3, 4096, BF16)),
    ("ddpm_softmax_fwd", (_p(48), _p(8), 77, 52, F32)),
    ("ddpm_softmax_bwd", (_p(), _p(), _p(32), 1000, 256, F32)),
    ("ddpm_softmax_bwd", (_p(), _p(), _p(), 5, 1024, BF16)),
    ("ddpm_silu_fwd", (_p(), _p(4), 100003)),
    ("ddpm_silu_bwd", (_p(), _p(), _p(), 100003, 0)),
    ("ddpm_silu_bwd", (_p(8), _p(), _p(4), 5000, 1)),
    ("ddpm_add_rows", (_p(), 264, _p(), 256, 1000, 256, 1, BF16)),
    ("ddpm_add_rows", (_p(16), 384, _p(), 128, 777, 128, 0, BF16)),
    ("ddpm_add_rows", (_p(), 132, _p(48), 260, 333, 128, 1, F32)),
    ("ddpm_add_rows", (_p(), 128, _p(), 128, 1, 128, 0, F32)),
    ("ddpm_timestep_embedding", (_p(), _p(), _p(), 300, 128)),
    ("ddpm_timestep_embedding", (_p(8), _p(4), _p(), 7, 127)),
    ("ddpm_gather_rows_f32", (_p(), _p(), _p(), 128, 4992, 1000)),
    ("ddpm_gather_rows_f32", (_p(), _p(8), _p(), 1, 4992, 1000)),
    ("ddpm_gather_rows_f32", (_p(), _p(), _p(), 7, 4, 3)),
    ("ddpm_weighted_sum_f32", (_p(), _p(), _p(), 128)),
    ("ddpm_weighted_sum_f32", (_p(4), _p(), _p(8), 1)),
    ("ddpm_weighted_sum_f32", (_p(), _p(), _p(), 100003)),
]


# ----------------------------------------------------------------------------------------------------------------- odd geometries
# Hand-written signatures at non-square images and pixel / token counts that are no power of two: the smallest shapes at which each
# kernel is still dispatched, so that tiles_x != tiles_y (1 x 3, 3 x 1, 3 x 3, 2 x 3 patches), Ho != Wo in the implicit-GEMM index
# arithmetic, ragged last iterations in the GroupNorm forms and token counts between the tested ones reach the kernels.  Operands are
# pitched as tests/test_kernels_gpu.py pitches them (x_ld = C + 16, y_ld = N + 32, row bias N + 8), every pointer 16-byte aligned.
# Each row is (signature, kernel id variant_of must name, or None for the entries without a dispatch query).
def _conv_sig(B, H, W, C, N, Ho=None, Wo=None, R=3, S=3, stride=1, pad=(1, 1), ups=0, dil=0, bias=0, rowbias=0, res=0, acc=0, mode=0,
              splits=1, dt=BF16, x_ld=None, y_ld=None):
    Ho, Wo = (H << ups if Ho is None else Ho), (W << ups if Wo is None else Wo)
    ws = splits > 1
    y_ld = N + 32 if y_ld is None else y_ld
    return ("ddpm_conv2d_nhwc", (_p(), C + 16 if x_ld is None else x_ld, _p(), _p(), y_ld, _p(null=not bias), _p(null=not rowbias),
                                 N + 8 if rowbias else 0, _p(null=not res), y_ld if res else 0, B, H, W, C, Ho, Wo, N, R, S, stride,
                                 pad[0], pad[1], ups, dil, acc, mode, splits, _p(null=not ws), _p(null=not ws), dt))


def _wg3_sig(B, H, W, C, N, up=False, slab=False):
    n_one = N * 9 * C
    return ("ddpm_conv3x3_wgrad_up_nhwc" if up else "ddpm_conv3x3_wgrad_nhwc",
            (_p(), N + 32, _p(), C + 16, _p(), n_one + 64 if slab else 0, _p(), N + 4 if slab else 0, B, H, W, C, N, N, 0, BF16))


def _wg_sig(B, H, W, C, N, R=3, S=3, splits=1, slab=False):
    return ("ddpm_conv2d_wgrad_nhwc", (_p(), N + 32, _p(), C + 16, _p(), N * R * S * C + 64 if slab else 0, B, H, W, C, C, H, W, N, N, R, S,
                                       1, R // 2, S // 2, 0, splits, BF16))


def _gn_sigs(HW, C, dt, silu, drop, full, B=3, G=32):
    """(forward, backward) of one GroupNorm geometry; full: the backward accumulates and has `add` and `dx_colsum` operands."""
    seed = 977 + HW + C
    fwd = ("ddpm_groupnorm_silu_fwd", (_p(), C + 16, _p(), C + 8, _p(), _p(), _p(), _p(), B, HW, C, G, 1e-6, silu, drop, seed,
                                       _p(null=not full), dt))
    bwd = ("ddpm_groupnorm_silu_bwd", (_p(), C + 16, _p(), C + 8, _p(), C + 24, _p(), _p(), _p(), _p(), _p(), _p(), B, HW, C, G, silu, drop,
                                       seed, _p(null=not full), int(full), _p(null=not full), C + 4 if full else 0, _p(null=not full),
                                       C + 32 if full else 0, dt))
    return [(fwd, None), (bwd, None)]


def _attn_sigs(B, L, C):
    scale = float(C) ** -0.5
    return [(("ddpm_attention_fwd_lse", (_p(), 3 * C + 16, _p(), C + 8, _p(), B, L, C, scale, BF16)), None),
            (("ddpm_attention_bwd", (_p(), 3 * C + 16, _p(), C + 8, _p(), C + 8, _p(), _p(), _p(), 3 * C + 24, B, L, C, scale, BF16)), None)]


ODD_GEOMETRY = [
    # ---- ddpm_conv2d_nhwc, forward and data gradient
    # 13 conv3x3_pc (wave-specialised, 16 x 16 patches)
    (_conv_sig(22, 16, 48, 64, 64, bias=1), 13),                            # 1 x 3 patches
    (_conv_sig(22, 48, 16, 64, 128), 13),                                   # 3 x 1 patches
    (_conv_sig(8, 48, 48, 64, 64), 13),                                     # 3 x 3 patches
    (_conv_sig(22, 8, 24, 64, 64, ups=1, bias=1), 13),                      # input stored at 8 x 24, gathered as 16 x 48
    # 8 conv3x3_stream<16> (the residual / "+=" epilogues of the 16 x 16 patches)
    (_conv_sig(22, 16, 48, 64, 64, bias=1, rowbias=1, res=1), 8),
    (_conv_sig(11, 48, 32, 64, 64, acc=1), 8),                              # 3 x 2 patches
    # 10 conv3x3_stream<8> (8 x 8 patches)
    (_conv_sig(22, 8, 24, 64, 64, bias=1, rowbias=1), 10),                  # 1 x 3
    (_conv_sig(8, 24, 24, 64, 128, res=1), 10),                             # 3 x 3
    (_conv_sig(22, 24, 8, 128, 64, acc=1), 10),                             # 3 x 1, two channel chunks
    (_conv_sig(11, 16, 24, 64, 64, bias=1), 10),                            # 2 x 3
    (_conv_sig(22, 12, 4, 64, 64, ups=1), 10),                              # input stored at 12 x 4, gathered as 24 x 8
    # 5 conv3x3_halo (N no multiple of 64)
    (_conv_sig(22, 16, 48, 64, 96, bias=1, res=1), 5),
    (_conv_sig(22, 48, 16, 64, 96, bias=1), 5),
    # 11 / 12 edge convs
    (_conv_sig(22, 16, 48, 64, 3, bias=1, mode=3), 11),
    (_conv_sig(22, 48, 16, 8, 64, bias=1, x_ld=8), 12),
    # 7 pw_conv (streaming 1x1)
    (_conv_sig(22, 24, 16, 128, 192, R=1, S=1, pad=(0, 0), bias=1, res=1), 7),
    # 4 gemm64 (generic implicit GEMM, 64 x 64 tiles): Ho != Wo in dHoWo / dWo
    (_conv_sig(3, 12, 20, 64, 96, bias=1, rowbias=1, res=1, acc=1), 4),
    (_conv_sig(3, 6, 10, 32, 64, bias=1, dt=F32), 4),
    (_conv_sig(2, 8, 12, 64, 64, Ho=4, Wo=6, stride=2, pad=(0, 0), bias=1), 4),       # the Downsample form (SamePad2d(3, 2))
    (_conv_sig(2, 10, 6, 64, 64, Ho=5, Wo=3, stride=2, pad=(0, 0), bias=1), 4),       # ... with odd output sides
    (_conv_sig(3, 6, 10, 64, 64, R=1, S=1, pad=(0, 0), bias=1, rowbias=1), 4),
    # 3 gemm_kernel, deep ring: the parity-phase data gradient of a stride-2 conv (dHhWh / dWh)
    (_conv_sig(4, 4, 8, 64, 64, Ho=8, Wo=16, pad=(2, 2), dil=1, acc=1), 3),
    (_conv_sig(8, 6, 8, 64, 64, Ho=12, Wo=16, pad=(1, 1), dil=1, acc=1), 3),
    # ---- weight gradients and reductions
    (_wg3_sig(4, 16, 48, 64, 64), 14),                                      # wgrad3x3_ws, atomics
    (_wg3_sig(4, 16, 48, 64, 64, slab=True), 14),                           # ... slabs
    (_wg3_sig(3, 48, 16, 64, 128, up=True), 14),                            # x stored at 24 x 8
    (_wg3_sig(3, 48, 16, 64, 128, up=True, slab=True), 14),
    (_wg_sig(3, 12, 20, 64, 64, splits=4), 2),                              # generic: K = 720 pixels in 4 slices, atomics
    (_wg_sig(3, 12, 20, 64, 64, splits=4, slab=True), 2),
    (_wg_sig(22, 8, 24, 64, 64, splits=6), 2),                              # W = 8 needs H = 8 for the patch kernel: generic, K = 4224
    (_wg_sig(22, 8, 24, 64, 64, splits=6, slab=True), 2),
    (("ddpm_conv1x1_wgrad_nhwc", (_p(), 64 + 32, _p(), 64 + 16, _p(), 64 * 64 + 64, _p(), 64 + 4, 22 * 8 * 24, 64, 64, 0, BF16)), 9),
    (("ddpm_upsample2x_bwd", (_p(), _p(), 64 + 16, 3, 4, 6, 64, 1, BF16)), None),
    (("ddpm_upsample2x_bwd", (_p(), _p(), 32 + 16, 3, 4, 6, 32, 0, F32)), None),
    (("ddpm_colsum", (_p(), 64 + 8, _p(), 64 + 4, _p(), 3, 192, 64, BF16)), None),
    (("ddpm_colsum", (_p(), 128 + 8, _p(), 128 + 4, _p(), 3, 192, 128, F32)), None),
]
# ---- GroupNorm forward / backward, B = 3, G = 32: HW chosen so that the last iteration of every form is ragged (HW is no multiple of
# the rows a block sweeps per iteration).  Form by the plan arithmetic of csrc/norm.hip (gn_fused_plan / gn_lds_plan), the same for the
# forward and the backward and for both dtypes: "256 x v" the 256-thread staged kernel with v vectors per thread, "512 x v" the
# 512-thread one, "streaming" the two-launch form.  P2: the backward takes the power-of-two-group instantiation.
for _dt in (BF16, F32):
    for _HW, _C, _silu, _drop, _full in (
            (9, 128, 1, 0.0, False),            # 256 x 1, P2
            (36, 256, 1, 0.1, True),            # 256 x 2, P2
            (96, 64, 1, 0.0, False),            # 512 x 2 (bf16: 2 channels per group, not P2)
            (96, 256, 0, 0.0, True),            # 512 x 2, P2
            (144, 512, 1, 0.1, False),          # 512 x 4, P2
            (576, 128, 1, 0.0, True),           # 512 x 8, P2
            (2304, 64, 1, 0.1, True),           # streaming
            (48, 384, 0, 0.0, True)):           # 512 x 2 with 12-channel groups (3 / 6 vector columns per group chunk: strided wave tree)
        ODD_GEOMETRY += _gn_sigs(_HW, _C, _dt, _silu, _drop, _full)
# ---- the fused attention pair at token counts between the tested ones
for _B, _L, _C in ((2, 96, 128), (2, 144, 256), (1, 192, 512), (2, 240, 64), (3, 48, 256), (2, 80, 128)):
    ODD_GEOMETRY += _attn_sigs(_B, _L, _C)


# ----------------------------------------------------------------------------------------------------------------- small extras
# Replayed entries that neither list above holds, at the smallest shapes that still take every path: ragged GEMM tiles, the batched
# form, the four transposes, every epilogue and output mode, the in-launch split-K reductions of the conv, the fused attention forward
# and the diffusion elementwise kernels at a batch and a row length that are no power of two.
def _up(n, m):
    return -(-n // m) * m


def _gemm_sig(M, N, K, batch, a_tr=0, b_tr=0, bias=0, res=0, acc=0, mode=0, alpha=1.0, dt=BF16):
    ar, ac = (K, M) if a_tr else (M, K)
    br, bc = (K, N) if b_tr else (N, K)
    a_ld, b_ld, c_ld, r_ld = _up(ac, 8) + 16, _up(bc, 8) + 16, _up(N, 8) + 32, _up(N, 8) + 8
    return ("ddpm_gemm", (_p(), a_ld, ar * a_ld + 32, a_tr, _p(), b_ld, br * b_ld + 64, b_tr, _p(), c_ld, M * c_ld + 16, _p(null=not bias),
                          _p(null=not res), r_ld if res else 0, M * r_ld + 8 if res else 0, M, N, K, batch, alpha, acc, mode, 1, dt))


EXTRA_SMALL = []
for _dt in (BF16, F32):
    # the contract wants the contiguous extent of an operand in whole 16-byte vectors: a transposed A of bf16 cannot have M = 300
    _Mt = 300 if _dt == F32 else 296
    EXTRA_SMALL += [
        _gemm_sig(300, 136, 200, 1, bias=1, res=1, acc=1, alpha=0.5, dt=_dt),
        _gemm_sig(_Mt, 136, 200, 1, a_tr=1, mode=1, dt=_dt),
        _gemm_sig(300, 136, 200, 1, b_tr=1, mode=2, dt=_dt),
        _gemm_sig(_Mt, 136, 200, 1, a_tr=1, b_tr=1, dt=_dt),
        _gemm_sig(16, 16, 16, 3, bias=1, res=1, acc=1, dt=_dt),
        _gemm_sig(16, 16, 16, 3, a_tr=1, b_tr=1, mode=2, dt=_dt),
        _gemm_sig(16, 16, 16, 3, a_tr=1, mode=1, alpha=0.25, dt=_dt),
        _conv_sig(2, 8, 8, 512, 512, splits=2, dt=_dt),
    ]
EXTRA_SMALL += [
    _conv_sig(16, 4, 4, 256, 256, splits=5),
    ("ddpm_atb_f32", (_p(), 136, _p(), 76, _p(), 80, 130, 70, 37)),
    ("ddpm_atb_f32", (_p(), 100, _p(), 72, _p(), 72, 100, 72, 96)),
    ("ddpm_attention_fwd", (_p(), 3 * 128 + 16, _p(), 128 + 8, 2, 128, 128, 128.0 ** -0.5, BF16)),
    ("ddpm_attention_fwd", (_p(), 3 * 256 + 16, _p(), 256 + 8, 2, 384, 256, 256.0 ** -0.5, BF16)),
    ("ddpm_q_sample", (_p(), _p(), _p(), _p(), _p(), _p(), 5, 192, 1000)),
    ("ddpm_mse_fwd", (_p(), _p(), _p(), 5, 192)),
    ("ddpm_mse_bwd", (_p(), _p(), _p(), _p(), 5, 192)),
    ("ddpm_p_sample_step", (_p(), _p(), _p(), _p(), _p(), _p(), _p(), _p(), _p(), _p(), _p(), 5, 192, 0, 1, 1000)),
    ("ddpm_p_sample_step", (_p(), _p(), _p(), _p(), _p(), _p(), _p(), _p(), _p(), _p(), _p(null=True), 5, 192, 0, 0, 1000)),
    ("ddpm_wgrad_reduce", (_p(), 1, 4100, 3, 4104)),
]


# ----------------------------------------------------------------------------------------------------------------- edge channel counts
# Hand-written signatures of what in_conv and out_conv launch when the network's edge channel counts are not 3 (W18-W24 record the same
# geometries live): 1 and 4 channels stored as 8 (bf16) or 4 (fp32), 12 stored as 16 (bf16) or 12 (fp32), at the images those networks
# see (B = 64 at 16 x 16, B = 16 at 32 x 32: 16384 pixels, the floor of the edge kernels).  Operands are pitched the way the engine
# pitches them (the staged image and the output gradient are dense).  Each row is (signature, kernel id variant_of must name).
def _wg3_edge_sig(B, H, W, C, N, Nreal, splits=16):
    return ("ddpm_conv3x3_wgrad_nhwc", (_p(), N, _p(), C, _p(), _up(Nreal * 9 * C, 4), _p(null=True), _up(Nreal, 4), B, H, W, C, N, Nreal, splits, BF16))


def _wg_edge_sig(B, H, W, C, Creal, N, Nreal, splits, dt):
    return ("ddpm_conv2d_wgrad_nhwc", (_p(), N if N <= 16 else N + 64, _p(), C if C <= 16 else C + 64, _p(), 0, B, H, W, C, Creal, H, W, N, Nreal, 3, 3,
                                       1, 1, 1, 0, splits, dt))


EDGE_CHANNELS = [
    # ---- bf16 forward: in_conv from the staged image, out_conv into NCHW fp32
    (_conv_sig(64, 16, 16, 8, 64, bias=1, x_ld=8), 12),                      # 1 or 4 channels in 8 lanes: the few-input-channel kernel
    (_conv_sig(64, 16, 16, 16, 64, bias=1, x_ld=16), 3),                     # 12 channels in 16 lanes: the tile GEMM, K = 144
    (_conv_sig(16, 32, 32, 64, 1, bias=1, mode=3), 11),
    (_conv_sig(64, 16, 16, 64, 4, bias=1, mode=3), 11),
    (_conv_sig(64, 16, 16, 64, 12, bias=1, mode=3), 11),
    (_conv_sig(64, 16, 16, 64, 24, bias=1, mode=3), 3),                      # past the edge kernel's 16: the tile GEMM writes NCHW
    # ---- bf16 backward: out_conv's data gradient (K = 9 Np), in_conv's data gradient when the input asks for it (want_dx)
    (_conv_sig(64, 16, 16, 8, 64, x_ld=8), 12),
    (_conv_sig(64, 16, 16, 16, 64, x_ld=16), 3),
    (_conv_sig(16, 32, 32, 64, 1, mode=3), 11),
    (_conv_sig(64, 16, 16, 64, 12, mode=3), 11),
    # ---- bf16 weight gradients: out_conv (Nreal / N) through the patch kernel, in_conv (Creal / C) through the generic GEMM
    (_wg3_edge_sig(16, 32, 32, 64, 8, 1), 6),
    (_wg3_edge_sig(64, 16, 16, 64, 8, 4), 6),
    (_wg3_edge_sig(64, 16, 16, 64, 16, 12), 6),
    (_wg_edge_sig(16, 32, 32, 8, 1, 64, 64, 12, BF16), 2),
    (_wg_edge_sig(64, 16, 16, 8, 4, 64, 64, 12, BF16), 2),
    (_wg_edge_sig(64, 16, 16, 16, 12, 64, 64, 12, BF16), 2),
    # ---- fp32 (vectors of 4): everything on the templated tile GEMMs
    (_conv_sig(64, 16, 16, 4, 64, bias=1, x_ld=4, dt=F32), 2),
    (_conv_sig(64, 16, 16, 12, 64, bias=1, x_ld=12, dt=F32), 3),
    (_conv_sig(16, 32, 32, 64, 1, bias=1, mode=3, dt=F32), 3),
    (_conv_sig(64, 16, 16, 64, 12, bias=1, mode=3, dt=F32), 3),
    (_conv_sig(64, 16, 16, 4, 64, x_ld=4, dt=F32), 2),
    (_wg_edge_sig(16, 32, 32, 64, 64, 4, 1, 25, F32), 1),
    (_wg_edge_sig(64, 16, 16, 64, 64, 12, 12, 25, F32), 1),
    (_wg_edge_sig(16, 32, 32, 4, 1, 64, 64, 25, F32), 1),
    (_wg_edge_sig(64, 16, 16, 12, 12, 64, 64, 25, F32), 1),
    # ---- bias gradients over the padded output gradient
    (("ddpm_colsum", (_p(), 8, _p(null=True), 0, _p(), 64, 256, 8, BF16)), None),
    (("ddpm_colsum", (_p(), 16, _p(null=True), 0, _p(), 64, 256, 16, BF16)), None),
    (("ddpm_colsum", (_p(), 4, _p(null=True), 0, _p(), 16, 1024, 4, F32)), None),
    (("ddpm_colsum", (_p(), 12, _p(null=True), 0, _p(), 64, 256, 12, F32)), None),
]


# ----------------------------------------------------------------------------------------------------------------- the 2 GiB operand limit
# Every GEMM-shaped kernel addresses its operands through buffer descriptors with 32-bit byte offsets; its launcher refuses an operand
# whose extent exceeds BUF_OOB bytes (csrc/gfx950.h).  LARGE_OPERANDS holds, for every entry behind such a guard, signatures whose largest
# guarded operand has an extent E in the window  BUF_OOB - unit < E <= BUF_OOB  (unit: the bytes of one image of that operand for the
# image-shaped entries, of one row for the others), E computed as the launcher computes it (guarded_extents), and next to each the
# NEIGHBOUR one image (dense rows) or one pitch step (stretched rows) larger, which the launcher must refuse with DDPM_ERR_SHAPE.
#   dense      natural pitch, B chosen to land in the window, the fewest channels at which the dispatch still names the kernel: the tile
#              counts, grid sizes and FastDiv inputs of the largest pixel count;
#   stretched  few pixels, the guarded operand's pitch raised until (rows - 1) * ld + cols lands in the window: the same byte offsets
#              with almost no arithmetic.  Only operands a kernel reads through a buffer descriptor are stretched (a descriptor
#              range-checks every load); every output keeps its natural pitch.
# Row: (signature, kernel id variant_of must name or None, neighbour signature, what the neighbour must be: "refused", or the kernel id
# that admits it, amplification (power of two, rows of one image) for the reductions or None).
BUF_OOB = 0x7FFFFFF0
ERR_SHAPE = 1                       # DDPM_ERR_SHAPE


def stretch_ld(rows, cols, es=2):
    """largest pitch (in whole 16-byte vectors) at which a [rows][cols] operand of es-byte elements still ends within BUF_OOB"""
    vec = 16 // es
    return (BUF_OOB // es - cols) // (rows - 1) // vec * vec


def guarded_extents(sig):
    """{operand: (extent in bytes as the launcher of that entry computes it, bytes of one window unit)} of the operands the entry's
    BUF_OOB guard covers."""
    name, w = sig
    conv = lambda pix, hw, ld, C, es: ((pix * ld - (ld - C)) * es, hw * ld * es)
    rows = lambda n, cols, ld, es: (pitched(n, cols, ld) * es, ld * es)
    if name == "ddpm_conv2d_nhwc":
        x_ld, B, H, W, C, N, R, S, dt = w[1], w[10], w[11], w[12], w[13], w[16], w[17], w[18], w[29]
        es = 2 if dt == BF16 else 4
        return {"x": conv(B * H * W, H * W, x_ld, C, es), "w": rows(N, R * S * C, R * S * C, es)}
    if name in ("ddpm_conv3x3_wgrad_nhwc", "ddpm_conv3x3_wgrad_up_nhwc"):
        dy_ld, x_ld, (B, H, W, C, N) = w[1], w[3], w[8:13]
        Hs, Ws = (H // 2, W // 2) if name.endswith("_up_nhwc") else (H, W)
        return {"dy": conv(B * H * W, H * W, dy_ld, N, 2), "x": conv(B * Hs * Ws, Hs * Ws, x_ld, C, 2)}
    if name == "ddpm_conv1x1_wgrad_nhwc":
        dy_ld, x_ld, P, C, N = w[1], w[3], w[8], w[9], w[10]
        return {"dy": rows(P, N, dy_ld, 2), "x": rows(P, C, x_ld, 2)}
    if name == "ddpm_conv2d_wgrad_nhwc":
        dy_ld, x_ld, B, H, W, C, Ho, Wo, N, dt = w[1], w[3], w[6], w[7], w[8], w[9], w[11], w[12], w[13], w[22]
        es = 2 if dt == BF16 else 4
        return {"dy": rows(B * Ho * Wo, N, dy_ld, es), "x": conv(B * H * W, H * W, x_ld, C, es)}
    if name == "ddpm_gemm":
        a_ld, a_tr, b_ld, b_tr, M, N, K, dt = w[1], w[3], w[5], w[7], w[15], w[16], w[17], w[23]
        es = 2 if dt == BF16 else 4
        return {"a": rows(*((K, M) if a_tr else (M, K)), a_ld, es), "b": rows(*((K, N) if b_tr else (N, K)), b_ld, es)}
    if name in ("ddpm_attention_fwd_lse", "ddpm_attention_mh_fwd"):
        return {"qkv": (w[6] * w[1] * 2, w[1] * 2)}                                                # L * ld * 2 per sample
    if name == "ddpm_attention_fwd":                  # finish_desc on q, k, v of one sample: [L][C] of pitch ld each
        return {"qkv": rows(w[5], w[6], w[1], 2)}
    if name == "ddpm_attention_bwd":                  # d_o goes through a descriptor as q, k, v do; o and dqkv through 64-bit pointers
        L = w[11]
        return {"qkv": (L * w[1] * 2, w[1] * 2), "d_o": (L * w[5] * 2, w[5] * 2)}
    if name == "ddpm_attention_mh_bwd":
        L = w[11]
        return {"qkv": (L * w[1] * 2, w[1] * 2), "o": (L * w[3] * 2, w[3] * 2), "d_o": (L * w[5] * 2, w[5] * 2)}
    raise KeyError(name)


def largest_extent(sig, rows_per_image=None):
    """(operand, extent bytes, unit bytes) of the largest guarded operand.  rows_per_image: the pixel rows a dense row of the table
    calls one image of ddpm_conv1x1_wgrad_nhwc, which takes a pixel count and knows no images."""
    k, (e, u) = max(guarded_extents(sig).items(), key=lambda kv: kv[1][0])
    return k, e, u * (rows_per_image if rows_per_image and sig[0] == "ddpm_conv1x1_wgrad_nhwc" else 1)


def refusal_status(sig):
    """Status of the LAUNCHING entry on made-up pointers.  Only for a signature guarded_extents puts beyond BUF_OOB: the launcher
    returns before any launch (tests/test_abi_surface.py relies on the same); an admitted size must never get here."""
    assert largest_extent(sig)[1] > BUF_OOB, f"{short(sig)} is within the limit: it would launch on made-up pointers"
    name, words = sig
    args = [(0 if w[1] else 0x10000 + w[2]) if isinstance(w, tuple) else w for w in words]
    if name == "ddpm_conv1x1_wgrad_nhwc" and args[11] <= 0:      # the slab count the library plans: a mismatch is refused on its own
        args[11] = int(_hip.lib().ddpm_conv1x1_wgrad_splits(args[8], args[9], args[10]))
        assert args[11] > 0
    return int(getattr(_hip.lib(), name)(*args, 0))


def _wider(sig, index, step=8):
    """the signature with the pitch word at `index` one vector wider"""
    name, w = sig
    return (name, w[:index] + (w[index] + step,) + w[index + 1:])


def _wg3_dense(B, H, W, C, N, up=False):
    return ("ddpm_conv3x3_wgrad_up_nhwc" if up else "ddpm_conv3x3_wgrad_nhwc",
            (_p(), N, _p(), C, _p(), N * 9 * C, _p(), N, B, H, W, C, N, N, 0, BF16))


def _wg1_sig(P, C, N, dy_ld=None, x_ld=None):
    return ("ddpm_conv1x1_wgrad_nhwc", (_p(), dy_ld or N, _p(), x_ld or C, _p(), N * C + 64, _p(), N + 4, P, C, N, 0, BF16))


def _with(sig, **kw):
    """a hand-written signature with words replaced by position: _with(sig, i3=ld) sets word 3"""
    name, w = sig
    w = list(w)
    for k, v in kw.items():
        w[int(k[1:])] = v
    return (name, tuple(w))


def _mh_sigs(B, L, C, heads, ld=None, o_ld=None, do_ld=None):
    scale = float(C // heads) ** -0.5
    ld = 3 * C + 16 if ld is None else ld
    return (("ddpm_attention_mh_fwd", (_p(), ld, _p(), C + 8, _p(), B, L, C, heads, scale, BF16)),
            ("ddpm_attention_mh_bwd", (_p(), ld, _p(), o_ld or C + 8, _p(), do_ld or C + 8, _p(), _p(), _p(), 3 * C + 24, B, L, C, heads, scale, BF16)))


def _large_rows():
    rows = []

    def dense(sig_of, B, variant, amp=None):
        rows.append((sig_of(B), variant, sig_of(B + 1), "refused", amp))

    def stretched(sig, index, variant, amp=None, neighbour="refused", step=8):
        rows.append((sig, variant, _wider(sig, index, step), neighbour, amp))

    S = stretch_ld
    # ---- ddpm_conv2d_nhwc.  Dense: 32 x 32 images of 64 channels, B = 16383 (16.8 M pixels, 65 532 tiles).
    dense(lambda B: _conv_sig(B, 32, 32, 64, 64, bias=1, x_ld=64, y_ld=64), 16383, 13)                                  # conv3x3_pc
    dense(lambda B: _conv_sig(B, 32, 32, 64, 64, R=1, S=1, pad=(0, 0), bias=1, res=1, x_ld=64, y_ld=64), 16383, 7)      # pw_conv
    stretched(_conv_sig(16, 32, 32, 64, 64, bias=1, rowbias=1, res=1, x_ld=S(16384, 64)), 1, 8)                         # conv3x3_stream<16>
    stretched(_conv_sig(16, 32, 32, 64, 64, acc=1, x_ld=S(16384, 64)), 1, 8)                                            # ... "+="
    stretched(_conv_sig(64, 8, 8, 64, 64, bias=1, rowbias=1, x_ld=S(4096, 64)), 1, 10)                                  # conv3x3_stream<8>
    stretched(_conv_sig(16, 32, 32, 64, 64, bias=1, x_ld=S(16384, 64)), 1, 13)                                          # conv3x3_pc
    stretched(_conv_sig(16, 32, 32, 64, 96, bias=1, res=1, x_ld=S(16384, 64)), 1, 5)                                    # conv3x3_halo
    stretched(_conv_sig(3, 12, 20, 64, 96, bias=1, rowbias=1, res=1, acc=1, x_ld=S(720, 64)), 1, 4)                     # gemm64
    stretched(_conv_sig(16, 32, 32, 64, 3, bias=1, mode=3, x_ld=S(16384, 64)), 1, 11)                                   # edge conv, few outputs
    # edge conv, few inputs: csrc/edgeconv.hip conv3x3_few_in_kernel reads x through 64-bit pointers and its launcher has no extent
    # guard, so the neighbour is ADMITTED (and names the same kernel): no operand limit applies to this form
    stretched(_conv_sig(16, 32, 32, 8, 64, bias=1, x_ld=S(16384, 8)), 1, 12, neighbour=12)
    stretched(_conv_sig(2, 8, 12, 64, 64, Ho=4, Wo=6, stride=2, pad=(0, 0), bias=1, x_ld=S(192, 64)), 1, 4)             # stride 2 (Downsample)
    stretched(_conv_sig(22, 8, 24, 64, 64, ups=1, bias=1, x_ld=S(22 * 192, 64)), 1, 13)                                 # Upsample: x stored at 8 x 24
    stretched(_conv_sig(4, 4, 8, 64, 64, Ho=8, Wo=16, pad=(2, 2), dil=1, acc=1, x_ld=S(128, 64)), 1, 3)                 # parity-phase data gradient
    stretched(_conv_sig(3, 6, 10, 32, 64, bias=1, dt=F32, x_ld=S(180, 32, 4)), 1, 4, step=4)                            # fp32
    stretched(_conv_sig(64, 16, 16, 64, 12, bias=1, mode=3, dt=F32, x_ld=S(16384, 64, 4)), 1, 3, step=4)                # fp32, tile GEMM
    # ---- weight gradients: dy amplified by 16 on three images (amplify_images)
    dense(lambda B: _wg3_dense(B, 32, 32, 64, 64), 16383, 14, amp=(16, 1024))                                            # wgrad3x3_ws, slabs
    stretched(_with(_wg3_sig(4, 16, 48, 64, 64), i1=S(4 * 768, 64)), 1, 14, amp=(16, 768))                              # ... atomics, dy stretched
    stretched(_with(_wg3_edge_sig(16, 32, 32, 64, 8, 1), i3=S(16384, 64)), 3, 6, amp=(16, 1024))                        # wgrad3x3, x stretched
    stretched(_with(_wg3_sig(3, 48, 16, 64, 128, up=True, slab=True), i1=S(3 * 768, 128)), 1, 14, amp=(16, 768))        # _up_, dy stretched
    stretched(_with(_wg3_sig(3, 48, 16, 64, 128, up=True), i3=S(3 * 192, 64)), 3, 14, amp=(16, 768))                    # _up_, x (24 x 8) stretched
    dense(lambda B: _wg1_sig(B * 1024, 64, 64), 16383, 9, amp=(16, 1024))                                                # wgrad1x1
    stretched(_wg1_sig(4224, 64, 64, dy_ld=S(4224, 64)), 1, 9, amp=(16, 192))
    stretched(_wg1_sig(4224, 64, 64, x_ld=S(4224, 64)), 3, 9, amp=(16, 192))
    stretched(_with(_wg_sig(3, 12, 20, 64, 64, splits=4), i3=S(720, 64)), 3, 2, amp=(16, 240))                          # generic, x (gathered)
    stretched(_with(_wg_sig(3, 12, 20, 64, 64, splits=4, slab=True), i1=S(720, 64)), 1, 2, amp=(16, 240))               # generic, dy
    # ---- ddpm_gemm: the limit is per batch; batch = 2 puts the second batch's base beyond 2^31 bytes
    g = _gemm_sig(304, 136, 200, 2, bias=1, res=1)
    a_ld, b_ld = S(304, 200), S(136, 200)
    stretched(_with(g, i1=a_ld, i2=304 * a_ld), 1, 4)
    stretched(_with(g, i5=b_ld, i6=136 * b_ld), 5, 4)
    gt = _gemm_sig(304, 136, 200, 2, a_tr=1, mode=1)
    stretched(_with(gt, i1=S(200, 304), i2=200 * S(200, 304)), 1, 2)
    # ---- attention: B = 2, the per-sample extent L * ld * 2 in the window, the second sample's base beyond 2^31 bytes
    for sg in _attn_sigs(2, 256, 64) + _attn_sigs(2, 144, 128):
        L = sg[0][1][6 if sg[0][0] == "ddpm_attention_fwd_lse" else 11]
        stretched(_with(sg[0], i1=BUF_OOB // 2 // L // 8 * 8), 1, None)
    for sg in (_attn_sigs(2, 256, 64)[1], _attn_sigs(2, 144, 128)[1]):                                                     # the flash backward's d_o
        stretched(_with(sg[0], i5=BUF_OOB // 2 // sg[0][1][11] // 8 * 8), 5, None)
    # ddpm_attention_stream_fwd / _bwd are the heads = 1 case of the mh entries (the same launcher and kernels, csrc/attention_stream.hip
    # stream_fwd / stream_bwd): the last two mh rows below run exactly that case.
    stretched(("ddpm_attention_fwd", (_p(), stretch_ld(128, 128), _p(), 128 + 8, 2, 128, 128, 128.0 ** -0.5, BF16)), 1, None)   # inference kernel
    ld = BUF_OOB // 2 // 200 // 8 * 8
    f, b = _mh_sigs(2, 200, 128, 2, ld=ld)
    stretched(f, 1, None)
    stretched(b, 1, None)
    stretched(_mh_sigs(2, 200, 128, 2, o_ld=ld)[1], 3, None)
    stretched(_mh_sigs(2, 200, 128, 2, do_ld=ld)[1], 5, None)
    f, b = _mh_sigs(2, 520, 512, 1, ld=BUF_OOB // 2 // 520 // 8 * 8)                                                       # d = 512, L > 256
    stretched(f, 1, None)
    stretched(b, 1, None)
    return rows


LARGE_OPERANDS = _large_rows()

# Entries with no guard: the activation-space kernels that index with 64-bit arithmetic.  One bf16 signature each whose operand holds
# just over 2^31 elements (just over 2^32 bytes), reached the stretched way where the entry takes a pitch: a few rows whose element
# offsets pass 2^31 while the float64 reference stays small.  The comment of a row quotes the lines of csrc/elementwise.hip that make
# its indexing 64-bit.  Row: (signature, amplification or None).
_E31 = 1 << 31


def _past(rows, vec=8):
    """smallest pitch (whole vectors) at which the last of `rows` rows starts beyond element offset 2^31"""
    return -(-(_E31 // (rows - 1) + 1) // vec) * vec


ACROSS_2_31 = [
    # add_kernel: `const long long r = i / cv;` ... `x + r * x_ld + c`, `y + r * y_ld + c` (x_ld, y_ld, rows are long long)
    (("ddpm_add_rows", (_p(), _past(1000), _p(), 256, 1000, 256, 1, BF16)), None),
    (("ddpm_add_rows", (_p(16), 384, _p(), _past(777), 777, 128, 0, BF16)), None),
    # colsum_kernel: `const T* base = dy + (long long)b * HW * ld + cx * VEC;` ... `base + (long long)p * ld`,
    # `per_sample + (long long)b * ps_ld + c` (ld, ps_ld are long long)
    (("ddpm_colsum", (_p(), _past(3 * 192), _p(), 64 + 4, _p(), 3, 192, 64, BF16)), (16, 192)),
    # upsample_bwd_kernel: `const long long b = r / H;` ... `dx + ((b * H + y) * W + x) * dx_ld + c` (dx_ld is long long); the dense
    # input `dyu + (((b * 2 * H + 2 * y + dy) * 2 * W) + 2 * x + dxx) * C + c` is formed in long long through b as well, but this
    # row stretches dx only: the dense dy_up stays small, its index is not taken past 2^31 here.  No amplification: every output
    # pixel is the sum of its own 2 x 2 block, no image enters another image's output, and every image of dx is compared.
    (("ddpm_upsample2x_bwd", (_p(), _p(), _past(3 * 24), 3, 4, 6, 64, 1, BF16)), None),
    # nchw_to_nhwc_kernel: `const long long n = (long long)B * HW * Cp;` the loop index i, `bp = i / Cp`, `b = bp / HW` are long long
    # and x is read at `(b * C + c) * HW + p`.  Dense (the entry takes no pitch): 2^28 + 4096 pixels of 8 stored channels.
    (("ddpm_nchw_to_nhwc", (_p(), _p(), 65537, 3, 4096, 8, BF16)), None),
]


# ----------------------------------------------------------------------------------------------------------------- the optimizer tail, by hand
# Hand-written tables of a few tensors each: the smallest shapes at which the tail's kernels can go wrong.  numel 0 (nothing may be
# written), 1, 3, 4, 5 and 1023 .. 1025 around the float4 body and its scalar tail; one grid sweep of mt_adam_ema_kernel (32 blocks x 256
# threads x 4) and of mt_sumsq_kernel (16 x 256 x 4) and one element either side; 512 x 512 x 9, the largest tensor of any shipped
# configuration.  Packings: every tensor its own 16-byte aligned buffer ("sep"); back to back with the trainer's rounding to 4 floats
# ("r4", what the flat gradient is); 1-float gaps ("g1": most rows misaligned, the scalar path next to the vector one); exactly one of
# p, g, m, v, shadow at 4, 8 or 12 bytes modulo 16 (misaligned).
SMALL_NUMELS = (0, 1, 3, 4, 5, 1023, 1024, 1025)
SWEEP_NUMELS = (32 * 256 * 4 - 1, 32 * 256 * 4, 32 * 256 * 4 + 1, 16 * 256 * 4 - 1, 16 * 256 * 4, 16 * 256 * 4 + 1)
MIS_NUMELS = (5, 1025, 16 * 256 * 4 + 1)
LARGEST = 512 * 512 * 9
_MT_COLS = ("p", "g", "m", "v", "shadow")


def _packed_cols(numels, k, pack="sep", mis=None, null=()):
    """[(numel, k columns)] of a table whose k pointer columns are packed as `pack`; mis = (column, bytes modulo 16); null = {(row,
    column)} pointers that are null."""
    rows = []
    mods = [0] * k
    for r, n in enumerate(numels):
        cols = []
        for c in range(k):
            if (r, c) in null:
                cols.append((True, 0, SEPARATE))
                mods[c] = 0
                continue
            last = r + 1 == len(numels) or (r + 1, c) in null
            if pack == "sep" or last:
                m = mis[1] if mis and mis[0] == c and pack == "sep" else mods[c]
                cols.append((False, m, SEPARATE))
                mods[c] = 0
            else:
                gap = 4 if pack == "g1" else 4 * (-n % 4)
                cols.append((False, mods[c], gap))
                mods[c] = (mods[c] + 4 * n + gap) % 16
        rows.append((n, tuple(cols)))
    return tuple(rows)


def _mt_table(numels, pack="sep", mis=None, no_shadow=(), **opts):
    mis = None if mis is None else (_MT_COLS.index(mis[0]), mis[1])
    return ("t", _packed_cols(numels, 5, pack, mis, {(r, 4) for r in no_shadow}), tuple(sorted(opts.items())))


def _adam_sig(table, k, max_norm=1.0, lr=2e-4, ema_w=1e-4, hyper=False, total=True):
    """ddpm_mt_adam_ema at optimizer step k; hyper: lr, the bias corrections and ema_w through hyper_dev instead of by value"""
    bc1, bc2 = bias_corrections(k)
    table = (table[0], table[1], tuple(sorted(dict(table[2], step=k, **({"lr": lr, "ema_w": ema_w} if hyper else {})).items())))
    scal = (0.0, BETA1, BETA2, ADAM_EPS, 1.0, 1.0, 0.0) if hyper else (lr, BETA1, BETA2, ADAM_EPS, bc1, bc2, ema_w)
    return ("ddpm_mt_adam_ema", (table, len(table[1]), _p(null=not total), max_norm) + scal + (_p(null=not hyper),))


def _sumsq_sig(table):
    n = len(table[1])
    return ("ddpm_mt_grad_sumsq", (table, n, _p(), 64 + SUMSQ_SLOT_BLOCKS * n))


def _unpack_table(shapes, **opts):
    """rows {src, dst, N, C, R*S}: sources 4 floats apart beyond the rounding to 4 (pad floats between segments), destinations rounded
    to 4 floats like the flat gradient; a shape with a 4th field shares the source of the row before it (fc.bias and conv1.bias)."""
    rows, so, do = [], 0, 0
    for sh in shapes:
        N, C, RS = sh[:3]
        c = N * C * RS
        if len(sh) > 3:
            rows.append((rows[-1][0], do, N, C, RS))
        else:
            rows.append((so, do, N, C, RS))
            so += (c + 3) // 4 * 4 + 4
        do += (c + 3) // 4 * 4
    return ("t", tuple(rows), tuple(sorted(opts.items())))


def _unpack_sig(table, scale, fused):
    n = len(table[1])
    if fused:
        return ("ddpm_wgrad_unpack_sumsq", (_p(), _p(), table, n, scale, _p(), 64 + SUMSQ_SLOT_BLOCKS * n))
    return ("ddpm_wgrad_unpack", (_p(), _p(), table, n, scale))


# R*S in {1, 9, 16}; C % 64 == 0 (the wave-slab form; 130 x 128 is more than one sweep of its 256 items) and C % 64 != 0 (the gather
# form; 64 x 96 x 9 is more than one sweep of 16384 elements); the edge-channel shapes Creal / Nreal in {1, 4, 12}; plain segments
UNPACK_SHAPES = [(130, 128, 9), (5, 64, 9), (64, 96, 9), (8, 40, 16), (1, 20000, 1), (1, 64, 1), (1, 64, 1, "shared"), (64, 1, 9), (64, 4, 9),
                 (64, 12, 9), (1, 64, 9), (4, 64, 9), (12, 64, 9), (1, 1, 1), (1, 4, 1), (1, 12, 1), (96, 72, 1), (3, 192, 9)]
UNPACK_SCALES = (1.0, 0.5, 0.125, 1.0 / 3.0)


def _pack_sig(shapes, dt, pack="sep"):
    """rows (N, C, R, up, with w_dgrad); Cp / Np: the channel counts rounded up to the 16-byte vector of dt"""
    vec = 8 if dt == BF16 else 4
    geo = [(N, C, R | (0x100 if up else 0), _up(C, vec), _up(N, vec)) for N, C, R, up, _ in shapes]
    es = 2 if dt == BF16 else 4
    ptrs, nbytes, mod = [], [], 0
    for g, sh in zip(geo, shapes):                 # w packed as `pack`; the derived layouts each in a buffer of their own
        e = _pack_extents(*g, es)
        nbytes.append(e)
        ptrs.append((mod, sh[4]))
        mod = (mod + e[0] + 4) % 16 if pack == "g1" else 0
    rows = []
    for r, (g, (m, wd)) in enumerate(zip(geo, ptrs)):
        wcol = (False, m, 4 if pack == "g1" and r + 1 < len(geo) else SEPARATE)
        rows.append((g, (wcol, (False, 0, SEPARATE), (not wd, 0, SEPARATE))))
    return ("ddpm_pack_weight_multi", (("t", tuple(rows), ()), len(rows), dt))


# both packs of 3x3, 1x1 and 2x2 kernels; ragged 32-tiles (40 x 72); the edge convs' pads (C or N in {1, 3, 4, 12}); the Upsample convs'
# 4 x 4 effective dgrad kernel; rows without a dgrad pack
PACK_SHAPES = [(64, 64, 3, 0, 1), (40, 72, 3, 0, 1), (64, 3, 3, 0, 1), (64, 1, 3, 0, 0), (64, 12, 3, 0, 1), (1, 64, 3, 0, 1), (4, 64, 3, 0, 1),
               (12, 64, 3, 0, 1), (96, 72, 1, 0, 1), (128, 64, 1, 0, 0), (8, 16, 2, 0, 1), (64, 64, 3, 1, 1), (40, 72, 3, 1, 1)]


def _gather_sig(numels, pack="sep", mis=None):
    """rows {a, b (null on odd rows), dst, numel}: the destinations packed like the rows of the concatenated projection"""
    null = {(r, 1) for r in range(len(numels)) if r % 2}
    rows = [(n, (ca, cb, cd)) for (n, (ca, cb)), (_, (cd,)) in zip(_packed_cols(numels, 2, "sep", mis, null), _packed_cols(numels, 1, pack))]
    return ("ddpm_mt_gather_f32", (("t", tuple(rows), ()), len(rows)))


def _single_adam(n, k, mods=(0, 0, 0, 0, 0), shadow=True, total=True, max_norm=1.0, ema_w=1e-4):
    bc1, bc2 = bias_corrections(k)
    return ("ddpm_adam_ema_step", tuple(_p(m) for m in mods[:4]) + (_p(mods[4], null=not shadow), n, _p(null=not total), max_norm, 2e-4, BETA1, BETA2,
                                                                   ADAM_EPS, bc1, bc2, ema_w))


TAIL_ALIGNED = _mt_table(MIS_NUMELS, g="loguniform")
TAIL_MISALIGNED = [_mt_table(MIS_NUMELS, mis=(c, b), g="loguniform") for c in _MT_COLS for b in (4, 8, 12)]
_QUIET = dict(g="normal", gscale=1e-4)         # a norm of 3e-3, below max_norm = 1: the coefficient is exactly 1
TAIL = [
    # ---- the update: steps 1, 2, 1000 and 10^6; ema_w 0.9 and 1e-4; scalars by value and through hyper_dev; both draws of the gradient
    _adam_sig(_mt_table(SMALL_NUMELS, g="loguniform"), 1, ema_w=0.9),
    _adam_sig(_mt_table(SMALL_NUMELS, g="loguniform"), 1, ema_w=0.9, hyper=True),
    _adam_sig(_mt_table(SWEEP_NUMELS, "r4"), 2),
    _adam_sig(_mt_table(SWEEP_NUMELS, "g1", g="loguniform"), 1000, hyper=True),
    _adam_sig(_mt_table(SMALL_NUMELS, "r4", no_shadow=(1, 3, 4, 6), g="loguniform"), 10 ** 6, ema_w=0.9),
    _adam_sig(_mt_table(SMALL_NUMELS, "g1", no_shadow=range(8)), 2),
    _adam_sig(_mt_table(SMALL_NUMELS, **_QUIET), 1000),
    _adam_sig(_mt_table(SMALL_NUMELS, **_QUIET), 1000, max_norm=0.0),
    _adam_sig(_mt_table(SMALL_NUMELS, **_QUIET), 1000, total=False),
    _adam_sig(_mt_table((LARGEST, 64), "r4"), 1000),
    _adam_sig(TAIL_ALIGNED, 1, ema_w=0.9),
] + [_adam_sig(t, 1, ema_w=0.9) for t in TAIL_MISALIGNED] + [
    # ---- the norm
    _sumsq_sig(_mt_table(SMALL_NUMELS)),
    _sumsq_sig(_mt_table(SWEEP_NUMELS, "r4")),
    _sumsq_sig(_mt_table(SWEEP_NUMELS + SMALL_NUMELS, "g1", g="loguniform")),
    _sumsq_sig(_mt_table((LARGEST, 64), "r4")),
] + [_sumsq_sig(_mt_table(MIS_NUMELS, mis=("g", b))) for b in (4, 8, 12)] + [
    # ---- the single-tensor pair: past the caps of their grids (1024 and 4096 blocks of 256), odd lengths, misaligned, no EMA, no clip
    ("ddpm_sumsq_accumulate", (_p(), 1, _p(), _p())),
    ("ddpm_sumsq_accumulate", (_p(4), 1025, _p(8), _p())),
    ("ddpm_sumsq_accumulate", (_p(), 1024 * 256 + 1, _p(), _p())),
    _single_adam(5, 1, ema_w=0.9),
    _single_adam(1025, 2, mods=(4, 8, 12, 0, 4)),
    _single_adam(1025, 1000, shadow=False),
    _single_adam(1025, 1000, total=False),
    _single_adam(1025, 10 ** 6, max_norm=0.0),
    _single_adam(4096 * 256 + 1, 1000),
] + [_unpack_sig(_unpack_table(UNPACK_SHAPES), sc, f) for sc in UNPACK_SCALES for f in (False, True)] + [
    _pack_sig(PACK_SHAPES, BF16), _pack_sig(PACK_SHAPES, F32), _pack_sig(PACK_SHAPES, F32, "g1"), _pack_sig(PACK_SHAPES, BF16, "g1"),
    _gather_sig((64 * 128, 64, 5, 1, 1025, 32 * 256 * 4 + 1, 0, 3)),
    _gather_sig((64 * 128, 64, 5, 1, 1025, 32 * 256 * 4 + 1, 0, 3), "g1"),
    _gather_sig((1025, 1025, 5, 5), mis=(0, 4)),
    _gather_sig((1025, 1025, 5, 5), mis=(1, 8)),
]
# The exact coverage check of the reductions (_planted): not part of hostile_rows(), a profile would undo the draw.
TAIL_PLANTED = [_sumsq_sig(_mt_table(nm, pk, g="planted")) for nm, pk in ((SMALL_NUMELS, "sep"), (SWEEP_NUMELS, "r4"), (SWEEP_NUMELS, "g1"), ((LARGEST, 64), "r4"),
                                                                         ((5,), "sep"), ((16 * 256 * 4 + 1, 1025), "sep"))] + \
               [_sumsq_sig(_mt_table(MIS_NUMELS, mis=("g", b), g="planted")) for b in (4, 8, 12)] + \
               [_unpack_sig(_unpack_table(sh, g="planted"), sc, True) for sc in (0.5, 2.0) for sh in (UNPACK_SHAPES, UNPACK_SHAPES[2:4], UNPACK_SHAPES[4:9] + UNPACK_SHAPES[:1])]


def tail_identities():
    """[(what, signature a, signature b, columns)]: replays of a and b with the same seed must give the same bits in every row of the
    named columns.  The scalar path against the aligned run; hyper_dev against by-value scalars; a norm below max_norm (coefficient
    exactly 1) against no clipping at all; the fused unpack against the plain one."""
    out = [(f"{_MT_COLS[i // 3]} at {4 * (i % 3 + 1)} bytes modulo 16", _adam_sig(TAIL_ALIGNED, 1, ema_w=0.9), _adam_sig(t, 1, ema_w=0.9), ("p", "m", "v", "shadow"))
           for i, t in enumerate(TAIL_MISALIGNED)]
    out.append(("hyper_dev", TAIL[0], TAIL[1], ("p", "m", "v", "shadow")))
    out.append(("norm below max_norm / max_norm = 0", TAIL[6], TAIL[7], ("p", "m", "v", "shadow")))
    out.append(("norm below max_norm / total_sq null", TAIL[6], TAIL[8], ("p", "m", "v", "shadow")))
    for sc in UNPACK_SCALES:
        out.append((f"fused / plain unpack, scale {sc:g}", _unpack_sig(_unpack_table(UNPACK_SHAPES), sc, False), _unpack_sig(_unpack_table(UNPACK_SHAPES), sc, True), ("gflat",)))
    return out


def assert_same_tensors(a, b, cols, what):
    keys = [k for k in a.tensors if k[1] in cols]
    assert keys and set(keys) == {k for k in b.tensors if k[1] in cols}, what
    for k in keys:
        assert same_bits(a.tensors[k], b.tensors[k]), f"{what}: {k[1]}[{k[0]}] differs in " \
            f"{int((a.tensors[k].view(_INT[a.tensors[k].dtype]) != b.tensors[k].view(_INT[b.tensors[k].dtype])).sum())} of {a.tensors[k].numel()} element(s)"


# ----------------------------------------------------------------------------------------------------------------- value profiles
# A profile transforms the data operands after the draw (Arena.shape); the float64 references read the stored values, so they follow.
# Each transform takes (arena, fp32 values of a [rows][cols] view, geometry keywords) and returns the new values.
def _scale(f):
    return lambda A, v, **kw: v * f


def _sparse(A, v, **kw):
    """90 % exact zeros: four rows (pixels) in five are zero whole, half of the rest element by element — so that 1x1 convs and GEMMs
    have outputs whose every term is zero, which must come out exactly zero (TINY)."""
    rows = torch.rand(v.shape[0], generator=A.pgen, device=v.device) < 0.2
    keep = torch.rand(v.shape, generator=A.pgen, device=v.device) < 0.5
    return v * (keep & rows.reshape(-1, *([1] * (v.dim() - 1))))


def _groups(v, B, HW, C, G):
    return v.reshape(B, HW, G, C // G)


def _corner_outlier(sigmas):
    def f(A, v, B, HW, C, G, **kw):
        g = _groups(v.clone(), B, HW, C, G)
        g[:, 0, :, 0] = g.mean((1, 3)) + sigmas * g.std((1, 3), unbiased=False)
        return g.reshape(v.shape)
    return f


def _constant_group(A, v, B, HW, C, G, **kw):
    return _groups(v, B, HW, C, G)[:, :1, :, :1].expand(B, HW, G, C // G).reshape(v.shape)


def _flat_keys(A, v, B, L, C, **kw):
    t = v.reshape(B, L, 3 * C).clone()
    t[..., C:2 * C] = t[:, :1, C:2 * C]
    return t.reshape(v.shape)


def _q_times(f):
    def g(A, v, C, **kw):
        v = v.clone()
        v[:, :C] *= f
        return v
    return g


def _plant(value):
    """one non-finite value at a fixed in-range position of the view: row rows/2 + 1 (an interior pixel, a middle sample), column 3"""
    def f(A, v, **kw):
        v = v.clone()
        v[v.shape[0] // 2 + 1 if v.shape[0] > 2 else v.shape[0] - 1, min(3, v.shape[-1] - 1)] = value
        return v
    return f


_LINEAR = ("ddpm_conv2d_nhwc", "ddpm_gemm", "ddpm_atb_f32", "ddpm_conv3x3_wgrad_nhwc", "ddpm_conv3x3_wgrad_up_nhwc", "ddpm_conv1x1_wgrad_nhwc",
           "ddpm_conv2d_wgrad_nhwc", "ddpm_wgrad_reduce", "ddpm_colsum", "ddpm_upsample2x_bwd", "ddpm_add_rows", "ddpm_wgrad_unpack")
_GN = ("ddpm_groupnorm_silu_fwd", "ddpm_groupnorm_silu_bwd")
_SOFT = ("ddpm_softmax_fwd", "ddpm_softmax_bwd", "ddpm_attention_fwd", "ddpm_attention_fwd_lse", "ddpm_attention_bwd")
_NONFINITE = ("ddpm_conv2d_nhwc", "ddpm_gemm", "ddpm_groupnorm_silu_fwd", "ddpm_softmax_fwd", "ddpm_attention_fwd", "ddpm_attention_fwd_lse",
              "ddpm_mse_fwd", "ddpm_q_sample")
_NF_ROLES = ("data", "gn_x", "logits", "qkv", "elem", "grad")
# the optimizer tail: `grad` is the gradient operand of the norm and of the update (with a NaN gradient and clipping on, the norm and
# with it every p, m, v and shadow of every row is NaN, as clip_grad_norm_ + Adam make them); the unpack's gpack is `data`
_OPT = ("ddpm_mt_grad_sumsq", "ddpm_mt_adam_ema", "ddpm_sumsq_accumulate", "ddpm_adam_ema_step")
_UNPACK = ("ddpm_wgrad_unpack", "ddpm_wgrad_unpack_sumsq")
# name -> (what it is for, {role: transform}, the entries it applies to).  Roles: data / additive (the linear families: the operand
# the sum runs over, and bias, row bias, residual and prior content), gn_x / gn_dy / gn_gamma, logits (softmax), qkv, attn_do, silu_x,
# elem (q_sample's x0, mse's prediction).  Yardstick figures: the worst err/bar of the plain fp32 torch composition over every row
# the profile applies to (tests/test_hostile_inputs_host.py holds them to 0.5); intensities are final.
PROFILES = {
    # linear in the data: every output is exactly 2^+-30 times the plain run's (power-of-two scaling commutes with rounding away from
    # the denormal and overflow ranges).  GroupNorm: x * 2^-30 is the eps-dominated regime (var = 2^-60 << eps), x * 2^30 the opposite.
    "scaled_up": ("operands 2^30 larger than unity", {"data": _scale(2.0 ** 30), "additive": _scale(2.0 ** 30), "gn_x": _scale(2.0 ** 30),
                                                      "grad": _scale(2.0 ** 30)}, _LINEAR + _GN + _OPT + _UNPACK),
    "scaled_down": ("operands 2^-30 of unity; GroupNorm: eps dominates", {"data": _scale(2.0 ** -30), "additive": _scale(2.0 ** -30),
                                                                          "gn_x": _scale(2.0 ** -30), "grad": _scale(2.0 ** -30)},
                    _LINEAR + _GN + _OPT + _UNPACK),
    "sparse": ("90 % exact zeros: an element whose every term is zero must be exactly zero",
               {"data": _sparse, "gn_dy": _sparse, "attn_do": _sparse, "grad": _sparse},
               ("ddpm_conv2d_nhwc", "ddpm_gemm", "ddpm_conv3x3_wgrad_nhwc", "ddpm_conv3x3_wgrad_up_nhwc", "ddpm_conv1x1_wgrad_nhwc",
                "ddpm_conv2d_wgrad_nhwc", "ddpm_groupnorm_silu_bwd", "ddpm_attention_bwd") + _OPT + _UNPACK),
    # csrc/norm.hip accumulates moments about the group's first element: pixel 0 of the group's first channel at mean + 64 sigma
    "corner_outlier": ("the pivot of the GroupNorm statistics is an outlier", {"gn_x": _corner_outlier(64.0)}, _GN),
    "far_mean": ("GroupNorm input 50 +- 0.1: |mean| >> std", {"gn_x": lambda A, v, **kw: 50.0 + 0.1 * (v - 1.5)}, _GN),
    "constant_group": ("every GroupNorm group constant: variance 0, rstd = eps^-1/2", {"gn_x": _constant_group}, _GN),
    # gamma x 40 puts z = gamma xh + beta beyond +-120; x of the SiLU entries is drawn at std 4, x 10 gives std 40: exp overflows
    "saturating": ("SiLU arguments beyond +-88.7, where exp overflows", {"gn_gamma": lambda A, v, silu=1, **kw: v * 40.0 if silu else v,
                                                                       "silu_x": _scale(10.0)}, _GN + ("ddpm_silu_fwd", "ddpm_silu_bwd")),
    # softmax logits are drawn at std 3, attention logits at std 1.5^2 = 2.25
    "wide_logits": ("logit std 40: one-hot rows, large lse", {"logits": _scale(40.0 / 3.0), "qkv": _q_times(40.0 / 2.25)}, _SOFT),
    "flat_logits": ("all keys identical: uniform rows", {"logits": lambda A, v, **kw: v[:, :1].expand_as(v).clone(), "qkv": _flat_keys}, _SOFT),
    "offset_logits": ("a common +1e4 on softmax logits; q x 8 for attention", {"logits": lambda A, v, **kw: v + 1.0e4, "qkv": _q_times(8.0)}, _SOFT),
    "nonfinite_nan": ("one NaN in a data operand: exactly what the reference makes non-finite is non-finite",
                      {r: _plant(float("nan")) for r in _NF_ROLES}, _NONFINITE + _OPT + _UNPACK),
    "nonfinite_inf": ("one +inf in a data operand", {r: _plant(float("inf")) for r in _NF_ROLES}, _NONFINITE + _OPT + _UNPACK),
}
YARDSTICK = _GN + _SOFT + ("ddpm_silu_fwd", "ddpm_silu_bwd", "ddpm_mt_adam_ema", "ddpm_adam_ema_step")   # the non-linear families: Result.yard is filled
# what Result.outputs of a deterministic entry must satisfy bit for bit against the plain run of the same seed
EXACT_SCALE = {"scaled_up": 2.0 ** 30, "scaled_down": 2.0 ** -30}


HOSTILE_FAMILIES = {
    "conv": ("ddpm_conv2d_nhwc",),
    "wgrad": ("ddpm_conv3x3_wgrad_nhwc", "ddpm_conv3x3_wgrad_up_nhwc", "ddpm_conv2d_wgrad_nhwc", "ddpm_conv1x1_wgrad_nhwc", "ddpm_wgrad_reduce"),
    "gemm": ("ddpm_gemm", "ddpm_atb_f32"),
    "reduce": ("ddpm_colsum", "ddpm_upsample2x_bwd", "ddpm_add_rows"),
    "groupnorm_fwd": ("ddpm_groupnorm_silu_fwd",),
    "groupnorm_bwd": ("ddpm_groupnorm_silu_bwd",),
    "attention": ("ddpm_attention_fwd", "ddpm_attention_fwd_lse", "ddpm_attention_bwd"),
    "softmax": ("ddpm_softmax_fwd", "ddpm_softmax_bwd"),
    "silu": ("ddpm_silu_fwd", "ddpm_silu_bwd"),
    "diffusion": ("ddpm_q_sample", "ddpm_mse_fwd", "ddpm_mse_bwd", "ddpm_p_sample_step"),
    "misc": ("ddpm_timestep_embedding", "ddpm_gather_rows_f32", "ddpm_weighted_sum_f32"),
    "optimizer": _OPT,
    "layout": _UNPACK + ("ddpm_pack_weight_multi", "ddpm_mt_gather_f32"),
}


def hostile_cases():
    """[(family, mode)]: poison for every family, then each profile that names one of the family's entries."""
    return [(fam, mode) for fam, names in HOSTILE_FAMILIES.items()
            for mode in ["poison"] + [p for p, (_, _, entries) in PROFILES.items() if set(entries) & set(names)]]


def hostile_replay(sig, device, seed, mode, plain):
    """One replay of `sig` in `mode` ("poison" or a profile).  plain: a dict that caches the plain replays by seed.  Besides what
    replay() checks, every output of a deterministic entry must equal the plain run of the same seed bit for bit (poison), or be
    exactly 2^+-30 times it (scaled_up / scaled_down on the linear families); fp32-atomic targets are held to their bars alone."""
    if mode == "poison":
        r = replay(sig, device, seed, poison=True)
    else:
        r = replay(sig, device, seed, profile=mode, yardstick=sig[0] in YARDSTICK)
    if mode == "poison" or (mode in EXACT_SCALE and sig[0] in _LINEAR):
        if seed not in plain:
            plain[seed] = replay(sig, device, seed).outputs
        f = EXACT_SCALE.get(mode)
        assert set(r.outputs) == set(plain[seed])
        for name, (t, atomic) in r.outputs.items():
            if atomic:
                continue
            want = plain[seed][name][0]
            want = want if f is None else want * f
            assert same_bits(t, want), (f"{short(sig)}: {name} differs from the plain run" + ("" if f is None else f" times {f:g}")
                                        + f" in {int((t.view(_INT[t.dtype]) != want.view(_INT[t.dtype])).sum())} of {t.numel()} element(s)")
    return r


def hostile_rows():
    """Every hand-written signature: ODD_GEOMETRY, SYNTHETIC, EXTRA_SMALL, EDGE_CHANNELS and TAIL, with the index that seeds its replay."""
    sigs = [s for s, _ in ODD_GEOMETRY] + SYNTHETIC + EXTRA_SMALL + [s for s, _ in EDGE_CHANNELS] + TAIL      # (appended: the seeds of the rows before stay)
    return list(enumerate(sigs))


# Entries a step launches that are not replayed here, the existing test that covers each (tests/test_kernels_gpu.py) and what that test
# holds it to: [exact] a bit-exact copy or integer comparison.
COVERED_ELSEWHERE = {
    "ddpm_pack_weight": "test_timestep_embedding_and_layout_kernels [exact]",
    "ddpm_gather_i64": "test_diffusion_algebra_kernels [exact]",
    "ddpm_add_i64": "test_diffusion_algebra_kernels [exact]",
    "ddpm_stream_order": "not a kernel of arithmetic (stream ordering edge)",
    "ddpm_fill_zero": "not a kernel of arithmetic (stream-ordered memset)",
}


def sync():
    if torch.device(_DEVICE[0]).type == "cuda":
        torch.cuda.synchronize()


def replay(sig, device, seed=0, poison=False, profile=None, yardstick=False, amplify=None, keep_outputs=True):
    """Replay one signature on `device`; returns a Result (worst err/bar and where).  Without keywords: the draws and checks the
    recorded and odd-geometry tests have always had.  poison: everything the contract does not let the call read holds POISON bytes
    (Buf.poison).  profile: a key of PROFILES.  yardstick: the non-linear families also put a plain fp32 torch composition through cmp."""
    _DEVICE[0] = device
    name, words = sig
    res = Result(sig, nonfinite=bool(profile) and profile.startswith("nonfinite"))
    A = Arena(device, seed, poison=poison, profile=profile, yardstick=yardstick)
    if amplify is not None:             # (power of two, rows of one image): the reduction replays scale three images (amplify_images)
        A.amplify, A.rows_per_image = amplify
    REPLAY[name](A, words, res)
    res.max_bytes = max((b.nbytes for b in A.bufs), default=0)
    for b in A.bufs:
        if not keep_outputs:            # the 2 GiB rows: no second copy of every output
            break
        if bool(b.written.any()) and not b.scratch:
            res.outputs[b.name] = (b.t[b.written if b.result is None else b.result].clone(), b.atomic)
    return res


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(_INT[a.dtype]), b.view(_INT[b.dtype]))


def geometry(sig, offsets=True):
    """The signature without its dropout seed (every dropout layer draws its own seed; the replay draws masks from the recorded one), and
    with offsets=False also without the pointer offsets, those inside a table word included (the host check replays each geometry
    once; the packings are on the host through the hand-written tables)."""
    name, words = sig
    types = _hip.PROTOTYPES[name]
    return (name, tuple(0 if t is ctypes.c_ulonglong else (w if offsets else _unplaced(name, w)) if is_table(w) else
                        (w[0], w[1], w[2] if offsets else 0) if isinstance(w, tuple) else w for w, t in zip(words, types)))


def _unplaced(name, table):
    """the table word without its pointer offsets: every tensor 16-byte aligned in a buffer of its own (descriptor tables hold none)"""
    if name in ("ddpm_wgrad_unpack", "ddpm_wgrad_unpack_sumsq"):
        return table
    return ("t", tuple((head, tuple((null, 0, SEPARATE) for null, _, _ in cols)) for head, cols in table[1]), table[2])


def short(sig):
    name, words = sig

    def word(w):
        if is_table(w):                    # rows and a checksum of the normalised table (and the options of a hand-written row)
            import zlib
            return f"T{len(w[1])}#{zlib.crc32(repr(w[1:]).encode()) & 0xffff:04x}" + "".join(f";{k}={v}" for k, v in w[2] if k != "step")
        return ("-" if w[1] else f"@{w[2]}") if isinstance(w, tuple) else (f"{w:g}" if isinstance(w, float) else str(w))
    return f"{name[5:]}({','.join(word(w) for w in words)})"


# ----------------------------------------------------------------------------------------------------------------- workloads
def _config(name):
    import json
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ddpm-torch_amd", "configs", name)
    with open(path) as f:
        return json.load(f)


def _net(cfg, device, seed=0, dtype=torch.bfloat16):
    import ddpm_torch
    torch.manual_seed(seed)
    kw = {k: v for k, v in cfg["model"].items() if k != "block_size"}
    kw.setdefault("out_channels", kw["in_channels"])
    return ddpm_torch.UNet(**kw).to(device).set_compute_dtype(dtype)


def _diffusion(cfg):
    import ddpm_torch
    d = cfg["diffusion"]
    return ddpm_torch.GaussianDiffusion(ddpm_torch.get_beta_schedule(d["beta_schedule"], d["beta_start"], d["beta_end"], d["timesteps"]),
                                        d["model_mean_type"], d["model_var_type"], d["loss_type"])


def _hw(size):
    """size: the side of a square image, or an (H, W) pair"""
    return (size, size) if isinstance(size, int) else tuple(size)


def _train_step(cfg, device, B, size, drop=None, dtype=torch.bfloat16):
    import ddpm_torch
    H, W = _hw(size)
    if drop is not None:
        cfg = dict(cfg, model=dict(cfg["model"], drop_rate=drop))
    m = _net(cfg, device, dtype=dtype)
    tc = cfg["train"]
    opt = torch.optim.Adam(m.parameters(), lr=tc["lr"], betas=(0.9, 0.999))
    tr = ddpm_torch.Trainer(m, opt, _diffusion(cfg), epochs=1, trainloader=None, use_ema=tc["use_ema"], grad_norm=tc["grad_norm"],
                            shape=(m.in_channels, H, W), device=torch.device(device), ema_decay=tc["ema_decay"])
    m.train()
    x = torch.rand(B, m.in_channels, H, W, generator=torch.Generator().manual_seed(1)) * 2 - 1
    def run():
        tr.step(x.to(device), global_steps=1)
    run.owners = (tr, m)
    return run


def _sample_step(cfg, device, B, size, ddim_steps=None, dtype=torch.bfloat16):
    H, W = _hw(size)
    m = _net(cfg, device, dtype=dtype).eval()
    dif = _diffusion(cfg)
    if ddim_steps:
        import ddim
        d = cfg["diffusion"]
        dif = ddim.DDIM(dif.betas if torch.is_tensor(dif.betas) else torch.as_tensor(dif.betas), d["model_mean_type"], "fixed-small",
                        d["loss_type"], eta=0.0, subsequence=ddim.get_selection_schedule("linear", ddim_steps, d["timesteps"]))
    g = torch.Generator().manual_seed(2)
    x = torch.randn(B, m.in_channels, H, W, generator=g).to(device)
    t = torch.full((B,), 500, dtype=torch.int64, device=device)
    if ddim_steps:
        t = torch.full((B,), ddim_steps // 2, dtype=torch.int64, device=device)

    def run():
        with torch.no_grad():
            dif.p_sample_step(m, x, t)
    run.owners = (None, m)
    return run


def _reduced(mult=(1, 2, 2), drop=0.0, ch=None):
    """cifar10.json with a reduced network (hid 64, one res block per level, attention at level 1 and in the middle block): the
    non-square workloads W14-W17 keep the levels, the kernels and the dispatch of a real configuration at a few seconds a test.
    ch = (in, out): the edge channel counts of W18-W24 instead of the configuration's 3 -> 3."""
    cfg = _config("cifar10.json")
    edge = {} if ch is None else dict(in_channels=ch[0], out_channels=ch[1])
    return dict(cfg, model=dict(cfg["model"], hid_channels=64, ch_multipliers=list(mult), num_res_blocks=1,
                                apply_attn=[i == 1 for i in range(len(mult))], drop_rate=drop, **edge))


# key -> (what it runs, builder(device, B, size), B, size); full size: the geometry the benchmark, the configs and the CLIs run; size is
# the side of a square image or an (H, W) pair
_F32 = torch.float32
WORKLOADS = {
    "W1": ("cifar10 train step, B=128, dropout 0.1", lambda dev, B=128, s=32: _train_step(_config("cifar10.json"), dev, B, s, drop=0.1), 128, 32),
    "W2": ("cifar10 ancestral sampling step, B=128", lambda dev, B=128, s=32: _sample_step(_config("cifar10.json"), dev, B, s), 128, 32),
    "W3": ("celebahq 256x256 train step, B=2", lambda dev, B=2, s=256: _train_step(_config("celebahq.json"), dev, B, s), 2, 256),
    "W4": ("celeba 64x64 DDIM step, B=128", lambda dev, B=128, s=64: _sample_step(_config("celeba.json"), dev, B, s, ddim_steps=50), 128, 64),
    # the fp32 compute mode (bench.py --full's fp32 leg, the parity configurations): its convs, weight gradients, GroupNorm backward
    # instantiations and the gemm + softmax + gemm attention are kernels the bf16 mode never reaches
    "W5": ("cifar10 train step, fp32, B=128, dropout 0.1",
           lambda dev, B=128, s=32: _train_step(_config("cifar10.json"), dev, B, s, drop=0.1, dtype=_F32), 128, 32),
    "W6": ("cifar10 ancestral sampling step, fp32, B=128", lambda dev, B=128, s=32: _sample_step(_config("cifar10.json"), dev, B, s, dtype=_F32), 128, 32),
    "W7": ("celebahq 256x256 train step, fp32, B=2", lambda dev, B=2, s=256: _train_step(_config("celebahq.json"), dev, B, s, dtype=_F32), 2, 256),
    "W8": ("celeba 64x64 DDIM step, fp32, B=128",
           lambda dev, B=128, s=64: _sample_step(_config("celeba.json"), dev, B, s, ddim_steps=50, dtype=_F32), 128, 64),
    # batch sizes the CLIs run besides the benchmark's: dispatch depends on the pixel count
    "W9": ("cifar10 train step, B=32 (train.py --num-accum 4), dropout 0.1",
           lambda dev, B=32, s=32: _train_step(_config("cifar10.json"), dev, B, s, drop=0.1), 32, 32),
    "W10": ("cifar10 sampling step, B=106 (generate.py's ragged last chain)", lambda dev, B=106, s=32: _sample_step(_config("cifar10.json"), dev, B, s), 106, 32),
    "W11": ("cifar10 sampling step, B=1", lambda dev, B=1, s=32: _sample_step(_config("cifar10.json"), dev, B, s), 1, 32),
    "W12": ("celeba 64x64 train step, B=128 (config 4)", lambda dev, B=128, s=64: _train_step(_config("celeba.json"), dev, B, s), 128, 64),
    "W13": ("cifar10 sampling step, B=2048 (operands >= 1 GiB)", lambda dev, B=2048, s=32: _sample_step(_config("cifar10.json"), dev, B, s), 2048, 32),
    # non-square images on the reduced network: 16 x 48 -> 8 x 24 (192 tokens) -> 4 x 12 (48 tokens in the middle block); 1 x 3 / 3 x 1
    # patches at level 0, 8 x 8 patches at level 1, the generic kernels below
    "W14": ("reduced net train step, B=22, 16x48, dropout 0.1", lambda dev, B=22, s=(16, 48): _train_step(_reduced(drop=0.1), dev, B, s), 22, (16, 48)),
    "W15": ("reduced net train step, fp32, B=22, 16x48, dropout 0.1",
            lambda dev, B=22, s=(16, 48): _train_step(_reduced(drop=0.1), dev, B, s, dtype=_F32), 22, (16, 48)),
    "W16": ("reduced net ancestral sampling step, B=22, 48x16", lambda dev, B=22, s=(48, 16): _sample_step(_reduced(), dev, B, s), 22, (48, 16)),
    # every level off the 8-pixel grid; 12 x 10 = 120 tokens, a multiple of 8 but not of 16: the bf16 gemm + softmax + gemm attention
    "W17": ("reduced net [1, 2] train step, B=2, 24x20, dropout 0.1",
            lambda dev, B=2, s=(24, 20): _train_step(_reduced(mult=(1, 2), drop=0.1), dev, B, s), 2, (24, 20)),
}
# edge channel counts other than 3 (EDGE_CHANNEL_WORKLOADS), on the reduced [1, 2] network at the smallest images that still reach the
# edge convs (H, W multiples of 16, >= 16384 pixels): 1 -> 1 is `--dataset mnist` (B = 16 at 32 x 32), 4 -> 4 and 12 -> 12 are what
# `train.py --block-size 2` makes of MNIST and of the RGB data sets (B = 64 at 16 x 16); each in bf16 and fp32, then one sampling step
for _i, (_ch, _B, _s, _dt) in enumerate([((1, 1), 16, 32, torch.bfloat16), ((1, 1), 16, 32, _F32), ((4, 4), 64, 16, torch.bfloat16),
                                         ((4, 4), 64, 16, _F32), ((12, 12), 64, 16, torch.bfloat16), ((12, 12), 64, 16, _F32)]):
    WORKLOADS[f"W{18 + _i}"] = (
        f"reduced net [1, 2] {_ch[0]} -> {_ch[1]} channels train step, {'bf16' if _dt == torch.bfloat16 else 'fp32'}, B={_B}, {_s}x{_s}, dropout 0.1",
        lambda dev, B=_B, s=_s, ch=_ch, dt=_dt: _train_step(_reduced(mult=(1, 2), drop=0.1, ch=ch), dev, B, s, dtype=dt), _B, _s)
WORKLOADS["W24"] = ("reduced net [1, 2] 12 -> 12 channels ancestral sampling step, B=64, 16x16",
                    lambda dev, B=64, s=16: _sample_step(_reduced(mult=(1, 2), ch=(12, 12)), dev, B, s), 64, 16)
EDGE_CHANNEL_WORKLOADS = tuple(f"W{i}" for i in range(18, 25))


def record(monkeypatch, key, device, B=None, size=None):
    """Run workload `key` once with every _invoke recorded; returns the Recorder."""
    _, build, B0, S0 = WORKLOADS[key]
    run = build(device, B or B0, size or S0)
    rec = Recorder(_hip._invoke)
    monkeypatch.setattr(_hip, "_invoke", rec)
    try:
        run()
        sync_dev(device)
    finally:
        monkeypatch.setattr(_hip, "_invoke", rec.inner)
    resolve_tables(rec, *run.owners)
    return rec


def resolve_tables(rec, trainer, unet):
    """After the workload has ended and the device is synchronised: every table-driven signature gets, in place of its table pointer,
    the normalised form (normalise_table) of the persistent table that lives at the recorded address — the trainer's fused-update
    table, the engine's wdesc, pack_table or fc_table.  An address that is none of them fails."""
    owned = {}
    fused = getattr(trainer, "_fused", None)
    eng = getattr(unet, "_eng", None)
    for owner, attr in ((fused, "table"), (eng, "wdesc"), (eng, "pack_table"), (eng, "fc_table")):
        t = getattr(owner, attr, None)
        if t is not None:
            owned[t.data_ptr()] = (attr, t)
    sigs = {}
    for sig in rec.sigs:
        name, words = sig
        if name in TABLE_ARG:
            ti, ni, width = TABLE_ARG[name]
            addr, n = rec.tables[sig], words[ni]
            assert addr in owned, f"{name}: the table at the recorded address is none of {[a for a, _ in owned.values()]}"
            attr, t = owned[addr]
            assert t.dim() == 2 and t.shape[1] == width and t.shape[0] >= n, f"{name}: {attr} is {tuple(t.shape)}, the launch read {n} rows of {width}"
            rows = t[:n].cpu().tolist()
            tw = normalise_table(name, rows, words[2] if name == "ddpm_pack_weight_multi" else None)
            sig = (name, words[:ti] + (tw,) + words[ti + 1:])
        sigs.setdefault(sig, None)
    rec.sigs = sigs


def _unpack_depth(rows):
    """chain length of ddpm_wgrad_unpack_sumsq's bound over a descriptor table (rep_wgrad_unpack_sumsq)"""
    its = 0
    for _, _, N, C, RS in rows:
        if N * C * RS:
            its = max(its, 1 + 9 * -(-(N * (C // 64)) // 256) if RS == 9 and C % 64 == 0 else 1 + -(-(N * C * RS) // (64 * 256)))
    return _sumsq_depth(its, 64 * len(rows))


def chained_tail(device, dtype, steps=3, seed=0):
    """Three optimizer steps of the tail on the tables Trainer and UNet build for the reduced network (_reduced: hid 64, multipliers
    (1, 2, 2), attention on), issued as Trainer.step issues them — ddpm_wgrad_unpack_sumsq over the engine's wdesc into the flat
    gradient, ddpm_mt_adam_ema over the trainer's table with the scalars in hyper_dev (warm-up LR, clip 1.0, EMA on), ddpm_pack_weight_multi
    over pack_table, ddpm_mt_gather_f32 over fc_table — on a drawn gpack.  After every step, against float64 (each step's reference starts
    from the state the kernels left): the flat gradient bit for bit, the norm within its bound, p / m / v / shadow within their bars
    (_adam_check), both packs of every conv equal to the pack of the fp32 parameters the update left — bit for bit, the 4 x 4 kernels of
    the Upsample convs within their rounding bar — and the time-bias projection.  Returns [(step, Result)]."""
    import ddpm_torch
    _DEVICE[0] = device
    cfg = _reduced()
    m = _net(cfg, device, seed=seed, dtype=dtype).train()
    tc = cfg["train"]
    opt = torch.optim.Adam(m.parameters(), lr=tc["lr"], betas=(BETA1, BETA2))
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lr_lambda=lambda t: min((t + 1) / 5000, 1.0))
    tr = ddpm_torch.Trainer(m, opt, _diffusion(cfg), epochs=1, trainloader=None, scheduler=sched, use_ema=True, grad_norm=1.0,
                            shape=(m.in_channels, 16, 16), device=torch.device(device), ema_decay=tc["ema_decay"])
    eng, fused = m.engine(), tr._fused
    wdesc = eng._wgrad_table()
    rows = [tuple(r) for r in wdesc.cpu().tolist()]
    gen = torch.Generator(device=device).manual_seed(seed + 1)
    gpack = torch.empty(eng.ptotal, dtype=torch.float32, device=device)
    gflat = torch.full((eng.gtotal,), float("nan"), dtype=torch.float32, device=device)
    order = tr._fused_param_order()
    fused.prepare(grad_ptrs=[gflat.data_ptr() + 4 * eng.goff[id(p)] for p in order], stable_grads=True)
    table = fused.table.cpu().tolist()
    assert [r[5] for r in table] == [p.numel() for p in order]
    hyper_dev = torch.zeros(4, dtype=torch.int64, device=device)
    shadow_of = {id(prm): sh for sh, prm in tr.ema._pairs()}
    eng._refresh_packs(True)
    eng._fc_all()
    out = []
    for step in range(1, steps + 1):
        res = Result(("chained_tail", (step,)))
        A = Arena(device, seed + step)
        # gradients of very different sizes from tensor to tensor, as a network has them
        gpack.copy_(torch.randn(eng.ptotal, generator=gen, device=device) * 10.0 ** (-3.0 * torch.rand(eng.ptotal, generator=gen, device=device)))
        scal = fused.scalars(tr.ema.weight_of_next_update())
        hyper_dev.view(torch.float32)[:4] = torch.tensor(scal, dtype=torch.float64).to(torch.float32).to(device)
        lr, bc1, bc2, w = (float(x) for x in hyper_dev.view(torch.float32)[:4])
        state = [(p.data, opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"], shadow_of.get(id(p))) for p in order]
        state = [tuple(None if t is None else t.reshape(-1) for t in st) for st in state]
        before = [(p.clone(), None, a.clone(), b.clone(), None if sh is None else sh.clone()) for p, a, b, sh in state]
        _hip.call("ddpm_wgrad_unpack_sumsq", gpack.data_ptr(), gflat.data_ptr(), wdesc.data_ptr(), wdesc.shape[0], 1.0, fused.total.data_ptr(),
                  _hip.SUMSQ_FLOATS, _hip.stream() if torch.device(device).type == "cuda" else 0)
        fused.launch(tr.grad_norm, hyper_dev=hyper_dev.data_ptr(), have_sumsq=True)
        fused.committed()
        tr.ema.num_updates += 1
        sched.step()
        eng._launch_pack()
        eng._launch_fc()
        sync()
        # ---- the flat gradient and its norm
        S = torch.zeros((), dtype=torch.float64, device=device)
        for r, (src, dst, N, C, RS) in enumerate(rows):
            c = N * C * RS
            ref = _d(gpack[src:src + c]).reshape(N, RS, C).transpose(1, 2).reshape(-1)
            res.cmp(f"gflat[{r}]", gflat[dst:dst + c], ref, torch.zeros(c, dtype=torch.float64, device=device))
            S = S + (ref * ref).sum()
        d = _unpack_depth(rows)
        _check_bank(res, "total_sq", fused.total[:64], S, d * U_F32 * S + eng.ptotal * DENORM)
        # ---- the update
        before = [(b[0], gflat[eng.goff[id(p)]:eng.goff[id(p)] + p.numel()].clone(), b[2], b[3], b[4]) for b, p in zip(before, order)]
        _adam_check(A, res, before, state, fused.total[:64].clone(), tr.grad_norm, lr, bc1, bc2, opt.param_groups[0]["eps"], w)
        # ---- the derived copies: the pack of the fp32 parameters the update left
        T = _TD[eng.dcode]
        u = U_BF16 if eng.dcode == BF16 else U_F32
        for i, cw in enumerate(eng.convs.values()):
            W = _d(cw.mod.weight.data)
            N, C, R = cw.N, cw.C, cw.R
            ref = W.new_zeros(N, R, R, cw.Cp)
            ref[..., :C] = W.permute(0, 2, 3, 1)
            res.cmp(f"w_fwd[{i}]", cw.wf, _d(ref.reshape(-1).to(T)), torch.zeros(cw.wf.numel(), dtype=torch.float64, device=device))
            D = W.flip(2, 3)
            if cw.up:
                E, mag = W.new_zeros(N, C, 4, 4), W.new_zeros(N, C, 4, 4)
                for a in range(2):
                    for b in range(2):
                        E[:, :, a:a + 3, b:b + 3] += D
                        mag[:, :, a:a + 3, b:b + 3] += D.abs()
                ref, bar = W.new_zeros(C, 4, 4, cw.Np), W.new_zeros(C, 4, 4, cw.Np)
                ref[..., :N], bar[..., :N] = E.permute(1, 2, 3, 0), C_GEMM * (U_F32 * mag + u * E.abs()).permute(1, 2, 3, 0)
                res.cmp(f"w_dgrad4x4[{i}]", cw.wd, ref.reshape(-1), bar.reshape(-1))
            else:
                ref = W.new_zeros(C, R, R, cw.Np)
                ref[..., :N] = D.permute(1, 2, 3, 0)
                res.cmp(f"w_dgrad[{i}]", cw.wd, _d(ref.reshape(-1).to(T)), torch.zeros(cw.wd.numel(), dtype=torch.float64, device=device))
        # ---- the concatenated time-bias projection
        for rb in eng.res_blocks:
            o, c = eng.tb_off[id(rb)], rb.out_channels
            res.cmp("fc_w", eng.fc_w[o:o + c].reshape(-1), _d(rb.fc.weight.data).reshape(-1), torch.zeros(c * eng.E, dtype=torch.float64, device=device))
            ref = (_d(rb.fc.bias.data) + _d(rb.conv1.bias.data)).to(torch.float32)
            res.cmp("fc_b", eng.fc_b[o:o + c], _d(ref), torch.zeros(c, dtype=torch.float64, device=device))
        out.append((step, res))
    return out


def sync_dev(device):
    if torch.device(device).type == "cuda":
        torch.cuda.synchronize()


def variant_of(sig):
    """Kernel the dispatch queries of include/ddpm_hip_debug.h name for a conv / wgrad / GEMM signature (None for other entries)."""
    lib = _hip.lib()
    name, w = sig
    if name == "ddpm_conv2d_nhwc":
        (_, x_ld, _, _, y_ld, pb, prb, _, pres, _, B, H, W, C, Ho, Wo, N, R, S, stride, pt, pl, ups, dil, acc, mode, splits, _, _, dt) = w
        epi = int(_opt(pres)) | (2 if acc else 0)            # bit 0: residual operand, bit 1: accumulate (gemm.hip, ddpm_conv2d_variant)
        # the query stands 16-byte aligned pointers in for the operands and y_ld for the residual pitch: it names the kernel that ran
        # only when the recorded call meets the same alignment conditions, so hold the recorded call to them
        assert all(p[2] % 16 == 0 for p in w if isinstance(p, tuple) and not p[1]), f"unaligned operand in {short(sig)}"
        assert not _opt(pres) or (w[9] % 8 == 0 and y_ld % 8 == 0), f"residual pitch the query cannot stand in for: {short(sig)}"
        return int(lib.ddpm_conv2d_variant(x_ld, y_ld, B, H, W, C, Ho, Wo, N, R, S, stride, pt, pl, ups, dil, mode, splits, dt, epi))
    if name == "ddpm_conv2d_wgrad_nhwc":
        (_, dy_ld, _, x_ld, _, _, B, H, W, C, Creal, Ho, Wo, N, Nreal, R, S, stride, pt, pl, ups, splits, dt) = w
        return int(lib.ddpm_conv2d_wgrad_variant(dy_ld, x_ld, B, H, W, C, Creal, Ho, Wo, N, Nreal, R, S, stride, pt, pl, ups, splits, dt))
    if name in ("ddpm_conv3x3_wgrad_nhwc", "ddpm_conv3x3_wgrad_up_nhwc"):
        B, H, W, C, N = w[8:13]
        return int(lib.ddpm_conv3x3_wgrad_variant(B, H, W, C, N))
    if name == "ddpm_conv1x1_wgrad_nhwc":
        return 9
    if name == "ddpm_gemm":
        (_, a_ld, _, a_tr, _, b_ld, _, b_tr, _, c_ld, _, _, _, _, _, M, N, K, batch, _, _, mode, splits, dt) = w
        return int(lib.ddpm_gemm_variant(a_ld, a_tr, b_ld, b_tr, c_ld, M, N, K, batch, mode, splits, dt))
    return None


# Kernel ids (variant_of) the dispatch reaches only with bf16 operands.  csrc/gemm.hip ddpm_conv2d_nhwc puts the edge convs (11, 12), the
# persistent 3x3 stream / wave-specialised kernels (8, 10, 13), the halo kernel (5) and the streaming 1x1 kernel (7) behind
# `dtype == DDPM_BF16`; csrc/wgrad.hip (6, 14) and csrc/wgrad1x1.hip (9) return DDPM_ERR_DTYPE for anything else.  What stays for fp32
# is the templated gemm_kernel (1, 2, 3) and gemm64_kernel (4).
BF16_ONLY = {5, 6, 7, 8, 9, 10, 11, 12, 13, 14}


def dtype_index(name):
    """Position of the `dtype` parameter in the declaration of `name` (include/ddpm_hip.h), None if it has none."""
    import os
    import re
    if not _DTYPE_INDEX:
        inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
        src = "".join(open(os.path.join(inc, f)).read() for f in ("ddpm_hip.h", "ddpm_hip_debug.h"))
        src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
        for m in re.finditer(r"\b(?:int|long long)\s+(ddpm_\w+)\s*\(([^;{]*?)\)\s*;", src, re.S):
            names = [re.findall(r"(\w+)\s*$", a.strip()) for a in m.group(2).split(",")]
            names = [n[0] if n else "" for n in names]
            _DTYPE_INDEX[m.group(1)] = names.index("dtype") if "dtype" in names else None
    return _DTYPE_INDEX[name]


_DTYPE_INDEX = {}
