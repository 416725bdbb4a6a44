"""Fork / join edges of a launch plan (csrc/plan.hip): inside ``ddpm_plan_run`` a ``ddpm_stream_order`` entry is bound to the kernel
that produces what it orders (the kernel's own completion event), falls back to a recorded event where no such kernel exists in the
segment, and is dropped where an earlier edge already orders the same work.  The guarantee must not move: every case below is a
chain whose consumer would read its NaN pre-fill if it were released before the producer has finished.

Producers run over 2^26 floats (>= 100 us), consumers over 2^20; every intermediate and output buffer is NaN before a run; each plan
runs three times back to back with no host synchronisation in between (the events come from a ring and are reused); results are
compared bit for bit with the same chain issued on ONE stream.  Values only: nothing here depends on a fault, a hang or a timeout.
"""
import ctypes
import struct

import pytest
import torch

from ddpm_torch import _hip

pytestmark = pytest.mark.gpu

N_BIG = 1 << 26
N_SMALL = 1 << 20
RUNS = 3
NAN = float("nan")


def _words(name, args):
    out = []
    for ty, v in zip(_hip.PROTOTYPES[name], args):
        if ty is _hip.F:
            out.append(struct.unpack("<I", struct.pack("<f", float(v)))[0])
        elif ty is _hip.I:
            out.append(int(v) & 0xFFFFFFFF)
        else:
            out.append(int(v) & ((1 << 64) - 1))
    return out


class Plan:
    """ddpm_plan_create / _append / _cut / _run through ctypes, out of existing entries only."""

    def __init__(self, calls):
        self.lib = _hip.lib()
        self.h = ctypes.c_void_p(self.lib.ddpm_plan_create())
        self.segments = 1
        for c in calls:
            if c == "cut":
                assert self.lib.ddpm_plan_cut(self.h) >= 0
                self.segments += 1
                continue
            name, *args = c
            w = _words(name, args)
            arr = (ctypes.c_ulonglong * len(w))(*w)
            assert self.lib.ddpm_plan_append(self.h, name.encode(), ctypes.cast(arr, ctypes.c_void_p), len(w)) >= 0, name

    def run(self):
        for s in range(self.segments):
            assert self.lib.ddpm_plan_run(self.h, s) == 0, s

    def close(self):
        self.lib.ddpm_plan_destroy(self.h)


def _eager(calls):
    for c in calls:
        if c != "cut":
            _hip.call(c[0], *c[1:])


def _bits(t):
    return t.contiguous().view(torch.int32)


class Bench:
    """Buffers shared by every case (allocated once) and the single-stream results they are compared with."""

    def __init__(self):
        dev = torch.device("cuda")
        g = torch.Generator(device=dev).manual_seed(20)
        self.x = torch.randn(N_BIG, device=dev, generator=g)
        self.y = torch.empty(N_BIG, device=dev)                 # producer's output
        self.z = torch.empty(N_SMALL, device=dev)               # first consumer's output
        self.w = torch.empty(N_SMALL, device=dev)               # second consumer's output
        # ddpm_mt_grad_sumsq over two small tensors: rows of {p, g, m, v, shadow, n}; only g and n are read
        self.g1 = torch.randn((1 << 20) + 3, device=dev, generator=g)
        self.g2 = torch.randn(1 << 18, device=dev, generator=g)
        self.table = torch.tensor([[0, t.data_ptr(), 0, 0, 0, t.numel()] for t in (self.g1, self.g2)], dtype=torch.int64, device=dev)
        self.total = torch.empty(_hip.lib().ddpm_mt_sumsq_slots(2), device=dev)
        self.zero_idx = torch.zeros(1, dtype=torch.int64, device=dev)
        self.out4 = torch.empty(4, device=dev)
        self.a, self.b = torch.cuda.Stream(), torch.cuda.Stream()
        self.intermediates = (self.y, self.z, self.w, self.total, self.out4)
        torch.cuda.synchronize()
        # the reference: each chain on one stream, computed once
        s = self.a.cuda_stream
        self.ref = {}
        for key in ("fork", "join", "memset", "sumsq"):
            self.poison(self.a)
            _eager(self.chain(key, s, s))
            self.a.synchronize()
            self.ref[key] = self.result(key).clone()
        assert not torch.isnan(self.ref["fork"]).any() and not torch.isnan(self.ref["join"]).any()
        assert int(self.ref["memset"].count_nonzero()) == 0
        want = float((self.g1.double() ** 2).sum() + (self.g2.double() ** 2).sum())
        assert abs(float(self.ref["sumsq"][0]) - want) <= 1e-4 * want and self.ref["sumsq"][1:].tolist() == [0.0, 0.0, 0.0]
        torch.cuda.synchronize()

    def poison(self, stream):
        with torch.cuda.stream(stream):
            for t in self.intermediates:
                t.fill_(NAN)

    def chain(self, key, a, b, edges=1):
        """The calls of one case with its producer stream ``a`` and consumer stream ``b`` (raw hipStream_t handles)."""
        x, y, z, w = self.x.data_ptr(), self.y.data_ptr(), self.z.data_ptr(), self.w.data_ptr()
        fork = [("ddpm_stream_order", b, a)] * edges
        if key == "fork":
            return [("ddpm_silu_fwd", x, y, N_BIG, a), *fork, ("ddpm_silu_fwd", y, z, N_SMALL, b)]
        if key == "join":
            return [*self.chain("fork", a, b), ("ddpm_stream_order", a, b), ("ddpm_silu_fwd", z, w, N_SMALL, a)]
        if key == "cut":
            return [("ddpm_silu_fwd", x, y, N_BIG, a), "cut", *fork, ("ddpm_silu_fwd", y, z, N_SMALL, b)]
        if key == "memset":
            return [("ddpm_fill_zero", y, N_BIG * 4, a), *fork, ("ddpm_silu_fwd", y, z, N_SMALL, b)]
        if key == "sumsq":
            return [("ddpm_mt_grad_sumsq", self.table.data_ptr(), 2, self.total.data_ptr(), self.total.numel(), a), *fork,
                    ("ddpm_gather_rows_f32", self.total.data_ptr(), self.zero_idx.data_ptr(), self.out4.data_ptr(), 1, 4, 1, b)]
        raise KeyError(key)

    def result(self, key):
        return {"fork": self.z, "cut": self.z, "memset": self.z, "join": self.w, "sumsq": self.out4}[key]

    def check(self, key, issue, ref=None, last="b"):
        """``issue()`` enqueues the case; RUNS times back to back, the result of each run copied out on the stream that produced it."""
        a, b = self.a, self.b
        last = a if last == "a" else b
        got = []
        for _ in range(RUNS):
            # stream-ordered re-poisoning, no host sync: the fill follows everything of the previous run, and both streams follow the fill
            a.wait_stream(b)
            self.poison(a)
            b.wait_stream(a)
            issue()
            with torch.cuda.stream(last):
                got.append(self.result(key).clone())
        torch.cuda.synchronize()
        want = self.ref[ref or key]
        for i, r in enumerate(got):
            assert not torch.isnan(r).any(), f"{key}: run {i} read the NaN pre-fill ({int(torch.isnan(r).sum())} values)"
            assert torch.equal(_bits(r), _bits(want)), f"{key}: run {i} differs from the single-stream chain"


@pytest.fixture(scope="module")
def bench():
    b = Bench()
    yield b
    torch.cuda.synchronize()


def _plan_case(bench, key, ref=None, last="b", edges=1):
    plan = Plan(bench.chain(key, bench.a.cuda_stream, bench.b.cuda_stream, edges))
    try:
        bench.check(key, plan.run, ref=ref, last=last)
    finally:
        torch.cuda.synchronize()
        plan.close()


def test_fork_waits_for_the_producing_kernel(bench):
    _plan_case(bench, "fork")


def test_join_after_a_fork(bench):
    _plan_case(bench, "join", last="a")


def test_second_of_two_forks_in_a_row_is_covered_by_the_first(bench):
    _plan_case(bench, "fork", edges=2)


def test_fork_behind_a_memset_records_an_event(bench):
    _plan_case(bench, "memset")
    assert int(bench.ref["memset"].count_nonzero()) == 0          # zeros, not the pre-fill


def test_edge_in_the_segment_after_its_producer(bench):
    _plan_case(bench, "cut", ref="fork")


def test_edge_follows_the_last_kernel_of_a_multi_kernel_entry(bench):
    _plan_case(bench, "sumsq")


def test_eager_call_is_unchanged(bench):
    calls = bench.chain("fork", bench.a.cuda_stream, bench.b.cuda_stream)
    bench.check("fork", lambda: _eager(calls))
