"""Time the streaming attention pair (ddpm_attention_stream_fwd / _bwd) against the materialised sequence it replaces above 256 tokens
(ddpm_gemm + ddpm_softmax_fwd + ddpm_gemm and its five-launch backward, as _Engine._attn / _attn_bwd issue them) on the GPU.

    python scripts/attn_stream_bench.py

Same inputs, one process, the sides alternating inside every block; device events; every shape and side warmed up; the median of seven
blocks.  The materialised sequence is timed TWICE per block ("again"): the ratio of its two medians is the run-to-run spread any
comparison has to clear.  Prints ms, achieved FLOP/s from the algorithmic 4 B L^2 C (forward) and 10 B L^2 C (backward), the share of
the bf16 matrix peak (2.5 PFLOP/s dense) and torch.cuda.max_memory_allocated of each side (operands included)."""
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "ddpm-torch_amd"))
from ddpm_torch import _hip, _ops as ops  # noqa: E402

PEAK = 2.5e15
BLOCKS = 7


def block_ms(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n


def peak_bytes(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated()


def main():
    dev, bf, BF16 = "cuda", torch.bfloat16, _hip.BF16
    for B, L, C in [(32, 1024, 128), (8, 4096, 128), (32, 1024, 256)]:
        gen = torch.Generator(device=dev).manual_seed(1)
        qkv = (torch.randn(B * L, 3 * C, device=dev, generator=gen) * 1.2).to(bf)
        d_o = torch.randn(B * L, C, device=dev, generator=gen).to(bf)
        o = torch.empty(B * L, C, device=dev, dtype=bf)
        dqkv = torch.empty_like(qkv)
        lse, dvec = torch.empty(B * L, device=dev), torch.empty(B * L, device=dev)
        sc, st, es, bs = 1.0 / math.sqrt(C), _hip.stream(), 2, L * 3 * C
        q, k, v = qkv.data_ptr(), qkv.data_ptr() + C * es, qkv.data_ptr() + 2 * C * es
        dq, dk, dv = dqkv.data_ptr(), dqkv.data_ptr() + C * es, dqkv.data_ptr() + 2 * C * es
        keep = {}

        def stream_fwd():
            _hip.call("ddpm_attention_stream_fwd", q, 3 * C, o.data_ptr(), C, lse.data_ptr(), B, L, C, sc, BF16, st)

        def stream_bwd():
            _hip.call("ddpm_attention_stream_bwd", q, 3 * C, o.data_ptr(), C, d_o.data_ptr(), C, lse.data_ptr(), dvec.data_ptr(), dq, 3 * C,
                      B, L, C, sc, BF16, st)

        def mat_fwd():
            logits = torch.empty((B, L, L), dtype=torch.float32, device=dev)
            ops.gemm(q, 3 * C, bs, 0, k, 3 * C, bs, 0, logits.data_ptr(), L, L * L, L, L, C, BF16, batch=B, alpha=sc, out_mode=1)
            prob = torch.empty((B, L, L), dtype=bf, device=dev)
            _hip.call("ddpm_softmax_fwd", logits.data_ptr(), prob.data_ptr(), B * L, L, BF16, st)
            ops.gemm(prob.data_ptr(), L, L * L, 0, v, 3 * C, bs, 1, o.data_ptr(), C, L * C, L, C, L, BF16, batch=B)
            keep["prob"] = prob                                   # what the tape holds from forward to backward

        def mat_bwd():
            prob = keep["prob"]
            dp = torch.empty((B, L, L), dtype=torch.float32, device=dev)
            ops.gemm(d_o.data_ptr(), C, L * C, 0, v, 3 * C, bs, 0, dp.data_ptr(), L, L * L, L, L, C, BF16, batch=B, out_mode=1)
            ops.gemm(prob.data_ptr(), L, L * L, 1, d_o.data_ptr(), C, L * C, 1, dv, 3 * C, bs, L, C, L, BF16, batch=B)
            ds = torch.empty((B, L, L), dtype=bf, device=dev)
            _hip.call("ddpm_softmax_bwd", prob.data_ptr(), dp.data_ptr(), ds.data_ptr(), B * L, L, BF16, st)
            ops.gemm(ds.data_ptr(), L, L * L, 0, k, 3 * C, bs, 1, dq, 3 * C, bs, L, C, L, BF16, batch=B, alpha=sc)
            ops.gemm(ds.data_ptr(), L, L * L, 1, q, 3 * C, bs, 1, dk, 3 * C, bs, L, C, L, BF16, batch=B, alpha=sc)

        def both(f, b):
            return lambda: (f(), b())

        flop = {"fwd": 4.0 * B * L * L * C, "fwd+bwd": 14.0 * B * L * L * C}
        legs = {"fwd": [("materialised", mat_fwd), ("streaming", stream_fwd), ("materialised again", mat_fwd)],
                "fwd+bwd": [("materialised", both(mat_fwd, mat_bwd)), ("streaming", both(stream_fwd, stream_bwd)),
                            ("materialised again", both(mat_fwd, mat_bwd))]}
        n = max(2, int(4e12 / flop["fwd+bwd"]))
        print(f"B={B} L={L} C={C}  ({n} calls per block, median of {BLOCKS} blocks)", flush=True)
        for leg, sides in legs.items():
            for _, fn in sides:                                   # warm-up: every side of every shape
                for _ in range(3):
                    fn()
            torch.cuda.synchronize()
            times = {nm: [] for nm, _ in sides}
            for _ in range(BLOCKS):
                for nm, fn in sides:
                    times[nm].append(block_ms(fn, n))
            for nm, fn in sides:
                ms = statistics.median(times[nm])
                fl = flop[leg] / (ms * 1e-3)
                keep.clear()
                mem = peak_bytes(fn)
                print(f"  {leg:8s} {nm:20s} {ms:8.3f} ms  (blocks {min(times[nm]):.3f} .. {max(times[nm]):.3f})  {fl / 1e12:7.1f} TFLOP/s  "
                      f"{100 * fl / PEAK:5.2f} % of peak  peak memory {mem / 2 ** 20:8.1f} MiB", flush=True)
        del qkv, d_o, o, dqkv
        keep.clear()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
