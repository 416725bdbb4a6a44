"""Time the streaming attention pair (ddpm_attention_stream_fwd / _bwd) against the materialised sequence it replaces above 256 tokens
(ddpm_gemm + ddpm_softmax_fwd + ddpm_gemm and its five-launch backward, as _Engine._attn / _attn_bwd issue them) on the GPU.

    python scripts/attn_stream_bench.py

Same inputs, one process, the sides alternating inside every block; device events; every shape and side warmed up; the median of seven
blocks.  The materialised sequence is timed TWICE per block ("again"): the ratio of its two medians is the run-to-run spread any
comparison has to clear.  Prints ms, achieved FLOP/s from the algorithmic 4 B L^2 C (forward) and 10 B L^2 C (backward), the share of
the bf16 matrix peak (2.5 PFLOP/s dense) and torch.cuda.max_memory_allocated of each side (operands included).

    python scripts/attn_stream_bench.py --heads

times the multi-head entry points (ddpm_attention_mh_fwd / _bwd) instead: B = 128, C = 256, L in {256, 1024}, heads in {1, 4, 8}.  One
multi-head call against `heads` single-head streaming calls at width d = C / heads on per-head packed buffers of their own (the same
work in `heads` launches), the multi-head call timed twice per block for the spread, and at L = 256 the on-chip pair
(ddpm_attention_fwd_lse / ddpm_attention_bwd) at C = 256 for context."""
import argparse
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


def heads_main():
    dev, bf, BF16, st = "cuda", torch.bfloat16, _hip.BF16, _hip.stream()
    B, C = 128, 256
    for L in (256, 1024):
        for H in (1, 4, 8):
            d = C // H
            gen = torch.Generator(device=dev).manual_seed(1)
            qkv = (torch.randn(B * L, 3, H, d, device=dev, generator=gen) * 1.2).to(bf)
            d_o = torch.randn(B * L, H, d, device=dev, generator=gen).to(bf)
            o, dqkv = torch.empty(B * L, C, device=dev, dtype=bf), torch.empty(B * L, 3 * C, device=dev, dtype=bf)
            lse, dvec = torch.empty(B * H * L, device=dev), torch.empty(B * H * L, device=dev)
            # every head's slices in a packed [B][L][3d] buffer of its own, with its own outputs
            per = [dict(qkv=qkv[:, :, h].reshape(B * L, 3 * d).contiguous(), d_o=d_o[:, h].contiguous(), o=torch.empty(B * L, d, device=dev, dtype=bf),
                        dqkv=torch.empty(B * L, 3 * d, device=dev, dtype=bf), lse=torch.empty(B * L, device=dev), dvec=torch.empty(B * L, device=dev))
                   for h in range(H)]
            sc = 1.0 / math.sqrt(d)

            def mh_fwd():
                _hip.call("ddpm_attention_mh_fwd", qkv.data_ptr(), 3 * C, o.data_ptr(), C, lse.data_ptr(), B, L, C, H, sc, BF16, st)

            def mh_bwd():
                _hip.call("ddpm_attention_mh_bwd", qkv.data_ptr(), 3 * C, o.data_ptr(), C, d_o.data_ptr(), C, lse.data_ptr(), dvec.data_ptr(),
                          dqkv.data_ptr(), 3 * C, B, L, C, H, sc, BF16, st)

            def pair(fwd, bwd, width, scale):
                def f():
                    for p in per:
                        _hip.call(fwd, p["qkv"].data_ptr(), 3 * width, p["o"].data_ptr(), width, p["lse"].data_ptr(), B, L, width, scale, BF16, st)

                def b():
                    for p in per:
                        _hip.call(bwd, p["qkv"].data_ptr(), 3 * width, p["o"].data_ptr(), width, p["d_o"].data_ptr(), width, p["lse"].data_ptr(),
                                  p["dvec"].data_ptr(), p["dqkv"].data_ptr(), 3 * width, B, L, width, scale, BF16, st)
                return f, b

            one_fwd, one_bwd = pair("ddpm_attention_stream_fwd", "ddpm_attention_stream_bwd", d, sc)
            sides = [("multi-head", mh_fwd, mh_bwd), (f"{H} x single-head d={d}", one_fwd, one_bwd), ("multi-head again", mh_fwd, mh_bwd)]
            if L == 256 and H == 1:                               # context: the on-chip pair the single-head engine takes at this L
                sides.append(("on-chip pair C=256", *pair("ddpm_attention_fwd_lse", "ddpm_attention_bwd", C, sc)))
            flop = {"fwd": 4.0 * B * L * L * d * H, "bwd": 10.0 * B * L * L * d * H}          # H heads of width d: B H L^2 d = B L^2 C
            n = max(2, int(2e12 / (flop["fwd"] + flop["bwd"])))
            print(f"B={B} L={L} C={C} heads={H} d={d}  ({n} calls per block, median of {BLOCKS} blocks)", flush=True)
            for leg in ("fwd", "bwd"):
                fns = [(nm, f if leg == "fwd" else b) for nm, f, b in sides]
                for _, f, _b in sides:                            # the backward reads the forward's o and lse
                    f()
                for _, fn in fns:
                    for _ in range(3):
                        fn()
                torch.cuda.synchronize()
                times = {nm: [] for nm, _ in fns}
                for _ in range(BLOCKS):
                    for nm, fn in fns:
                        times[nm].append(block_ms(fn, n))
                for nm, _ in fns:
                    ms = statistics.median(times[nm])
                    fl = flop[leg] / (ms * 1e-3)
                    print(f"  {leg:4s} {nm:24s} {ms:8.4f} ms  (blocks {min(times[nm]):.4f} .. {max(times[nm]):.4f})  {fl / 1e12:7.1f} TFLOP/s  "
                          f"{100 * fl / PEAK:5.2f} % of peak", flush=True)
            del qkv, d_o, o, dqkv, per
            torch.cuda.empty_cache()


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--heads", action="store_true", help="time the multi-head entry points against per-head single-head calls")
    heads_main() if ap.parse_args().heads else main()
