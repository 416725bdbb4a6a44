"""What do the fork / join edges (ddpm_stream_order) cost the training step's main stream?

    rocprofv3 --kernel-trace --hip-runtime-trace --output-format csv -d DIR -- \\
        python scripts/fork_edges.py run DIR/plan_edges.json bench.py --steps 40 --warmup 10
    python scripts/fork_edges.py table DIR [first_step last_step] [--gaps-from KDIR]

`run` starts the given script (bench.py) unchanged, and writes how csrc/plan.hip resolves the edges of every launch plan the run builds
(the same walk over the recorded entries: bound to a producing kernel / recorded / dropped) to the JSON file.

`table` reads the kernel trace and the HIP call trace of the same run.  The call trace places every hipStreamWaitEvent between two
kernel launches in host order (a kernel row and the call that launched it share a correlation id), so for every boundary between two
consecutive kernels of the main stream it knows whether an edge was issued there.  It prints, per boundary of the last step, the gap,
the kernels on both sides, the edge flag, whether a kernel of another stream BEGAN inside the gap and whether the host issued the next launch only after the previous
kernel had ended (then the gap waits for the host, which the call tracer slows down, not for the GPU); then the same folded over all
steps of the window, and three numbers: the mean gap at boundaries with an edge, without one, and the share of edge gaps in which
a side-stream kernel started.  Call tracing slows the host down, and where the kernels are short the main stream then waits for the
host: `--gaps-from KDIR` takes the gaps from the kernel trace of a second run of the same command under --kernel-trace alone (the step
launches the same kernels in the same order, so the edges found in DIR are matched to it by position in the step).
"""
import bisect
import collections
import csv
import glob
import json
import os
import sys


# ------------------------------------------------------------------ run: classify the edges of every plan, then run the script
def classify(segments):
    """csrc/plan.hip resolve() over LaunchPlan.segments: [(entry index in the plan, mode, producer's entry point or None), ...]"""
    out, base = [], 0
    for seg in segments:
        for i, (name, args) in enumerate(seg):
            if name != "ddpm_stream_order" or args[0] == args[1]:
                continue
            waiter, signaller = args
            mode, producer = "record", None
            for j in range(i - 1, -1, -1):
                n, a = seg[j]
                if n == "ddpm_stream_order":
                    if a[0] == waiter and a[1] == signaller:
                        mode = "skip"
                        break
                    if a[0] == signaller and a[1] != signaller:
                        break
                    continue
                if a[-1] != signaller:
                    continue
                if n != "ddpm_fill_zero":
                    mode, producer = "wait", n
                break
            out.append((base + i, mode, producer))
        base += len(seg)
    return out


def run(argv):
    out_path, script, rest = argv[0], argv[1], argv[2:]
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "ddpm-torch_amd"))
    from ddpm_torch import _plan
    plans = []
    build = _plan.LaunchPlan._build_native

    def build_and_classify(self):
        edges = classify(self.segments)
        count = collections.Counter(m for _, m, _ in edges)
        plans.append({"entries": self.launches, "segments": len(self.segments), "edges": len(edges), "bound_to_a_kernel": count["wait"],
                      "recorded": count["record"], "skipped": count["skip"],
                      "producers": dict(collections.Counter(p for _, m, p in edges if m == "wait"))})
        print("launch plan:", json.dumps(plans[-1]), flush=True)
        with open(out_path, "w") as f:
            json.dump(plans, f, indent=1)
        return build(self)
    _plan.LaunchPlan._build_native = build_and_classify
    import runpy
    sys.argv = [script, *rest]
    runpy.run_path(script, run_name="__main__")


# ------------------------------------------------------------------ table
def _csv(d, suffix):
    f = glob.glob(d + "/**/*" + suffix, recursive=True)
    return list(csv.DictReader(open(f[0]))) if f else []


def short(k):
    return k.split("(")[0].replace("void ", "").replace("(anonymous namespace)::", "")[-52:] or "?"


def _kernels(d):
    ev = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"], (r.get("Queue_Id", "0"), r.get("Stream_Id", "")),
                 r["Correlation_Id"]) for r in _csv(d, "kernel_trace.csv"))
    ends = [e for s, e, k, q, c in ev if "mt_adam_ema" in k]          # the optimiser kernel ends a step
    busy = collections.Counter()
    for s, e, k, q, c in ev:
        busy[q] += e - s
    return ev, ends, busy.most_common(1)[0][0]


def _steps(ev, ends, main, lo, hi):
    """{step: main-stream kernels that end in (ends[step - 1], ends[step]]}, in start order"""
    out = collections.defaultdict(list)
    for r in ev:
        if r[3] == main and ends[lo] < r[1] <= ends[hi]:
            out[bisect.bisect_left(ends, r[1])].append(r)
    return out


def table(argv):
    gaps_dir = None
    if "--gaps-from" in argv:
        k = argv.index("--gaps-from")
        gaps_dir = argv[k + 1]
        argv = argv[:k] + argv[k + 2:]
    d = argv[0]
    api = _csv(d, "hip_api_trace.csv")
    if not api:
        sys.exit("no *hip_api_trace.csv under " + d + ": trace with --kernel-trace --hip-runtime-trace")
    ev, ends, main = _kernels(d)
    # host order of the calls: position of every launch (by correlation id) and of every edge call
    calls = sorted((int(r["Start_Timestamp"]), r["Function"], r["Correlation_Id"]) for r in api)
    pos = {c: i for i, (t, f, c) in enumerate(calls)}
    issued = {c: t for t, f, c in calls}          # when the host made the call (same clock as the kernel rows)
    waits = [i for i, (t, f, c) in enumerate(calls) if f == "hipStreamWaitEvent"]
    records = [i for i, (t, f, c) in enumerate(calls) if f == "hipEventRecord"]

    def between(idx, a, b):
        return bisect.bisect_left(idx, b) - bisect.bisect_right(idx, a)
    # the template: one steady step of the call-traced run, (kernel name, wait calls, record calls before it) per main-stream launch
    t_step = len(ends) - 2
    seq = _steps(ev, ends, main, t_step - 2, t_step)
    prev, template = seq[t_step - 1][-1], []
    for r in seq[t_step]:
        template.append((short(r[2]), between(waits, pos[prev[4]], pos[r[4]]), between(records, pos[prev[4]], pos[r[4]])))
        prev = r
    print(f"edges placed from the HIP call trace of {d}, step {t_step}: {len(template)} main-stream launches, {sum(w for _, w, _ in template)} "
          f"hipStreamWaitEvent and {sum(r for _, _, r in template)} hipEventRecord calls between them")
    plan_json = os.path.join(d, "plan_edges.json")
    if os.path.exists(plan_json):
        for p in json.load(open(plan_json)):
            print("launch plan (how csrc/plan.hip resolves its edges):", json.dumps(p))
    same = gaps_dir is None
    if not same:
        ev, ends, main = _kernels(gaps_dir)
        print(f"gaps from the kernel trace of {gaps_dir} (no call tracing in that run), matched to the template by position in the step")
    lo = int(argv[1]) if len(argv) > 1 else len(ends) - 12
    hi = int(argv[2]) if len(argv) > 2 else len(ends) - 2
    nsteps = hi - lo
    seq = _steps(ev, ends, main, lo - 1, hi)
    side_starts = sorted(r[0] for r in ev if r[3] != main)
    main_busy = sum(r[1] - r[0] for s in range(lo + 1, hi + 1) for r in seq[s])
    side_busy = sum(r[1] - r[0] for r in ev if r[3] != main and ends[lo] < r[1] <= ends[hi])
    rows = []       # (step, gap, after, before, wait calls, record calls, side kernel began inside, launch call came after the previous kernel's end)
    unmatched = 0
    for step in range(lo + 1, hi + 1):
        ks = seq[step]
        if [short(r[2]) for r in ks] != [t[0] for t in template]:
            unmatched += 1
            continue
        a = seq[step - 1][-1]
        for b, (name, w, rec) in zip(ks, template):
            began = bisect.bisect_left(side_starts, b[0]) - bisect.bisect_right(side_starts, a[1]) > 0
            late = issued[b[4]] > a[1] if same else None
            rows.append((step, b[0] - a[1], short(a[2]), name, w, rec, began, late))
            a = b
    n_ok = nsteps - unmatched
    print(f"steps {lo + 1}..{hi}: span {(ends[hi] - ends[lo]) / nsteps / 1e6:.3f} ms/step; main stream = queue {main[0]} stream {main[1]}, busy "
          f"{main_busy / nsteps / 1e6:.3f} ms/step; other streams busy {side_busy / nsteps / 1e6:.3f} ms/step; {unmatched} steps whose launch sequence "
          f"differs from the template left out")
    nsteps = n_ok
    last = max(r[0] for r in rows)
    flag = lambda late: "    " if not late else "host"
    print(f"--- every main-stream boundary of step {last}: gap us | edge (wait calls / record calls) | side kernel began in the gap | launch issued late | after -> before")
    for step, gap, a, b, w, rec, began, late in rows:
        if step == last:
            print(f"  {gap / 1e3:7.2f}  {'edge' if w else '    '} {w}/{rec}  {'side' if began else '    '}  {flag(late)}  {a} -> {b}")
    agg = collections.defaultdict(lambda: [0, 0, 0, 0])
    for step, gap, a, b, w, rec, began, late in rows:
        v = agg[(bool(w), a, b)]
        v[0] += 1; v[1] += gap; v[2] += began; v[3] += bool(late)
    print(f"--- boundaries folded over {nsteps} steps, by total gap: us/step | n/step | mean us | side-start share | issued-late share | edge | after -> before")
    for (w, a, b), (n, g, s, h) in sorted(agg.items(), key=lambda kv: -kv[1][1])[:40]:
        print(f"  {g / nsteps / 1e3:7.1f}  {n / nsteps:5.1f}  {g / n / 1e3:6.2f}  {s / n:4.2f}  {h / n if same else float('nan'):4.2f}  {'edge' if w else '    '}  {a} -> {b}")
    e = [r for r in rows if r[4]]
    o = [r for r in rows if not r[4] and "mt_adam_ema" not in r[2]]       # (the step boundary waits for the host: not a kernel boundary)
    mean = lambda v: sum(r[1] for r in v) / max(len(v), 1) / 1e3
    print(f"--- summary: boundaries with an edge {len(e) / nsteps:.1f}/step, mean gap {mean(e):.2f} us, total {sum(r[1] for r in e) / nsteps / 1e3:.1f} us/step; "
          f"without {len(o) / nsteps:.1f}/step, mean gap {mean(o):.2f} us, total {sum(r[1] for r in o) / nsteps / 1e3:.1f} us/step; "
          f"edge gaps in which a side-stream kernel began: {sum(r[6] for r in e) / max(len(e), 1):.2f}")
    if same:
        print(f"    the next kernel's launch call came only after the previous kernel had ended (the gap waits for the host, which the call tracer slows "
              f"down): {sum(r[7] for r in e) / max(len(e), 1):.2f} of the edge boundaries, {sum(r[7] for r in o) / max(len(o), 1):.2f} of the others; "
              f"edge boundaries where it did not: mean gap {mean([r for r in e if not r[7]]):.2f} us")
    es = [r for r in e if r[6]]
    en = [r for r in e if not r[6]]
    print(f"    edge gaps with a side start: mean {mean(es):.2f} us (n/step {len(es) / nsteps:.1f}); without: mean {mean(en):.2f} us (n/step {len(en) / nsteps:.1f})")
    print(f"    main-stream gap time: {sum(r[1] for r in rows) / nsteps / 1e3:.1f} us/step in all, {sum(r[1] for r in rows if r[1] > 3000) / nsteps / 1e3:.1f} us/step in gaps > 3 us")
    g = [r[1] for r in rows if "wgrad_unpack_kernel" in r[3]]
    if g:
        print(f"    gap before wgrad_unpack_kernel (the join at the end of the backward): mean {sum(g) / len(g) / 1e3:.1f} us")


if __name__ == "__main__":
    {"run": run, "table": table}[sys.argv[1]](sys.argv[2:])
