"""Kernel-by-kernel comparison of the gfx950 device code of two csrc/ directories (hipcc cross-compiles: no GPU needed).
    python scripts/isa_diff.py PARENT_CSRC BRANCH_CSRC [--allow NAME ...] [--map OLD=NEW ...] [--show] [--only SOURCE ...]

Every file of build.SOURCES is compiled from both directories with build.FLAGS + -S --cuda-device-only.  Per kernel symbol the text from
its label to its end plus its .amdhsa_kernel descriptor is kept, comments and white space stripped, the per-file function number in
local labels (.LBB<n>_, .LJTI<n>_, .Ltmp<n>: they shift when a function before them comes or goes) and the __hip_cuid_* symbol masked.
Prints identical / differ / disappeared / appeared with demangled names; exits 1 when a kernel whose demangled name contains none of the
--allow strings differs, disappears or appears.  --show adds a unified diff of each kernel that differs.  --map OLD=NEW (substrings of
demangled names, repeatable) pairs a parent kernel that has no branch kernel of its symbol with the renamed or re-templated branch kernel
that replaces it: the two are compared as one kernel (listed as "OLD -> NEW") with the symbol masked; each side must match exactly once
per file, and a --map that pairs nothing in any file is an error."""
import argparse, concurrent.futures, difflib, os, re, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ddpm-torch_amd", "csrc"))
import build  # noqa: E402

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
MASKS = [(re.compile(r"\.(LBB|LJTI|Ltmp|Lfunc_begin|Lfunc_end)\d+"), r".\1#"), (re.compile(r"__hip_cuid_\w+"), "__hip_cuid_#")]


def compile_s(csrc, src, out):
    path = os.path.join(csrc, src)
    if not os.path.exists(path):
        return ""
    subprocess.run([HIPCC, *build.FLAGS, "-S", "--cuda-device-only", path, "-o", out], check=True, stderr=subprocess.PIPE)
    with open(out) as f:
        return f.read()


def kernels(text):
    """{symbol: [normalised lines]} for every symbol that has an .amdhsa_kernel descriptor"""
    lines = []
    for ln in text.splitlines():
        ln = re.sub(r"\s+", " ", ln.split(";", 1)[0]).strip()
        if ln:
            for rx, to in MASKS:
                ln = rx.sub(to, ln)
            lines.append(ln)
    names = [ln.split()[1] for ln in lines if ln.startswith(".amdhsa_kernel ")]
    out = {}
    for n in names:
        body = lines[lines.index(n + ":"):]
        body = body[:next(i for i, ln in enumerate(body) if ln.startswith(".Lfunc_end")) + 1]
        desc = lines[lines.index(".amdhsa_kernel " + n):]
        out[n] = body + desc[:desc.index(".end_amdhsa_kernel") + 1]
    return out


def demangle(names):
    if not names:
        return {}
    try:
        res = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    except (OSError, subprocess.CalledProcessError):
        res = names
    return {n: re.sub(r"\(anonymous namespace\)::", "", d) for n, d in zip(names, res)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("parent_csrc")
    ap.add_argument("branch_csrc")
    ap.add_argument("--allow", nargs="*", default=[], metavar="NAME", help="kernels (substring of the demangled name) that may differ")
    ap.add_argument("--map", action="append", default=[], metavar="OLD=NEW", help="compare parent kernel OLD with branch kernel NEW (substrings of demangled names)")
    ap.add_argument("--show", action="store_true", help="print a unified diff of each kernel that differs")
    ap.add_argument("--only", nargs="*", metavar="SOURCE", help="compare these files of build.SOURCES only (while looking for a spelling)")
    args = ap.parse_args()
    sources = [s for s in build.SOURCES if not args.only or s in args.only]
    with tempfile.TemporaryDirectory() as tmp, concurrent.futures.ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:
        jobs = {(side, s): pool.submit(compile_s, d, s, os.path.join(tmp, side + "_" + s.replace(".hip", ".s")))
                for side, d in (("p", args.parent_csrc), ("b", args.branch_csrc)) for s in sources}
        asm = {k: kernels(j.result()) for k, j in jobs.items()}
    rows = {"identical": [], "differ": [], "disappeared": [], "appeared": []}
    diffs = []
    paired = set()
    for s in sources:
        p, b = asm[("p", s)], asm[("b", s)]
        names = demangle(sorted(set(p) | set(b)))
        for m in args.map:
            old, new = m.split("=", 1)
            po, bn = [n for n in p if n not in b and old in names[n]], [n for n in b if n not in p and new in names[n]]
            if len(po) == 1 and len(bn) == 1:
                paired.add(m)
                names[po[0]] += " -> " + names[bn[0]]
                p[po[0]] = [ln.replace(po[0], "@KERNEL") for ln in p[po[0]]]
                b[po[0]] = [ln.replace(bn[0], "@KERNEL") for ln in b.pop(bn[0])]
            elif po or bn:
                sys.exit("--map %s=%s in %s: %d parent and %d branch kernels match (want one each)" % (old, new, s, len(po), len(bn)))
        for n in list(p) + [n for n in b if n not in p]:
            state = "disappeared" if n not in b else "appeared" if n not in p else "identical" if p[n] == b[n] else "differ"
            rows[state].append((s.replace(".hip", ".s"), names[n]))
            if state == "differ":
                d = list(difflib.unified_diff(p[n], b[n], "parent", "branch", lineterm="", n=2))
                changed = sum(1 for ln in d[2:] if ln[0] in "+-")
                diffs.append((names[n], changed, len(p[n]), len(b[n]), d))
    if set(args.map) - paired:
        sys.exit("--map paired nothing in any file: " + ", ".join(sorted(set(args.map) - paired)))
    print("parent kernels %d, branch kernels %d: identical %d, differ %d, disappeared %d, appeared %d" % (
        sum(len(asm[("p", s)]) for s in sources), sum(len(asm[("b", s)]) for s in sources),
        *(len(rows[k]) for k in ("identical", "differ", "disappeared", "appeared"))))
    bad = 0
    for state in ("differ", "disappeared", "appeared"):
        print("--- " + state.upper())
        for f, name in rows[state]:
            ok = any(a in name for a in args.allow)
            bad += not ok
            print("  %s: %s%s" % (f, name, "   (allowed)" if ok else ""))
    for name, changed, np_, nb, d in diffs:
        print("--- %s: %d changed lines (parent %d, branch %d lines)" % (name, changed, np_, nb))
        if args.show:
            print("\n".join(d))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
