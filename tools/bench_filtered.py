"""Filtered top-k (rlr_search_topk_filtered) against the unfiltered search on the same index, and the crossover of the
filter's two paths (list path / masked scan).

    python tools/bench_filtered.py [--rows 1000000] [--dim 768] [--k 100] [--calls 50] [--out FILE]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_filtered.py --trace-run --out PLAN
    python tools/bench_filtered.py --parse-trace DIR --plan PLAN [--out FILE]
    python tools/bench_filtered.py --queries 2 4 8 --baseline-root CHECKOUT [--out FILE]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_filtered.py --queries 8 --trace-run

Corpus: f32 rows filled on the device (rlr_index_fill_synthetic, seeded); the query is a noisy copy of a stored row.
Timed mode: per fraction of allowed rows {1.0, 0.5, 0.1, 0.01, 0.001}, as one contiguous range and as scattered rows, the
median wall time of a call (host clock around a call that returns after its device synchronisation), warm, alternating
with the unfiltered rlr_search_topk of the same query -- the baseline -- and its ratio to it; then both paths at
n_allowed in {256, 1 k, 4 k, 8 k, 16 k, 64 k, 256 k} scattered rows (rlr_filter_set_path) and the crossover.  Before any
timing, fraction 1.0 is checked against the unfiltered result and the two paths against each other (rows, score bits).
Trace mode: the same points with every filter on the masked scan, a fixed number of calls each, for a profiler run of
its own (with --queries N: N-query calls over the points on the masked scan; set RLR_BATCH_MIN=2 so that each shares);
--parse-trace reads the kernel trace back: the masked scan kernel's median time per point, the bytes it has to move
(allowed rows x row bytes + the mask + the scores it stores) and the rate that makes.  One JSON line on stdout.
Batch mode (--queries N ...): the wall time of ONE rlr_search_topk_filtered call with N distinct queries, per fraction
{1.0, 0.5, 0.1, 0.01} as a range and as scattered rows, and on the list path at 256 / 4096 scattered rows.  The baseline
is the same call with the same arguments on ANOTHER BUILD of the library in the same process: --baseline-root names a
checkout of the commit to compare against, built in place (python CHECKOUT/rust-local-rag_amd/build.py); it is loaded as
a second copy of the package with an index of its own, filled from the same seed.  Warm, then `calls` rounds of
baseline leg A | this build | baseline leg B, alternating call by call: the baseline's spread is the distance of its two
legs' medians, and a point is `ok` when this build's median is at most the baseline's median plus that spread.  The
results of both builds are compared first (rows, score bits).
"""
from __future__ import annotations

import argparse
import csv
import glob
import importlib
import importlib.util
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FRACTIONS = [1.0, 0.5, 0.1, 0.01, 0.001]
CROSSOVER = [256, 1024, 4096, 8192, 16384, 65536, 262144]
WARM, TRACE_CALLS = 5, 20


def load():
    return importlib.import_module("rust-local-rag_amd")


def points(n_rows, seed):
    """(name, kind, allowed rows or range) for every fraction and both shapes"""
    rng = np.random.default_rng(seed)
    out = []
    for fr in FRACTIONS:
        m = max(1, int(round(n_rows * fr)))
        first = (n_rows - m) // 2
        out.append((f"range_{fr}", "ranges", [(first, m)], m))
        rows = np.arange(n_rows) if m == n_rows else np.sort(rng.choice(n_rows, size=m, replace=False))
        out.append((f"scattered_{fr}", "rows", rows, m))
    return out


def load_checkout(root, name="rlr_baseline"):
    """the package of another checkout (built in place) as a second module: its own ctypes handle on its own library"""
    d = os.path.join(os.path.abspath(root), "rust-local-rag_amd")
    spec = importlib.util.spec_from_file_location(name, os.path.join(d, "__init__.py"), submodule_search_locations=[d])
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


BATCH_FRACTIONS = [1.0, 0.5, 0.1, 0.01]
LIST_ROWS = [256, 4096]


def batch_points(n_rows, seed):
    out = [p for p in points(n_rows, seed) if float(p[0].split("_")[1]) in BATCH_FRACTIONS]
    rng = np.random.default_rng(seed + 100)
    for m in LIST_ROWS:
        out.append((f"list_{m}", "rows", np.sort(rng.choice(n_rows, size=m, replace=False)), m))
    return out


def batch_queries(ix, dim, n_rows, n):
    rng = np.random.default_rng(70)
    rows = ix.fetch_rows(rng.integers(0, n_rows, size=n))
    q = rows + 0.05 * rng.standard_normal((n, dim)).astype(np.float32)
    return np.ascontiguousarray(q / np.linalg.norm(q, axis=1, keepdims=True), dtype=np.float32)


def timed_batch(pkg, a):
    base_pkg = load_checkout(a.baseline_root) if a.baseline_root else None
    ix, _ = build(pkg, a)
    bix = build(base_pkg, a)[0] if base_pkg else None
    res = {"bench": "filtered_batch", "rows": a.rows, "dim": a.dim, "k": a.k, "calls": a.calls,
           "baseline": "another build, same process, legs alternating" if bix else None, "points": []}
    for name, kind, spec, m in batch_points(a.rows, seed=1):
        f = make_filter(ix, kind, spec)
        bf = make_filter(bix, kind, spec) if bix else None
        for nq in a.queries:
            qs = batch_queries(ix, a.dim, a.rows, nq)
            run = lambda: ix.search_topk(qs, a.k, filter=f)
            base = (lambda: bix.search_topk(qs, a.k, filter=bf)) if bix else None
            ix.profile_read(reset=True)
            got = run()
            prof = ix.profile_read()
            if base:
                want = base()
                assert np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32)), \
                    f"{name} x {nq}: differs from the baseline build"
            for _ in range(WARM):
                run()
                if base:
                    base()
            tn, ta, tb = [], [], []
            for _ in range(a.calls):
                if base:
                    t0 = time.perf_counter(); base(); ta.append(time.perf_counter() - t0)
                t0 = time.perf_counter(); run(); tn.append(time.perf_counter() - t0)
                if base:
                    t0 = time.perf_counter(); base(); tb.append(time.perf_counter() - t0)
            p = {"point": name, "n_allowed": m, "path": f.info()["path"], "queries": nq, "shared_passes": int(prof.n_batches),
                 "handed_back": int(prof.n_batch_fallbacks), "ms": round(1e3 * float(np.median(tn)), 4),
                 "p10_ms": round(1e3 * float(np.percentile(tn, 10)), 4), "p90_ms": round(1e3 * float(np.percentile(tn, 90)), 4)}
            if base:
                la, lb = 1e3 * float(np.median(ta)), 1e3 * float(np.median(tb))
                b = 1e3 * float(np.median(ta + tb))
                p.update(baseline_ms=round(b, 4), baseline_legs_ms=[round(la, 4), round(lb, 4)], baseline_spread_ms=round(abs(la - lb), 4),
                         ratio_to_baseline=round(p["ms"] / b, 3), ok=bool(p["ms"] <= b + abs(la - lb)))
            res["points"].append(p)
            print(json.dumps(p), file=sys.stderr, flush=True)
        f.close()
        if bf:
            bf.close()
    ix.close()
    if bix:
        bix.close()
    return res


def make_filter(ix, kind, spec):
    return ix.filter_ranges(spec) if kind == "ranges" else ix.filter_rows(spec)


def median_ms(fn, calls):
    t = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(t)), 1e3 * float(np.percentile(t, 10)), 1e3 * float(np.percentile(t, 90))


def same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))


def build(pkg, a):
    ix = pkg.GpuIndex(a.dim)
    ix.fill_synthetic(a.rows, seed=20261017, n_clusters=64)
    rng = np.random.default_rng(7)
    row = ix.fetch_rows([int(rng.integers(0, a.rows))])[0]
    q = row + 0.05 * rng.standard_normal(a.dim).astype(np.float32)
    q = (q / np.linalg.norm(q)).astype(np.float32)
    return ix, q


def timed(pkg, a):
    ix, q = build(pkg, a)
    k = a.k
    res = {"bench": "filtered", "rows": a.rows, "dim": a.dim, "k": k, "calls": a.calls, "points": [], "crossover": []}
    base = lambda: ix.search_topk(q, k)
    for _ in range(WARM):
        base()
    unfiltered = base()
    base_all = []
    for name, kind, spec, m in points(a.rows, seed=1):
        with make_filter(ix, kind, spec) as f:
            info = f.info()
            run = lambda: ix.search_topk(q, k, filter=f)
            got = run()
            if m == a.rows:
                assert same(got, unfiltered), f"{name}: differs from the unfiltered search"
            other = "list" if info["path"] == "scan" else "scan"
            if m <= 65536 or other == "scan":
                f.set_path(other)
                assert same(run(), got), f"{name}: the two paths differ"
                f.set_path(info["path"])
            for _ in range(WARM):
                run()
                base()
            # alternate: the same number of baseline calls beside this point's calls
            tf, tb = [], []
            for _ in range(a.calls):
                t0 = time.perf_counter(); run(); tf.append(time.perf_counter() - t0)
                t0 = time.perf_counter(); base(); tb.append(time.perf_counter() - t0)
            ms, b = 1e3 * float(np.median(tf)), 1e3 * float(np.median(tb))
            base_all.append(b)
            p = {"point": name, "n_allowed": m, "path": info["path"], "ms": round(ms, 4), "p10_ms": round(1e3 * float(np.percentile(tf, 10)), 4),
                 "p90_ms": round(1e3 * float(np.percentile(tf, 90)), 4), "baseline_ms": round(b, 4), "ratio_to_baseline": round(ms / b, 3)}
            res["points"].append(p)
            print(json.dumps(p), file=sys.stderr, flush=True)
    res["baseline_ms_median"] = round(float(np.median(base_all)), 4)
    res["baseline_ms_spread"] = [round(min(base_all), 4), round(max(base_all), 4)]   # run-to-run spread of the baseline medians
    rng = np.random.default_rng(3)
    cross = None
    for m in CROSSOVER:
        if m > a.rows:
            continue
        rows = np.sort(rng.choice(a.rows, size=m, replace=False))
        with ix.filter_rows(rows) as f:
            row = {"n_allowed": m, "natural_path": f.info()["path"]}
            for path in ("list", "scan"):
                f.set_path(path)
                run = lambda: ix.search_topk(q, k, filter=f)
                for _ in range(WARM):
                    run()
                row[path + "_ms"] = round(median_ms(run, a.calls)[0], 4)
            res["crossover"].append(row)
            print(json.dumps(row), file=sys.stderr, flush=True)
            if cross is None and row["scan_ms"] < row["list_ms"]:
                cross = m
    res["scan_wins_from_n_allowed"] = cross
    ix.close()
    return res


def trace_run(pkg, a):
    """every point on the masked scan, WARM + TRACE_CALLS calls each, in a fixed order (the plan --parse-trace reads)"""
    ix, q = build(pkg, a)
    plan = {"rows": a.rows, "dim": a.dim, "k": a.k, "per_point": WARM + TRACE_CALLS, "keep": TRACE_CALLS, "points": []}
    if a.queries:                                            # N-query calls: one masked launch per call where the pass is shared
        plan["queries"] = a.queries[0]
        q = batch_queries(ix, a.dim, a.rows, a.queries[0])
    for _ in range(WARM + TRACE_CALLS):
        ix.search_topk(q[0] if a.queries else q, a.k)
    for name, kind, spec, m in ([p for p in batch_points(a.rows, seed=1) if p[3] >= 8192] if a.queries else points(a.rows, seed=1)):
        with make_filter(ix, kind, spec) as f:
            f.set_path("scan")
            for _ in range(WARM + TRACE_CALLS):
                ix.search_topk(q, a.k, filter=f)
        plan["points"].append({"point": name, "n_allowed": m})
    ix.close()
    return plan


def parse_trace(a):
    with open(a.plan) as f:
        plan = json.load(f)
    files = glob.glob(os.path.join(a.parse_trace, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        raise SystemExit(f"no *kernel_trace.csv under {a.parse_trace}")
    masked, fixed = [], []
    for path in files:
        with open(path, newline="") as f:
            for r in csv.DictReader(f):
                name = r.get("Kernel_Name", "")
                t0, t1 = int(r["Start_Timestamp"]), int(r["End_Timestamp"])
                if "scan_masked" in name:
                    masked.append((t0, (t1 - t0) / 1e3))
                elif "scan_fixed_kernel" in name:
                    fixed.append((t0, (t1 - t0) / 1e3))
    masked.sort()
    fixed.sort()
    per, keep = plan["per_point"], plan["keep"]
    if len(masked) != per * len(plan["points"]):             # (with --queries: a point that ran one by one has N launches per call)
        raise SystemExit(f"{len(masked)} masked scan launches in the trace, the plan has {per * len(plan['points'])}")
    row_bytes = plan["dim"] * 4
    out = {"bench": "filtered_kernels", "rows": plan["rows"], "dim": plan["dim"],
           "unfiltered_scan_us": round(float(np.median([d for _, d in fixed[-keep:]])), 2) if fixed else None, "points": []}
    for i, p in enumerate(plan["points"]):
        us = float(np.median([d for _, d in masked[i * per + (per - keep):(i + 1) * per]]))
        # allowed rows + mask + scores stored (one array per query of a shared pass)
        nbytes = p["n_allowed"] * row_bytes + plan["rows"] // 8 + plan["rows"] * 4 * plan.get("queries", 1)
        out["points"].append({"point": p["point"], "n_allowed": p["n_allowed"], "masked_scan_us": round(us, 2), "bytes": nbytes,
                              "gb_per_s": round(nbytes / us / 1e3, 1)})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--trace-run", action="store_true")
    ap.add_argument("--parse-trace", default=None)
    ap.add_argument("--plan", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--queries", type=int, nargs="+", default=None, help="batch mode: queries per rlr_search_topk_filtered call")
    ap.add_argument("--baseline-root", default=None, help="batch mode: a built checkout of the commit to compare against")
    a = ap.parse_args()
    if a.parse_trace:
        result = parse_trace(a)
    else:
        pkg = load()
        if pkg.device_count() < 1:
            raise SystemExit("bench_filtered needs a GPU: the library has no CPU path")
        result = trace_run(pkg, a) if a.trace_run else timed_batch(pkg, a) if a.queries else timed(pkg, a)
    line = json.dumps(result)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
