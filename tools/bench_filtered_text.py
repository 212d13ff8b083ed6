"""N scoped text queries as ONE rlr_engine_search_text_batch_filtered call against N calls of
rlr_engine_search_text_filtered -- the way the same requests were served before the batched call existed -- in the same
process, the legs alternating.

    python tools/bench_filtered_text.py [--rows 1000000] [--dim 768] [--queries 2 4 8 32] [--k 10] [--lam 0.3]
                                        [--calls 50] [--scattered | --small] [--out FILE]
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/bench_filtered_text.py --trace-run [--out PLAN]
    python tools/bench_filtered_text.py --parse-trace DIR --plan PLAN [--out FILE]

Corpus: the one of tools/bench_text_batch.py (f32 rows filled on the device, one Zipf text of 4..25 words per row in the
GPU LexicalIndex), queries likewise (a noisy copy of a stored row, 2..4 Zipf words).  Scopes: the allowed fractions
{1.0, 0.5, 0.1, 0.01} of tools/bench_filtered.py's batch table as one contiguous range -- a set of documents is a few runs
of rows -- with --scattered as scattered rows too, with --small only 256 and 4096 scattered rows.  Per (scope, N): the
results of both ways are compared first (rows and every score bit), then WARM rounds, then `calls` rounds of loop leg A | the batched call | loop leg B.  Reported: the
median ms of the batched call and of the loop, the two loop legs' medians and their distance (the spread), the ratio, how the
batch served its queries (rlr_text_batch_info), and `gain`: the batched median lies below the loop's by more than the
spread (`loss`: above it by more than the spread).  One JSON line on stdout.
Trace mode: WARM + TRACE_CALLS calls of rlr_lexical_score_batch (8 queries) without a filter, then of
rlr_lexical_score_batch_filtered per range fraction {1.0, 0.1, 0.01}, for a profiler run of its own; --parse-trace reads the
kernel trace back: the median time of bm25_batch_kernel<false> and of bm25_batch_kernel<true> per fraction.
"""
from __future__ import annotations

import argparse
import csv
import ctypes as C
import glob
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_filtered import batch_points, make_filter  # noqa: E402
from bench_text_batch import build, load, queries  # noqa: E402

WARM, TRACE_CALLS, TRACE_QUERIES = 5, 20, 8
TRACE_FRACTIONS = [1.0, 0.1, 0.01]


def scopes(n_rows, scattered, small=False):
    if small:                                               # 256 and 4096 scattered rows: the top-k's list path
        return [p for p in batch_points(n_rows, seed=1) if p[0].startswith("list")]
    return [p for p in batch_points(n_rows, seed=1) if p[1] == "ranges" or (scattered and not p[0].startswith("list"))]


def timed(pkg, a):
    N = importlib.import_module("rust-local-rag_amd._native")
    L = N.lib()
    k, lam, dim = a.k, a.lam, a.dim
    cap = max(3 * max(k, 1), k + 10)
    sz = C.sizeof(N.SearchHitC)
    t0 = time.perf_counter()
    eng, names = build(pkg, a.rows, dim, seed=20261016 + a.rows)
    res = {"bench": "filtered_text_batch", "rows": a.rows, "dim": dim, "top_k": k, "lambda": lam, "calls": a.calls,
           "baseline": "N calls of rlr_engine_search_text_filtered, same process, legs alternating",
           "corpus_build_s": round(time.perf_counter() - t0, 1), "points": []}
    for name, kind, spec, m in scopes(a.rows, a.scattered, a.small):
        f = make_filter(eng.index, kind, spec)
        for nq in a.queries:
            qs, toks = queries(eng, names, nq, dim, seed=nq)
            blob = b"".join(toks)
            offs = np.zeros(nq + 1, np.uint64)
            offs[1:] = np.cumsum([len(t) for t in toks])
            hits_b, hits_s = (N.SearchHitC * (cap * nq))(), (N.SearchHitC * (cap * nq))()
            n_b, n_s = np.zeros(nq, np.uint32), np.zeros(nq, np.uint32)
            info, one = N.TextBatchInfoC(), C.c_uint32()

            def batched():
                N.check(L.rlr_engine_search_text_batch_filtered(
                    eng.index.handle, eng.lexical._h, f.handle, qs.ctypes.data_as(N.f32p), dim, nq, blob, offs.ctypes.data_as(N.u64p),
                    k, lam, 0, None, hits_b, cap, n_b.ctypes.data_as(N.u32p), C.byref(info)))

            def loop():
                for q in range(nq):
                    view = (N.SearchHitC * cap).from_buffer(hits_s, q * cap * sz)
                    N.check(L.rlr_engine_search_text_filtered(eng.index.handle, eng.lexical._h, f.handle, qs[q].ctypes.data_as(N.f32p),
                                                              dim, toks[q], len(toks[q]), k, lam, 0, None, view, cap, C.byref(one)))
                    n_s[q] = one.value

            loop()
            batched()
            assert np.array_equal(n_b, n_s), f"{name} x {nq}: hit counts differ"
            rb = np.frombuffer(hits_b, dtype=np.uint8).reshape(nq, cap * sz)
            rs = np.frombuffer(hits_s, dtype=np.uint8).reshape(nq, cap * sz)
            for q in range(nq):
                assert np.array_equal(rb[q, :n_b[q] * sz], rs[q, :n_s[q] * sz]), f"{name} x {nq}: query {q} differs"
            for _ in range(WARM):
                loop()
                batched()
            tn, ta, tb = [], [], []
            for _ in range(a.calls):
                t = time.perf_counter(); loop(); ta.append(time.perf_counter() - t)
                t = time.perf_counter(); batched(); tn.append(time.perf_counter() - t)
                t = time.perf_counter(); loop(); tb.append(time.perf_counter() - t)
            ms = 1e3 * float(np.median(tn))
            la, lb, b = 1e3 * float(np.median(ta)), 1e3 * float(np.median(tb)), 1e3 * float(np.median(ta + tb))
            spread = abs(la - lb)
            p = {"point": name, "n_allowed": m, "queries": nq, "batched_ms": round(ms, 4),
                 "p10_ms": round(1e3 * float(np.percentile(tn, 10)), 4), "p90_ms": round(1e3 * float(np.percentile(tn, 90)), 4),
                 "loop_ms": round(b, 4), "loop_legs_ms": [round(la, 4), round(lb, 4)], "loop_spread_ms": round(spread, 4),
                 "ratio_to_loop": round(ms / b, 3), "gain": bool(ms < b - spread), "loss": bool(ms > b + spread),
                 "info": {nm: int(getattr(info, nm)) for nm, _ in N.TextBatchInfoC._fields_}}
            res["points"].append(p)
            print(json.dumps(p), file=sys.stderr, flush=True)
        f.close()
    eng.close()
    return res


def trace_run(pkg, a):
    eng, names = build(pkg, a.rows, a.dim, seed=20261016 + a.rows)
    _, toks = queries(eng, names, TRACE_QUERIES, a.dim, seed=TRACE_QUERIES)
    texts = [t.decode() for t in toks]
    limit = 5 * max(3 * a.k, a.k + 10)
    plan = {"rows": a.rows, "queries": TRACE_QUERIES, "limit": limit, "per_point": WARM + TRACE_CALLS, "keep": TRACE_CALLS, "points": []}
    for _ in range(WARM + TRACE_CALLS):
        eng.lexical.score_batch(texts, limit)
    for name, kind, spec, m in scopes(a.rows, False):
        if float(name.split("_")[1]) not in TRACE_FRACTIONS:
            continue
        with make_filter(eng.index, kind, spec) as f:
            for _ in range(WARM + TRACE_CALLS):
                eng.lexical.score_batch(texts, limit, filter=f)
        plan["points"].append({"point": name, "n_allowed": m})
    eng.close()
    return plan


def parse_trace(a):
    with open(a.plan) as f:
        plan = json.load(f)
    files = glob.glob(os.path.join(a.parse_trace, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        raise SystemExit(f"no *kernel_trace.csv under {a.parse_trace}")
    plain, masked = [], []
    for path in files:
        with open(path, newline="") as f:
            for r in csv.DictReader(f):
                name = r.get("Kernel_Name", "")
                if "bm25_batch_kernel" not in name:
                    continue
                t0, t1 = int(r["Start_Timestamp"]), int(r["End_Timestamp"])
                (masked if ("<true>" in name or "ILb1E" in name) else plain).append((t0, (t1 - t0) / 1e3))
    plain.sort()
    masked.sort()
    per, keep = plan["per_point"], plan["keep"]
    if len(plain) != per or len(masked) != per * len(plan["points"]):
        raise SystemExit(f"{len(plain)} unmasked and {len(masked)} masked launches in the trace, the plan has {per} and "
                         f"{per * len(plan['points'])}")
    out = {"bench": "filtered_text_batch_kernels", "rows": plan["rows"], "queries": plan["queries"], "limit": plan["limit"],
           "bm25_batch_kernel_false_us": round(float(np.median([d for _, d in plain[-keep:]])), 2), "points": []}
    for i, p in enumerate(plan["points"]):
        us = float(np.median([d for _, d in masked[i * per + (per - keep):(i + 1) * per]]))
        out["points"].append({"point": p["point"], "n_allowed": p["n_allowed"], "bm25_batch_kernel_true_us": round(us, 2)})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--queries", type=int, nargs="+", default=[2, 4, 8, 32])
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--lam", type=float, default=0.3)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--scattered", action="store_true")
    ap.add_argument("--small", action="store_true", help="only the scopes of 256 and 4096 scattered rows")
    ap.add_argument("--trace-run", action="store_true")
    ap.add_argument("--parse-trace", default=None)
    ap.add_argument("--plan", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.parse_trace:
        result = parse_trace(a)
    else:
        pkg = load()
        if pkg.device_count() < 1:
            raise SystemExit("bench_filtered_text needs a GPU: the library has no CPU path")
        result = trace_run(pkg, a) if a.trace_run else timed(pkg, a)
    line = json.dumps(result)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
