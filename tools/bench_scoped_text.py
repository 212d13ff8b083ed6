"""N text queries with a document scope EACH as ONE rlr_engine_search_text_batch_scoped call against N calls of
rlr_engine_search_text_filtered -- the way a request that is alone in its scope is served without the scoped call -- in the
same process, the legs alternating.

    python tools/bench_scoped_text.py [--rows 1000000] [--dim 768] [--queries 2 4 8 32] [--k 10] [--lam 0.3]
                                      [--calls 50] [--scopes NAME ...] [--out FILE]
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/bench_scoped_text.py --trace-run [--out PLAN]
    python tools/bench_scoped_text.py --parse-trace DIR --plan PLAN [--out FILE]

Corpus and queries: those of tools/bench_text_batch.py (f32 rows filled on the device, one Zipf text of 4..25 words per row
in the GPU LexicalIndex; a noisy copy of a stored row and 2..4 Zipf words per query).  Scope sets, one scope per query:
    disjoint_8th    contiguous ranges of 1/8 of the rows, query q in eighth q mod 8 (pairwise disjoint up to 8 queries)
    disjoint_80th   pairwise disjoint contiguous ranges of 1/80 of the rows each
    random_halves   an independent random half of the rows per query (heavy overlap: the union is nearly everything)
    identical       one range of 1/8 of the rows, the same filter object in every slot
Per (scope set, N): the results of both ways are compared first (hit counts, rows and every score bit), then WARM rounds,
then `calls` rounds of loop leg A | the scoped call | [the one-filter batched call, `identical` only] | loop leg B.
Reported: the median ms of each, the two loop legs' medians and their distance (the spread), the ratio, how the batch
served its queries (rlr_text_batch_info), `gain`: the scoped median lies below the loop's by more than the spread
(`loss`: above it by more than the spread), and for `identical` the same verdict against the one-filter call.  One JSON
line on stdout.
Trace mode: WARM + TRACE_CALLS calls of rlr_lexical_score_batch_scoped (8 queries) per scope set, for a profiler run of
its own; --parse-trace reads the kernel trace back: the median time of the scoped bm25_batch_kernel per scope set.
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

from bench_text_batch import build, load, queries  # noqa: E402

WARM, TRACE_CALLS, TRACE_QUERIES = 5, 20, 8
SCOPE_SETS = ["disjoint_8th", "disjoint_80th", "random_halves", "identical"]


def scope_filters(ix, name, n_rows, nq):
    """(the filter of every query slot, the filters to close, rows per scope)"""
    if name == "disjoint_8th":
        m = n_rows // 8
        own = [ix.filter_ranges([(e * m, m)]) for e in range(min(nq, 8))]
        return [own[q % 8] for q in range(nq)], own, m
    if name == "disjoint_80th":
        m = n_rows // 80
        fs = [ix.filter_ranges([(q * m, m)]) for q in range(nq)]
        return fs, fs, m
    if name == "identical":
        f = ix.filter_ranges([(n_rows // 3, n_rows // 8)])
        return [f] * nq, [f], n_rows // 8
    rng = np.random.default_rng(5)
    fs, total = [], 0
    for _ in range(nq):
        keep = np.flatnonzero(rng.random(n_rows) < 0.5)
        total += keep.size
        fs.append(ix.filter_rows(keep))
    return fs, fs, total // nq


def timed(pkg, a):
    N = importlib.import_module("rust-local-rag_amd._native")
    L = N.lib()
    k, lam, dim = a.k, a.lam, a.dim
    cap = max(3 * max(k, 1), k + 10)
    sz = C.sizeof(N.SearchHitC)
    t0 = time.perf_counter()
    eng, names = build(pkg, a.rows, dim, seed=20261016 + a.rows)
    res = {"bench": "scoped_text_batch", "rows": a.rows, "dim": dim, "top_k": k, "lambda": lam, "calls": a.calls,
           "baseline": "N calls of rlr_engine_search_text_filtered with filters[q], same process, legs alternating",
           "corpus_build_s": round(time.perf_counter() - t0, 1), "points": []}
    for name in a.scopes:
        for nq in a.queries:
            fs, close, per_scope = scope_filters(eng.index, name, a.rows, nq)
            handles = (C.c_void_p * nq)(*[f.handle for f in fs])
            qs, toks = queries(eng, names, nq, dim, seed=nq)
            blob = b"".join(toks)
            offs = np.zeros(nq + 1, np.uint64)
            offs[1:] = np.cumsum([len(t) for t in toks])
            hits_b, hits_s, hits_f = ((N.SearchHitC * (cap * nq))() for _ in range(3))
            n_b, n_s, n_f = (np.zeros(nq, np.uint32) for _ in range(3))
            info, one = N.TextBatchInfoC(), C.c_uint32()
            tail = (qs.ctypes.data_as(N.f32p), dim, nq, blob, offs.ctypes.data_as(N.u64p), k, lam, 0, None)

            def scoped():
                N.check(L.rlr_engine_search_text_batch_scoped(eng.index.handle, eng.lexical._h, handles, *tail, hits_b, cap,
                                                              n_b.ctypes.data_as(N.u32p), C.byref(info)))

            def one_filter():                                    # (`identical` only: every slot holds fs[0])
                N.check(L.rlr_engine_search_text_batch_filtered(eng.index.handle, eng.lexical._h, fs[0].handle, *tail, hits_f, cap,
                                                                n_f.ctypes.data_as(N.u32p), None))

            def loop():
                for q in range(nq):
                    view = (N.SearchHitC * cap).from_buffer(hits_s, q * cap * sz)
                    N.check(L.rlr_engine_search_text_filtered(eng.index.handle, eng.lexical._h, fs[q].handle,
                                                              qs[q].ctypes.data_as(N.f32p), dim, toks[q], len(toks[q]), k, lam, 0, None,
                                                              view, cap, C.byref(one)))
                    n_s[q] = one.value

            identical = name == "identical"
            loop()
            scoped()
            others = [("scoped", hits_b, n_b)]
            if identical:
                one_filter()
                others.append(("one filter", hits_f, n_f))
            rs = np.frombuffer(hits_s, dtype=np.uint8).reshape(nq, cap * sz)
            for leg, h, n in others:
                assert np.array_equal(n, n_s), f"{name} x {nq}: {leg}: hit counts differ"
                rb = np.frombuffer(h, dtype=np.uint8).reshape(nq, cap * sz)
                for q in range(nq):
                    assert np.array_equal(rb[q, :n[q] * sz], rs[q, :n_s[q] * sz]), f"{name} x {nq}: {leg}: query {q} differs"
            for _ in range(WARM):
                loop()
                scoped()
                if identical:
                    one_filter()
            tn, ta, tb, tf = [], [], [], []
            for _ in range(a.calls):
                t = time.perf_counter(); loop(); ta.append(time.perf_counter() - t)
                t = time.perf_counter(); scoped(); tn.append(time.perf_counter() - t)
                if identical:
                    t = time.perf_counter(); one_filter(); tf.append(time.perf_counter() - t)
                t = time.perf_counter(); loop(); tb.append(time.perf_counter() - t)
            ms = 1e3 * float(np.median(tn))
            la, lb, b = 1e3 * float(np.median(ta)), 1e3 * float(np.median(tb)), 1e3 * float(np.median(ta + tb))
            spread = abs(la - lb)
            p = {"scopes": name, "rows_per_scope": per_scope, "queries": nq, "scoped_ms": round(ms, 4),
                 "p10_ms": round(1e3 * float(np.percentile(tn, 10)), 4), "p90_ms": round(1e3 * float(np.percentile(tn, 90)), 4),
                 "loop_ms": round(b, 4), "loop_legs_ms": [round(la, 4), round(lb, 4)], "loop_spread_ms": round(spread, 4),
                 "ratio_to_loop": round(ms / b, 3), "gain": bool(ms < b - spread), "loss": bool(ms > b + spread),
                 "info": {nm: int(getattr(info, nm)) for nm, _ in N.TextBatchInfoC._fields_}}
            if identical:
                f_ms = 1e3 * float(np.median(tf))
                p.update({"one_filter_ms": round(f_ms, 4), "ratio_to_one_filter": round(ms / f_ms, 3),
                          "gain_vs_one_filter": bool(ms < f_ms - spread), "loss_vs_one_filter": bool(ms > f_ms + spread)})
            res["points"].append(p)
            print(json.dumps(p), file=sys.stderr, flush=True)
            for f in close:
                f.close()
    eng.close()
    return res


def trace_run(pkg, a):
    eng, names = build(pkg, a.rows, a.dim, seed=20261016 + a.rows)
    _, toks = queries(eng, names, TRACE_QUERIES, a.dim, seed=TRACE_QUERIES)
    texts = [t.decode() for t in toks]
    limit = 5 * max(3 * a.k, a.k + 10)
    plan = {"rows": a.rows, "queries": TRACE_QUERIES, "limit": limit, "per_point": WARM + TRACE_CALLS, "keep": TRACE_CALLS, "points": []}
    for name in a.scopes:
        fs, close, per_scope = scope_filters(eng.index, name, a.rows, TRACE_QUERIES)
        for _ in range(WARM + TRACE_CALLS):
            eng.lexical.score_batch(texts, limit, filters=fs)
        plan["points"].append({"scopes": name, "rows_per_scope": per_scope})
        for f in close:
            f.close()
    eng.close()
    return plan


def parse_trace(a):
    with open(a.plan) as f:
        plan = json.load(f)
    files = glob.glob(os.path.join(a.parse_trace, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        raise SystemExit(f"no *kernel_trace.csv under {a.parse_trace}")
    scoped = []
    for path in files:
        with open(path, newline="") as f:
            for r in csv.DictReader(f):
                name = r.get("Kernel_Name", "")
                if "bm25_batch_kernel" in name and ("<true, true>" in name or "ILb1ELb1E" in name):
                    t0, t1 = int(r["Start_Timestamp"]), int(r["End_Timestamp"])
                    scoped.append((t0, (t1 - t0) / 1e3))
    scoped.sort()
    per, keep = plan["per_point"], plan["keep"]
    if len(scoped) != per * len(plan["points"]):
        raise SystemExit(f"{len(scoped)} scoped launches in the trace, the plan has {per * len(plan['points'])}")
    out = {"bench": "scoped_text_batch_kernels", "rows": plan["rows"], "queries": plan["queries"], "limit": plan["limit"], "points": []}
    for i, p in enumerate(plan["points"]):
        us = float(np.median([d for _, d in scoped[i * per + (per - keep):(i + 1) * per]]))
        out["points"].append({"scopes": p["scopes"], "rows_per_scope": p["rows_per_scope"], "bm25_batch_kernel_scoped_us": round(us, 2)})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--queries", type=int, nargs="+", default=[2, 4, 8, 32])
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--lam", type=float, default=0.3)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--scopes", nargs="+", default=SCOPE_SETS, choices=SCOPE_SETS)
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
            raise SystemExit("bench_scoped_text needs a GPU: the library has no CPU path")
        result = trace_run(pkg, a) if a.trace_run else timed(pkg, a)
    line = json.dumps(result)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
