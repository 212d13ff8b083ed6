"""Batched range search: the queries of a call sharing passes over the rows, against the same queries one by one.

    python tools/bench_range_batch.py [--calls 15] [--out profiles/range_batch_bench.json] [--small-only] [--max-queries N]

Corpora: f32 rows of 768 elements filled on the device (rlr_index_fill_synthetic, seeded, 64 clusters): 100 k rows and
1 M rows; the queries are stored rows (an ingest batch checked for duplicates).  Per corpus and batch size (2, 8, 32, 256,
1024 queries) three thresholds PER QUERY: above every score (0 hits), and by bisection over the exact count about 10 and
about 1000 hits.  At 1 M rows also: the nomination image enabled, a document filter over a tenth of the rows, and the
count-only call.  Per cell three sides, alternating call by call, warm, a host clock around whole calls (each returns
after its device synchronisation); median and p10 / p90 of `calls` calls:
  (a2)  search_range_batch with sharing forced (rlr_index_set_range_sharing mode 2)
  (a0)  search_range_batch in the default mode 0 (the cost model decides)
  (b)   search_range with the same queries: one by one, the behaviour without this entry
All three are checked to return the same rows and totals.  `forms_*` = rlr_index_range_batch_forms over the timed calls of
that side.  A side counts as slower than (b) only when the p10..p90 ranges of the two are disjoint: `mode0_slower` must be
false in every cell, and where `mode2_slower` is true mode 0 must have declined (`mode0_declined`).  One JSON line on
stdout."""
from __future__ import annotations

import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WARM = 2
BATCHES = (2, 8, 32, 256, 1024)
TARGETS = (0, 10, 1000)


def stats(t):
    t = 1e3 * np.asarray(t)
    return {"ms": round(float(np.median(t)), 4), "p10_ms": round(float(np.percentile(t, 10)), 4),
            "p90_ms": round(float(np.percentile(t, 90)), 4)}


def taus_for(ix, qs, target, f=None):
    """one threshold per query with about `target` hits: bisection over the exact counts, all queries at once"""
    nq = qs.shape[0]
    if target == 0:
        return np.full(nq, 1.5, np.float32)
    lo, hi = np.full(nq, -1.0), np.full(nq, 1.01)            # count(lo) >= target > count(hi)
    for _ in range(24):
        mid = 0.5 * (lo + hi)
        n = np.asarray(ix.count_range_batch(qs, mid.astype(np.float32), filter=f))
        ge = n >= target
        lo, hi = np.where(ge, mid, lo), np.where(ge, hi, mid)
    return lo.astype(np.float32)


def same(x, y):
    return all(np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)) and a[2] == b[2]
               for a, b in zip(x, y))


def run_cell(ix, name, n, qs, target, calls, f=None, n_allowed=None, image=False, count_only=False):
    nq = qs.shape[0]
    ix.set_range_sharing(2)
    taus = taus_for(ix, qs, target, f)
    hits = np.asarray(ix.count_range_batch(qs, taus, filter=f))
    cap = 0 if count_only else int(hits.max()) + 64

    def side(mode):
        def call():
            ix.set_range_sharing(mode)
            return ix.search_range_batch(qs, taus, cap, filter=f)
        return call

    a2, a0 = side(2), side(0)
    b = lambda: ix.search_range(qs, taus, cap, filter=f)
    r2, r0, rb = a2(), a0(), b()
    assert same(r2, rb) and same(r0, rb), (name, nq, target, "the batched call and the one-by-one calls disagree")
    for _ in range(WARM):
        a2(); a0(); b()
    t2, t0, tb = [], [], []
    forms = {2: np.zeros(4, np.int64), 0: np.zeros(4, np.int64)}
    for _ in range(calls):
        for mode, fn, ts in ((2, a2, t2), (0, a0, t0)):
            ix.range_batch_forms(reset=True)
            s = time.perf_counter(); fn(); ts.append(time.perf_counter() - s)
            forms[mode] += np.asarray(ix.range_batch_forms())
        s = time.perf_counter(); b(); tb.append(time.perf_counter() - s)
    s2, s0, sb = stats(t2), stats(t0), stats(tb)
    cell = {"corpus": name, "rows": n, "queries": nq, "target_hits": target, "hits_median": int(np.median(hits)),
            "hits_max": int(hits.max()), "cap": cap, "image": image, "filtered": f is not None,
            "allowed_rows": n if n_allowed is None else n_allowed, "count_only": count_only,
            "mode2": s2, "mode0": s0, "one_by_one": sb, "forms_mode2": forms[2].tolist(), "forms_mode0": forms[0].tolist(),
            "speedup_mode2": round(sb["ms"] / s2["ms"], 2), "speedup_mode0": round(sb["ms"] / s0["ms"], 2),
            "mode2_slower": bool(s2["p10_ms"] > sb["p90_ms"]), "mode0_slower": bool(s0["p10_ms"] > sb["p90_ms"]),
            "mode0_declined": bool(forms[0][3] == nq * calls)}
    print(json.dumps(cell), file=sys.stderr, flush=True)
    return cell


def run_corpus(pkg, name, n, calls, max_queries, extras):
    ix = pkg.GpuIndex(768)
    ix.fill_synthetic(n, seed=20261021 + n, n_clusters=64)
    pick = (np.arange(max(BATCHES)) * 7919 + n // 3) % n
    pool = ix.fetch_rows(pick)
    pool = (pool / np.linalg.norm(pool, axis=1, keepdims=True)).astype(np.float32)
    batches = [b for b in BATCHES if b <= max_queries]
    cells = [run_cell(ix, name, n, pool[:nq], t, calls) for nq in batches for t in TARGETS]
    if extras:
        for nq in (8, 256):
            if nq <= max_queries:
                cells.append(run_cell(ix, name, n, pool[:nq], 10, calls, count_only=True))
        ids = (np.arange(n) // 1000).astype(np.uint32)
        ix.set_documents(ids)
        docs = np.unique(ids)[::10]
        with ix.filter_documents(docs) as f:
            n_allowed = int(np.isin(ids, docs).sum())
            for nq in (8, 256):
                if nq <= max_queries:
                    cells.append(run_cell(ix, name, n, pool[:nq], 10, calls, f, n_allowed))
        ix.enable_batch_image(True)
        for nq in (32, 256, 1024):
            if nq <= max_queries:
                cells.append(run_cell(ix, name, n, pool[:nq], 10, calls, image=True))
    ix.close()
    return cells


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=15)
    ap.add_argument("--out", default=None)
    ap.add_argument("--small-only", action="store_true", help="the 100 k corpus alone")
    ap.add_argument("--max-queries", type=int, default=max(BATCHES))
    a = ap.parse_args()
    pkg = importlib.import_module("rust-local-rag_amd")
    if pkg.device_count() < 1:
        raise SystemExit("bench_range_batch needs a GPU: the library has no CPU path")
    res = {"bench": "range_batch", "dim": 768, "calls": a.calls, "cells": []}
    res["cells"] += run_corpus(pkg, "100k", 100_000, a.calls, a.max_queries, extras=False)
    if not a.small_only:
        res["cells"] += run_corpus(pkg, "1M", 1_000_000, a.calls, a.max_queries, extras=True)
    key = lambda c: (c["corpus"], c["queries"], c["target_hits"], c["image"], c["filtered"], c["count_only"])
    res["mode0_slower_cells"] = [key(c) for c in res["cells"] if c["mode0_slower"]]
    res["mode2_slower_cells"] = [key(c) for c in res["cells"] if c["mode2_slower"]]
    res["mode2_slower_where_mode0_shared"] = [key(c) for c in res["cells"] if c["mode2_slower"] and not c["mode0_declined"]]
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
