"""Batched grouped top-k: the queries of a call sharing passes over the rows, against the same queries one by one.

    python tools/bench_grouped_batch.py [--calls 15] [--out profiles/grouped_batch_bench.json] [--small-only] [--max-queries N]

Corpora (those of tools/bench_grouped.py): f32 rows of 768 elements filled on the device (rlr_index_fill_synthetic,
seeded, 64 clusters): 100 k rows in 100 documents of consecutive rows; 1 M rows in 1000 documents; and the 1 M corpus
SKEWED -- the 200 000 rows nearest the first query re-tagged as one document.  The queries are stored rows.  Per corpus,
k = 100, per_document 1 and 3, and 2, 4, 8, 32 and 256 queries, three sides, alternating call by call, warm, a host clock
around whole calls through the Python layer (each returns after its device synchronisation); median and p10 / p90 of
`calls` calls:
  (a2)  search_topk_grouped_batch with sharing forced (rlr_index_set_grouped_sharing mode 2)
  (a0)  search_topk_grouped_batch in the default mode 0 (the gate decides)
  (b)   search_topk_grouped with the same queries: one by one, the behaviour without this entry
All three are checked to return the same rows, scores and document ids.  `forms_*` = rlr_index_grouped_batch_forms over
the timed calls of that side.  A side counts as slower than (b) only when its p10..p90 range lies wholly above (b)'s:
`mode0_slower` must be false in every cell, or mode 0 must have declined there (`mode0_declined`).  One JSON line on
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
K = 100
BATCHES = (2, 4, 8, 32, 256)
PER_DOCUMENT = (1, 3)


def stats(t):
    t = 1e3 * np.asarray(t)
    return {"ms": round(float(np.median(t)), 4), "p10_ms": round(float(np.percentile(t, 10)), 4),
            "p90_ms": round(float(np.percentile(t, 90)), 4)}


def same(x, y):
    return all(np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)) and
               np.array_equal(a[2], b[2]) for a, b in zip(x, y))


def run_cell(ix, name, n, qs, m, calls):
    nq = qs.shape[0]

    def side(mode):
        def call():
            ix.set_grouped_sharing(mode)
            return ix.search_topk_grouped_batch(qs, K, m)
        return call

    a2, a0 = side(2), side(0)
    b = lambda: ix.search_topk_grouped(qs, K, m)
    r2, r0, rb = a2(), a0(), b()
    assert same(r2, rb) and same(r0, rb), (name, nq, m, "the batched call and the one-by-one calls disagree")
    for _ in range(WARM):
        a2(); a0(); b()
    t2, t0, tb = [], [], []
    forms = {2: np.zeros(4, np.int64), 0: np.zeros(4, np.int64)}
    for _ in range(calls):
        for mode, fn, ts in ((2, a2, t2), (0, a0, t0)):
            ix.grouped_batch_forms(reset=True)
            s = time.perf_counter(); fn(); ts.append(time.perf_counter() - s)
            forms[mode] += np.asarray(ix.grouped_batch_forms())
        s = time.perf_counter(); b(); tb.append(time.perf_counter() - s)
    s2, s0, sb = stats(t2), stats(t0), stats(tb)
    cell = {"corpus": name, "rows": n, "queries": nq, "per_document": m, "k": K,
            "mode2": s2, "mode0": s0, "one_by_one": sb, "forms_mode2": forms[2].tolist(), "forms_mode0": forms[0].tolist(),
            "per_query_ms": {"mode2": round(s2["ms"] / nq, 4), "mode0": round(s0["ms"] / nq, 4), "one_by_one": round(sb["ms"] / nq, 4)},
            "speedup_mode2": round(sb["ms"] / s2["ms"], 2), "speedup_mode0": round(sb["ms"] / s0["ms"], 2),
            "mode2_slower": bool(s2["p10_ms"] > sb["p90_ms"]), "mode0_slower": bool(s0["p10_ms"] > sb["p90_ms"]),
            "mode0_declined": bool(forms[0][3] == nq * calls)}
    print(json.dumps(cell), file=sys.stderr, flush=True)
    return cell


def run_corpus(pkg, name, n, docs, calls, max_queries, skew):
    ix = pkg.GpuIndex(768)
    ix.fill_synthetic(n, seed=20261020 + n, n_clusters=64)
    ids = (np.arange(n) // (n // docs)).astype(np.uint32)
    pick = (np.arange(max(BATCHES)) * 7919 + n // 3) % n
    pool = ix.fetch_rows(pick)
    pool = (pool / np.linalg.norm(pool, axis=1, keepdims=True)).astype(np.float32)
    if skew:
        near, _ = ix.search_topk(pool[0], skew)
        ids[near[0].astype(np.int64)] = 1_000_000
    ix.set_documents(ids)
    cells = [run_cell(ix, name, n, pool[:nq], m, calls) for m in PER_DOCUMENT for nq in BATCHES if nq <= max_queries]
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
        raise SystemExit("bench_grouped_batch needs a GPU: the library has no CPU path")
    corpora = [("100k_100_documents", 100_000, 100, 0)]
    if not a.small_only:
        corpora += [("1M_1000_documents", 1_000_000, 1000, 0), ("1M_skewed_200k_document", 1_000_000, 1000, 200_000)]
    res = {"bench": "grouped_batch", "dim": 768, "k": K, "calls": a.calls, "cells": []}
    for name, n, docs, skew in corpora:
        res["cells"] += run_corpus(pkg, name, n, docs, a.calls, a.max_queries, skew)
    key = lambda c: (c["corpus"], c["queries"], c["per_document"])
    res["mode0_slower_cells"] = [key(c) for c in res["cells"] if c["mode0_slower"] and not c["mode0_declined"]]
    res["mode2_slower_cells"] = [key(c) for c in res["cells"] if c["mode2_slower"]]
    res["mode0_declined_cells"] = [key(c) for c in res["cells"] if c["mode0_declined"]]
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
