"""Grouped top-k on the device against the host's way to the same answer.

    python tools/bench_grouped.py [--calls 15] [--out FILE] [--small-only]

Corpora: f32 rows of 768 elements filled on the device (rlr_index_fill_synthetic, seeded, 64 clusters):
  1 M rows in 1000 documents of 1000 consecutive rows; 100 k rows in 100 documents; and the 1 M corpus SKEWED -- the
  200 000 rows nearest the query re-tagged as one document, so that the plain ranking is one document deep.
Per corpus, k = 100 and per_document 1 and 3, three sides, alternating call by call, warm, host clock around calls that
return after their device synchronisation; median and p10 / p90 of `calls` calls:
  (a) grouped    GpuIndex.search_topk_grouped (rlr_search_topk_grouped)
  (b) host       what a host does without it: rlr_search_topk with k' doubling from 2 k, a cap walk in numpy over the
                 host's own id table, again until k rows are accepted (or k' reaches the corpus)
  (c) plain      rlr_search_topk at k: the floor the grouped call adds to
(a) and (b) are checked to return the same rows.  `round_ms` = ((a) at per_document 3 - (a) at per_document 1) / 2: the
added time of one more round of per-document maxima.  The form counters must show form 0 alone in every timed cell
(`forms`).  (a) counts as faster when its median lies below (b)'s by more than (b)'s own p10..p90 spread; a cell where it
does not is marked `loss`.  One JSON line on stdout."""
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

DOC_NONE = 0xFFFFFFFF
WARM = 3
K = 100


def stats(t):
    t = 1e3 * np.asarray(t)
    return {"ms": round(float(np.median(t)), 4), "p10_ms": round(float(np.percentile(t, 10)), 4),
            "p90_ms": round(float(np.percentile(t, 90)), 4)}


def cap_walk(rows, ids, k, m):
    """rows in result order -> the first k of them with at most m per document (untagged rows are never capped)"""
    d = ids[rows.astype(np.int64)]
    o = np.argsort(d, kind="stable")
    ds = d[o]
    start = np.r_[0, np.flatnonzero(ds[1:] != ds[:-1]) + 1]
    rank = np.empty(d.size, np.int64)
    rank[o] = np.arange(d.size) - np.repeat(start, np.diff(np.r_[start, d.size]))
    return rows[(rank < m) | (d == DOC_NONE)][:k]


def host_way(ix, q, ids, k, m, n):
    kk, fetches = 2 * k, 0
    while True:
        kk = min(kk, n)
        rows, _ = ix.search_topk(q, kk)
        fetches += 1
        got = cap_walk(rows[0], ids, k, m)
        if got.size >= k or kk >= n:
            return got, fetches, kk
        kk *= 2


def run_corpus(pkg, name, n, docs, calls, skew):
    ix = pkg.GpuIndex(768)
    ix.fill_synthetic(n, seed=20261020 + n, n_clusters=64)
    ids = (np.arange(n) // (n // docs)).astype(np.uint32)
    q = ix.fetch_rows([n // 3])[0]
    q = (q / np.linalg.norm(q)).astype(np.float32)
    if skew:
        near, _ = ix.search_topk(q, skew)
        ids[near[0].astype(np.int64)] = 1_000_000
    ix.set_documents(ids)
    cells = []
    for m in (1, 3):
        a = lambda: ix.search_topk_grouped(q, K, m)[0]
        b = lambda: host_way(ix, q, ids, K, m, n)
        c = lambda: ix.search_topk(q, K)
        ra, (rb, fetches, k_last) = a(), b()
        assert np.array_equal(ra[0], rb), (name, m, "the grouped call and the host's way disagree")
        for _ in range(WARM):
            a(); b(); c()
        ix.grouped_forms(reset=True)
        ta, tb, tc = [], [], []
        for _ in range(calls):
            t0 = time.perf_counter(); a(); ta.append(time.perf_counter() - t0)
            t0 = time.perf_counter(); b(); tb.append(time.perf_counter() - t0)
            t0 = time.perf_counter(); c(); tc.append(time.perf_counter() - t0)
        forms = ix.grouped_forms()
        sa, sb, sc = stats(ta), stats(tb), stats(tc)
        spread = sb["p90_ms"] - sb["p10_ms"]
        cell = {"corpus": name, "rows": n, "per_document": m, "k": K, "grouped": sa, "host": sb, "plain": sc,
                "host_fetches": fetches, "host_last_k": k_last, "forms": forms, "only_form_0": forms == [calls, 0, 0, 0],
                "added_to_plain_ms": round(sa["ms"] - sc["ms"], 4), "speedup_over_host": round(sb["ms"] / sa["ms"], 2),
                "faster_beyond_spread": bool(sa["ms"] < sb["ms"] - spread)}
        cell["loss"] = not cell["faster_beyond_spread"]
        cells.append(cell)
        print(json.dumps(cell), file=sys.stderr, flush=True)
    round_ms = round((cells[1]["grouped"]["ms"] - cells[0]["grouped"]["ms"]) / 2.0, 4)
    for cell in cells:
        cell["round_ms"] = round_ms
    ix.close()
    return cells


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=15)
    ap.add_argument("--out", default=None)
    ap.add_argument("--small-only", action="store_true", help="the 100 k corpus alone")
    a = ap.parse_args()
    pkg = importlib.import_module("rust-local-rag_amd")
    if pkg.device_count() < 1:
        raise SystemExit("bench_grouped needs a GPU: the library has no CPU path")
    corpora = [("100k_100_documents", 100_000, 100, 0)]
    if not a.small_only:
        corpora += [("1M_1000_documents", 1_000_000, 1000, 0), ("1M_skewed_200k_document", 1_000_000, 1000, 200_000)]
    res = {"bench": "grouped", "dim": 768, "calls": a.calls, "cells": []}
    for name, n, docs, skew in corpora:
        res["cells"] += run_corpus(pkg, name, n, docs, a.calls, skew)
    res["only_form_0_everywhere"] = all(c["only_form_0"] for c in res["cells"])
    res["losses"] = [(c["corpus"], c["per_document"]) for c in res["cells"] if c["loss"]]
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
