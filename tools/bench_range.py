"""Range search on the device against the host's way to the same answer.

    python tools/bench_range.py [--calls 15] [--out FILE] [--small-only]

Corpora: f32 rows of 768 elements filled on the device (rlr_index_fill_synthetic, seeded, 64 clusters): 100 k rows and
1 M rows, the query a stored row.  Per corpus a threshold tau for about 10, 100, 1 000 and 20 000 hits (found by
bisection over count_range), and one cell inside a document filter (every tenth document of 1000 rows, about 100 hits).
Per cell four sides, alternating call by call, warm, host clock around calls that return after their device
synchronisation; median and p10 / p90 of `calls` calls:
  (a)  range     GpuIndex.search_range with a cap above the hits (rlr_search_range)
  (a') count     GpuIndex.count_range: the count alone, nothing fetched
  (b)  host      what a host does without it: search_topk with k doubling from 100 until the k-th score < tau (or k
                 reaches the rows); `host_fetches` calls.  It still has no count beyond what it fetched.
  (c)  plain     search_topk at k = the number of hits, where the plain path accepts that k: the floor
(a) and (b) are checked to return the same rows.  `forms` = rlr_index_range_forms over the timed (a) and (a') calls.
(a) counts as faster when its median lies below (b)'s by more than (b)'s own p10..p90 spread; a cell where it does not
is marked `loss`.  One JSON line on stdout."""
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

WARM = 3
TARGETS = (10, 100, 1000, 20000)


def stats(t):
    t = 1e3 * np.asarray(t)
    return {"ms": round(float(np.median(t)), 4), "p10_ms": round(float(np.percentile(t, 10)), 4),
            "p90_ms": round(float(np.percentile(t, 90)), 4)}


def tau_for(ix, q, target, f=None):
    """a threshold with about `target` hits: bisection over the exact count"""
    lo, hi = -1.0, 1.0                                       # count(lo) >= target >= count(hi)
    for _ in range(40):
        mid = 0.5 * (lo + hi)
        n = ix.count_range(q, mid, filter=f)[0]
        if n >= target:
            lo = mid
        else:
            hi = mid
        if target <= n <= target + max(target // 20, 1):
            break
    return np.float32(lo)


def host_way(ix, q, tau, n_rows, f=None):
    k, fetches = 100, 0
    while True:
        k = min(k, n_rows)
        rows, cos = ix.search_topk(q, k, filter=f)
        fetches += 1
        below = np.flatnonzero(~(cos[0] >= tau))
        if below.size or k >= n_rows or rows.shape[1] < k:
            take = int(below[0]) if below.size else rows.shape[1]
            return rows[0, :take], fetches, k
        k *= 2


def run_cell(ix, name, n, q, tau, calls, f=None, n_allowed=None):
    n_allowed = n if n_allowed is None else n_allowed
    hits = ix.count_range(q, tau, filter=f)[0]
    cap = hits + 64
    a = lambda: ix.search_range(q, tau, cap, filter=f)[0]
    a0 = lambda: ix.count_range(q, tau, filter=f)
    b = lambda: host_way(ix, q, tau, n_allowed, f)
    try:
        ix.search_topk(q, max(hits, 1), filter=f)
        c = lambda: ix.search_topk(q, max(hits, 1), filter=f)
    except Exception:                                        # noqa: BLE001 (the plain path does not take this k)
        c = None
    ra, (rb, fetches, k_last) = a(), b()
    assert ra[2] == hits and np.array_equal(ra[0], rb), (name, hits, "the range call and the host's way disagree")
    for _ in range(WARM):
        a(); a0(); b()
        if c:
            c()
    ix.range_forms(reset=True)
    ta, ta0, tb, tc = [], [], [], []
    for _ in range(calls):
        t0 = time.perf_counter(); a(); ta.append(time.perf_counter() - t0)
        t0 = time.perf_counter(); a0(); ta0.append(time.perf_counter() - t0)
        t0 = time.perf_counter(); b(); tb.append(time.perf_counter() - t0)
        if c:
            t0 = time.perf_counter(); c(); tc.append(time.perf_counter() - t0)
    forms = ix.range_forms()
    sa, sa0, sb = stats(ta), stats(ta0), stats(tb)
    spread = sb["p90_ms"] - sb["p10_ms"]
    cell = {"corpus": name, "rows": n, "filtered": f is not None, "allowed_rows": n_allowed, "tau": float(tau), "hits": hits,
            "cap": cap, "range": sa, "count": sa0, "host": sb, "plain": stats(tc) if c else None, "host_fetches": fetches,
            "host_last_k": k_last, "forms": forms, "only_form_0": forms == [2 * calls, 0, 0, 0],
            "added_to_plain_ms": round(sa["ms"] - stats(tc)["ms"], 4) if c else None,
            "speedup_over_host": round(sb["ms"] / sa["ms"], 2), "count_speedup_over_host": round(sb["ms"] / sa0["ms"], 2),
            "faster_beyond_spread": bool(sa["ms"] < sb["ms"] - spread)}
    cell["loss"] = not cell["faster_beyond_spread"]
    print(json.dumps(cell), file=sys.stderr, flush=True)
    return cell


def run_corpus(pkg, name, n, calls):
    ix = pkg.GpuIndex(768)
    ix.fill_synthetic(n, seed=20261021 + n, n_clusters=64)
    q = ix.fetch_rows([n // 3])[0]
    q = (q / np.linalg.norm(q)).astype(np.float32)
    cells = [run_cell(ix, name, n, q, tau_for(ix, q, t), calls) for t in TARGETS]
    ids = (np.arange(n) // 1000).astype(np.uint32)
    ix.set_documents(ids)
    docs = np.unique(ids)[::10]
    with ix.filter_documents(docs) as f:
        n_allowed = int(np.isin(ids, docs).sum())
        cells.append(run_cell(ix, name, n, q, tau_for(ix, q, 100, f), calls, f, n_allowed))
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
        raise SystemExit("bench_range needs a GPU: the library has no CPU path")
    corpora = [("100k", 100_000)]
    if not a.small_only:
        corpora.append(("1M", 1_000_000))
    res = {"bench": "range", "dim": 768, "calls": a.calls, "cells": []}
    for name, n in corpora:
        res["cells"] += run_corpus(pkg, name, n, a.calls)
    res["only_form_0_everywhere"] = all(c["only_form_0"] for c in res["cells"])
    res["losses"] = [(c["corpus"], c["hits"], c["filtered"]) for c in res["cells"] if c["loss"]]
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
