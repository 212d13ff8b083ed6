"""The per-document cap inside hybrid, diversified search on the device against the host's way to the same answer.

    python tools/bench_capped.py [--calls 15] [--out FILE] [--small-only]

Corpora: f32 rows of 768 elements filled on the device (rlr_index_fill_synthetic, seeded, 64 clusters), every row with a
text of 4..12 words from a Zipf vocabulary of 50 000 words in the GPU LexicalIndex:
  100 k rows in 100 documents of 1000 consecutive rows; 1 M rows in 1000 documents; and the 1 M corpus SKEWED -- the
  200 000 rows nearest the query re-tagged as one document, so that the plain ranking is one document deep.
The request: a query embedding (a stored row) with a query text of three words, diversity 0.3, default weights.  Per corpus,
top_k = 5 and 100 and per_document 1 and 3, three sides, alternating call by call, warm, host clock around calls that
return after their device synchronisation; median and p10 / p90 of `calls` calls:
  (a) capped     rlr_engine_search_text_capped: BM25, one scan, the cap in combined order and the MMR chain on the device
  (b) host       what a host does without it: BM25 once (the same pairs), then rlr_engine_search at stage 0 with top_k'
                 doubling from twice the pool, a cap walk in numpy over the host's own id table, again until the pool
                 (max(3 top_k, top_k + 10) rows) survives or top_k' reaches the corpus; then rlr_mmr_select over the pool
  (c) uncapped   rlr_engine_search_text: the floor -- (a) - (c) is the price of the cap
(a) and (b) are checked to return the same rows.  `forms` = rlr_index_capped_forms over the timed calls of (a).  (a) counts
as faster when its median lies below (b)'s by more than (b)'s own p10..p90 spread; a cell where it does not is marked
`loss`.  One JSON line on stdout."""
from __future__ import annotations

import argparse
import ctypes as C
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
VOCAB = 50_000
LAM = 0.3


def stats(t):
    t = 1e3 * np.asarray(t)
    return {"ms": round(float(np.median(t)), 4), "p10_ms": round(float(np.percentile(t, 10)), 4),
            "p90_ms": round(float(np.percentile(t, 90)), 4)}


def zipf_words(rng, n):
    w = 1.0 / np.arange(1, VOCAB + 1)
    cdf = np.cumsum(w / w.sum())
    return np.minimum(np.searchsorted(cdf, rng.random(n)), VOCAB - 1)


def cap_walk(rows, ids, need, m):
    """rows in result order -> the first `need` of them with at most m per document (untagged rows are never capped)"""
    d = ids[rows.astype(np.int64)]
    o = np.argsort(d, kind="stable")
    ds = d[o]
    start = np.r_[0, np.flatnonzero(ds[1:] != ds[:-1]) + 1]
    rank = np.empty(d.size, np.int64)
    rank[o] = np.arange(d.size) - np.repeat(start, np.diff(np.r_[start, d.size]))
    return np.flatnonzero((rank < m) | (d == DOC_NONE))[:need]


class Sides:
    def __init__(self, pkg, ix, lex, q, tokens, ids):
        self.N, self.L = pkg._native, pkg._native.lib()
        self.ix, self.lex, self.q, self.tok, self.ids, self.n = ix, lex, q, tokens, ids, len(ix)
        self.hit = np.dtype([("row", "<u8"), ("score", "<f4"), ("embedding_score", "<f4"), ("lexical_score", "<f4"),
                             ("initial_score", "<f4")])

    def _hits(self, cap):
        return (self.N.SearchHitC * cap)(), C.c_uint32()

    def capped(self, top_k, m):
        hits, n = self._hits(max(3 * top_k, top_k + 10))
        self.N.check(self.L.rlr_engine_search_text_capped(self.ix.handle, self.lex._h, None, self.q.ctypes.data_as(self.N.f32p),
                                                          self.q.size, self.tok, len(self.tok), top_k, LAM, 0, None, m, hits,
                                                          len(hits), C.byref(n)))
        return np.frombuffer(hits, dtype=self.hit, count=n.value)["row"].copy()

    def uncapped(self, top_k):
        hits, n = self._hits(max(3 * top_k, top_k + 10))
        self.N.check(self.L.rlr_engine_search_text(self.ix.handle, self.lex._h, self.q.ctypes.data_as(self.N.f32p), self.q.size,
                                                   self.tok, len(self.tok), top_k, LAM, 0, None, hits, len(hits), C.byref(n)))
        return np.frombuffer(hits, dtype=self.hit, count=n.value)["row"].copy()

    def host(self, top_k, m):
        N = self.N
        pool = min(self.n, max(3 * top_k, top_k + 10))
        lr, ls = self.lex.score_tokens(self.tok.decode().split(), 5 * pool)
        o = np.argsort(lr, kind="stable")
        lr, ls = np.ascontiguousarray(lr[o]), np.ascontiguousarray(ls[o])
        kk, fetches = 2 * pool, 0
        while True:
            kk = min(kk, self.n)
            hits, n = self._hits(kk)
            N.check(self.L.rlr_engine_search(self.ix.handle, self.q.ctypes.data_as(N.f32p), self.q.size, kk, None,
                                             lr.ctypes.data_as(N.u64p) if lr.size else None,
                                             ls.ctypes.data_as(N.f32p) if ls.size else None, lr.size, 0, hits, kk, C.byref(n)))
            fetches += 1
            got = np.frombuffer(hits, dtype=self.hit, count=n.value)
            keep = cap_walk(got["row"], self.ids, pool, m)
            if keep.size >= pool or kk >= self.n:
                break
            kk *= 2
        rows, scores = got["row"][keep].copy(), got["score"][keep].copy()
        order, _ = self.ix.mmr_select(rows, scores, top_k, LAM)
        return rows[order], fetches, kk


def build(pkg, n, docs):
    ix = pkg.GpuIndex(768)
    ix.fill_synthetic(n, seed=20261021 + n, n_clusters=64)
    lex = pkg.LexicalIndex()
    rng = np.random.default_rng(n)
    lens = rng.integers(4, 13, size=n)
    words = zipf_words(rng, int(lens.sum()))
    names = [f"w{i:05d}" for i in range(VOCAB)]
    at = 0
    for r in range(n):
        m = int(lens[r])
        lex.add_tokens(r, [names[w] for w in words[at:at + m]])
        at += m
    ids = (np.arange(n) // (n // docs)).astype(np.uint32)
    q = ix.fetch_rows([n // 3])[0]
    q = (q / np.linalg.norm(q)).astype(np.float32)
    tokens = " ".join(names[w] for w in (3, 40, 700)).encode()
    return ix, lex, ids, q, tokens


def run_corpus(pkg, name, ix, lex, ids, q, tokens, calls):
    ix.set_documents(ids)
    s = Sides(pkg, ix, lex, q, tokens, ids)
    cells = []
    for top_k in (5, 100):
        for m in (1, 3):
            a = lambda: s.capped(top_k, m)
            b = lambda: s.host(top_k, m)
            c = lambda: s.uncapped(top_k)
            ra, (rb, fetches, k_last) = a(), b()
            assert np.array_equal(ra, rb), (name, top_k, m, "the capped call and the host's way disagree", ra[:8], rb[:8])
            for _ in range(WARM):
                a(); b(); c()
            ix.capped_forms(reset=True)
            ta, tb, tc = [], [], []
            for _ in range(calls):
                t0 = time.perf_counter(); a(); ta.append(time.perf_counter() - t0)
                t0 = time.perf_counter(); b(); tb.append(time.perf_counter() - t0)
                t0 = time.perf_counter(); c(); tc.append(time.perf_counter() - t0)
            forms = ix.capped_forms()
            sa, sb, sc = stats(ta), stats(tb), stats(tc)
            spread = sb["p90_ms"] - sb["p10_ms"]
            cell = {"corpus": name, "rows": len(ix), "top_k": top_k, "per_document": m, "diversity": LAM, "capped": sa, "host": sb,
                    "uncapped": sc, "host_fetches": fetches, "host_last_k": k_last, "forms": forms,
                    "price_of_the_cap_ms": round(sa["ms"] - sc["ms"], 4), "speedup_over_host": round(sb["ms"] / sa["ms"], 2),
                    "faster_beyond_spread": bool(sa["ms"] < sb["ms"] - spread)}
            cell["loss"] = not cell["faster_beyond_spread"]
            cells.append(cell)
            print(json.dumps(cell), file=sys.stderr, flush=True)
    return cells


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=15)
    ap.add_argument("--out", default=None)
    ap.add_argument("--small-only", action="store_true", help="the 100 k corpus alone")
    a = ap.parse_args()
    pkg = importlib.import_module("rust-local-rag_amd")
    if pkg.device_count() < 1:
        raise SystemExit("bench_capped needs a GPU: the library has no CPU path")
    res = {"bench": "capped", "dim": 768, "calls": a.calls, "cells": []}
    ix, lex, ids, q, tokens = build(pkg, 100_000, 100)
    res["cells"] += run_corpus(pkg, "100k_100_documents", ix, lex, ids, q, tokens, a.calls)
    ix.close(); lex.close()
    if not a.small_only:
        ix, lex, ids, q, tokens = build(pkg, 1_000_000, 1000)
        res["cells"] += run_corpus(pkg, "1M_1000_documents", ix, lex, ids, q, tokens, a.calls)
        near, _ = ix.search_topk(q, 200_000)
        ids = ids.copy()
        ids[near[0].astype(np.int64)] = 1_000_000
        res["cells"] += run_corpus(pkg, "1M_skewed_200k_document", ix, lex, ids, q, tokens, a.calls)
        ix.close(); lex.close()
    res["forms_total"] = [int(sum(c["forms"][i] for c in res["cells"])) for i in range(4)]
    res["losses"] = [(c["corpus"], c["top_k"], c["per_document"]) for c in res["cells"] if c["loss"]]
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
