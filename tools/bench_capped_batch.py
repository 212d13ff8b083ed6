"""Batched capped search: the requests of a call sharing passes over the rows, against the same requests one by one.

    python tools/bench_capped_batch.py [--calls 15] [--out profiles/capped_batch_bench.json] [--small-only] [--max-queries N]

Corpora (those of tools/bench_capped.py): f32 rows of 768 elements filled on the device (rlr_index_fill_synthetic, seeded,
64 clusters), every row with a text of 4..12 words from a Zipf vocabulary of 50 000 words in the GPU LexicalIndex: 100 k rows
in 100 documents of consecutive rows; 1 M rows in 1000 documents; and the 1 M corpus SKEWED -- the 200 000 rows nearest
the first query re-tagged as one document.  The requests: query embeddings (stored rows), each with a query text of three
words, diversity 0.3, default weights.  Per corpus, top_k = 5 and 100, per_document 1 and 3, and 2, 4, 8, 32 and 256
requests, three sides, alternating call by call, warm, a host clock around whole calls through the C ABI (each returns
after its device synchronisation); median and p10 / p90 of `calls` calls:
  (a2)  rlr_engine_search_text_capped_batch with sharing forced (rlr_index_set_capped_sharing mode 2)
  (a0)  rlr_engine_search_text_capped_batch in the default mode 0 (the gate decides)
  (b)   rlr_engine_search_text_capped for every request, one by one: unchanged code, the behaviour without this entry
All three are checked to return the same hits, field for field.  `forms_*` = rlr_index_capped_batch_forms over the timed
calls of that side.  A side counts as slower than (b) only when its p10..p90 range lies wholly above (b)'s: `mode0_slower`
must be false in every cell; where `mode2_slower` holds the gate must have declined (`mode0_declined`).  One JSON line on
stdout."""
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bench_capped as BC  # noqa: E402  (the corpora and the text of tools/bench_capped.py)

WARM = 2
LAM = BC.LAM
BATCHES = (2, 4, 8, 32, 256)
TOP_K = (5, 100)
PER_DOCUMENT = (1, 3)


class Sides:
    def __init__(self, pkg, ix, lex, qs, texts):
        self.N, self.L = pkg._native, pkg._native.lib()
        self.ix, self.lex, self.qs = ix, lex, np.ascontiguousarray(qs, np.float32)
        self.toks = texts
        self.off = np.zeros(len(texts) + 1, np.uint64)
        self.off[1:] = np.cumsum([len(t) for t in texts], dtype=np.uint64)
        self.blob = b"".join(texts)

    def batch(self, top_k, m):
        N, nq = self.N, self.qs.shape[0]
        cap = max(3 * top_k, top_k + 10)
        hits = (N.SearchHitC * (cap * nq))()
        n_out = np.zeros(nq, np.uint32)
        N.check(self.L.rlr_engine_search_text_capped_batch(self.ix.handle, self.lex._h, None, self.qs.ctypes.data_as(N.f32p),
                                                           self.qs.shape[1], nq, self.blob, self.off.ctypes.data_as(N.u64p), top_k,
                                                           LAM, 0, None, m, hits, cap, n_out.ctypes.data_as(N.u32p)))
        raw = np.frombuffer(hits, dtype=np.uint8).reshape(nq, cap * C.sizeof(N.SearchHitC))
        return [raw[i, :int(n_out[i]) * C.sizeof(N.SearchHitC)].tobytes() for i in range(nq)]

    def one_by_one(self, top_k, m):
        N = self.N
        cap = max(3 * top_k, top_k + 10)
        out = []
        for i in range(self.qs.shape[0]):
            hits, n = (N.SearchHitC * cap)(), C.c_uint32()
            N.check(self.L.rlr_engine_search_text_capped(self.ix.handle, self.lex._h, None, self.qs[i].ctypes.data_as(N.f32p),
                                                         self.qs.shape[1], self.toks[i], len(self.toks[i]), top_k, LAM, 0, None, m,
                                                         hits, cap, C.byref(n)))
            out.append(bytes(hits)[:n.value * C.sizeof(N.SearchHitC)])
        return out


def run_cell(pkg, ix, lex, name, n, qs, texts, top_k, m, calls):
    nq = qs.shape[0]
    s = Sides(pkg, ix, lex, qs, texts)

    def side(mode):
        def call():
            ix.set_capped_sharing(mode)
            return s.batch(top_k, m)
        return call

    a2, a0 = side(2), side(0)
    b = lambda: s.one_by_one(top_k, m)
    r2, r0, rb = a2(), a0(), b()
    assert r2 == rb and r0 == rb, (name, nq, top_k, m, "the batched call and the one-by-one calls disagree")
    for _ in range(WARM):
        a2(); a0(); b()
    t2, t0, tb = [], [], []
    forms = {2: np.zeros(4, np.int64), 0: np.zeros(4, np.int64)}
    for _ in range(calls):
        for mode, fn, ts in ((2, a2, t2), (0, a0, t0)):
            ix.capped_batch_forms(reset=True)
            t = time.perf_counter(); fn(); ts.append(time.perf_counter() - t)
            forms[mode] += np.asarray(ix.capped_batch_forms())
        t = time.perf_counter(); b(); tb.append(time.perf_counter() - t)
    s2, s0, sb = BC.stats(t2), BC.stats(t0), BC.stats(tb)
    cell = {"corpus": name, "rows": n, "queries": nq, "top_k": top_k, "per_document": m, "diversity": LAM,
            "mode2": s2, "mode0": s0, "one_by_one": sb, "forms_mode2": forms[2].tolist(), "forms_mode0": forms[0].tolist(),
            "per_query_ms": {"mode2": round(s2["ms"] / nq, 4), "mode0": round(s0["ms"] / nq, 4), "one_by_one": round(sb["ms"] / nq, 4)},
            "speedup_mode2": round(sb["ms"] / s2["ms"], 2), "speedup_mode0": round(sb["ms"] / s0["ms"], 2),
            "mode2_slower": bool(s2["p10_ms"] > sb["p90_ms"]), "mode0_slower": bool(s0["p10_ms"] > sb["p90_ms"]),
            "mode0_declined": bool(forms[0][3] == nq * calls)}
    print(json.dumps(cell), file=sys.stderr, flush=True)
    return cell


def run_corpus(pkg, name, ix, lex, ids, calls, max_queries, skew):
    n = len(ix)
    pick = (np.arange(max(BATCHES)) * 7919 + n // 3) % n
    pool = ix.fetch_rows(pick)
    pool = (pool / np.linalg.norm(pool, axis=1, keepdims=True)).astype(np.float32)
    words = (np.arange(max(BATCHES))[:, None] * np.array([3, 41, 701]) + np.array([3, 40, 700])) % 2000  # frequent words: every text has postings
    texts = [" ".join(f"w{w:05d}" for w in ws).encode() for ws in words]
    if skew:
        near, _ = ix.search_topk(pool[0], skew)
        ids = ids.copy()
        ids[near[0].astype(np.int64)] = 1_000_000
    ix.set_documents(ids)
    return [run_cell(pkg, ix, lex, name, n, pool[:nq], texts[:nq], top_k, m, calls)
            for top_k in TOP_K for m in PER_DOCUMENT for nq in BATCHES if nq <= max_queries]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=15)
    ap.add_argument("--out", default=None)
    ap.add_argument("--small-only", action="store_true", help="the 100 k corpus alone")
    ap.add_argument("--max-queries", type=int, default=max(BATCHES))
    a = ap.parse_args()
    pkg = importlib.import_module("rust-local-rag_amd")
    if pkg.device_count() < 1:
        raise SystemExit("bench_capped_batch needs a GPU: the library has no CPU path")
    res = {"bench": "capped_batch", "dim": 768, "calls": a.calls, "cells": []}
    ix, lex, ids, _, _ = BC.build(pkg, 100_000, 100)
    res["cells"] += run_corpus(pkg, "100k_100_documents", ix, lex, ids, a.calls, a.max_queries, 0)
    ix.close(); lex.close()
    if not a.small_only:
        ix, lex, ids, _, _ = BC.build(pkg, 1_000_000, 1000)
        res["cells"] += run_corpus(pkg, "1M_1000_documents", ix, lex, ids, a.calls, a.max_queries, 0)
        res["cells"] += run_corpus(pkg, "1M_skewed_200k_document", ix, lex, ids, a.calls, a.max_queries, 200_000)
        ix.close(); lex.close()
    key = lambda c: (c["corpus"], c["queries"], c["top_k"], c["per_document"])
    res["mode0_slower_cells"] = [key(c) for c in res["cells"] if c["mode0_slower"] and not c["mode0_declined"]]
    res["mode2_slower_cells"] = [key(c) for c in res["cells"] if c["mode2_slower"]]
    res["mode0_declined_cells"] = [key(c) for c in res["cells"] if c["mode0_declined"]]
    res["forms_mode2_total"] = [int(sum(c["forms_mode2"][i] for c in res["cells"])) for i in range(4)]
    res["forms_mode0_total"] = [int(sum(c["forms_mode0"][i] for c in res["cells"])) for i in range(4)]
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
