"""Batched hybrid search with query text (rlr_engine_search_text_batch) against the same queries one call at a time
(rlr_engine_search_text).

    python tools/bench_text_batch.py [--rows 100000,1000000] [--dim 768] [--batches 8,64,256] [--k 10] [--lam 0.3]
                                     [--reps 5] [--out FILE]

Corpus: seeded synthetic, generated here -- f32 rows filled on the device (rlr_index_fill_synthetic), one chunk text per
row of 4..25 words drawn from a Zipf vocabulary of 50 000 words, every chunk added to the GPU LexicalIndex.  Queries: a
noisy copy of a random stored row and 2..4 Zipf words.  Before any timing the batch's hits (rows and every score bit) are
checked against the sequential calls.  Reported per (rows, batch): sequential and batched queries/s, p50 per batch, and
how the batch served its queries (rlr_text_batch_info).  One JSON line on stdout.
"""
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

VOCAB = 50_000


def load():
    return importlib.import_module("rust-local-rag_amd")


def zipf_words(rng, n):
    # rank r with probability ~ 1 / r over the vocabulary (inverse CDF of the harmonic weights)
    w = 1.0 / np.arange(1, VOCAB + 1)
    cdf = np.cumsum(w / w.sum())
    return np.minimum(np.searchsorted(cdf, rng.random(n)), VOCAB - 1)


def build(pkg, n_rows, dim, seed):
    eng = pkg.RagEngine(dim)
    eng.index.fill_synthetic(n_rows, seed=seed, n_clusters=64)
    rng = np.random.default_rng(seed)
    lens = rng.integers(4, 26, size=n_rows)
    words = zipf_words(rng, int(lens.sum()))
    names = np.array([f"w{i:05d}" for i in range(VOCAB)])
    at = 0
    for r in range(n_rows):
        m = int(lens[r])
        eng.lexical.add_chunk(r, " ".join(names[words[at:at + m]]))
        at += m
    return eng, names


def queries(eng, names, nq, dim, seed):
    rng = np.random.default_rng(seed)
    n = len(eng.index)
    rows = eng.index.fetch_rows(rng.integers(0, n, size=nq)).astype(np.float32)
    qs = np.ascontiguousarray(rows + 0.05 * rng.standard_normal(rows.shape).astype(np.float32), np.float32)
    texts = [" ".join(names[zipf_words(rng, int(rng.integers(2, 5)))]) for _ in range(nq)]
    return qs, [t.encode() for t in texts]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="100000,1000000")
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--batches", default="8,64,256")
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--lam", type=float, default=0.3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    pkg = load()
    N = importlib.import_module("rust-local-rag_amd._native")
    L = N.lib()
    k, lam, dim = a.k, a.lam, a.dim
    cap = max(3 * max(k, 1), k + 10)
    result = {"bench": "text_batch", "dim": dim, "top_k": k, "lambda": lam, "reps": a.reps, "configs": []}
    for n_rows in [int(x) for x in a.rows.split(",")]:
        t0 = time.perf_counter()
        eng, names = build(pkg, n_rows, dim, seed=20261016 + n_rows)
        build_s = time.perf_counter() - t0
        for nq in [int(x) for x in a.batches.split(",")]:
            qs, toks = queries(eng, names, nq, dim, seed=nq)
            blob = b"".join(toks)
            offs = np.zeros(nq + 1, np.uint64)
            offs[1:] = np.cumsum([len(t) for t in toks])
            hits_b = (N.SearchHitC * (cap * nq))()
            n_b = np.zeros(nq, np.uint32)
            hits_s = (N.SearchHitC * (cap * nq))()
            n_s = np.zeros(nq, np.uint32)
            info = N.TextBatchInfoC()

            def batched():
                N.check(L.rlr_engine_search_text_batch(eng.index.handle, eng.lexical._h, qs.ctypes.data_as(N.f32p), dim, nq,
                                                       blob, offs.ctypes.data_as(N.u64p), k, lam, 0, None, hits_b, cap,
                                                       n_b.ctypes.data_as(N.u32p), C.byref(info)))

            one = C.c_uint32()
            sz = C.sizeof(N.SearchHitC)

            def sequential():
                for q in range(nq):
                    view = (N.SearchHitC * cap).from_buffer(hits_s, q * cap * sz)
                    N.check(L.rlr_engine_search_text(eng.index.handle, eng.lexical._h,
                                                     qs[q].ctypes.data_as(N.f32p), dim, toks[q], len(toks[q]), k, lam, 0,
                                                     None, view, cap, C.byref(one)))
                    n_s[q] = one.value

            sequential()
            batched()
            # check first: rows and every score bit of every query
            assert np.array_equal(n_b, n_s), "hit counts differ"
            rb = np.frombuffer(hits_b, dtype=np.uint8).reshape(nq, cap * sz)
            rs = np.frombuffer(hits_s, dtype=np.uint8).reshape(nq, cap * sz)
            for q in range(nq):
                assert np.array_equal(rb[q, :n_b[q] * sz], rs[q, :n_s[q] * sz]), f"query {q} differs"
            tb, ts = [], []
            for _ in range(a.reps):
                t = time.perf_counter()
                sequential()
                ts.append(time.perf_counter() - t)
                t = time.perf_counter()
                batched()
                tb.append(time.perf_counter() - t)
            pb, ps = float(np.median(tb)), float(np.median(ts))
            cfg = {"rows": n_rows, "batch": nq, "sequential_qps": round(nq / ps, 1), "batched_qps": round(nq / pb, 1),
                   "speedup": round(ps / pb, 2), "p50_batch_ms": round(1e3 * pb, 3), "p50_sequential_batch_ms": round(1e3 * ps, 3),
                   "info": {name: int(getattr(info, name)) for name, _ in N.TextBatchInfoC._fields_},
                   "corpus_build_s": round(build_s, 1)}
            result["configs"].append(cfg)
            print(json.dumps(cfg), file=sys.stderr, flush=True)
        eng.close()
    line = json.dumps(result)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
