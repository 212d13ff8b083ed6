"""Queries with a scope EACH in one call (rlr_search_topk_scoped) against the same requests one by one
(rlr_search_topk_filtered with one query per call -- the only way to serve them without the scoped call).

    python tools/bench_scoped.py [--rows 1000000] [--dim 768] [--k 100] [--queries 2 4 8] [--rounds 50] [--out FILE]

Corpus: f32 rows filled on the device (rlr_index_fill_synthetic, seeded), twice: one index with the natural gate and
one created under RLR_BATCH_MIN=2, which forces the shared pass.  The queries are noisy copies of stored rows.
Scope sets, one scope per query:
    disjoint_8th    pairwise disjoint contiguous ranges of 1/8 of the rows each
    disjoint_80th   pairwise disjoint contiguous ranges of 1/80 of the rows each
    random_halves   an independent random half of the rows per query (heavy overlap: the union is nearly everything)
    identical       one range of 1/8 of the rows, the same filter object in every slot
Legs, in ONE process, interleaved round by round (one-by-one A | natural | forced | one-by-one B), warm, the median of
`rounds` rounds each: `natural` is the scoped call as a caller gets it (the cost model decides whether the chunk shares a
pass), `forced` the scoped call with the pass forced, `one_by_one` the yardstick.  The yardstick's spread is the distance
of the medians of its two legs; a configuration is `ok` when the natural leg's median is at most the yardstick's median
plus that spread.  Before any timing the scoped results are compared with the one-by-one results (rows, score bits).
One JSON line on stdout."""
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

WARM = 5


def build(pkg, a, batch_min):
    old = os.environ.pop("RLR_BATCH_MIN", None)
    try:
        if batch_min is not None:
            os.environ["RLR_BATCH_MIN"] = batch_min           # (read when the index is created)
        ix = pkg.GpuIndex(a.dim)
    finally:
        os.environ.pop("RLR_BATCH_MIN", None)
        if old is not None:
            os.environ["RLR_BATCH_MIN"] = old
    ix.fill_synthetic(a.rows, seed=20261017, n_clusters=64)
    return ix


def queries(ix, dim, n_rows, n):
    rng = np.random.default_rng(70)
    rows = ix.fetch_rows(rng.integers(0, n_rows, size=n))
    q = rows + 0.05 * rng.standard_normal((n, dim)).astype(np.float32)
    return np.ascontiguousarray(q / np.linalg.norm(q, axis=1, keepdims=True), dtype=np.float32)


def scope_filters(ix, name, n_rows, nq):
    """(the filter of every query slot, the filters to close, rows per scope, rows of the union)"""
    if name in ("disjoint_8th", "disjoint_80th"):
        m = n_rows // (8 if name == "disjoint_8th" else 80)
        fs = [ix.filter_ranges([(q * (n_rows // 8), m)]) for q in range(nq)]
        return fs, fs, m, m * nq
    if name == "identical":
        f = ix.filter_ranges([(n_rows // 3, n_rows // 8)])
        return [f] * nq, [f], n_rows // 8, n_rows // 8
    rng = np.random.default_rng(5)
    keep = [rng.random(n_rows) < 0.5 for _ in range(nq)]
    fs = [ix.filter_rows(np.flatnonzero(k)) for k in keep]
    return fs, fs, int(np.mean([k.sum() for k in keep])), int(np.logical_or.reduce(keep).sum())


def same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--queries", type=int, nargs="+", default=[2, 4, 8])
    ap.add_argument("--rounds", type=int, default=50)
    ap.add_argument("--scopes", nargs="+", default=["disjoint_8th", "disjoint_80th", "random_halves", "identical"])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    pkg = importlib.import_module("rust-local-rag_amd")
    if pkg.device_count() < 1:
        raise SystemExit("bench_scoped needs a GPU: the library has no CPU path")
    nat, forced = build(pkg, a, None), build(pkg, a, "2")
    res = {"bench": "scoped", "rows": a.rows, "dim": a.dim, "k": a.k, "rounds": a.rounds,
           "legs": "one process, interleaved: one_by_one A | natural | forced | one_by_one B", "points": []}
    for name in a.scopes:
        for nq in a.queries:
            qs = queries(nat, a.dim, a.rows, nq)
            fn, close_n, per_scope, union = scope_filters(nat, name, a.rows, nq)
            ff, close_f, _, _ = scope_filters(forced, name, a.rows, nq)
            legs = {
                "one_by_one": lambda: [nat.search_topk(qs[i], a.k, filter=fn[i]) for i in range(nq)],
                "natural": lambda: nat.search_topk_scoped(qs, a.k, fn),
                "forced": lambda: forced.search_topk_scoped(qs, a.k, ff),
            }
            want = legs["one_by_one"]()
            prof = {}
            for leg, ix in (("natural", nat), ("forced", forced)):
                ix.profile_read(reset=True)
                got = legs[leg]()
                prof[leg] = ix.profile_read()
                for i in range(nq):
                    assert same(got[i], (want[i][0][0], want[i][1][0])), f"{name} x {nq}: {leg} query {i} differs from the single call"
            for _ in range(WARM):
                for fn_ in legs.values():
                    fn_()
            t = {"a": [], "natural": [], "forced": [], "b": []}
            for _ in range(a.rounds):
                for slot, leg in (("a", "one_by_one"), ("natural", "natural"), ("forced", "forced"), ("b", "one_by_one")):
                    t0 = time.perf_counter()
                    legs[leg]()
                    t[slot].append(time.perf_counter() - t0)
            med = lambda v: 1e3 * float(np.median(v))             # noqa: E731
            la, lb, base = med(t["a"]), med(t["b"]), med(t["a"] + t["b"])
            p = {"scopes": name, "queries": nq, "rows_per_scope": per_scope, "union_rows": union,
                 "natural_shares": int(prof["natural"].n_batches), "handed_back": int(prof["forced"].n_batch_fallbacks),
                 "natural_ms": round(med(t["natural"]), 4), "forced_ms": round(med(t["forced"]), 4),
                 "one_by_one_ms": round(base, 4), "one_by_one_legs_ms": [round(la, 4), round(lb, 4)],
                 "one_by_one_spread_ms": round(abs(la - lb), 4), "natural_to_one_by_one": round(med(t["natural"]) / base, 3),
                 "forced_to_one_by_one": round(med(t["forced"]) / base, 3), "ok": bool(med(t["natural"]) <= base + abs(la - lb))}
            res["points"].append(p)
            print(json.dumps(p), file=sys.stderr, flush=True)
            for f in close_n + close_f:
                f.close()
    nat.close()
    forced.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
