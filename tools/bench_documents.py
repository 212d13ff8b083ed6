"""The document column against the host-built scopes it replaces: building a document scope, and removing a document.

    python tools/bench_documents.py [--rows 1000000] [--dim 768] [--documents 1000] [--calls 15] [--out FILE]

Corpus: f32 rows filled on the device (rlr_index_fill_synthetic, seeded) in `documents` equal documents, the chunk table
planted beside them (empty texts: the lexical index holds nothing, its share of a removal is the same on both sides).
Timed, host clock around calls that return after their device synchronisation, warm, the two sides alternating call by
call, median and p10 / p90 of `calls` calls:
  scope build   for scopes of 1, 10, 100 and 500 documents (seeded choices of names):
                  parent   RagEngine._filter_for as it was before the column (kept below: a walk over the chunk table,
                           document_ranges, then rlr_filter_create_ranges -- host mask, host row list, two uploads)
                  device   name -> id lookups, then rlr_filter_create_documents
                both build the filter anew every call (as after every ingest) and are checked to be the same filter.
  removal       of one document at the front of the corpus (compaction moves every other row) and of one at the back:
                  parent   RagEngine.remove_document as it was (a walk over the chunk table, rlr_index_delete_rows)
                  device   RagEngine.remove_document (rlr_index_delete_documents)
                the removed document's rows are appended again (untimed) so that every call sees the same corpus size.
A point counts as faster when the device side's median lies below the parent's median by more than the parent's own
p10..p90 spread.  One JSON line on stdout."""
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

SCOPES = [1, 10, 100, 500]
WARM = 3


# ---- the parent's host paths, kept as they were ---------------------------------------------------------------------
def parent_filter_for(eng, eng_mod, documents):
    return eng.index.filter_ranges(eng_mod.document_ranges(eng._chunks, frozenset(documents)))


def parent_remove_document(eng, document_name):
    dead = [r for r, ch in enumerate(eng._chunks) if ch.document_name == document_name]
    if dead:
        eng._drop_filters()
        eng.index.delete_rows(dead)
        eng.lexical.remove_rows(dead)
        dead_set = set(dead)
        eng._chunks = [ch for r, ch in enumerate(eng._chunks) if r not in dead_set]
        eng._row_of = {ch.id: r for r, ch in enumerate(eng._chunks)}
    return len(dead)


# ---- helpers -----------------------------------------------------------------------------------------------------------
def stats(t):
    t = 1e3 * np.asarray(t)
    return {"ms": round(float(np.median(t)), 4), "p10_ms": round(float(np.percentile(t, 10)), 4),
            "p90_ms": round(float(np.percentile(t, 90)), 4)}


def verdict(parent, device):
    spread = parent["p90_ms"] - parent["p10_ms"]
    return {"parent": parent, "device": device, "parent_spread_ms": round(spread, 4),
            "speedup": round(parent["ms"] / device["ms"], 2), "faster_beyond_spread": bool(device["ms"] < parent["ms"] - spread)}


def put_back(pkg, eng, name, rows):
    """append the document again, as add_document does for its rows (untimed)"""
    first = eng.index.append(rows)
    eng.index.tag_rows(first, rows.shape[0], eng._doc_id(name))
    eng._chunks.extend(pkg.DocumentChunk(f"{name}/{i}/{first}", name, "", i) for i in range(rows.shape[0]))
    for r in range(first, len(eng._chunks)):
        eng._row_of[eng._chunks[r].id] = r
    eng._tagged, eng._tagged_len = eng._chunks, len(eng._chunks)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--documents", type=int, default=1000)
    ap.add_argument("--calls", type=int, default=15)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    pkg = importlib.import_module("rust-local-rag_amd")
    eng_mod = importlib.import_module("rust-local-rag_amd.engine")
    if pkg.device_count() < 1:
        raise SystemExit("bench_documents needs a GPU: the library has no CPU path")
    per = a.rows // a.documents
    n = per * a.documents
    eng = pkg.RagEngine(a.dim)
    eng.index.fill_synthetic(n, seed=20261020, n_clusters=64)
    eng._chunks = [pkg.DocumentChunk(str(r), f"doc{r // per}.pdf", "", r % per) for r in range(n)]
    eng._row_of = {ch.id: r for r, ch in enumerate(eng._chunks)}   # (the tables as add_document keeps them)
    eng._sync_documents()
    res = {"bench": "documents", "rows": n, "dim": a.dim, "documents": a.documents, "calls": a.calls, "scope_build": [], "removal": []}

    rng = np.random.default_rng(5)
    for m in SCOPES:
        names = [f"doc{d}.pdf" for d in rng.choice(a.documents, size=min(m, a.documents), replace=False)]
        parent = lambda: parent_filter_for(eng, eng_mod, names)
        device = lambda: eng.index.filter_documents([eng._doc_ids[nm] for nm in names if nm in eng._doc_ids])
        with parent() as fp, device() as fd:
            (mp, lp), (md, ld) = fp.read(), fd.read()
            assert np.array_equal(mp, md) and np.array_equal(lp, ld) and fp.info() == fd.info(), f"scope of {m}: the filters differ"
            n_allowed = fd.info()["n_allowed"]
        for _ in range(WARM):
            parent().close()
            device().close()
        tp, td = [], []
        for _ in range(a.calls):
            t0 = time.perf_counter(); f = parent(); tp.append(time.perf_counter() - t0); f.close()
            t0 = time.perf_counter(); f = device(); td.append(time.perf_counter() - t0); f.close()
        p = {"scope_documents": m, "n_allowed": n_allowed, **verdict(stats(tp), stats(td))}
        res["scope_build"].append(p)
        print(json.dumps(p), file=sys.stderr, flush=True)

    for where in ("front", "back"):
        tp, td = [], []
        for i in range(WARM + a.calls):
            for side, sink in (("parent", tp), ("device", td)):
                name = eng._chunks[0 if where == "front" else -1].document_name
                at = 0 if where == "front" else len(eng._chunks) - per
                rows = eng.index.fetch_rows(np.arange(at, at + per))
                t0 = time.perf_counter()
                got = parent_remove_document(eng, name) if side == "parent" else eng.remove_document(name)
                dt = time.perf_counter() - t0
                assert got == per and len(eng.index) == n - per, (where, side, got)
                if side == "parent":
                    eng._tagged, eng._tagged_len = eng._chunks, len(eng._chunks)   # (delete_rows compacted the column)
                if i >= WARM:
                    sink.append(dt)
                put_back(pkg, eng, name, rows)
        p = {"document_at": where, "rows_removed": per, **verdict(stats(tp), stats(td))}
        res["removal"].append(p)
        print(json.dumps(p), file=sys.stderr, flush=True)
    want = np.array([eng._doc_ids[ch.document_name] for ch in eng._chunks], np.uint32)
    assert np.array_equal(eng.index.get_documents(), want), "the column and the chunk table disagree after the removals"
    res["all_faster_beyond_spread"] = all(p["faster_beyond_spread"] for p in res["scope_build"] + res["removal"])
    eng.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
