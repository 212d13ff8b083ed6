"""One search context regrowing its buffers across calls.  Every workspace buffer of a context is sized by the call that
needs it and kept for the next; this walks ONE context (RLR_MAX_CONTEXTS=1, read at index creation) through calls that
each outgrow another group of buffers -- per-query states, the shared pass's sample and candidates, the matrix-core
query fragments, the large-candidate arrays, row lists, the MMR pool, the score array after an append -- and then
repeats the first small calls on the now-large buffers.  Every call is held to the oracle, rows and score bits exact.
The same sequence runs once more in a child process whose allocations start out as 0xFF bytes (RLR_POISON_ALLOC=1).
Standalone: python tests/test_gpu_workspace_growth.py."""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, DIM, N_MORE = 6000, 256, 3000  # just above the batched path's 4096-row floor, dim % 128 == 0


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def expected(e_full, allowed, k):
    """the oracle's scan reduced to the ascending rows `allowed`, ordered (score desc, row asc), cut to k"""
    allowed = np.asarray(allowed, dtype=np.uint64)
    e = e_full[allowed.astype(np.int64)]
    order = np.lexsort((np.arange(len(e)), -e.astype(np.float64)))[:k]
    return allowed[order], e[order]


def growth_sequence(rlr, O):
    rows = O.synth_rows(N + N_MORE, DIM, seed=6100, n_clusters=11)
    qs = np.stack([O.normalize(O.synth_query(DIM, seed=6200 + i)) for i in range(300)]).astype(np.float32)
    ix = rlr.GpuIndex(DIM, "f32")
    try:
        ix.upload(rows[:N])
        stored = ix.fetch_rows(np.arange(N))
        e_all = np.stack([O.scan(stored, q) for q in qs])  # the one reference of the first N rows, never changed
        e_all.setflags(write=False)
        every = np.arange(N)

        def check(sel, k, allowed=every, f=None, e=e_all, ctx=""):
            r, c = ix.search_topk(qs[sel], k, filter=f)
            for j, i in enumerate(range(len(qs))[sel]):
                wr, wc = expected(e[i], allowed, k)
                assert r.shape[1] == len(wr), (ctx, r.shape, len(wr))
                assert np.array_equal(r[j], wr), (ctx, i, r[j][:8], wr[:8])
                assert np.array_equal(bits(c[j]), bits(wc)), (ctx, i)

        check(slice(0, 1), 10, ctx="1: one query")
        check(slice(0, 8), 100, ctx="2: eight queries, the shared pass")
        check(slice(0, 300), 10, ctx="3: 300 queries, the matrix cores")
        check(slice(1, 2), 5000, ctx="4: one query, k = 5000")
        few = every[7::20][:300]
        with ix.filter_rows(few) as f:
            assert f.info()["path"] == "list" and len(few) == 300
            check(slice(2, 3), 50, few, f, ctx="5: list filter, one query")
            check(slice(2, 18), 50, few, f, ctx="5: list filter, 16 queries")
        many = np.delete(every, np.arange(0, N, 6))
        with ix.filter_rows(many) as f:
            f.set_path("scan")
            assert len(many) == 5000
            check(slice(4, 8), 25, many, f, ctx="6: masked scan, four queries")
        r, c = ix.search_topk(qs[9], 64)
        sc = (np.float32(0.7) * c[0]).astype(np.float32)
        o, m = ix.mmr_select(r[0], sc, 20, 0.3)
        wo, wm = O.mmr(stored[r[0].astype(np.int64)], sc, 20, 0.3)
        assert np.array_equal(o, wo) and np.array_equal(bits(m[1:]), bits(wm[1:])), "7: MMR over a pool of 64"
        assert ix.append(rows[N:]) == N and len(ix) == N + N_MORE
        stored = ix.fetch_rows(np.arange(N + N_MORE))
        e_big = {i: O.scan(stored, qs[i]) for i in range(8)}
        check(slice(0, 1), 10, np.arange(N + N_MORE), e=e_big, ctx="9: one query after the append")
        check(slice(0, 8), 100, np.arange(N + N_MORE), e=e_big, ctx="9: eight queries after the append")
    finally:
        ix.close()


def test_one_context_regrows_every_buffer_group(rlr, oracle, monkeypatch):
    monkeypatch.setenv("RLR_MAX_CONTEXTS", "1")
    growth_sequence(rlr, oracle)


def test_one_context_regrows_every_buffer_group_poisoned():
    env = dict(os.environ, RLR_POISON_ALLOC="1", RLR_MAX_CONTEXTS="1")
    out = subprocess.run([sys.executable, "-u", os.path.abspath(__file__)], cwd=ROOT, env=env, capture_output=True, text=True,
                         timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert "growth sequence ok" in out.stdout


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    from oracle import oracle as _O

    _O.lib()
    growth_sequence(importlib.import_module("rust-local-rag_amd"), _O)
    print("growth sequence ok")
