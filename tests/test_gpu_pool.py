"""Every branch of the fused pool and blend stage on the designed rows of tests/pool_vectors.py: hybrid_pool_body
(csrc/index_fused.hip) through rlr_search_hybrid and, for many queries, through rlr_engine_search_text_batch; pool_prepare_body
(csrc/pool_prepare.h) through rlr_search_diverse in its three forms -- pool_prepare_kernel<true> (fetch <= 512, RLR_TAIL=0),
the fused tail's finish (fetch <= 512, RLR_TAIL=1) and sort_emit + pool_prepare_kernel<false> (fetch > 512).

The entries are called directly: they report *fallback, which the engine would answer silently through its host path.
The status must be the predicted one; on status 0 the count, the rows and the bits of the cosine, combined and lexical
scores must equal the restatement's, on any other status nothing may have been written.  test_pool_vectors_cpu.py
proves that the cases reach the states they are named after and that the rows' cosines and Gram entries are exact, so a
difference here is the blend's.  No tolerance anywhere."""
import collections
import ctypes as C
import importlib

import numpy as np
import pytest

import pool_vectors as V
from pool_vectors import bits

pytestmark = pytest.mark.gpu
N = importlib.import_module("rust-local-rag_amd._native")
E0 = np.zeros(V.DIM, np.float32)
E0[0] = 1.0
SENTINEL_ROW, SENTINEL_F = 0xDEADBEEFDEADBEEF, np.float32(-7.25)
ENV = {"default": ("RLR_HYBRID_FETCH", None), "full": ("RLR_HYBRID_FETCH", "full"), "tail0": ("RLR_TAIL", "0"),
       "tail1": ("RLR_TAIL", "1")}


def call(ix, c):
    """one direct call -> (status of the call, fallback, n_out, rows, cos, combined, lexical); the outputs are prefilled"""
    cap = max(c.need, 1) + 8
    rows = np.full(cap, SENTINEL_ROW, np.uint64)
    cos, comb, lex = (np.full(cap, SENTINEL_F, np.float32) for _ in range(3))
    n_out, fb = C.c_uint32(0xDEADBEEF), C.c_int32(-99)
    L = N.lib()
    if c.entry == "diverse":
        st = L.rlr_search_diverse(ix.handle, E0.ctypes.data_as(N.f32p), c.need, c.k, float(c.lam), float(c.w_e), float(c.w_l), -1.0,
                                  rows.ctypes.data_as(N.u64p), cos.ctypes.data_as(N.f32p), comb.ctypes.data_as(N.f32p),
                                  C.byref(n_out), C.byref(fb))
        lex = None
    else:
        lr = np.ascontiguousarray(c.lex_rows if c.n_lex else np.zeros(1, np.uint64), np.uint64)
        ls = np.ascontiguousarray(c.lex_scores if c.n_lex else np.zeros(1, np.float32), np.float32)
        st = L.rlr_search_hybrid(ix.handle, E0.ctypes.data_as(N.f32p), c.need, c.k, float(c.lam), c.diversify, float(c.w_e),
                                 float(c.w_l), lr.ctypes.data_as(N.u64p), ls.ctypes.data_as(N.f32p), c.n_lex, float(c.max_lex), -1.0,
                                 rows.ctypes.data_as(N.u64p), cos.ctypes.data_as(N.f32p), comb.ctypes.data_as(N.f32p),
                                 lex.ctypes.data_as(N.f32p), C.byref(n_out), C.byref(fb))
    return st, fb.value, n_out.value, rows, cos, comb, lex


def check(c, mode, dtype, e, got):
    """-> None, or what differs"""
    st, fb, n, rows, cos, comb, lex = got
    outs = [("cos", cos, e.cos), ("combined", comb, e.comb)] + ([("lexical", lex, e.lex)] if lex is not None else [])
    if st != N.RLR_OK:
        return f"the call failed with status {st}"
    if fb != e.status:
        return f"fallback {fb}, predicted status {e.status} ({ {k: v for k, v in e.info.items() if k != 'picks'} })"
    if e.status:
        if n != 0 or (rows != SENTINEL_ROW).any() or any((bits(a) != bits(SENTINEL_F)).any() for _, a, _ in outs):
            return f"status {fb} but n_out = {n} or an output was written"
        return None
    if n != e.n:
        return f"n_out {n}, want {e.n}"
    if (rows[n:] != SENTINEL_ROW).any() or any((bits(a[n:]) != bits(SENTINEL_F)).any() for _, a, _ in outs):
        return f"written beyond n_out = {n}"
    if not np.array_equal(rows[:n], e.rows):
        i = int(np.flatnonzero(rows[:n] != e.rows)[0])
        return (f"rows differ from position {i}: got {rows[max(i - 2, 0): i + 6].tolist()} want {e.rows[max(i - 2, 0): i + 6].tolist()}, "
                f"combined there {[hex(x) for x in bits(comb[max(i - 2, 0): i + 6])]} want {[hex(x) for x in bits(e.comb[max(i - 2, 0): i + 6])]}")
    for what, a, w in outs:
        if not np.array_equal(bits(a[:n]), bits(w)):
            i = int(np.flatnonzero(bits(a[:n]) != bits(w))[0])
            return f"{what} bits differ from position {i} (row {int(rows[i])}): got {hex(bits(a[i: i + 1])[0])} want {hex(bits(w[i: i + 1])[0])}"
    return None


class IndexCache:
    """one index per (corpus, dtype, mode), made on first use and shared by every plan and case of the module.  The mode is
    part of the key because RLR_HYBRID_FETCH and RLR_TAIL are read when an index is created: `get` is called with the
    variable already set by the test.  At most LIMIT indexes stay open (the least recently used one is closed)."""
    LIMIT = 16

    def __init__(self, rlr):
        self.rlr, self.open, self.made = rlr, collections.OrderedDict(), 0

    def get(self, corpus, dtype, mode):
        key = (corpus, dtype, mode)
        if key in self.open:
            self.open.move_to_end(key)
            return self.open[key]
        while len(self.open) >= self.LIMIT:
            self.open.popitem(last=False)[1].close()
        ix = self.rlr.GpuIndex(V.DIM, dtype)
        ix.upload(V.corpus(corpus).rows())
        self.open[key], self.made = ix, self.made + 1
        return ix

    def close(self):
        while self.open:
            self.open.popitem()[1].close()


@pytest.fixture(scope="module")
def indexes(rlr):
    cache = IndexCache(rlr)
    yield cache
    cache.close()


def run_plan(cache, entry, name, mode, dtype, setenv):
    """every case of the plan that runs on `dtype` -> (cases run, [what differs])"""
    var, val = ENV[mode]
    setenv(var, val)
    bad, ran = [], 0
    for i, c in enumerate(V.plan(entry, name)):
        if dtype not in c.dtypes:
            continue
        e = V.want(entry, name, i, mode)
        why = check(c, mode, dtype, e, call(cache.get(c.corpus, dtype, mode), c))
        ran += 1
        if why:
            bad.append(f"{c.describe()} [{mode}, {dtype}]: {why}")
    return ran, bad


def _params(entry, names, modes):
    return [(nm, m, dt) for nm in names for m in modes for dt in ("f32", "f16")
            if any(dt in c.dtypes for c in V.plan(entry, nm))]


def _setenv(monkeypatch):
    return lambda var, val: monkeypatch.delenv(var, raising=False) if val is None else monkeypatch.setenv(var, val)


@pytest.mark.parametrize("name,mode,dtype", _params("hybrid", V.HYBRID_PLANS, V.HYBRID_MODES))
def test_hybrid(indexes, monkeypatch, name, mode, dtype):
    """rlr_search_hybrid: hybrid_pool_kernel (and the greedy chain's emit under diversification); `full` = an index created
    under RLR_HYBRID_FETCH=full, whose fetch is need + n_lex + 8"""
    ran, bad = run_plan(indexes, "hybrid", name, mode, dtype, _setenv(monkeypatch))
    assert ran >= 1
    assert not bad, f"{len(bad)} of {ran} cases of hybrid/{name} differ:\n" + "\n".join(bad)


@pytest.mark.parametrize("name,mode,dtype", _params("diverse", V.DIVERSE_PLANS, V.DIVERSE_MODES))
def test_diverse(indexes, monkeypatch, name, mode, dtype):
    """rlr_search_diverse: RLR_TAIL=0 -> pool_prepare_kernel<true>, RLR_TAIL=1 -> the fused tail's finish (both for a fetch of
    at most 512 rows), and sort_emit + pool_prepare_kernel<false> above that; every plan holds cases on both sides of 512
    (test_pool_vectors_cpu.py).  Which tail an index takes is read from the library's code (enqueue_query_rest: RLR_TAIL=1
    and rows that fit the staged layout, which 16 elements do); the library reports no counter for it."""
    ran, bad = run_plan(indexes, "diverse", name, mode, dtype, _setenv(monkeypatch))
    assert ran >= 1
    assert not bad, f"{len(bad)} of {ran} cases of diverse/{name} differ:\n" + "\n".join(bad)


def test_text_batch_puts_different_states_side_by_side(rlr, oracle):
    """hybrid_pool_batch_kernel: the same body with per-query offsets (pairs at q * bound, pool at q * need, candidates at
    q * 3 * 4096, info at 2 q).  One batch whose neighbours differ in everything the offsets carry: no pair, one pair, as many
    pairs as the BM25 limit, pairs that all lie outside the index, and one query that fails the boundary rule and is re-run
    alone.  Each query must equal the restatement (the oracle for the re-run one) and the single call; the counters must say
    that exactly the one query left the batched kernels."""
    n = V.TEXT_N
    unit = np.zeros((n, V.DIM), np.float32)
    unit[:, 0] = 1.0
    eng = rlr.RagEngine(V.DIM)
    try:
        eng.add_document("d", V.text_rows(), unit)
        eng.index.upload(V.corpus("text").rows())                 # the designed rows as they are (add_document normalises)
        for g in V.TEXT_GHOSTS:
            eng.lexical.add_chunk(g, "ghost")
        o = V.text_oracle()
        stored = eng.index.fetch_rows(np.arange(n))
        assert np.array_equal(bits(stored), bits(V.corpus("text").rows()))
        qs = np.zeros((len(V.TEXT_QUERIES), V.DIM), np.float32)
        for i, (_, _, axis) in enumerate(V.TEXT_QUERIES):
            qs[i, axis] = 1.0
        texts = [t for _, t, _ in V.TEXT_QUERIES]
        got, info = eng.search_text_batch(qs, texts, V.TEXT_TOP_K, 0.0, stage=1, return_info=True)
        n_blend = 0
        for i, (state, text, axis) in enumerate(V.TEXT_QUERIES):
            pairs = V.text_pairs(o, text)
            e = V.expected(V.text_case(state, axis, pairs), "batch")
            n_blend += e.status == 2
            if e.status == 0:
                want = (e.rows, e.cos, e.comb, e.lex)
            else:
                wr, wc, we, wl = oracle.search(stored, qs[i], V.TEXT_TOP_K, lex=pairs or None, stage=1)
                want = (wr, we, wc, wl)
            alone = eng.search(qs[i], V.TEXT_TOP_K, stage=1, query_text=text)
            for what, hits in (("batch", got[i]), ("single call", alone)):
                ctx = (what, i, state, text, f"predicted status {e.status}")
                assert [h.row for h in hits] == want[0].tolist(), ctx
                assert np.array_equal(bits([h.embedding_score for h in hits]), bits(want[1])), ctx
                assert np.array_equal(bits([h.score for h in hits]), bits(want[2])), ctx
                assert np.array_equal(bits([h.lexical_score for h in hits]), bits(want[3])), ctx
        assert n_blend == 1
        assert info["n_single_blend"] == n_blend and info["n_batched"] == len(texts) - n_blend, info
        assert info["n_single_lexical"] == 0 and info["n_single_shape"] == 0 and info["n_single"] == n_blend, info
    finally:
        eng.close()
