"""RagEngine.search_text_batch(scopes=...) (rlr_engine_search_text_batch_scoped): every query of a batch is held to
Corpus.expect over ITS scope -- the oracle's search over the sub-corpus, BM25 statistics global -- and, bit for bit, to the
single call with query_text= and documents=scope_i.  N, need, the pool and the result count differ inside one batch.  For
every vector that tests/test_scoped_text_cpu.py cleared the batch must have served every query with a non-empty scope
itself (info: n_batched): a loop over the single entry point does not pass."""
import ctypes as C
import importlib

import numpy as np
import pytest

import scoped_text_vectors as SV
import text_batch_filtered_vectors as V
from test_gpu_filter_engine import DOC_LENGTHS, Corpus, make_texts

pytestmark = pytest.mark.gpu
assert DOC_LENGTHS == V.DOC_LENGTHS

eng_mod = importlib.import_module("rust-local-rag_amd.engine")
N = importlib.import_module("rust-local-rag_amd._native")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same(a, b):
    key = lambda r: (r.row, bits([r.score])[0], bits([r.embedding_score])[0], bits([r.lexical_score])[0], r.chunk_id)
    return [key(x) for x in a] == [key(x) for x in b]


_corpora, _queries, _singles = {}, {}, {}


@pytest.fixture(scope="module")
def corpora(rlr, oracle):
    def get(name):
        if name not in _corpora:
            dim, dtype, seed = V.CORPORA[name]
            _corpora[name] = Corpus(rlr, oracle, dim, dtype, seed)
        return _corpora[name]
    yield get
    for c in _corpora.values():
        c.close()
    _corpora.clear()
    _singles.clear()


def query(c, i):
    if (c.dim, i) not in _queries:
        _queries[(c.dim, i)] = c.O.synth_query(c.dim, seed=V.QUERY_SEED0 + i)
    return _queries[(c.dim, i)]


def single(c, name, s, i, text, k, lam, stage, wi, w):
    """the single call and the oracle's answer for (scope, query, text, sizes, weights), computed once and shared"""
    key = (name, s, i, text, k, lam, stage, wi)
    if key not in _singles:
        docs, q = SV.SCOPES[s], query(c, i)
        _, w_e, w_l = V.WEIGHTS[wi]
        if lam == 0.0:
            one = c.eng.search(q, k, weights=w, stage=stage, query_text=text, documents=docs)
        else:
            one = c.eng.search_with_diversity(q, k, lam, weights=w, query_text=text, documents=docs)
        _singles[key] = (one, c.expect(docs, q, k, lam, text, stage, w_e, w_l))
    return _singles[key]


def run_vector(c, name, vec):
    rot, wi, lam, stage, k, n, shift = vec
    wts, w_e, w_l = V.WEIGHTS[wi]
    w = c.rlr.QueryWeights(**wts) if wts else None
    qs, texts, sc = [query(c, i) for i in range(n)], V.batch_texts(n, shift), SV.batch_scopes(n, rot)
    got, info = c.eng.search_text_batch(np.stack(qs), texts, k, lam, w, stage=stage, return_info=True,
                                        scopes=[SV.SCOPES[s] for s in sc])
    assert len(got) == n
    n_live = 0
    for i in range(n):
        one, want = single(c, name, sc[i], i, texts[i], k, lam, stage, wi, w)
        c.check(got[i], want, (vec, i, sc[i], texts[i]))
        assert same(got[i], one), (vec, i, sc[i], texts[i])
        rows = SV.SCOPE_ROWS[sc[i]]
        n_live += rows > 0
        _, _, need = V.sizes(rows, k, lam, stage)
        assert len(got[i]) == (need if lam == 0.0 else min(max(k, 1), need)), (vec, i, sc[i])   # |F_q| decides, per query
    assert n_live > 0                                           # (the empty scopes are never neighbours)
    if w_e == 0.0:
        assert info["n_single_shape"] == n and info["n_single"] == n and info["n_batched"] == 0, (vec, info)
    else:                                                       # cleared on the CPU: nothing may be handed back
        assert info["n_batched"] == n_live and info["n_single"] == 0, (vec, info)


@pytest.mark.parametrize("wi", range(len(V.WEIGHTS)))
def test_the_grid_on_768d_rows(corpora, wi):
    c = corpora("f32_768")
    vecs = [v for v in SV.engine_grid("f32_768") if v[1] == wi]
    assert len(vecs) == len(V.MODES) * len(V.TOP_KS)
    for vec in vecs:
        run_vector(c, "f32_768", vec)


@pytest.mark.parametrize("name", ["f32_256", "f32_1024", "f16_1024"])
def test_other_widths_and_binary16_rows(corpora, name):
    c = corpora(name)
    for vec in SV.engine_grid(name):
        run_vector(c, name, vec)


def test_a_batch_beyond_one_sub_batch(corpora):
    """257 queries without diversification: the engine's sub-batch is 256, so query 256 runs in the second one, where the
    filter array must be offset with the queries -- its scope (6) differs from query 0's (0).  Query i repeats the cleared
    query i mod 17, so the batch must serve every non-empty scope itself."""
    c = corpora("f32_768")
    n, k = 257, 7
    qs, texts, sc = [query(c, i % 17) for i in range(n)], V.batch_texts(n, 0), SV.batch_scopes(n, 0)
    assert sc[256] != sc[0] and sc[256] != sc[256 % 256]
    got, info = c.eng.search_text_batch(np.stack(qs), texts, k, 0.0, stage=1, return_info=True, scopes=[SV.SCOPES[s] for s in sc])
    n_live = 0
    for i in range(n):
        one, want = single(c, "f32_768", sc[i], i % 17, texts[i], k, 0.0, 1, 0, None)
        assert same(got[i], one), (i, sc[i], texts[i])
        if i >= 250:
            c.check(got[i], want, (i, sc[i], texts[i]))
        n_live += SV.SCOPE_ROWS[sc[i]] > 0
    assert info["n_batched"] == n_live and info["n_single"] == 0, info


def raw_batch(c, handles, qs, texts, k, lam, stage, cap):
    n = len(qs)
    toks = [" ".join(eng_mod.tokenize(t)).encode() for t in texts]
    off = np.zeros(n + 1, np.uint64)
    off[1:] = np.cumsum([len(t) for t in toks])
    q, hits, n_out = np.ascontiguousarray(np.stack(qs)), (N.SearchHitC * (n * cap))(), np.zeros(n, np.uint32)
    arr = (C.c_void_p * n)(*handles)
    info = N.TextBatchInfoC()
    st = N.lib().rlr_engine_search_text_batch_scoped(
        c.eng.index.handle, c.eng.lexical._h, arr, q.ctypes.data_as(N.f32p), c.dim, n, b"".join(toks),
        off.ctypes.data_as(N.u64p), k, lam, stage, None, hits, cap, n_out.ctypes.data_as(N.u32p), C.byref(info))
    return st, [[h.row for h in hits[i * cap: i * cap + n_out[i]]] for i in range(n)], info


def test_a_cap_below_the_largest_scopes_result_count_is_refused(corpora):
    """stage 1, top_k 7: query q returns min(|F_q|, 21) hits -- 10 for the ten-row scope, 21 for the 611-row scope"""
    c = corpora("f32_768")
    scopes = [["doc1.pdf", "doc5.pdf"], ["doc10.pdf", "doc11.pdf"], ["doc1.pdf", "doc5.pdf"]]
    fs = [c.eng.index.filter_ranges(eng_mod.document_ranges(c.eng._chunks, s)) for s in scopes]
    try:
        qs, texts = [query(c, i) for i in range(3)], V.batch_texts(3, 0)
        for cap in (10, 20):                                                 # enough for queries 0 and 2, not for query 1
            st, _, _ = raw_batch(c, [f.handle for f in fs], qs, texts, 7, 0.0, 1, cap)
            assert st == -1
        st, rows, info = raw_batch(c, [f.handle for f in fs], qs, texts, 7, 0.0, 1, 21)
        assert st == 0 and [len(r) for r in rows] == [10, 21, 10] and info.n_batched == 3 and info.n_single == 0
        for i in range(3):
            assert rows[i] == [r.row for r in c.eng.search(qs[i], 7, stage=1, query_text=texts[i], documents=scopes[i])]
        st, _, _ = raw_batch(c, [fs[0].handle, None, fs[2].handle], qs, texts, 7, 0.0, 1, 21)    # a null entry
        assert st == -1
    finally:
        for f in fs:
            f.close()


def test_search_documents_batch_shares_the_text_scopes(corpora):
    c = corpora("f32_768")
    R = c.rlr.SearchRequest
    w = c.rlr.QueryWeights(embedding=0.6, lexical=0.4)
    a, b = ["doc4.pdf"], ["doc8.pdf", "doc2.pdf"]
    spec = [(a, "w000x w001x common", None), (None, "w017x frequent the", None), (a, None, None), (b, "the of", None),
            (["doc0.pdf"], "w002x w003x common", None), (b, "", None), (["doc7.pdf"], "w005x w040x", None), (a, "common", w),
            (None, None, None), (["doc1.pdf", "doc5.pdf"], "frequent w001x", w), (["no-such.pdf"], "common", None),
            ([], "the of", None), (b, "w000x", None), (["doc10.pdf"], "common", None)]
    reqs = [R(query_embedding=query(c, i), query=t, documents=d, weights=wt, top_k=7, diversity_factor=0.3)
            for i, (d, t, wt) in enumerate(spec)]
    reqs.append(R(query_embedding=query(c, 14), query="common", documents=a, top_k=3, diversity_factor=0.3))   # alone under its key
    calls = []
    orig = c.eng.search_text_batch
    c.eng.search_text_batch = lambda *a_, **k_: (calls.append((len(a_[0]), k_.get("documents"), k_.get("scopes"))), orig(*a_, **k_))[1]
    try:
        out = c.eng.search_documents_batch(reqs, share_text_scopes=True)
    finally:
        del c.eng.search_text_batch
    for i, r in enumerate(reqs):
        assert same(out[i], c.eng.search_documents(r)), (i, r.documents, r.query)
    shared = sorted((n, s) for n, d, s in calls if s is not None)
    assert shared == sorted([(8, [["doc4.pdf"], ["doc2.pdf", "doc8.pdf"], ["doc0.pdf"], ["doc7.pdf"], ["no-such.pdf"], [],
                                  ["doc2.pdf", "doc8.pdf"], ["doc10.pdf"]]),
                             (2, [["doc4.pdf"], ["doc1.pdf", "doc5.pdf"]])])         # ONE scopes= call per key
    assert [(n, d) for n, d, s in calls if s is None] == [(2, None)]                # the unscoped group; no documents= call
    assert out[10] == [] and out[11] == [] and len(out[4]) == 1


def test_an_append_refuses_the_old_filter_array_and_fresh_scopes_work(rlr, oracle):
    c = Corpus(rlr, oracle, 768, "f32", seed=21)
    try:
        scopes, k, lam = [["doc7.pdf", "doc9.pdf"], ["doc1.pdf"], ["doc7.pdf", "doc9.pdf"]], 7, 0.3
        qs, texts = [query(c, i) for i in range(3)], V.batch_texts(3, 0)
        raws = [c.eng.index.filter_ranges(eng_mod.document_ranges(c.eng._chunks, s)) for s in scopes[:2]]   # not the engine's
        handles = [raws[0].handle, raws[1].handle, raws[0].handle]                                          # an entry repeats
        before = c.eng.search_text_batch(np.stack(qs), texts, k, lam, scopes=scopes)
        st, rows, _ = raw_batch(c, handles, qs, texts, k, lam, 0, 31)
        assert st == 0
        for i in range(3):
            c.check(before[i], c.expect(scopes[i], qs[i], k, lam, texts[i], 0, 0.7, 0.3), ("before", i))
            assert rows[i] == [r.row for r in before[i]]
        c.eng.add_document("doc12.pdf", make_texts(40, seed=702), oracle.synth_rows(40, 768, seed=701))
        c.refresh()
        st, _, _ = raw_batch(c, handles, qs, texts, k, lam, 0, 31)
        assert st == -1 and b"stale" in N.lib().rlr_last_error()                       # RLR_E_INVALID before any GPU work
        fresh = [scopes[0] + ["doc12.pdf"], ["doc12.pdf"], scopes[2]]
        after = c.eng.search_text_batch(np.stack(qs), texts, k, lam, scopes=fresh)
        for i in range(3):
            c.check(after[i], c.expect(fresh[i], qs[i], k, lam, texts[i], 0, 0.7, 0.3), ("after", i))
        for f in raws:
            f.close()
    finally:
        c.close()
