"""RagEngine.search_text_batch(documents=...) (rlr_engine_search_text_batch_filtered): every query of a batch is held to
Corpus.expect -- the oracle's search over the sub-corpus of the scope, BM25 statistics global -- and, bit for bit, to the
single call with query_text= and documents=.  For every vector that tests/test_text_batch_filtered_cpu.py cleared the
batch must have served every query itself (info: n_batched == n): a loop over the single entry point does not pass."""
import ctypes as C
import importlib

import numpy as np
import pytest

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


_corpora, _queries = {}, {}


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


def query(c, i):
    if (c.dim, i) not in _queries:
        _queries[(c.dim, i)] = c.O.synth_query(c.dim, seed=V.QUERY_SEED0 + i)
    return _queries[(c.dim, i)]


def run_vector(c, vec):
    s, wi, lam, stage, k, n, shift = vec
    docs = V.SCOPES[s]
    wts, w_e, w_l = V.WEIGHTS[wi]
    w = c.rlr.QueryWeights(**wts) if wts else None
    qs, texts = [query(c, i) for i in range(n)], V.batch_texts(n, shift)
    got, info = c.eng.search_text_batch(np.stack(qs), texts, k, lam, w, stage=stage, return_info=True, documents=docs)
    assert len(got) == n
    for i in range(n):
        c.check(got[i], c.expect(docs, qs[i], k, lam, texts[i], stage, w_e, w_l), (vec, i, texts[i]))
        if lam == 0.0:
            one = c.eng.search(qs[i], k, weights=w, stage=stage, query_text=texts[i], documents=docs)
        else:
            one = c.eng.search_with_diversity(qs[i], k, lam, weights=w, query_text=texts[i], documents=docs)
        assert same(got[i], one), (vec, i, texts[i])
    if c.rows_of(docs).size == 0:
        assert all(r == [] for r in got) and info["n_batched"] == 0 and info["n_single"] == 0
    elif w_e == 0.0:
        assert info["n_single_shape"] == n and info["n_single"] == n and info["n_batched"] == 0, (vec, info)
    else:                                                       # cleared on the CPU: nothing may be handed back
        assert info["n_batched"] == n and info["n_single"] == 0, (vec, info)


@pytest.mark.parametrize("s", range(len(V.SCOPES)))
def test_the_grid_on_768d_rows(corpora, s):
    c = corpora("f32_768")
    vecs = [v for v in V.engine_grid("f32_768") if v[0] == s]
    assert len(vecs) == len(V.WEIGHTS) * len(V.MODES) * len(V.TOP_KS)
    for vec in vecs:
        run_vector(c, vec)


@pytest.mark.parametrize("name", ["f32_256", "f32_1024", "f16_1024"])
def test_other_widths_and_binary16_rows(corpora, name):
    c = corpora(name)
    for vec in V.engine_grid(name):
        run_vector(c, vec)


def test_search_documents_batch_routes_scoped_text_through_the_batch(corpora):
    c = corpora("f32_768")
    R = c.rlr.SearchRequest
    w = c.rlr.QueryWeights(embedding=0.6, lexical=0.4)
    a, b = ["doc4.pdf"], ["doc8.pdf", "doc2.pdf"]
    spec = [(a, "w000x w001x common", None), (None, "w017x frequent the", None), (a, None, None), (b, "the of", None),
            (a, "w002x w003x common", None), (b, "", None), (a, "", None), (b, "w005x w040x", None), (a, "common", w),
            (None, None, None), (a, "frequent w001x", w), (["no-such.pdf"], "common", None), (["no-such.pdf"], "the of", None),
            (b, "w000x", None), ([], "common", None)]
    reqs = [R(query_embedding=query(c, i), query=t, documents=d, weights=wt, top_k=7, diversity_factor=0.3)
            for i, (d, t, wt) in enumerate(spec)]
    calls = []
    orig = c.eng.search_text_batch
    c.eng.search_text_batch = lambda *a_, **k_: (calls.append((len(a_[0]), k_.get("documents"))), orig(*a_, **k_))[1]
    try:
        out = c.eng.search_documents_batch(reqs)
    finally:
        del c.eng.search_text_batch
    for i, r in enumerate(reqs):
        assert same(out[i], c.eng.search_documents(r)), (i, spec[i][:2])
    assert sorted(calls, key=str) == sorted([(2, None), (2, ["doc4.pdf"]), (3, ["doc2.pdf", "doc8.pdf"]), (2, ["doc4.pdf"]),
                                             (2, ["no-such.pdf"])], key=str)       # (doc4 twice: two weights)


def test_an_append_drops_the_scope_and_refuses_the_old_filter(rlr, oracle):
    c = Corpus(rlr, oracle, 768, "f32", seed=21)
    try:
        docs, k, lam = ["doc7.pdf", "doc9.pdf"], 7, 0.3
        qs, texts = [query(c, i) for i in range(3)], V.batch_texts(3, 0)
        raw = c.eng.index.filter_ranges(eng_mod.document_ranges(c.eng._chunks, docs))   # a filter the engine does not own
        toks = [" ".join(eng_mod.tokenize(t)).encode() for t in texts]
        off = np.zeros(4, np.uint64)
        off[1:] = np.cumsum([len(t) for t in toks])
        q, hits, n_out = np.ascontiguousarray(np.stack(qs)), (N.SearchHitC * (3 * 31))(), np.zeros(3, np.uint32)

        def raw_call():
            return N.lib().rlr_engine_search_text_batch_filtered(
                c.eng.index.handle, c.eng.lexical._h, raw.handle, q.ctypes.data_as(N.f32p), 768, 3, b"".join(toks),
                off.ctypes.data_as(N.u64p), k, lam, 0, None, hits, 31, n_out.ctypes.data_as(N.u32p), None)

        before = c.eng.search_text_batch(np.stack(qs), texts, k, lam, documents=docs)
        assert raw_call() == 0
        for i in range(3):
            c.check(before[i], c.expect(docs, qs[i], k, lam, texts[i], 0, 0.7, 0.3), ("before", i))
            assert [h.row for h in hits[i * 31: i * 31 + n_out[i]]] == [r.row for r in before[i]]
        c.eng.add_document("doc12.pdf", make_texts(40, seed=702), oracle.synth_rows(40, 768, seed=701))
        c.refresh()
        assert raw_call() == -1 and b"stale" in N.lib().rlr_last_error()               # RLR_E_INVALID before any GPU work
        after = c.eng.search_text_batch(np.stack(qs), texts, k, lam, documents=docs + ["doc12.pdf"])
        for i in range(3):
            c.check(after[i], c.expect(docs + ["doc12.pdf"], qs[i], k, lam, texts[i], 0, 0.7, 0.3), ("after", i))
        again = c.eng.search_text_batch(np.stack(qs), texts, k, lam, documents=docs)
        for i in range(3):
            c.check(again[i], c.expect(docs, qs[i], k, lam, texts[i], 0, 0.7, 0.3), ("same scope after", i))
        raw.close()
    finally:
        c.close()
