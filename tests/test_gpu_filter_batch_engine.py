"""RagEngine.search_with_diversity_batch(documents=...) and search_documents_batch with scoped requests: every query of a
batch equals the single call of the same query with the same scope (which test_gpu_filter_engine.py holds to the
sub-corpus oracle), results compared field by field and bit by bit."""
import importlib

import numpy as np
import pytest

from test_gpu_filter_engine import Corpus, make_texts

pytestmark = pytest.mark.gpu

EVERY = [f"doc{d}.pdf" for d in range(12)]
SCOPES = [["doc4.pdf"], ["doc2.pdf", "doc8.pdf", "doc10.pdf"], EVERY, ["no-such.pdf"], ["doc3.pdf", "no-such.pdf"], []]


def key(results):
    f = lambda x: None if x is None else int(np.float32(x).view(np.uint32))  # noqa: E731
    return [(r.row, r.chunk_id, r.document, f(r.score), f(r.embedding_score), f(r.lexical_score), f(r.initial_score))
            for r in results]


@pytest.fixture(scope="module")
def corpus(rlr, oracle):
    mp = pytest.MonkeyPatch()
    mp.setenv("RLR_BATCH_MIN", "2")                          # (read when the index is created)
    try:
        c = Corpus(rlr, oracle, 768, "f32", seed=11)
    finally:
        mp.undo()
    yield c
    c.close()


def queries(c, n, seed):
    return np.stack([c.O.synth_query(c.dim, seed=seed + i) for i in range(n)]).astype(np.float32)


@pytest.mark.parametrize("lam", [0.0, 0.3, 0.7])
def test_a_scoped_batch_equals_its_single_calls(corpus, lam):
    c = corpus
    qs = queries(c, 11, 500)                                 # a chunk of 8 and a chunk of 3
    for docs in SCOPES:
        for k in (7, 100):
            for path in ("list", "scan"):
                if c.rows_of(docs).size:
                    c.eng._filter_for(docs).set_path(path)   # (the engine caches the filter: both routes of the top-k)
                got = c.eng.search_with_diversity_batch(qs, k, lam, documents=docs)
                assert len(got) == len(qs)
                for i, q in enumerate(qs):
                    want = c.eng.search_with_diversity(q, k, lam, documents=docs)
                    assert key(got[i]) == key(want), (docs, k, path, lam, i)
                    if not c.rows_of(docs).size:
                        assert got[i] == []
    # every document = the whole corpus = documents=None
    a = c.eng.search_with_diversity_batch(qs, 10, lam, documents=EVERY)
    b = c.eng.search_with_diversity_batch(qs, 10, lam)
    assert [key(x) for x in a] == [key(x) for x in b]
    # a scope of 4 rows with top_k = 100: clamped
    got = c.eng.search_with_diversity_batch(qs, 100, lam, documents=["doc5.pdf", "doc0.pdf"])
    assert all(len(g) == 4 and {r.document for r in g} <= {"doc5.pdf", "doc0.pdf"} for g in got)
    for i, q in enumerate(qs):
        assert key(got[i]) == key(c.eng.search_with_diversity(q, 100, lam, documents=["doc5.pdf", "doc0.pdf"])), i


def test_the_scoped_batch_shares_a_pass(corpus):
    c = corpus
    qs = queries(c, 8, 900)
    docs = ["doc8.pdf", "doc10.pdf", "doc11.pdf"]
    c.eng._filter_for(docs).set_path("scan")
    c.eng.index.profile_read(reset=True)
    got = c.eng.search_with_diversity_batch(qs, 10, 0.3, documents=docs)
    p = c.eng.index.profile_read()
    assert p.n_batches == 1 and p.n_batch_queries == 8 and p.n_batch_fallbacks == 0, p
    assert all(len(g) == 10 and {r.document for r in g} <= set(docs) for g in got)


def test_search_documents_batch_with_mixed_requests(corpus):
    c, rlr = corpus, corpus.rlr
    qs = queries(c, 12, 600)
    R = rlr.SearchRequest
    small, three = ["doc1.pdf"], ["doc2.pdf", "doc8.pdf", "doc10.pdf"]
    reqs = [
        R(query_embedding=qs[0], query="w000x w001x common"),                                   # unscoped with text
        R(query_embedding=qs[1], documents=small),                                               # scoped without text
        R(query_embedding=qs[2], query="w017x frequent the", documents=three),                  # scoped with text
        R(query_embedding=qs[3], documents=three),                                               # another scope
        R(query_embedding=qs[4], documents=small, top_k=3),
        R(query_embedding=qs[5], documents=three, diversity_factor=0.0),
        R(query_embedding=qs[6], query="common"),
        R(query_embedding=qs[7], documents=small),
        R(query_embedding=qs[8], documents=[]),
        R(query_embedding=qs[9], documents=["no-such.pdf"]),
        R(query_embedding=qs[10], documents=three),
        R(query_embedding=qs[11], documents=three, weights=rlr.QueryWeights(embedding=1.0, lexical=0.0)),
    ]
    got = c.eng.search_documents_batch(reqs)
    assert len(got) == len(reqs)
    for i, r in enumerate(reqs):
        assert key(got[i]) == key(c.eng.search_documents(r)), i
    # a request scoped to a small document returns only that document's chunks (all seven of them: top_k 5, diversity 0.3
    # -> 5 results out of a pool of 7)
    for i in (1, 4, 7):
        assert got[i] and {x.document for x in got[i]} == {"doc1.pdf"}, i
    assert len(got[1]) == 5 and len(got[4]) == 3
    assert got[8] == [] and got[9] == []
    assert {x.document for x in got[3]} <= set(three) and {x.document for x in got[2]} <= set(three)


def test_the_scoped_batch_follows_document_mutations(rlr, oracle):
    mp = pytest.MonkeyPatch()
    mp.setenv("RLR_BATCH_MIN", "2")
    try:
        c = Corpus(rlr, oracle, 768, "f32", seed=21)
    finally:
        mp.undo()
    try:
        qs = queries(c, 5, 700)
        docs = ["doc7.pdf", "doc9.pdf"]

        def check(ctx):
            got = c.eng.search_with_diversity_batch(qs, 10, 0.3, documents=docs)
            for i, q in enumerate(qs):
                want = c.eng.search_with_diversity(q, 10, 0.3, documents=docs)
                assert key(got[i]) == key(want), (ctx, i)
                c.check(got[i], c.expect(docs, q, 10, 0.3, None, 0, 0.7, 0.3), (ctx, i))
                assert {x.document for x in got[i]} <= set(docs), (ctx, i)
            return got

        before = check("before")
        c.eng.remove_document("doc4.pdf")                 # every row behind it moves down by 200
        c.refresh()
        after = check("after remove")
        assert [x.row for x in after[0]] != [x.row for x in before[0]]
        assert [x.chunk_id for x in after[0]] == [x.chunk_id for x in before[0]]
        c.eng.add_document("doc7.pdf", make_texts(40, seed=702), oracle.synth_rows(40, 768, seed=701))
        c.refresh()
        check("after replace")
        n = len(c.eng)
        assert set(c.rows_of(["doc7.pdf"]).tolist()) == set(range(n - 40, n))
    finally:
        c.close()


def test_the_entry_point_checks_its_filter(rlr, oracle):
    """rlr_engine_search_with_diversity_batch_filtered called directly: a filter of another index and a stale filter are
    RLR_E_INVALID, an empty filter is RLR_OK with every n_out = 0 -- the Python layer never reaches these (it returns early
    for empty scopes and rebuilds stale filters)"""
    N = importlib.import_module("rust-local-rag_amd._native")
    L = rlr.lib()
    dim, n, nq, cap = 256, 300, 3, 20
    rows = oracle.synth_rows(n + 10, dim, seed=91)
    qs = np.ascontiguousarray(np.stack([oracle.synth_query(dim, seed=9100 + i) for i in range(nq)]), dtype=np.float32)
    ix, other = rlr.GpuIndex(dim), rlr.GpuIndex(dim)
    try:
        ix.upload(rows[:n])
        other.upload(rows[:n])
        hits = (N.SearchHitC * (cap * nq))()

        def call(index, flt):
            n_out = np.full(nq, 77, dtype=np.uint32)
            st = L.rlr_engine_search_with_diversity_batch_filtered(
                index.handle, flt.handle, qs.ctypes.data_as(N.f32p), dim, nq, 5, 0.3, None, hits, cap, n_out.ctypes.data_as(N.u32p))
            return st, n_out.tolist()

        with ix.filter_ranges([(10, 50)]) as f, other.filter_ranges([(10, 50)]) as g, ix.filter_ranges([(5, 0)]) as empty:
            st, n_out = call(ix, f)
            assert st == 0 and n_out == [5, 5, 5]
            assert all(10 <= hits[q * cap + i].row < 60 for q in range(nq) for i in range(5))   # (rows inside the filter)
            st, n_out = call(ix, g)                              # made for `other`
            assert st == -1 and n_out == [0, 0, 0]
            st, n_out = call(ix, empty)
            assert st == 0 and n_out == [0, 0, 0]
            ix.append(rows[n:])                                  # every filter of ix is stale now
            st, n_out = call(ix, f)
            assert st == -1 and n_out == [0, 0, 0] and b"stale" in L.rlr_last_error()
    finally:
        ix.close()
        other.close()
