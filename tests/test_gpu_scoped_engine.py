"""RagEngine.search_with_diversity_batch(scopes=...) and search_documents_batch(share_scopes=True): every query of a
batch equals the single call of the same query with ITS OWN scope (which test_gpu_filter_engine.py holds to the sub-corpus
oracle), results compared field by field and bit by bit -- on the list path the filters of a 1500-chunk corpus take by
themselves, and forced onto the masked scan, where chunks of up to 8 queries share one pass over the union of their
scopes."""
import numpy as np
import pytest

from test_gpu_filter_engine import Corpus

pytestmark = pytest.mark.gpu

EVERY = [f"doc{d}.pdf" for d in range(12)]
# large documents, the 7-chunk document (the MMR pool is clamped to 7), an unknown document (no hits), [] (no hits), the
# 1- and 3-chunk documents (top_k 5 is clamped), two scopes that share a document, the whole corpus
SCOPES = [["doc10.pdf"], ["doc1.pdf"], ["no-such.pdf"], ["doc8.pdf", "doc4.pdf"], [], ["doc0.pdf"], ["doc5.pdf", "doc0.pdf"],
          ["doc8.pdf", "doc11.pdf"], EVERY, ["doc3.pdf", "no-such.pdf"], ["doc2.pdf", "doc6.pdf", "doc9.pdf"]]


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


def force(c, scopes, path):
    for docs in scopes:
        if c.rows_of(docs).size:
            c.eng._filter_for(docs).set_path(path)           # (the engine caches the filter: both routes of the top-k)


@pytest.fixture(scope="module")
def singles(corpus):
    """the single calls, computed once per (query, scope, top_k, diversity) and shared by both routes"""
    cache = {}

    def want(qs, i, docs, k, lam):
        at = (i, tuple(docs), k, lam)
        if at not in cache:
            cache[at] = key(corpus.eng.search_with_diversity(qs[i], k, lam, documents=docs))
        return cache[at]
    return want


@pytest.mark.parametrize("lam", [0.0, 0.3, 1.0])
@pytest.mark.parametrize("path", ["list", "scan"])
def test_a_batch_with_a_scope_per_query_equals_its_single_calls(corpus, singles, path, lam):
    c = corpus
    qs = queries(c, 19, 500)                                  # 19 queries over 11 scopes: every scope at least once
    scopes = [SCOPES[i % len(SCOPES)] for i in range(len(qs))]
    force(c, SCOPES, path)
    for k in (5, 100):
        got = c.eng.search_with_diversity_batch(qs, k, lam, scopes=scopes)
        assert len(got) == len(qs)
        for i in range(len(qs)):
            assert key(got[i]) == singles(qs, i, scopes[i], k, lam), (path, lam, k, i, scopes[i])
            assert {r.document for r in got[i]} <= set(scopes[i]), (path, lam, k, i)
            if not c.rows_of(scopes[i]).size:
                assert got[i] == []
    # the 7-chunk document: top_k 5 with diversity keeps 5 of a pool of 7, top_k 100 all 7
    got = c.eng.search_with_diversity_batch(qs[:2], 5, lam, scopes=[["doc1.pdf"], ["doc10.pdf"]])
    assert len(got[0]) == 5 and len(got[1]) == 5


def test_the_scoped_batch_shares_a_pass_over_the_union(corpus):
    c = corpus
    qs = queries(c, 8, 900)
    scopes = [["doc8.pdf"], ["doc10.pdf"], ["doc11.pdf"], ["doc8.pdf", "doc4.pdf"]] * 2
    force(c, scopes, "scan")
    c.eng.index.profile_read(reset=True)
    got = c.eng.search_with_diversity_batch(qs, 10, 0.3, scopes=scopes)
    p = c.eng.index.profile_read()
    assert p.n_batches == 1 and p.n_batch_queries == 8 and p.n_batch_fallbacks == 0, p
    assert all(len(g) == 10 and {r.document for r in g} <= set(s) for g, s in zip(got, scopes))


def test_scopes_and_documents_exclude_each_other(corpus):
    qs = queries(corpus, 2, 950)
    with pytest.raises(ValueError):
        corpus.eng.search_with_diversity_batch(qs, 5, 0.3, documents=["doc1.pdf"], scopes=[["doc1.pdf"], []])
    with pytest.raises(ValueError):
        corpus.eng.search_with_diversity_batch(qs, 5, 0.3, scopes=[["doc1.pdf"]])


@pytest.mark.parametrize("path", ["list", "scan"])
def test_search_documents_batch_sharing_scopes(corpus, path):
    """a mix of scoped and unscoped requests with and without text: with share_scopes=True every request still equals its
    search_documents call"""
    c, rlr = corpus, corpus.rlr
    qs = queries(c, 14, 600)
    R = rlr.SearchRequest
    small, three, big = ["doc1.pdf"], ["doc2.pdf", "doc8.pdf", "doc10.pdf"], ["doc10.pdf"]
    force(c, [small, three, big, ["doc4.pdf"]], path)
    reqs = [
        R(query_embedding=qs[0], query="w000x w001x common"),                                   # unscoped with text
        R(query_embedding=qs[1], documents=small),                                               # scoped without text
        R(query_embedding=qs[2], query="w017x frequent the", documents=three),                  # scoped with text
        R(query_embedding=qs[3], documents=three),                                               # another scope
        R(query_embedding=qs[4], documents=small, top_k=3),
        R(query_embedding=qs[5], documents=three, diversity_factor=0.0),
        R(query_embedding=qs[6], query="common"),
        R(query_embedding=qs[7], documents=big),
        R(query_embedding=qs[8], documents=[]),
        R(query_embedding=qs[9], documents=["no-such.pdf"]),
        R(query_embedding=qs[10], documents=["doc4.pdf"]),
        R(query_embedding=qs[11], documents=three, weights=rlr.QueryWeights(embedding=1.0, lexical=0.0)),
        R(query_embedding=qs[12], documents=big, weights=rlr.QueryWeights(embedding=1.0, lexical=0.0)),
        R(query_embedding=qs[13]),                                                               # unscoped without text
    ]
    got = c.eng.search_documents_batch(reqs, share_scopes=True)
    assert len(got) == len(reqs)
    for i, r in enumerate(reqs):
        assert key(got[i]) == key(c.eng.search_documents(r)), (path, i)
    assert [key(g) for g in c.eng.search_documents_batch(reqs)] == [key(g) for g in got]        # ... and the default routing
    for i in (1, 4):
        assert got[i] and {x.document for x in got[i]} == {"doc1.pdf"}, i
    assert len(got[1]) == 5 and len(got[4]) == 3
    assert got[8] == [] and got[9] == []
    assert {x.document for x in got[7]} == {"doc10.pdf"} and {x.document for x in got[10]} == {"doc4.pdf"}
