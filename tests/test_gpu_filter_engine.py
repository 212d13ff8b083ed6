"""RagEngine.search / search_with_diversity / search_documents with `documents=`: each result is the reference's search
over the corpus that holds only the chunks of those documents (oracle.search on the sub-corpus, positions mapped back to
index rows).  The candidate universe is the documents' rows -- top_k, initial_k and the MMR pool are clamped by their
number -- while the BM25 statistics stay those of the whole lexical index: the lexical pairs are the oracle's unfiltered,
untruncated list reduced to the documents' rows, cut to 5 x the top_k `search` sees, and re-keyed to sub-corpus positions."""
import importlib

import numpy as np
import pytest

from oracle import lexical as OL

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


VOCAB = [f"w{i:03d}x" for i in range(400)] + ["common", "frequent", "the", "of"]
DOC_LENGTHS = [1, 7, 64, 65, 200, 3, 128, 31, 300, 90, 411, 200]            # 1500 chunks in 12 documents


def make_texts(n, seed, lo=3, hi=40):
    rng = np.random.default_rng(seed)
    zipf = 1.0 / np.arange(1, len(VOCAB) + 1)
    zipf /= zipf.sum()
    return [" ".join(rng.choice(VOCAB, size=int(rng.integers(lo, hi)), p=zipf)) for _ in range(n)]


class Corpus:
    """an engine with its documents, the oracle's view of the same chunks (stored rows, BM25 index, row ranges)"""

    def __init__(self, rlr, oracle, dim, dtype, seed):
        self.rlr, self.O, self.dim = rlr, oracle, dim
        self.eng = rlr.RagEngine(dim, dtype)
        n = sum(DOC_LENGTHS)
        texts, rows = make_texts(n, seed), oracle.synth_rows(n, dim, seed=seed + 1, n_clusters=6)
        at = 0
        for d, m in enumerate(DOC_LENGTHS):
            self.eng.add_document(f"doc{d}.pdf", texts[at:at + m], rows[at:at + m])
            at += m
        self.refresh()

    def refresh(self):
        chunks = self.eng._chunks
        self.stored = self.eng.index.fetch_rows(np.arange(len(chunks)))
        self.olex = OL.LexicalIndex()
        for r, ch in enumerate(chunks):
            self.olex.add_chunk(r, ch.text, rank=r)
        self.lex_full = {}

    def rows_of(self, documents):
        want = set(documents)
        return np.array([r for r, ch in enumerate(self.eng._chunks) if ch.document_name in want], dtype=np.int64)

    def expect(self, documents, q, k, lam, text, stage, w_e, w_l):
        allowed = self.rows_of(documents) if documents is not None else np.arange(len(self.eng._chunks))
        if allowed.size == 0:
            return [], [], [], []
        k_eff = max(k, 1) if lam == 0.0 else max(3 * k, k + 10)
        lex = None
        if text is not None:
            if text not in self.lex_full:
                self.lex_full[text] = self.olex.score(text, 0, keep_zero=False)
            pos = {int(r): i for i, r in enumerate(allowed)}
            lex = [(pos[c], float(s)) for c, s in self.lex_full[text] if c in pos][:5 * k_eff]
        sub = self.stored[allowed]
        if lam == 0.0:
            wr, wc, we, wl = self.O.search(sub, q, k, w_e, w_l, lex=lex, stage=stage)
        else:
            wr, wc, we, wl = self.O.search_with_diversity(sub, q, k, lam, w_e, w_l, lex=lex)
        return list(allowed[wr.astype(np.int64)]), wc, we, wl

    def check(self, got, want, ctx):
        wr, wc, we, wl = want
        assert [g.row for g in got] == [int(r) for r in wr], (ctx, [g.row for g in got][:6], list(wr)[:6])
        assert np.array_equal(bits([g.score for g in got]), bits(wc)), ctx
        assert np.array_equal(bits([g.embedding_score for g in got]), bits(we)), ctx
        assert np.array_equal(bits([g.lexical_score for g in got]), bits(wl)), ctx

    def close(self):
        self.eng.close()


WEIGHTS = [(None, 0.7, 0.3), (dict(embedding=0.0, lexical=1.0), 0.0, 1.0), (dict(embedding=1.0, lexical=0.0), 1.0, 0.0)]
SCOPES = [["doc4.pdf"], ["doc2.pdf", "doc8.pdf", "doc10.pdf"], [f"doc{d}.pdf" for d in range(12)], ["no-such.pdf"],
          ["doc3.pdf", "no-such.pdf"], []]


@pytest.fixture(scope="module")
def corpus(rlr, oracle):
    c = Corpus(rlr, oracle, 768, "f32", seed=11)
    yield c
    c.close()


@pytest.mark.parametrize("text", [None, "w000x w001x common", "w017x frequent the"])
def test_document_scopes_match_the_sub_corpus_oracle(corpus, text):
    c, rlr = corpus, corpus.rlr
    qs = [c.O.synth_query(c.dim, seed=500 + i) for i in range(3)]
    i = 0
    for docs in SCOPES:
        for wts, w_e, w_l in WEIGHTS:
            w = rlr.QueryWeights(**wts) if wts else None
            q = qs[i % len(qs)]
            i += 1
            for stage in (0, 1):
                got = c.eng.search(q, 10, weights=w, stage=stage, query_text=text, documents=docs)
                c.check(got, c.expect(docs, q, 10, 0.0, text, stage, w_e, w_l), ("search", docs, wts, stage, text))
            for lam in (0.0, 0.3, 1.0):
                got = c.eng.search_with_diversity(q, 7, lam, weights=w, query_text=text, documents=docs)
                c.check(got, c.expect(docs, q, 7, lam, text, 0, w_e, w_l), ("diversity", docs, wts, lam, text))
            req = rlr.SearchRequest(query_embedding=q, top_k=12, diversity_factor=0.3, weights=w, query=text, documents=docs)
            c.check(c.eng.search_documents(req), c.expect(docs, q, 12, 0.3, text, 0, w_e, w_l), ("documents", docs, wts, text))
    # unknown names contribute no rows; an empty list is "no rows", not "no filter"
    assert c.eng.search(qs[0], 5, query_text=text, documents=["no-such.pdf"]) == []
    assert c.eng.search_with_diversity(qs[0], 5, 0.3, query_text=text, documents=[]) == []
    # every document = the whole corpus: what documents=None returns (the statistics are global either way)
    every = [f"doc{d}.pdf" for d in range(12)]
    for lam in (0.0, 0.3):
        a = c.eng.search_with_diversity(qs[1], 10, lam, query_text=text, documents=every)
        b = c.eng.search_with_diversity(qs[1], 10, lam, query_text=text)
        assert [(x.row, bits([x.score])[0], bits([x.lexical_score])[0]) for x in a] == \
               [(x.row, bits([x.score])[0], bits([x.lexical_score])[0]) for x in b], lam
        c.check(b, c.expect(None, qs[1], 10, lam, text, 0, 0.7, 0.3), ("documents=None", lam, text))


def test_caller_supplied_pairs_are_blended_inside_the_documents(corpus):
    """lexical=(chunk_id, score) pairs computed by the caller instead of a query text"""
    c = corpus
    q = c.O.synth_query(c.dim, seed=600)
    docs = ["doc6.pdf", "doc9.pdf"]
    allowed = c.rows_of(docs)
    inside = [(int(allowed[3]), 2.5), (int(allowed[40]), 1.25), (int(allowed[41]), 2.5)]
    pairs = [(c.eng._chunks[r].id, s) for r, s in inside]
    pos = {int(r): i for i, r in enumerate(allowed)}
    for lam in (0.0, 0.4):
        got = c.eng.search_with_diversity(q, 8, lam, lexical=pairs, documents=docs)
        sub = c.stored[allowed]
        lex = [(pos[r], s) for r, s in inside]
        if lam == 0.0:
            wr, wc, we, wl = c.O.search(sub, q, 8, lex=lex)
        else:
            wr, wc, we, wl = c.O.search_with_diversity(sub, q, 8, lam, lex=lex)
        c.check(got, (list(allowed[wr.astype(np.int64)]), wc, we, wl), ("pairs", lam))


def test_sizes_are_clamped_by_the_documents_rows(corpus):
    """a one-chunk document: top_k 5 with lambda 0.3 asks the reference for a pool of 15 and initial_k 15 -- of one row"""
    c = corpus
    q = c.O.synth_query(c.dim, seed=601)
    for text in (None, "w000x common"):
        got = c.eng.search_with_diversity(q, 5, 0.3, query_text=text, documents=["doc0.pdf"])
        assert len(got) == 1 and got[0].document == "doc0.pdf"
        c.check(got, c.expect(["doc0.pdf"], q, 5, 0.3, text, 0, 0.7, 0.3), ("one chunk", text))
        got = c.eng.search(q, 5, stage=1, query_text=text, documents=["doc1.pdf"])       # initial_k = min(7, 15)
        assert len(got) == 7
        c.check(got, c.expect(["doc1.pdf"], q, 5, 0.0, text, 1, 0.7, 0.3), ("seven chunks", text))
        got = c.eng.search(q, 100, query_text=text, documents=["doc5.pdf", "doc0.pdf"])   # top_k clamped to 4 rows
        assert len(got) == 4


def test_scopes_follow_document_mutations(rlr, oracle):
    """the engine caches a filter per set of names: add_document / remove_document must drop it (rows are renumbered)"""
    c = Corpus(rlr, oracle, 768, "f32", seed=21)
    try:
        q = oracle.synth_query(768, seed=700)
        docs = ["doc7.pdf", "doc9.pdf"]
        text = "w002x w003x common"
        before = c.eng.search(q, 10, query_text=text, documents=docs)
        c.check(before, c.expect(docs, q, 10, 0.0, text, 0, 0.7, 0.3), "before")
        c.eng.remove_document("doc4.pdf")                 # every row behind it moves down by 200
        c.refresh()
        after = c.eng.search(q, 10, query_text=text, documents=docs)
        c.check(after, c.expect(docs, q, 10, 0.0, text, 0, 0.7, 0.3), "after remove")
        assert [r.row for r in after] != [r.row for r in before]
        assert [r.chunk_id for r in after] != [] and {r.document for r in after} <= set(docs)
        new_rows = oracle.synth_rows(40, 768, seed=701)
        c.eng.add_document("doc7.pdf", make_texts(40, seed=702), new_rows)   # replaces doc7: its rows are the last 40 now
        c.refresh()
        again = c.eng.search_with_diversity(q, 10, 0.3, query_text=text, documents=docs)
        c.check(again, c.expect(docs, q, 10, 0.3, text, 0, 0.7, 0.3), "after replace")
        n = len(c.eng)
        assert set(c.rows_of(["doc7.pdf"]).tolist()) == set(range(n - 40, n))
        c.check(c.eng.search(q, 10, query_text=text), c.expect(None, q, 10, 0.0, text, 0, 0.7, 0.3), "documents=None")
    finally:
        c.close()


def test_binary16_rows(rlr, oracle):
    c = Corpus(rlr, oracle, 1024, "f16", seed=31)
    try:
        q = oracle.synth_query(1024, seed=800)
        for docs in (["doc8.pdf"], ["doc1.pdf", "doc10.pdf", "doc11.pdf"]):
            for text in (None, "w001x w005x the"):
                got = c.eng.search(q, 10, stage=1, query_text=text, documents=docs)
                c.check(got, c.expect(docs, q, 10, 0.0, text, 1, 0.7, 0.3), ("f16 search", docs, text))
                got = c.eng.search_with_diversity(q, 10, 0.3, query_text=text, documents=docs)
                c.check(got, c.expect(docs, q, 10, 0.3, text, 0, 0.7, 0.3), ("f16 diversity", docs, text))
    finally:
        c.close()
