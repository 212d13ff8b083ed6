"""GPU BM25 inside a row filter (rlr_lexical_score_filtered).  The filter restricts the candidates, not the corpus
statistics: the expected list is the oracle's unfiltered, untruncated list (`score(q, 0, keep_zero=False)`: global
total_docs, average length, df, idf) reduced to the filter's rows and THEN truncated to the limit -- rows and score bits
exact.  Masked rows are never accumulated, so the dense accumulator and the touched list must be as clean after a
filtered call as after an unfiltered one: every filtered call is followed by an unfiltered one against the oracle."""
import importlib

import numpy as np
import pytest

from oracle import lexical as OL

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


VOCAB = [f"w{i:03d}x" for i in range(400)] + ["common", "frequent", "the", "of", "né", "Straße", "ÉTÉ"]

# the queries and limits of the unfiltered BM25 test
QUERIES = [("w000x", 25), ("w017x w101x", 50), ("W399X, w250x; w250x w003x", 500), ("unknown words only", 10),
           ("né Straße été", 100), ("w005x", 0), ("the of", 1500), ("it is", 5), ("", 5),
           ("w001x w002x w003x w004x w005x w006x w007x w008x w009x w010x w011x", 7)]
QUERIES_MANY = [("ubiquitous", 100), ("ubiquitous", 1500), ("ubiquitous rare w000x", 8192), ("w000x w001x common", 300),
                ("ubiquitous", 0)]


def make_texts(n, seed, lo=3, hi=40, common_every=0):
    rng = np.random.default_rng(seed)
    zipf = 1.0 / np.arange(1, len(VOCAB) + 1)
    zipf /= zipf.sum()
    texts = []
    for i in range(n):
        m = int(rng.integers(lo, hi))
        words = list(rng.choice(VOCAB, size=m, p=zipf))
        if common_every and i % common_every == 0:
            words.append("ubiquitous")
        texts.append(" ".join(words) + (", " if i % 3 else " - "))
    return texts


def build(rlr, texts, dim=8):
    """the GPU lexical index, the oracle, and an embedding index of as many rows (what a filter is made for)"""
    lex = importlib.import_module("rust-local-rag_amd.lexical")
    g = lex.LexicalIndex(0)
    o = OL.LexicalIndex()
    for r, t in enumerate(texts):
        g.add_chunk(r, t)
        o.add_chunk(r, t, rank=r)
    ix = rlr.GpuIndex(dim)
    ix.upload(np.ones((len(texts), dim), np.float32))
    return g, o, ix


def check(g, o, full, query, limit, flt, allowed):
    """filtered against the reduced oracle list, then unfiltered against the oracle (a clean accumulator)"""
    if query not in full:                                                   # one oracle pass per query, shared
        full[query] = o.score(query, 0, keep_zero=False)
    want_all = full[query]
    inside = set(int(r) for r in allowed)
    want = [(c, s) for c, s in want_all if c in inside][: (limit if limit else 8192)]
    rows, sc = g.score(query, limit, filter=flt)
    assert [int(r) for r in rows] == [c for c, _ in want], (query, limit, len(allowed))
    assert np.array_equal(bits(sc), bits([s for _, s in want])), (query, limit, len(allowed))
    want_u = want_all[: (limit if limit else 8192)]
    rows, sc = g.score(query, limit)
    assert [int(r) for r in rows] == [c for c, _ in want_u], (query, limit, "unfiltered after")
    assert np.array_equal(bits(sc), bits([s for _, s in want_u])), (query, limit, "unfiltered after")
    return len(want)


def masks_of(n):
    return {"every_other": np.arange(n)[::2], "one_document": np.arange(n // 3, n // 3 + max(1, n // 5)), "none": np.arange(0)}


@pytest.mark.parametrize("n,terms", [(1500, None), (130, None), (1500, "global")])
def test_filtered_bm25_small_corpora(rlr, monkeypatch, n, terms):
    """touched rows below the one-workgroup sort's capacity; `terms`: the accumulate kernel that adds in device memory
    instead of LDS (RLR_LEX_TERMS=global), the form larger indexes take"""
    if terms:
        monkeypatch.setenv("RLR_LEX_TERMS", terms)
    g, o, ix = build(rlr, make_texts(n, seed=1))
    try:
        full, n_hit = {}, 0
        for name, allowed in masks_of(n).items():
            with ix.filter_rows(allowed) as f:
                for q, lim in QUERIES:
                    got = check(g, o, full, q, lim, f, allowed)
                    n_hit += got
                    assert got == 0 or name != "none"
        assert n_hit > (200 if n > 1000 else 20)
    finally:
        g.close()
        ix.close()


def test_filtered_bm25_select_regime_and_ties(rlr):
    """more than 8192 touched rows without the filter: the sampled / radix selection chain (and its retry), massive exact
    score ties resolved to the lower allowed row; a filter that leaves fewer rows than the limit returns them all"""
    texts = make_texts(40000, seed=2, lo=2, hi=6, common_every=3)
    texts += ["ubiquitous rare"] * 50 + ["rare"] * 3
    n = len(texts)
    g, o, ix = build(rlr, texts)
    try:
        full = {}
        masks = masks_of(n)
        masks["few"] = np.arange(n)[::611]
        for name, allowed in masks.items():
            with ix.filter_rows(allowed) as f:
                for q, lim in QUERIES_MANY:
                    got = check(g, o, full, q, lim, f, allowed)
                    if name == "every_other" and q == "ubiquitous":   # ~6700 allowed rows hold the word
                        assert got >= min(lim if lim else 6000, 6000)
    finally:
        g.close()
        ix.close()


def test_rows_beyond_the_filters_index_are_masked_and_stale_filters_refused(rlr):
    """the lexical index holds rows the filter's index does not (a host that indexed text first): they are masked"""
    texts = make_texts(200, seed=5)
    g, o, ix = build(rlr, texts)
    small = rlr.GpuIndex(8)
    try:
        small.upload(np.ones((150, 8), np.float32))
        with small.filter_ranges([(0, 150)]) as f:
            check(g, o, {}, "w000x w001x common", 0, f, np.arange(150))
        with ix.filter_rows([3, 4]) as f:
            ix.append(np.ones((1, 8), np.float32))
            with pytest.raises(rlr.RlrError) as ei:
                g.score("w000x", 5, filter=f)
            assert ei.value.status == -1 and "stale" in str(ei.value)
    finally:
        g.close()
        ix.close()
        small.close()
