"""The batched BM25 chain under a row mask (rlr_lexical_score_batch_filtered): every query of a batch is held to the
oracle's unfiltered, untruncated list reduced to the allowed rows and then cut to the limit -- rows and score bits -- and,
bit for bit, to LexicalIndex.score(filter=) for the same text.  Every filtered batch is followed by an unfiltered one
against the oracle: the masked chain must leave nothing behind.  Masks and sizes are built around the accumulate kernel's
2048-row slices (32 mask words each) and the 64-row mask words."""
import numpy as np
import pytest

import text_batch_filtered_vectors as V
from test_gpu_filter_lexical import build, make_texts

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def check_batch(g, o, full, texts, limit, flt, allowed, n_single=0, singles=True):
    """filtered batch against the reduced oracle lists and the single filtered call, then an unfiltered batch"""
    for t in set(texts):
        if t not in full:                                                   # one oracle pass per text, shared
            full[t] = o.score(t, 0, keep_zero=False)
    inside = set(int(r) for r in allowed)
    got, info = g.score_batch(texts, limit, return_info=True, filter=flt)
    assert info["n_single"] == n_single and len(got) == len(texts)
    n_hit, done = 0, {}
    for i, (t, (rows, sc)) in enumerate(zip(texts, got)):
        want = [(c, s) for c, s in full[t] if c in inside][:limit]
        assert [int(r) for r in rows] == [c for c, _ in want], (i, t, limit, len(allowed))
        assert np.array_equal(bits(sc), bits([s for _, s in want])), (i, t, limit, len(allowed))
        mx = max([float(s) for _, s in want] + [0.0])
        assert info["max_lexical"][i] == np.float32(mx if mx >= 1.1920929e-07 else 1.1920929e-07), (i, t)
        if singles and t not in done:                                       # the single call, once per text
            done[t] = g.score(t, limit, filter=flt)
        if singles:
            assert np.array_equal(rows, done[t][0]) and np.array_equal(bits(sc), bits(done[t][1])), (i, t, limit)
        n_hit += len(want)
    for t, (rows, sc) in zip(texts, g.score_batch(texts, limit)):            # nothing of the mask is left behind
        want = full[t][:limit]
        assert [int(r) for r in rows] == [c for c, _ in want], (t, limit, "unfiltered after")
        assert np.array_equal(bits(sc), bits([s for _, s in want])), (t, limit, "unfiltered after")
    return n_hit


@pytest.fixture(scope="module")
def small(rlr):
    texts = make_texts(V.LEX_ROWS, seed=7)
    g, o, ix = build(rlr, texts)
    yield g, o, ix, {}, V.lex_masks(V.LEX_ROWS, texts)
    g.close()
    ix.close()


@pytest.mark.parametrize("name", sorted(V.lex_masks(V.LEX_ROWS)))
def test_masks_around_slices_and_mask_words(small, name):
    g, o, ix, full, masks = small
    allowed = masks[name]
    n_hit = 0
    with ix.filter_rows(allowed) as f:
        for limit, n in zip(V.LIMITS, (9, 2, 1, 9)):
            n_hit += check_batch(g, o, full, V.lex_batch(n), limit, f, allowed)
    assert (n_hit == 0) == (name == "none")


def test_a_batch_beyond_one_sub_batch_and_a_query_of_129_terms(small):
    g, o, ix, full, masks = small
    allowed = masks["every_other"]
    texts = V.lex_batch(257)
    texts[200] = V.MANY_TERMS                                               # more than 128 unique known terms: scored alone
    with ix.filter_rows(allowed) as f:
        assert check_batch(g, o, full, texts, 5, f, allowed, n_single=1, singles=False) > 500
        assert check_batch(g, o, full, [V.MANY_TERMS, "w000x"], 150, f, allowed, n_single=1) >= 150


def test_rows_beyond_the_filters_index_are_masked(rlr, small):
    """an embedding index of 4100 rows under the 4200-row lexical index: index_rows falls inside the third slice and inside
    a mask word (4100 = 64 * 64 + 4), and rows 4100 .. 4199 hold postings"""
    g, o, _, full, _ = small
    ix = rlr.GpuIndex(8)
    try:
        ix.upload(np.ones((V.SMALL_INDEX, 8), np.float32))
        for allowed in (np.arange(V.SMALL_INDEX), np.arange(4090, V.SMALL_INDEX), np.arange(V.SMALL_INDEX)[::3]):
            with ix.filter_rows(allowed) as f:
                assert check_batch(g, o, full, V.lex_batch(9), 8192, f, allowed) > 0
                check_batch(g, o, full, V.lex_batch(2), 5, f, allowed)
    finally:
        ix.close()


def test_stale_and_foreign_filters_are_refused(rlr, small):
    g, o, _, full, _ = small
    ix = rlr.GpuIndex(8)
    other = None
    try:
        ix.upload(np.ones((V.LEX_ROWS, 8), np.float32))
        with ix.filter_rows([3, 4, 2050]) as f:
            check_batch(g, o, full, V.lex_batch(2), 5, f, [3, 4, 2050])
            ix.append(np.ones((1, 8), np.float32))
            with pytest.raises(rlr.RlrError) as ei:
                g.score_batch(V.lex_batch(2), 5, filter=f)
            assert ei.value.status == -1 and "stale" in str(ei.value)
        if rlr.device_count() > 1:                                          # a filter that lives on another device
            other = rlr.GpuIndex(8, device=1)
            other.upload(np.ones((V.LEX_ROWS, 8), np.float32))
            with other.filter_rows([3, 4]) as f:
                with pytest.raises(rlr.RlrError) as ei:
                    g.score_batch(V.lex_batch(2), 5, filter=f)
                assert ei.value.status == -1 and "device" in str(ei.value)
        with ix.filter_rows([]) as f:                                       # an empty filter: no pairs, no error
            got, info = g.score_batch(V.lex_batch(3), 5, return_info=True, filter=f)
            assert [len(r) for r, _ in got] == [0, 0, 0] and info["n_single"] == 0
    finally:
        ix.close()
        if other is not None:
            other.close()


def test_select_regimes_and_exact_ties(rlr):
    """the 40 000-row recipe of test_filtered_bm25_select_regime_and_ties: a filter that leaves more than 8192 rows with the
    common word (the batched radix passes), every other row (the LDS sort, ~6700 keys), and fewer rows than the limit"""
    texts = make_texts(40000, seed=2, lo=2, hi=6, common_every=3)
    texts += ["ubiquitous rare"] * 50 + ["rare"] * 3
    n = len(texts)
    g, o, ix = build(rlr, texts)
    try:
        full = {}
        batch = ["ubiquitous", "ubiquitous rare w000x", "w000x w001x common", "rare", "ubiquitous"]
        masks = {"most": np.delete(np.arange(n), np.arange(0, n, 7)), "every_other": np.arange(n)[::2], "few": np.arange(n)[::611]}
        for name, allowed in masks.items():
            with ix.filter_rows(allowed) as f:
                for limit in V.LIMITS:
                    got = check_batch(g, o, full, batch, limit, f, allowed)
                    if name == "most":                                      # 6/7 of ~13 350 rows hold the word: > 8192 keys
                        assert sum(1 for c, _ in full["ubiquitous"] if c % 7) > 8192 and got >= 2 * limit
    finally:
        g.close()
        ix.close()
