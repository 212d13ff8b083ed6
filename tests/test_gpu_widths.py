"""Every path that returns a reference-order score, at the row widths where its re-score changes form (width_vectors.py:
the dispatch restated, the ladder, the corpora; test_width_vectors_cpu.py: why a wrong re-score shows on them).

Everything is bit for bit against the oracle: one oracle.scan per (corpus, query), shared by all paths (width_vectors.case);
rows compared in order, scores as uint32 patterns, every NaN as the one quiet NaN the result unpacking writes.  The corpora
hold an all-zero row, a row with +Inf and a row with NaN in the last column: the device has to rank them as the oracle does.
A row of infinite norm also scales the guard band by the largest float (csrc/index.hip: plan_bands), so that on the
single-query paths every row that scores a number is a candidate and is re-scored, whatever k."""
import numpy as np
import pytest

import width_vectors as W
from test_gpu_lexical import make_texts
from test_gpu_parity import make_index, oracle_topk
from test_gpu_tail import MODES, tail_mode

pytestmark = pytest.mark.gpu

DTYPES = ("f32", "f16")
pb = W.pattern_bits


def check_topk(got, scores, k, ctx):
    r, c = got
    wr, wc = W.topk(scores, k)
    assert r.shape == (1, len(wr)), (ctx, r.shape)
    assert np.array_equal(r[0], wr), (ctx, r[0][:8], wr[:8])
    assert np.array_equal(pb(c[0]), pb(wc)), (ctx, c[0][:8], wc[:8])


# ---------------------------------------------------------------- single-query search, every tail form
@pytest.mark.parametrize("dtype,dim,mode", [(t, d, m) for t in DTYPES for d in W.LADDER["single"][t] for m in MODES])
def test_single_query_search_at_every_ladder_width(rlr, oracle, dtype, dim, mode):
    rows, qs, scores = W.case(W.N_SINGLE, dim, dtype == "f16")
    n = rows.shape[0]
    with tail_mode(mode):
        ix = make_index(rlr, rows, dtype=dtype)
    try:
        ix.profile_read(reset=True)
        for k in (1, 10, n):
            for i, q in enumerate(qs):
                check_topk(ix.search_topk(q, k), scores[i], k, (W.form("split" if mode == "split" else "tail", dim, dtype), k, i))
        assert ix.profile_read().n_retries == 0          # no query left the form under test for the large-candidate path
    finally:
        ix.close()


# ---------------------------------------------------------------- the large-candidate path
@pytest.mark.parametrize("dtype,dim", [(t, d) for t in DTYPES for d in (1, 2, 3, 13, 101, 1592)])
def test_large_candidate_path_rescore(rlr, oracle, dtype, dim):
    """k beyond the one-workgroup sort: big_query collects every row at or above the band floor and re-scores it through
    rescore_kernel (one lane per row), whatever the width; one retry per query"""
    assert W.form("big", dim, dtype) == ("rescore_kernel", 0)
    rows, qs, scores = W.case(W.N_BIG, dim, dtype == "f16", nq=2)
    k = W.LDS_SORT_CAP + 4
    ix = make_index(rlr, rows, dtype=dtype)
    try:
        for i, q in enumerate(qs):
            ix.profile_read(reset=True)
            check_topk(ix.search_topk(q, k), scores[i], k, (dim, dtype, i))
            assert ix.profile_read().n_retries == 1
            wr, wc = oracle_topk(oracle, rows, q, 10)     # and an ordinary query on the same contexts afterwards
            r, c = ix.search_topk(q, 10)
            assert np.array_equal(r[0], wr) and np.array_equal(pb(c[0]), pb(wc))
    finally:
        ix.close()


# ---------------------------------------------------------------- rlr_score_rows, both kernels
@pytest.mark.parametrize("dtype,dim", [(t, d) for t in DTYPES for d in W.LADDER["score_rows"][t]])
def test_score_rows_at_every_ladder_width(rlr, oracle, dtype, dim):
    rows, qs, scores = W.case(W.N_SINGLE, dim, dtype == "f16")
    n = rows.shape[0]
    rng = np.random.default_rng([8400, dim])
    ix = make_index(rlr, rows, dtype=dtype)
    try:
        for length in (1, W.SCORE_ROWS_STAGED_MIN - 1, W.SCORE_ROWS_STAGED_MIN, n):
            for i, q in enumerate(qs):
                lst = rng.permutation(n)[:length]
                if length > 1:
                    lst[-1] = lst[0]                      # shuffled, one row twice
                got = ix.score_rows(q, lst)
                path = "score_rows" if length >= W.SCORE_ROWS_STAGED_MIN else "score_rows_small"
                assert np.array_equal(pb(got), pb(scores[i][lst])), (W.form(path, dim, dtype), length, i)
    finally:
        ix.close()


# ---------------------------------------------------------------- the batched pipeline
BATCH = [(t, img, d) for t, img in (("f32", False), ("f32", True), ("f16", False)) for d in W.LADDER["batch"][t]]


@pytest.mark.parametrize("dtype,image,dim", sorted(BATCH, key=lambda c: (c[0], c[2], c[1])))
def test_batched_pipeline_at_every_batched_width(rlr, oracle, monkeypatch, dtype, image, dim):
    """9 queries, and the first 3 of them (no batched width has the shape the shared scan of 2..8 queries takes --
    csrc/index.hip: batch_multi_shape wants f32 rows of 256 / 512 / 768 / 1024 columns -- so both go through the GEMM
    nomination), k = 100: one batch, no query handed back, every query's rows and score bits the oracle's"""
    monkeypatch.setenv("RLR_BATCH_MIN", "2")              # (read at index creation)
    rows, qs, scores = W.case(W.N_BATCH, dim, dtype == "f16", nq=9, inf_row=False)
    assert dim not in (256, 512, 768, 1024)
    ix = make_index(rlr, rows, dtype=dtype)
    try:
        if image:
            ix.enable_batch_image(True)                   # accepted at every batched width (dim % 64 == 0)
        for nq in (9, 3):
            ix.profile_read(reset=True)
            r, c = ix.search_topk(qs[:nq], 100)
            p = ix.profile_read()
            assert p.n_batches == 1 and p.n_batch_queries == nq and p.n_batch_fallbacks == 0 and p.n_retries == 0, p
            assert r.shape == (nq, 100)
            for i in range(nq):
                wr, wc = W.topk(scores[i], 100)
                ctx = (W.form("batch", dim, dtype), nq, i)
                assert np.array_equal(r[i], wr), ctx
                assert np.array_equal(pb(c[i]), pb(wc)), ctx
    finally:
        ix.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_batched_pipeline_with_a_row_of_infinite_norm(rlr, oracle, monkeypatch, dtype):
    """what keeps the +Inf row out of the batched corpora above: an f32 index that holds an element beyond binary16 range
    stays on the f32 paths (no batch); over binary16 rows the band, scaled by the infinite row norm, takes in more rows than
    the finish re-scores and every query is handed back to the single-query pipeline.  The results are the oracle's either way."""
    monkeypatch.setenv("RLR_BATCH_MIN", "2")
    rows, qs, scores = W.case(W.N_BATCH, 128, dtype == "f16", nq=9)
    ix = make_index(rlr, rows, dtype=dtype)
    try:
        ix.profile_read(reset=True)
        r, c = ix.search_topk(qs, 100)
        p = ix.profile_read()
        if dtype == "f32":
            assert p.n_batches == 0 and p.n_batch_fallbacks == 0, p
        else:
            assert p.n_batches == 1 and p.n_batch_fallbacks == len(qs), p
        for i in range(len(qs)):
            wr, wc = W.topk(scores[i], 100)
            assert np.array_equal(r[i], wr) and np.array_equal(pb(c[i]), pb(wc)), i
    finally:
        ix.close()


# ---------------------------------------------------------------- row filters, both paths
def one_width_per_class(dtype):
    by_class = {}
    for w in W.LADDER["score_rows"][dtype]:
        by_class.setdefault(W.form("score_rows", w, dtype), w)     # the narrowest ladder width of the class
    return sorted(by_class.values())


# (7680: the one-lane class again, where it is the width and not the pitch that refuses the staged form)
FILTERED = [("f32", d) for d in sorted({5, 13, 101, 7680} | set(one_width_per_class("f32")))] + \
           [("f16", d) for d in sorted({100, 7680} | set(one_width_per_class("f16")))]


@pytest.mark.parametrize("dtype,dim", FILTERED)
def test_filtered_search_on_both_paths(rlr, oracle, dtype, dim):
    """the list path scores the allowed rows through launch_score_rows (more than 64 of them: staged where it fits), the
    masked scan nominates over the rows as stored (scan_masked_generic_kernel at these widths) and the tail re-scores"""
    rows, qs, scores = W.case(W.N_SINGLE, dim, dtype == "f16")
    n = rows.shape[0]
    rng = np.random.default_rng([8500, dim])
    allowed = np.sort(np.r_[np.arange(W.N_SPECIAL), W.N_SPECIAL + rng.choice(n - W.N_SPECIAL, 99, replace=False)])
    ix = make_index(rlr, rows, dtype=dtype)
    try:
        with ix.filter_rows(allowed[::-1]) as f:
            assert f.info()["n_allowed"] == len(allowed) and f.info()["path"] == "list"
            for path in ("list", "scan"):
                f.set_path(path)
                for k in (1, 10, len(allowed)):
                    for i, q in enumerate(qs):
                        r, c = ix.search_topk(q, k, filter=f)
                        wr, wc = W.topk(scores[i][allowed], k)
                        ctx = (path, k, i)
                        assert r.shape == (1, k), ctx
                        assert np.array_equal(r[0], allowed[wr.astype(np.int64)].astype(np.uint64)), ctx
                        assert np.array_equal(pb(c[0]), pb(wc)), ctx
    finally:
        ix.close()


# ---------------------------------------------------------------- hybrid engine search
@pytest.mark.parametrize("dtype,dim", [("f32", 13), ("f32", 101), ("f16", 100)])
def test_hybrid_engine_search_with_lexical_pairs(rlr, oracle, dtype, dim):
    """the lexical rows of a hybrid search are scored by launch_score_rows (hybrid_finish_impl: up to 5 k of them -- k = 5
    stays on the one-lane kernel, k = 20 takes the staged one), those of search_text_batch by score_rows_batch_kernel;
    against oracle.search given the oracle's lexical pairs, as test_gpu_lexical.py does at round widths"""
    from oracle import lexical as OL
    rows, qs, _ = W.case(W.N_SINGLE, dim, dtype == "f16")
    n = rows.shape[0]
    texts = make_texts(n, seed=dim)
    o = OL.LexicalIndex()
    eng = rlr.RagEngine(dim, dtype)
    try:
        eng.index.upload(rows)
        eng._chunks = [rlr.DocumentChunk(str(i), "d", texts[i], i) for i in range(n)]
        eng._row_of = {str(i): i for i in range(n)}
        for r, t in enumerate(texts):
            eng.lexical.add_chunk(r, t)
            o.add_chunk(r, t, rank=r)
        stored = eng.index.fetch_rows(np.arange(n))
        assert np.array_equal(pb(stored), pb(rows))

        def check(got, q, k, text):
            pairs = [(c, float(s)) for c, s in o.score(text, 5 * k, keep_zero=False)]
            wr, wc, we, wl = oracle.search(rows, q, k, lex=pairs)
            ctx = (k, text, len(pairs))
            assert [g.row for g in got] == list(wr), ctx
            assert np.array_equal(pb([g.score for g in got]), pb(wc)), ctx
            assert np.array_equal(pb([g.embedding_score for g in got]), pb(we)), ctx
            assert np.array_equal(pb([g.lexical_score for g in got]), pb(wl)), ctx
            return len(pairs)

        text = "w004x w005x w006x w007x w008x w009x w010x"      # (more than 100 chunks hold one of them, none holds half)
        for k in (5, 20):
            for q in qs:
                assert check(eng.search(q, k, query_text=text), q, k, text) == 5 * k
        batch_texts = [text, "w020x", "w012x frequent", "nothing known here"]
        for k in (5, 20):
            for got, q, t in zip(eng.search_text_batch(qs, batch_texts, k), qs, batch_texts):
                check(got, q, k, t)
    finally:
        eng.close()
