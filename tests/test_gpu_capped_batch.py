"""rlr_search_capped_batch on the device: every query of a batch held to rlr_search_capped called with that query alone
and to the definition of tests/capped_vectors.py (oracle.scan, the f32 blend, the walk in combined order, the greedy MMR
over the accepted pool) -- rows, cosine, combined, lexn, document ids and n_out as bit patterns.  The batch forms counter
says WHICH path answered: [0] decided on the device behind a shared scan, handed to the single path [1] on a capacity, [2]
as undecidable there, [3] by rule.  Sharing is forced (mode 2) unless a test says otherwise; the forms are read back after
every call and held to what the workspace rule and the split (tests/grouped_batch_vectors.py) leave to the chunks.

Shapes: 256 and 768 f32 elements at 65 and 4097 rows (one word and a bit, more than one workgroup); batches of 2, 3, 8 and
9 queries; per_doc 1, 3, 8; diversity 0, 0.3, 1.0.  At 768 elements eight queries fit a chunk for every per_doc, so 9
queries are 5 + 4; at 256 x 4097 and per_doc 8 the workspace rule narrows the chunk to 3, at 256 x 65 it leaves none."""
import ctypes as C
import threading

import numpy as np
import pytest

import capped_batch_vectors as CB
import capped_vectors as V
import document_vectors as DV
import grouped_batch_vectors as W
import grouped_vectors as G
import mmr_restatement as M
from conftest import bits

pytestmark = pytest.mark.gpu
F32 = np.float32
NONE = (np.zeros(0, np.uint64), np.zeros(0, np.float32))


def same_f32(got, want):
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    return got.shape == want.shape and bool(np.all((bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want))))


def same_answer(a, b):
    return (np.array_equal(a[0], b[0]) and same_f32(a[1], b[1]) and same_f32(a[2], b[2]) and same_f32(a[3], b[3]) and
            np.array_equal(a[4], b[4]))


def lex_pairs(n, n_lex, seed):
    rng = np.random.default_rng(seed)
    rows = np.sort(rng.choice(n, size=min(n_lex, n), replace=False)).astype(np.uint64)
    return rows, (rng.random(rows.size) * 7.0 + 0.01).astype(np.float32)


class Corpus:
    """an index, its rows on the host, a pool of queries and their reference-order scores, made once"""

    def __init__(self, rlr, O, dim, n, n_queries, seed, rows=None, queries=None):
        self.O, self.dim, self.n = O, dim, n
        self.rows = O.synth_rows(n, dim, seed=seed) if rows is None else rows
        self.qs = np.stack([O.normalize(O.synth_query(dim, seed=seed + 1 + i)) for i in range(n_queries)]) if queries is None else queries
        self.e = np.stack([O.scan(self.rows, q) for q in self.qs])
        self.ix = rlr.GpuIndex(dim, "f32")
        self.ix.upload(self.rows)
        self.ix.set_capped_sharing(2)

    def shared_forms(self, nq, m, n_allowed=None, by_rule=0):
        """the forms of nq queries the device can decide, `by_rule` of them (inside shared chunks) sent alone by rule"""
        w = W.chunk_width(self.n, self.dim * 4, self.n if n_allowed is None else n_allowed, m)
        shared, lone = W.forms_by_rule(nq, w)
        return [shared - by_rule, 0, 0, lone + by_rule] if shared else [0, 0, 0, nq]

    def want(self, q, docs, lr, ls, ml, w_e, w_l, need, m, k, lam, allowed):
        pool = V.define(self.e[q], docs, lr, ls, w_e, w_l, need, m, allowed, max_lex=ml)
        if lam != 0.0 and pool["rows"].size:
            order, _ = M.mmr_from_gram(M.gram(self.O, self.rows[pool["rows"].astype(np.int64)]), pool["comb"], k, lam)
            pool = {key: v[order] for key, v in pool.items()}
        return pool

    def check(self, sel, docs, lex, w_e, w_l, top_k, m, lam, forms, ctx, allowed=None, filter=None, guard_eps=-1.0, need=None,
              mode=2, max_lex=None, single=True):
        """the batch == the single entry per query == the definition; the forms counter == `forms` (None: not held)"""
        ix = self.ix
        sel = list(sel)
        n_allowed = V.allowed_rows(self.n, allowed).size
        diversify = lam != 0.0
        need = V.need_of(n_allowed, top_k, 0, diversify) if need is None else need
        ml = [float(V.max_lex_of(ls)) for _, ls in lex] if max_lex is None else list(max_lex)
        kw = dict(k=top_k, lam=lam, diversify=diversify, w_embedding=w_e, w_lexical=w_l, filter=filter, guard_eps=guard_eps)
        ix.set_capped_sharing(mode)
        ix.capped_batch_forms(reset=True)
        got = ix.search_capped_batch(self.qs[sel], need, m, lex_rows=[lr for lr, _ in lex], lex_scores=[ls for _, ls in lex],
                                     max_lex=ml, **kw)
        counted = ix.capped_batch_forms()
        ix.set_capped_sharing(2)
        assert len(got) == len(sel)
        for i, q in enumerate(sel):
            lr, ls = lex[i]
            if single:
                one = ix.search_capped(self.qs[q], need, m, lex_rows=lr, lex_scores=ls, max_lex=ml[i], **kw)
                assert same_answer(got[i], one), (ctx, i, "single", counted, got[i][0][:8], one[0][:8])
            want = self.want(q, docs, lr, ls, ml[i], w_e, w_l, need, m, top_k, lam, allowed)
            r, cos, comb, lexn, d = got[i]
            assert np.array_equal(r, want["rows"]), (ctx, i, counted, r[:8], want["rows"][:8])
            assert same_f32(comb, want["comb"]) and same_f32(cos, want["cos"]) and same_f32(lexn, want["lexn"]), (ctx, i, counted)
            assert np.array_equal(d, want["docs"]), (ctx, i, counted)
        if forms is not None:
            assert counted == list(forms), (ctx, counted, forms)
        assert sum(counted) == len(sel), (ctx, counted)
        return got

    def close(self):
        self.ix.close()


@pytest.fixture(scope="module")
def corpus_of(rlr, oracle):
    made = {}

    def get(dim, n, n_queries=9):
        key = (dim, n)
        if key not in made:
            made[key] = Corpus(rlr, oracle, dim, n, n_queries, seed=0x7D00 + n + dim)
        assert made[key].qs.shape[0] >= n_queries
        return made[key]

    yield get
    for c in made.values():
        c.close()


def id_patterns(n):
    r = np.arange(n)
    return [("consecutive", (r // 5).astype(np.uint32)), ("random_1000_documents", DV.random_1000(n)),
            ("all_one_document", np.full(n, 7, np.uint32)),
            ("mostly_untagged", np.where(r % 7 == 0, r % 3, G.DOC_NONE).astype(np.uint32)),
            ("colliding_ids", ((r % 1000).astype(np.uint32) << 20) | 5), ("own_documents", r.astype(np.uint32) + 5)]


# ---- equals the single entry and the definition ---------------------------------------------------------------------------
@pytest.mark.parametrize("dim,n", [(256, 65), (256, 4097), (768, 65), (768, 4097)])
def test_every_batch_equals_the_single_entry_and_the_definition(corpus_of, dim, n):
    cp = corpus_of(dim, n)
    combos = [(nq, m, lam) for nq in (2, 3, 8, 9) for m in (1, 3, 8) for lam in (0.0, 0.3, 1.0)]   # 36
    for p, (name, ids) in enumerate(id_patterns(n)):
        cp.ix.set_documents(ids)
        for j in range(2):                                   # every (batch, per_doc, diversity) over the patterns and shapes
            nq, m, lam = combos[(7 * (2 * p + j) + 5 * (dim // 256) + n) % len(combos)]
            top_k = (5, 100, 1)[(p + j) % 3]
            n_lex = (0, 1, 50, 500)[(p + 2 * j) % 4]
            w_e, w_l = ((0.7, 0.3), (0.3, 0.7), (1.0, 0.0))[(p + j) % 3]
            lex = [lex_pairs(n, n_lex if i % 3 else n_lex // 2, seed=n + 100 * p + 10 * j + i) for i in range(nq)]
            forms = cp.shared_forms(nq, m)
            if dim == 768 and n == 4097:
                assert forms == [nq, 0, 0, 0]                # eight queries a chunk for every per_doc; 9 = 5 + 4
            cp.check(range(nq), ids, lex, w_e, w_l, top_k, m, lam, forms, (dim, n, name, nq, m, lam, top_k, n_lex))


def test_nine_queries_are_five_and_four_and_the_lone_remainder_goes_by_rule(corpus_of):
    cp = corpus_of(768, 4097)
    ids = (np.arange(4097) // 5).astype(np.uint32)
    cp.ix.set_documents(ids)
    assert W.chunk_width(4097, 768 * 4, 4097, 8) == 8 and W.split(9, 8) == [5, 4]
    lex = [lex_pairs(4097, 50, seed=i) for i in range(9)]
    cp.check(range(9), ids, lex, 0.7, 0.3, 5, 8, 0.3, [9, 0, 0, 0], "nine: 8 + 1 would send one query by rule")
    small = corpus_of(256, 65)
    ids = (np.arange(65) // 5).astype(np.uint32)
    small.ix.set_documents(ids)
    assert W.chunk_width(65, 1024, 65, 3) == 2 and W.split(3, 2) == [2, 1]
    small.check(range(3), ids, [lex_pairs(65, 5, seed=i) for i in range(3)], 0.7, 0.3, 5, 3, 0.0, [2, 0, 0, 1], "the lone remainder")
    assert W.chunk_width(65, 1024, 65, 8) == 0
    small.check(range(3), ids, [NONE] * 3, 0.7, 0.3, 5, 8, 0.0, [0, 0, 0, 3], "no width of two within the workspace rule")


# ---- the lexical slices ----------------------------------------------------------------------------------------------------
def test_zero_one_2048_and_2049_lexical_rows_and_a_negative_score_in_one_chunk(corpus_of):
    cp = corpus_of(768, 4097)
    ids = DV.random_1000(4097)
    cp.ix.set_documents(ids)
    neg = lex_pairs(4097, 50, seed=3)
    neg[1][7] = -1.0
    lex = [NONE, lex_pairs(4097, 1, seed=1), lex_pairs(4097, 2048, seed=2), lex_pairs(4097, 2049, seed=4), neg]
    assert [lr.size for lr, _ in lex] == [0, 1, 2048, 2049, 50]
    for lam in (0.0, 0.3):                                   # the 2049 rows and the negative score go by rule, alone
        cp.check(range(5), ids, lex, 0.7, 0.3, 5, 2, lam, [3, 0, 0, 2], ("lexical counts", lam))
    # max_lex per query: a non-positive and a NaN normaliser send their queries alone, the neighbours stay
    lex = [lex_pairs(4097, 20, seed=i) for i in range(4)]
    ix = cp.ix
    ix.capped_batch_forms(reset=True)
    got = ix.search_capped_batch(cp.qs[:4], 5, 2, w_embedding=0.7, w_lexical=0.3, lex_rows=[l[0] for l in lex],
                                 lex_scores=[l[1] for l in lex], max_lex=[3.0, 0.0, np.nan, 7.5])
    assert ix.capped_batch_forms() == [2, 0, 0, 2]
    for i, ml in enumerate([3.0, 0.0, np.nan, 7.5]):
        one = ix.search_capped(cp.qs[i], 5, 2, w_embedding=0.7, w_lexical=0.3, lex_rows=lex[i][0], lex_scores=lex[i][1], max_lex=ml)
        assert same_answer(got[i], one), i


def test_each_query_reads_its_own_slice_and_normaliser(corpus_of):
    """the same cosines for every query (one query, repeated): only the lexical slices and max_lex tell the answers apart"""
    cp = corpus_of(768, 4097)
    ids = (np.arange(4097) // 5).astype(np.uint32)
    cp.ix.set_documents(ids)
    lex = [lex_pairs(4097, nl, seed=40 + i) for i, nl in enumerate((30, 7, 0, 200, 30, 1))]
    lex[4] = (lex[0][0], lex[0][1])                          # the pairs of query 0 under another normaliser
    ml = [float(V.max_lex_of(ls)) for _, ls in lex]
    ml[4] = 4.0 * ml[0]
    got = cp.check([0] * 6, ids, lex, 0.3, 0.7, 5, 1, 0.0, [6, 0, 0, 0], "slices", max_lex=ml)
    assert len({tuple(g[0].tolist()) for g in got}) >= 5 and not same_f32(got[0][3], got[4][3])


# ---- pools shorter than need, under MMR ------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,n", [(256, 4097), (768, 65)])
def test_pools_shorter_than_need_under_mmr(corpus_of, dim, n):
    """three documents, two rows each at the most: every pool of the chunk holds 6 of its 15 / 25 slots (the column is the
    call's, so the pools of a chunk run short together) and the greedy launch reads each size from the finish"""
    cp = corpus_of(dim, n)
    ids = (np.arange(n) % 3).astype(np.uint32)
    cp.ix.set_documents(ids)
    lex = [lex_pairs(n, 20, seed=i) for i in range(4)]
    for top_k, lam in ((5, 0.3), (15, 1.0), (15, 0.0)):     # need 15, 45, 15
        got = cp.check(range(4), ids, lex, 0.7, 0.3, top_k, 2, lam, cp.shared_forms(4, 2), ("short pools", dim, top_k, lam))
        assert all(g[0].size == min(6, top_k) for g in got)


# ---- hand-backs: one query, its neighbours stay ------------------------------------------------------------------------------
def designed_chunk(n=2200, dim=256):
    """Eight unit queries e_0 .. e_7 over rows whose component q IS the row's score for query q (every dot product exact).
    Query 0: capped_vectors' rounding tie (rows 0..9), undecidable under the 5e-9 band.  Query 1: every row scores 0.01 --
    2200 candidates, more than the finish holds.  Queries 2..7: five rows well apart at the top, decided.  The rows the
    designed scores live on are untagged (a band below one ulp closes no tagged group); the last 100 rows, at the bottom
    of every ranking, carry document ids."""
    t = V.case_rounding_tie_outside_the_band()
    rows = np.zeros((n, dim), np.float32)
    r = np.arange(n)
    rows[:, 0] = F32(0.001) + r.astype(np.float32) * F32(1.0e-7)
    rows[:10, 0] = t["e"]
    rows[:, 1] = F32(0.01)
    for q in range(2, 8):
        rows[:, q] = F32(0.001) + ((r * 7 + q) % n).astype(np.float32) * F32(1.0e-7)
        rows[20 * q:20 * q + 8, q] = F32(0.02) - np.arange(8, dtype=np.float32) * F32(1.0e-4)
    ids = np.full(n, G.DOC_NONE, np.uint32)
    ids[-100:] = (np.arange(100) // 4 + 3).astype(np.uint32)
    rows[-100:, :8] *= F32(0.5)
    rows[-100:, 1] = F32(0.01)
    queries = np.eye(8, dim, dtype=np.float32)
    return rows, ids, queries, t


def test_a_boundary_tie_and_an_overflow_hand_back_two_queries_of_eight(rlr, oracle):
    """(The third hand-back of a chunk, a NaN row that is wanted, cannot stand in this chunk: a nomination that is NaN for
    one query only needs an infinite row element, which widens the call's band until every row is a candidate, and a NaN
    row is only wanted when need reaches the rows, at most 1024, while an overflow takes more than 2048 candidates.  It
    has the next test.)"""
    rows, ids, queries, t = designed_chunk()
    assert float(np.sqrt((rows.astype(np.float64) ** 2).sum(axis=1).max())) <= 1.0      # the band is the caller's 5e-9
    cp = Corpus(rlr, oracle, 256, rows.shape[0], 0, seed=0, rows=rows, queries=queries)
    try:
        assert all(same_f32(cp.e[q], rows[:, q]) for q in range(8))
        cp.ix.set_documents(ids)
        model = [CB.single_device_path(cp.e[q], cp.e[q], ids, [], [], t["w_e"], 0.0, 5, 1, t["eps"])[0] for q in range(8)]
        assert model == [2, 1, 0, 0, 0, 0, 0, 0]              # the design holds in the restated device path
        cp.ix.capped_forms(reset=True)
        got = cp.check(range(8), ids, [NONE] * 8, t["w_e"], 0.0, 5, 1, 0.0, [6, 1, 1, 0], "tie and overflow", guard_eps=t["eps"],
                       need=5, single=False)
        assert cp.ix.capped_forms() == [0, 1, 1, 0]          # the two were answered by the single path, each once
        assert got[0][0].tolist() == [1, 2, 3, 4, 0] and got[1][0].tolist() == [0, 1, 2, 3, 4]
        assert got[5][0].tolist() == list(range(100, 105))
        # the same chunk with the MMR chain behind the finish, held to the single entry as well
        cp.check(range(8), ids, [NONE] * 8, t["w_e"], 0.0, 2, 1, 0.3, [6, 1, 1, 0], "tie and overflow, diversified",
                 guard_eps=t["eps"], need=5)
    finally:
        cp.close()


def special_corpus(O):
    """Row 123 holds +Inf in element 2, row 124 -Inf in element 3.  Query 0 = e_0 has zeros there: both rows score NaN for
    it (Inf * 0) and for it alone.  Queries 1..3 have a negative element 2 and a positive element 3: both rows score -Inf,
    numbers at the bottom of the ranking.  Query 4 is all positive: row 123 scores +Inf and leads.  (An infinite element
    makes the call's band infinite: every row is a candidate, and a group whose per_doc-th value is +Inf has no number
    for a bound, so query 4 is handed to the exact form by the finish -- the single path's behaviour, held as bits only.)"""
    rows = O.synth_rows(300, 256, seed=31)
    q0 = np.zeros(256, np.float32)
    q0[0] = 1.0
    rows[:, 0] = -np.abs(rows[:, 0]) - F32(0.001)            # every other score against q0 is negative ...
    rows[[5, 6, 150], 0] = 0.0                               # ... these score +0
    rows[7] = 0.0
    rows[8, 0] = -0.0                                        # (a -0 product: the sum is +0 all the same)
    pos = O.normalize(np.abs(O.synth_query(256, seed=42)) + F32(0.01))
    neg, other = pos.copy(), O.normalize(O.synth_query(256, seed=43))
    neg[2] = -neg[2]
    other[2], other[3] = -abs(other[2]) - F32(0.01), abs(other[3]) + F32(0.01)
    rows[123, 2] = np.inf
    rows[124, 3] = -np.inf
    return rows, (np.arange(300) // 3).astype(np.uint32), np.stack([q0, neg, other, neg, pos])


def test_zeros_infinities_and_a_nan_row_that_is_wanted(rlr, oracle):
    rows, ids, queries = special_corpus(oracle)
    cp = Corpus(rlr, oracle, 256, 300, 0, seed=0, rows=rows.copy(), queries=queries)
    try:
        cp.ix.set_documents(ids)
        assert np.isnan(cp.e[0][[123, 124]]).all() and (cp.e[1:4, 123:125] == -np.inf).all() and cp.e[4][123] == np.inf
        assert (cp.e[0][[5, 6, 7, 8, 150]] == 0.0).all() and np.isnan(cp.e).sum(axis=1).tolist() == [2, 0, 0, 0, 0]
        lex = [lex_pairs(300, 10, seed=i) for i in range(4)]
        # need = 10 leaves the NaN rows out of every answer: nobody is short, everybody is decided on the device
        got = cp.check(range(4), ids, [NONE] * 4, 1.0, 0.0, 10, 1, 0.0, [4, 0, 0, 0], "zeros and -inf")
        assert got[0][0][:3].tolist() == [5, 6, 150]
        cp.check(range(4), ids, lex, 0.7, 0.3, 10, 3, 0.3, [4, 0, 0, 0], "zeros and -inf, lexical, diversified")
        # need = every row: query 0 -- the only one with NaN nominations -- is short and is handed back, alone
        got = cp.check(range(4), ids, lex, 0.7, 0.3, 300, 8, 0.0, [3, 0, 1, 0], "the NaN rows are wanted")
        assert got[0][0].size == 300 and sorted(got[0][0][-2:].tolist()) == [123, 124] and np.isnan(got[0][1][-2:]).all()
        assert got[1][0].size == 300 and sorted(got[1][0][-2:].tolist()) == [123, 124] and (got[1][1][-2:] == -np.inf).all()
        # +Inf at the top of a ranking, beside the NaN query: the bits of the single entry and of the definition
        got = cp.check([0, 4], ids, [NONE] * 2, 1.0, 0.0, 10, 1, 0.0, None, "+inf leads")
        assert got[1][0][0] == 123 and got[1][1][0] == np.inf
    finally:
        cp.close()


# ---- filters -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,n", [(256, 4097), (768, 65)])
def test_inside_a_filter_on_both_paths(rlr, corpus_of, dim, n):
    cp = corpus_of(dim, n)
    ix = cp.ix
    ids = (np.arange(n) // 5).astype(np.uint32)
    ix.set_documents(ids)
    docs = np.unique(ids)[::2]
    allowed = np.flatnonzero(np.isin(ids, docs))
    lex = [lex_pairs(n, 40, seed=70 + i) for i in range(3)]  # (pairs inside and outside the filter)
    assert any((~np.isin(lr.astype(np.int64), allowed)).any() for lr, _ in lex)
    with ix.filter_documents(docs) as f:
        f.set_path("scan")
        cp.check(range(3), ids, lex, 0.7, 0.3, 5, 2, 0.3, cp.shared_forms(3, 2, allowed.size), (dim, "mask path"), allowed=allowed,
                 filter=f)
        f.set_path("list")                                   # the whole call by rule
        cp.check(range(3), ids, lex, 0.7, 0.3, 5, 2, 0.3, [0, 0, 0, 3], (dim, "list path"), allowed=allowed, filter=f)
    with ix.filter_rows(np.arange(0, n, 3)) as f:            # a row filter that cuts across documents
        f.set_path("scan")
        allowed = np.arange(0, n, 3)
        cp.check(range(2), ids, lex[:2], 0.3, 0.7, 5, 1, 0.0, cp.shared_forms(2, 1, allowed.size), (dim, "every third row"),
                 allowed=allowed, filter=f)
    with ix.filter_documents([0xABCDEF]) as f:               # an empty filter: RLR_OK, no result, no query counted
        ix.capped_batch_forms(reset=True)
        got = ix.search_capped_batch(cp.qs[:3], 5, 1, filter=f)
        assert all(g[0].size == 0 for g in got) and sum(ix.capped_batch_forms()) == 0


def test_a_stale_filter_is_refused(rlr, oracle):
    rows = oracle.synth_rows(70, 256, seed=5)
    ix = rlr.GpuIndex(256)
    try:
        ix.upload(rows)
        qs = rows[:2].copy()
        with ix.filter_rows([1, 2, 3]) as f:
            assert [g[0].size for g in ix.search_capped_batch(qs, 5, 1, filter=f)] == [3, 3]
            ix.append(rows[:2])
            with pytest.raises(rlr.RlrError) as ei:
                ix.search_capped_batch(qs, 5, 1, filter=f)
            assert ei.value.status == -1
    finally:
        ix.close()


# ---- identities --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,n", [(256, 65), (768, 4097)])
def test_an_index_without_a_column_equals_search_hybrid(rlr, oracle, dim, n):
    N = rlr._native
    cp = Corpus(rlr, oracle, dim, n, 3, seed=0x7E00 + n)
    compared = 0
    try:
        for (m, k, lam, nl), (w_e, w_l) in zip([(1, 1, 0.0, 0), (2, 5, 0.3, 50), (3, 100, 1.0, 500)], ((0.7, 0.3), (0.3, 0.7), (1.0, 0.0))):
            lex = [lex_pairs(n, nl, seed=n + nl + i) for i in range(3)]
            need = V.need_of(n, k, 0, lam != 0.0)
            got = cp.check(range(3), None, lex, w_e, w_l, k, m, lam, cp.shared_forms(3, m), (n, "no column", m, k, lam, nl))
            for i, (lr, ls) in enumerate(lex):
                cap = max(need, 1)
                rows, cos, comb, lexn = np.zeros(cap, np.uint64), *(np.zeros(cap, np.float32) for _ in range(3))
                n_out, fb = C.c_uint32(), C.c_int32()
                st = N.lib().rlr_search_hybrid(cp.ix.handle, cp.qs[i].ctypes.data_as(N.f32p), need, k, lam, int(lam != 0.0), w_e, w_l,
                                               lr.ctypes.data_as(N.u64p) if lr.size else None,
                                               ls.ctypes.data_as(N.f32p) if ls.size else None, lr.size, float(V.max_lex_of(ls)), -1.0,
                                               rows.ctypes.data_as(N.u64p), cos.ctypes.data_as(N.f32p), comb.ctypes.data_as(N.f32p),
                                               lexn.ctypes.data_as(N.f32p), C.byref(n_out), C.byref(fb))
                assert st == 0
                if fb.value == 0:                            # (a hand-back of the uncapped entry says nothing about this one)
                    k_out = n_out.value
                    assert np.array_equal(rows[:k_out], got[i][0]) and same_f32(cos[:k_out], got[i][1])
                    assert same_f32(comb[:k_out], got[i][2]) and same_f32(lexn[:k_out], got[i][3])
                    compared += 1
                assert (got[i][4] == G.DOC_NONE).all()
        assert compared >= 1, "the uncapped entry handed every call back: nothing was compared"
    finally:
        cp.close()


# ---- rules ---------------------------------------------------------------------------------------------------------------------
def test_by_rule_every_query_goes_to_the_single_path(rlr, oracle, corpus_of):
    cp = corpus_of(768, 4097)
    ids = (np.arange(4097) // 5).astype(np.uint32)
    cp.ix.set_documents(ids)
    lex = [lex_pairs(4097, 50, seed=i) for i in range(3)]
    for w_e, w_l in ((0.0, 0.3), (-0.5, 0.3), (0.7, -0.25)):  # weights outside the proof's assumptions
        cp.check(range(3), ids, lex, w_e, w_l, 5, 2, 0.3, [0, 0, 0, 3], ("weights", w_e, w_l))
    cp.check(range(2), ids, lex[:2], 0.7, 0.3, 400, 2, 0.3, [0, 0, 0, 2], "need above 1024")
    cp.check(range(1), ids, lex[:1], 0.7, 0.3, 5, 2, 0.0, [0, 0, 0, 1], "one query")
    ix = rlr.GpuIndex(256, "f16")                            # binary16 rows: no shared scan serves them
    try:
        rows = oracle.synth_rows(4100, 256, seed=77, f16=True)
        ix.upload(rows)
        ix.set_documents((np.arange(4100) // 5).astype(np.uint32))
        ix.set_capped_sharing(2)
        qs = np.stack([oracle.normalize(oracle.synth_query(256, seed=80 + i)) for i in range(2)])
        lr, ls = lex_pairs(4100, 50, seed=1)
        got = ix.search_capped_batch(qs, 5, 2, w_embedding=0.7, w_lexical=0.3, lex_rows=[lr, lr], lex_scores=[ls, ls],
                                     max_lex=[float(ls.max())] * 2)
        assert ix.capped_batch_forms() == [0, 0, 0, 2]
        for i in range(2):
            assert same_answer(got[i], ix.search_capped(qs[i], 5, 2, w_embedding=0.7, w_lexical=0.3, lex_rows=lr, lex_scores=ls,
                                                        max_lex=float(ls.max())))
    finally:
        ix.close()


def test_argument_rules(rlr, corpus_of):
    cp = corpus_of(256, 65)
    other = corpus_of(768, 65)
    N = rlr._native
    ix = cp.ix
    qs = cp.qs[:2]
    for bad in (0, 9):
        with pytest.raises(rlr.RlrError) as ei:
            ix.search_capped_batch(qs, 5, bad)
        assert ei.value.status == -1
    for bad_rows in ([5, 5], [7, 3], [65]):                  # repeated, descending, outside the index -- in the SECOND query
        with pytest.raises(rlr.RlrError) as ei:
            ix.search_capped_batch(qs, 5, 1, lex_rows=[[1, 2], bad_rows], lex_scores=[[1.0, 2.0], [1.0] * len(bad_rows)])
        assert ei.value.status == -1
    # the end of one query's rows above the start of the next is no error: every slice ascends on its own
    assert len(ix.search_capped_batch(qs, 5, 1, lex_rows=[[60, 61], [1, 2]], lex_scores=[[1.0, 2.0], [1.0, 2.0]])) == 2
    assert all(g[0].size == 0 for g in ix.search_capped_batch(qs, 0, 1))        # need = 0: nothing asked for
    assert ix.search_capped_batch(np.zeros((0, 256), np.float32), 5, 1) == []
    with other.ix.filter_rows([1, 2, 3]) as f, pytest.raises(rlr.RlrError) as ei:
        ix.search_capped_batch(qs, 5, 1, filter=f)            # another index's filter
    assert ei.value.status == -1
    # offsets that decrease, through the C ABI
    rows, cos, comb, lexn = np.zeros(10, np.uint64), *(np.zeros(10, np.float32) for _ in range(3))
    n_out = np.zeros(2, np.uint32)
    lr, ls = np.asarray([1, 2], np.uint64), np.asarray([1.0, 2.0], np.float32)
    for off, status in (([0, 2, 1], -1), ([0, 1, 2], 0)):
        off = np.asarray(off, np.uint64)
        st = N.lib().rlr_search_capped_batch(ix.handle, None, qs.ctypes.data_as(N.f32p), 2, 5, 0, 0.0, 0, 0.7, 0.3, lr.ctypes.data_as(N.u64p),
                                             ls.ctypes.data_as(N.f32p), off.ctypes.data_as(N.u64p), np.ones(2, np.float32).ctypes.data_as(N.f32p),
                                             1, -1.0, rows.ctypes.data_as(N.u64p), cos.ctypes.data_as(N.f32p), comb.ctypes.data_as(N.f32p),
                                             lexn.ctypes.data_as(N.f32p), None, n_out.ctypes.data_as(N.u32p))
        assert st == status
    for mode in (-1, 3):
        with pytest.raises(rlr.RlrError) as ei:
            ix.set_capped_sharing(mode)
        assert ei.value.status == -1
    ix.set_capped_sharing(2)


# ---- the context afterwards, threads, modes ------------------------------------------------------------------------------------
def test_other_searches_after_a_capped_batch_on_the_same_context(rlr, oracle):
    rows = oracle.synth_rows(4097, 768, seed=0x7F00)
    ids = (np.arange(4097) // 5).astype(np.uint32)
    qs = np.stack([oracle.normalize(oracle.synth_query(768, seed=0x7F01 + i)) for i in range(8)])
    lr, ls = lex_pairs(4097, 50, seed=9)

    def others(ix):
        plain = ix.search_topk(qs[0], 10)
        capped = ix.search_capped(qs[1], 25, 2, k=5, lam=0.3, diversify=True, w_embedding=0.7, w_lexical=0.3, lex_rows=lr,
                                  lex_scores=ls, max_lex=float(ls.max()))
        grouped = ix.search_topk_grouped_batch(qs[:3], 10, 2)
        return plain, capped, grouped

    def flat(res):
        plain, capped, grouped = res
        return [np.asarray(a) for a in plain] + list(capped) + [a for g in grouped for a in g]

    made = []
    try:
        for used in (False, True):
            ix = rlr.GpuIndex(768)
            made.append(ix)
            ix.upload(rows)
            ix.set_documents(ids)
            ix.set_capped_sharing(2)
            ix.set_grouped_sharing(2)
            if used:
                for lam in (0.0, 0.3):
                    ix.capped_batch_forms(reset=True)
                    ix.search_capped_batch(qs, 25, 2, k=5, lam=lam, diversify=lam != 0.0, w_embedding=0.7, w_lexical=0.3,
                                           lex_rows=[lr] * 8, lex_scores=[ls] * 8, max_lex=[float(ls.max())] * 8)
                    assert ix.capped_batch_forms() == [8, 0, 0, 0]
            made.append(flat(others(ix)))
        fresh, after = made[1], made[3]
        assert len(fresh) == len(after)
        for a, b in zip(fresh, after):
            a, b = np.asarray(a), np.asarray(b)
            assert a.dtype == b.dtype and a.tobytes() == b.tobytes()
    finally:
        for ix in made[::2]:
            ix.close()


def test_four_threads_return_what_the_serial_calls_return(corpus_of):
    cp = corpus_of(768, 4097)
    ix = cp.ix
    ids = DV.random_1000(4097)
    ix.set_documents(ids)
    lex = [[lex_pairs(4097, 50, seed=10 * t + i) for i in range(4)] for t in range(4)]

    def call(t):
        sel = [(t + i) % 9 for i in range(4)]
        return ix.search_capped_batch(cp.qs[sel], 25, 2, k=5, lam=0.3, diversify=True, w_embedding=0.7, w_lexical=0.3,
                                      lex_rows=[l[0] for l in lex[t]], lex_scores=[l[1] for l in lex[t]],
                                      max_lex=[float(l[1].max()) for l in lex[t]])

    serial = [call(t) for t in range(4)]
    errors = []

    def work(t):
        try:
            for _ in range(10):
                got = call(t)
                if not all(same_answer(a, b) for a, b in zip(got, serial[t])):
                    errors.append(t)
        except Exception as e:                               # noqa: BLE001 (reported below)
            errors.append(e)

    ix.capped_batch_forms(reset=True)
    threads = [threading.Thread(target=work, args=(t,)) for t in range(4)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    assert ix.capped_batch_forms() == [160, 0, 0, 0]


def test_modes_one_and_zero_return_the_bits_of_mode_two(corpus_of):
    cp = corpus_of(768, 4097)
    ids = (np.arange(4097) // 5).astype(np.uint32)
    cp.ix.set_documents(ids)
    lex = [lex_pairs(4097, 50, seed=i) for i in range(8)]
    for lam in (0.0, 0.3):
        two = cp.check(range(8), ids, lex, 0.7, 0.3, 5, 2, lam, [8, 0, 0, 0], ("mode 2", lam), single=False)
        one = cp.check(range(8), ids, lex, 0.7, 0.3, 5, 2, lam, [0, 0, 0, 8], ("mode 1", lam), mode=1, single=False)
        zero = cp.check(range(8), ids, lex, 0.7, 0.3, 5, 2, lam, None, ("mode 0", lam), mode=0, single=False)
        assert all(same_answer(a, b) and same_answer(a, c) for a, b, c in zip(two, one, zero))


# ---- the engine ------------------------------------------------------------------------------------------------------------------
WORDS = ["alpha", "beta", "gamma", "delta", "kernel", "wave", "cache", "tensor", "matrix", "vector", "stream", "queue"]


def _engine(rlr, rng, dim=256):
    eng = rlr.RagEngine(dim)
    for name, n in {"a.pdf": 40, "b.pdf": 7, "c.pdf": 1, "d.pdf": 25, "e.pdf": 30}.items():
        texts = [" ".join(rng.choice(WORDS, size=6)) + f" {name[0]}{i}" for i in range(n)]
        eng.add_document(name, texts, rng.standard_normal((n, dim)).astype(np.float32))
    return eng


def _same_results(a, b):
    return len(a) == len(b) and all(
        x.row == y.row and x.document == y.document and bits(F32(x.score)) == bits(F32(y.score)) and
        bits(F32(x.embedding_score)) == bits(F32(y.embedding_score)) and bits(F32(x.lexical_score)) == bits(F32(y.lexical_score))
        for x, y in zip(a, b))


def test_engine_batches_equal_the_per_request_methods(rlr):
    rng = np.random.default_rng(47)
    eng = _engine(rlr, rng)
    try:
        eng.index.set_capped_sharing(2)
        qs = (2.0 * rng.standard_normal((5, 256))).astype(np.float32)
        texts = ["kernel wave cache", "tensor", "", "matrix vector stream queue", "alpha beta"]
        eng.index.capped_batch_forms(reset=True)
        for names in (None, ["a.pdf", "d.pdf", "e.pdf"], ["nothing.pdf"]):
            for top_k, div, m in ((5, 0.3, 2), (3, 0.0, 1), (10, 1.0, 3)):
                got = eng.search_text_batch(qs, texts, top_k, div, documents=names, per_document=m)
                for i in range(5):
                    one = eng.search_with_diversity(qs[i], top_k, div, query_text=texts[i], documents=names, per_document=m)
                    assert _same_results(got[i], one), ("text", names, top_k, div, m, i)
                    counts = {}
                    for g in got[i]:
                        counts[g.document] = counts.get(g.document, 0) + 1
                    assert all(v <= m for v in counts.values())
                got = eng.search_with_diversity_batch(qs, top_k, div, documents=names, per_document=m)
                for i in range(5):
                    assert _same_results(got[i], eng.search_with_diversity(qs[i], top_k, div, documents=names, per_document=m))
        got = eng.search_text_batch(qs, texts, 4, 0.0, stage=1, per_document=1)
        for i in range(5):
            assert _same_results(got[i], eng.search(qs[i], 4, query_text=texts[i], stage=1, per_document=1))
        assert eng.index.capped_batch_forms()[0] > 0          # shared chunks have run
        with pytest.raises(ValueError):
            eng.search_text_batch(qs, texts, 5, per_document=2, scopes=[["a.pdf"]] * 5)
        with pytest.raises(ValueError):
            eng.search_with_diversity_batch(qs, 5, 0.3, per_document=2, scopes=[["a.pdf"]] * 5)
        with pytest.raises(ValueError):
            eng.search_text_batch(qs, texts, 5, per_document=9)
        # None keeps the uncapped batch
        plain = eng.search_text_batch(qs, texts, 3, 0.3)
        assert all(_same_results(p, eng.search_with_diversity(qs[i], 3, 0.3, query_text=texts[i])) for i, p in enumerate(plain))
        # search_documents_batch: capped requests of one key share a call, a lone one and the uncapped ones route as before
        R = rlr.engine.SearchRequest
        reqs = [R(qs[0], 5, 0.3, None, (), texts[0], None, 2), R(qs[1], 5, 0.3, None, (), texts[1], None, 2),
                R(qs[2], 5, 0.3, None, (), texts[3], ["a.pdf", "e.pdf"], 2), R(qs[3], 5, 0.3, None, (), texts[3], ["e.pdf", "a.pdf"], 2),
                R(qs[4], 5, 0.3, None, (), texts[4], None, 1), R(qs[0], 5, 0.3, None, (), texts[0], None, None),
                R(qs[1], 5, 0.3, None, (), None, None, 2), R(qs[2], 5, 0.3, None, (), None, None, 2)]
        want = [eng.search_documents(r) for r in reqs]
        eng.index.capped_batch_forms(reset=True)
        for share in (False, True):
            got = eng.search_documents_batch(reqs, share_capped=share)
            assert all(_same_results(g, w) for g, w in zip(got, want)), share
            assert sum(eng.index.capped_batch_forms()) == (6 if share else 0)   # three batched calls of two; the lone one not
    finally:
        eng.close()
