"""rlr_search_topk_grouped_batch on the device: every query of a batch held to rlr_search_topk_grouped called with that
query alone -- rows equal, score bits equal, document ids equal, n_out equal -- AND to the model of tests/grouped_vectors.py
over oracle.scan; the batch forms counter says WHICH path answered: [0] selected on the device behind a shared scan, handed
to the single-query path [1] on a capacity, [2] for a NaN nomination / a masked row / the workspace, [3] by rule.  Sharing
is forced (mode 2) unless a test says otherwise, and the forms are read back after every call.

Shapes, the smallest at which the shared chunk can still go wrong: 256-d and 768-d f32 (the shapes the shared scans
serve) at 65 rows (one wave plus one row) and 4097 (a partial workgroup, more than one collect workgroup); 2, 3, 8, 9 and
17 queries (every instance of the shared scan, a split 5 + 4, three chunks); per_doc 1, 3, 8 (one round, several, the
most: at 256-d x 4097 rows the workspace rule narrows the chunk to 3).  What the forms must be follows from the workspace
rule and the split of tests/grouped_batch_vectors.py."""
import threading

import numpy as np
import pytest

import grouped_batch_vectors as W
import grouped_vectors as G
from conftest import bits

pytestmark = pytest.mark.gpu

F32 = np.float32


def same_scores(got, want):
    """bit equality; a NaN equals a NaN (the library returns the canonical quiet NaN for every NaN score)"""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    return got.shape == want.shape and bool(np.all((bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want))))


class Corpus:
    """an index, its rows on the host, a pool of queries and their reference-order scores, made once"""

    def __init__(self, rlr, O, dim, dtype, n, n_queries, seed, rows=None, queries=None):
        self.O, self.dim, self.n = O, dim, n
        self.rows = O.synth_rows(n, dim, seed=seed, f16=dtype == "f16") if rows is None else rows
        self.qs = np.stack([O.normalize(O.synth_query(dim, seed=seed + 1 + i)) for i in range(n_queries)]) if queries is None else queries
        self.e = np.stack([O.scan(self.rows, q) for q in self.qs])
        self.row_bytes = dim * (2 if dtype == "f16" else 4)
        self.ix = rlr.GpuIndex(dim, dtype)
        self.ix.upload(self.rows)
        self.ix.set_grouped_sharing(2)

    def shared_forms(self, nq, m, n_allowed=None):
        """the forms of nq queries the device can decide: what the workspace rule and the split leave to the chunks"""
        w = W.chunk_width(self.n, self.row_bytes, self.n if n_allowed is None else n_allowed, m)
        shared, by_rule = W.forms_by_rule(nq, w)
        return [shared, 0, 0, by_rule]

    def check(self, sel, k, m, docs, forms, ctx, allowed=None, filter=None, mode=2):
        """the batch == the single entry per query == the model; the forms counter == `forms` (None: not held)"""
        ix = self.ix
        sel = list(sel)
        ix.set_grouped_sharing(mode)
        ix.grouped_batch_forms(reset=True)
        got = ix.search_topk_grouped_batch(self.qs[sel], k, m, filter=filter)
        counted = ix.grouped_batch_forms()
        ix.set_grouped_sharing(2)
        assert len(got) == len(sel)
        col = np.full(self.n, G.DOC_NONE, np.uint32) if docs is None else np.asarray(docs, np.uint32)
        for i, q in enumerate(sel):
            r, c, d = got[i]
            one_r, one_c, one_d = ix.search_topk_grouped(self.qs[q], k, m, filter=filter)[0]
            assert np.array_equal(r, one_r) and same_scores(c, one_c) and np.array_equal(d, one_d), (ctx, i, "single", r[:8], one_r[:8])
            want = G.expect(self.e[q], col, k, m, allowed)
            assert np.array_equal(r, want), (ctx, i, k, m, r[:8], want[:8])
            assert same_scores(c, self.e[q][want.astype(np.int64)]), (ctx, i, k, m)
            assert np.array_equal(d, col[want.astype(np.int64)]), (ctx, i, k, m)
        if forms is not None:
            assert counted == list(forms), (ctx, counted, forms)
        assert sum(counted) == len(sel), (ctx, counted)
        return got

    def close(self):
        self.ix.close()


@pytest.fixture(scope="module")
def corpus_of(rlr, oracle):
    made = {}

    def get(dim, dtype, n, n_queries=17):
        key = (dim, dtype, n)
        if key not in made:
            made[key] = Corpus(rlr, oracle, dim, dtype, n, n_queries, seed=0x7B00 + n + dim)
        assert made[key].qs.shape[0] >= n_queries
        return made[key]

    yield get
    for c in made.values():
        c.close()


def id_patterns(n):
    rng = np.random.default_rng(n)
    r = np.arange(n)
    crossing = (r + 100).astype(np.uint32)
    crossing[60:71] = 7                                      # one document across the first wave boundary
    scattered = rng.integers(0, max(2, n // 10), n).astype(np.uint32)
    mixed = scattered.copy()
    mixed[rng.random(n) < 0.3] = G.DOC_NONE
    return [("runs_of_16", (r // 16 + 3).astype(np.uint32)), ("scattered", scattered), ("rows_60_to_70", crossing),
            ("one_document", np.full(n, 9, np.uint32)), ("tagged_and_untagged", mixed)]


# ---- equals the definition ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,n", [(256, 65), (256, 4097), (768, 65), (768, 4097)])
def test_every_batch_equals_the_single_entry_and_the_model(corpus_of, dim, n):
    cp = corpus_of(dim, "f32", n)
    k_big = 600 if n > 1000 else 60                          # more than the groups of most patterns: a short answer
    combos = [(1, 1), (10, 3), (k_big, 8), (10, 1), (k_big, 1), (1, 3), (10, 8), (k_big, 3)]
    step = 0
    for name, ids in id_patterns(n):
        cp.ix.set_documents(ids)
        for nq in (2, 3, 8, 9, 17):
            for _ in range(2):                               # (two of the eight (k, per_doc) pairs per batch size, all over a pattern)
                k, m = combos[step % len(combos)]
                step += 1
                forms = cp.shared_forms(nq, m)
                if (dim, n) == (768, 4097):
                    assert forms == [nq, 0, 0, 0]            # eight queries a chunk for every per_doc; 9 = 5 + 4, 17 = 6 + 6 + 5
                got = cp.check(range(nq), k, m, ids, forms, (dim, n, name, nq, k, m))
                if name == "one_document":
                    assert all(g[0].size == min(k, m, n) for g in got)
    # every (k, per_doc) pair at the widest and at a split batch, on the pattern with tagged and untagged rows
    for k, m in combos:
        for nq in (8, 9):
            cp.check(range(nq), k, m, ids, cp.shared_forms(nq, m), (dim, n, "all pairs", nq, k, m))


@pytest.mark.parametrize("dim,n", [(256, 65), (768, 4097)])
def test_an_index_without_a_column(rlr, oracle, dim, n):
    cp = Corpus(rlr, oracle, dim, "f32", n, 9, seed=0x7C00 + n)
    try:
        plain_r, plain_c = cp.ix.search_topk(cp.qs[:9], 10)
        for nq, k, m in ((2, 1, 1), (8, 10, 3), (9, 10, 8), (3, 60, 1)):
            got = cp.check(range(nq), k, m, None, cp.shared_forms(nq, m), (dim, n, "no column", nq, k, m))
            assert all((g[2] == G.DOC_NONE).all() for g in got)
            if k == 10:
                assert all(np.array_equal(got[i][0], plain_r[i]) and same_scores(got[i][1], plain_c[i]) for i in range(nq))
    finally:
        cp.close()


def test_nine_queries_are_five_and_four_and_the_lone_remainder_goes_by_rule(corpus_of):
    cp = corpus_of(768, "f32", 4097)
    ids = id_patterns(4097)[1][1]
    cp.ix.set_documents(ids)
    cp.check(range(9), 10, 1, ids, [9, 0, 0, 0], "5 + 4")
    cp.check(range(17), 10, 3, ids, [17, 0, 0, 0], "6 + 6 + 5")
    small = corpus_of(256, "f32", 65)
    ids = id_patterns(65)[0][1]
    small.ix.set_documents(ids)
    assert W.chunk_width(65, 1024, 65, 3) == 2 and W.split(3, 2) == [2, 1]
    small.check(range(3), 5, 3, ids, [2, 0, 0, 1], "2 + a lone remainder")
    assert W.chunk_width(65, 1024, 65, 8) == 0
    small.check(range(8), 5, 8, ids, [0, 0, 0, 8], "no width fits the workspace rule")


# ---- the queries of a chunk do not leak into each other ------------------------------------------------------------------
def leak_corpus(O, dim=256, n=4097):
    """Query i is the stored row 100 * (i + 1), the only row of document i.  Query 0's nearest rows are a 300-row document
    (500); query i > 0 has 3 * i near copies in documents of their own -- with k = 10 the k-th head, and with it U, is a
    near copy (about 0.99) for the queries with ten or more and a random row (about 0.2) for the others."""
    rng = np.random.default_rng(0x1EA)
    rows = O.synth_rows(n, dim, seed=0x7D00)
    ids = (np.arange(n) + 1000).astype(np.uint32)
    qrows = [100 * (i + 1) for i in range(8)]
    for i, r in enumerate(qrows):
        ids[r] = i
    free = iter(range(1000, n))

    def near(v):
        return O.normalize((v + rng.standard_normal(dim).astype(np.float32) * F32(0.005)).astype(np.float32))

    for _ in range(300):
        r = next(free)
        rows[r], ids[r] = near(rows[qrows[0]]), 500
    for i in range(1, 8):
        for _ in range(3 * i):
            rows[next(free)] = near(rows[qrows[i]])
    return rows, ids, rows[qrows].copy(), qrows


def test_the_queries_of_a_chunk_do_not_leak_into_each_other(rlr, oracle):
    rows, ids, queries, qrows = leak_corpus(oracle)
    cp = Corpus(rlr, oracle, 256, "f32", rows.shape[0], 0, seed=0, rows=rows, queries=queries)
    try:
        cp.ix.set_documents(ids)
        for k, m in ((10, 1), (10, 3), (1, 1)):
            got = cp.check(range(8), k, m, ids, [8, 0, 0, 0], ("leak", k, m))
            for i in range(8):
                assert got[i][0][0] == qrows[i] and got[i][2][0] == i          # every query's best document is its own
            if k == 10:
                assert (got[0][2] == 500).sum() == m                          # the long document gives per_doc rows, no more
                tenth = [float(g[1][9]) for g in got]
                assert min(tenth) < 0.5 and max(tenth) > 0.9                  # widely different thresholds in one chunk
    finally:
        cp.close()


# ---- a narrowed chunk -------------------------------------------------------------------------------------------------------
def test_eight_per_document_at_256_elements_narrow_the_chunk(corpus_of):
    cp = corpus_of(256, "f32", 4097)
    assert W.chunk_width(4097, 1024, 4097, 8) == 3 and W.split(8, 3) == [3, 3, 2]
    for name, ids in id_patterns(4097)[:2]:
        cp.ix.set_documents(ids)
        cp.check(range(8), 10, 8, ids, [8, 0, 0, 0], ("narrowed", name))


# ---- filters -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,n", [(256, 4097), (768, 4097)])
def test_inside_a_filter_on_both_paths(corpus_of, dim, n):
    cp = corpus_of(dim, "f32", n)
    ix = cp.ix
    ids = id_patterns(n)[1][1]
    ix.set_documents(ids)
    members = np.unique(ids)[::3]
    allowed = np.flatnonzero(np.isin(ids, members))
    with ix.filter_documents(members) as f:
        f.set_path("scan")
        for nq, k, m in ((3, 10, 1), (8, 10, 3), (8, 600, 1)):
            cp.check(range(nq), k, m, ids, cp.shared_forms(nq, m, allowed.size), (dim, "document filter", nq, k, m), allowed=allowed, filter=f)
        f.set_path("list")
        for nq in (3, 8):
            cp.check(range(nq), 10, 2, ids, [0, 0, 0, nq], (dim, "list path", nq), allowed=allowed, filter=f)
    allowed = np.arange(1000, 3500)
    with ix.filter_rows(allowed) as f:
        f.set_path("scan")
        for nq, k, m in ((3, 10, 3), (8, 1, 1), (8, 10, 1)):
            cp.check(range(nq), k, m, ids, cp.shared_forms(nq, m, allowed.size), (dim, "row range", nq, k, m), allowed=allowed, filter=f)
    with ix.filter_rows([]) as f:                            # an empty filter: RLR_OK, no result, no query counted
        ix.grouped_batch_forms(reset=True)
        got = ix.search_topk_grouped_batch(cp.qs[:3], 5, 1, filter=f)
        assert all(g[0].size == 0 for g in got) and sum(ix.grouped_batch_forms()) == 0


# ---- one query of a chunk is handed back; its neighbours stay ----------------------------------------------------------------
def overflow_corpus(O, dim=256, n=4097):
    """3000 identical untagged rows that are query 3's vector: they tie for its top place; the other queries are stored
    rows of the rest, each with twelve near copies, so the identical rows lie far below their tenth result"""
    rng = np.random.default_rng(0x0F10)
    rows = O.synth_rows(n, dim, seed=0x7E00)
    ids = (np.arange(n) // 4).astype(np.uint32)
    v = O.normalize(O.synth_query(dim, seed=0x7E01))
    rows[500:3500] = v
    ids[500:3500] = G.DOC_NONE
    queries = []
    free = iter(range(3600, n))
    for i in range(8):
        if i == 3:
            queries.append(v)
            continue
        base = rows[10 + 20 * i].copy()
        queries.append(base)
        for _ in range(12):
            r = next(free)
            rows[r] = O.normalize((base + rng.standard_normal(dim).astype(np.float32) * F32(0.005)).astype(np.float32))
            ids[r] = G.DOC_NONE
    return rows, ids, np.stack(queries)


def test_one_query_of_eight_overflows_and_the_other_seven_stay(rlr, oracle):
    rows, ids, queries = overflow_corpus(oracle)
    cp = Corpus(rlr, oracle, 256, "f32", rows.shape[0], 0, seed=0, rows=rows, queries=queries)
    try:
        cp.ix.set_documents(ids)
        for i in range(8):                                   # the design holds: only query 3 sees the tie in its band
            tenth = np.sort(cp.e[i])[::-1][9]
            assert (cp.e[i][500:3500] == cp.e[i][500]).all() and ((cp.e[i][500] < tenth - 0.3) != (i == 3))
        cp.ix.grouped_forms(reset=True)
        got = cp.check(range(8), 10, 1, ids, [7, 1, 0, 0], "3000 ties")
        assert got[3][0].tolist() == list(range(500, 510))
    finally:
        cp.close()


def test_infinity_nan_and_zeros_in_one_batch(rlr, oracle):
    rows = oracle.synth_rows(300, 256, seed=31)
    q0 = np.zeros(256, np.float32)
    q0[0] = 1.0
    rows[:, 0] = -np.abs(rows[:, 0]) - F32(0.001)            # every other score against q0 is negative ...
    rows[[5, 6, 150], 0] = 0.0                               # ... these score +0
    rows[7] = 0.0
    rows[8, 0] = -0.0                                        # (a -0 product: the sum is +0 all the same)
    q1 = oracle.normalize(np.abs(oracle.synth_query(256, seed=42)) + F32(0.01))  # all positive: the Inf row scores +Inf
    rows[123, 2] = np.inf
    queries = np.stack([q0, q1, oracle.normalize(oracle.synth_query(256, seed=43)), q1])
    ids = (np.arange(300) // 3).astype(np.uint32)            # rows 5 | 6, 7, 8 | 150 in three documents
    cp = Corpus(rlr, oracle, 256, "f32", 300, 0, seed=0, rows=rows.copy(), queries=queries)
    try:
        cp.ix.set_documents(ids)
        assert cp.e[1][123] == np.inf and np.isnan(cp.e[0][123]) and (cp.e[0][[5, 6, 7, 8, 150]] == 0.0).all()
        assert np.isnan(cp.e).sum(axis=1).tolist() == [1, 0, 0, 0]
        # k = 10 leaves the NaN row out of every answer: nobody is short, everybody is decided on the device
        got = cp.check(range(4), 10, 1, ids, [4, 0, 0, 0], "inf and zeros")
        assert got[0][0][:3].tolist() == [5, 6, 150] and got[1][0][0] == 123 and got[1][1][0] == np.inf
        got = cp.check(range(4), 10, 3, ids, [4, 0, 0, 0], "inf and zeros, three per document")
        assert got[0][0][:5].tolist() == [5, 6, 7, 8, 150]   # the zeros tie: rows ascending, three of the document 6..8
        # k = every row: query 0 -- the only one with a NaN nomination -- is short and is handed back, alone
        got = cp.check(range(4), 300, 8, ids, [3, 0, 1, 0], "the NaN row is wanted")
        assert got[0][0][-1] == 123 and np.isnan(got[0][1][-1]) and got[0][0].size == 300
    finally:
        cp.close()


# ---- by rule ---------------------------------------------------------------------------------------------------------------------
def test_by_rule_every_query_goes_to_the_single_path(rlr, oracle, corpus_of):
    cp = corpus_of(768, "f32", 4097)
    ids = id_patterns(4097)[0][1]
    cp.ix.set_documents(ids)
    cp.check(range(1), 10, 1, ids, [0, 0, 0, 1], "one query")
    cp.check(range(3), 1025, 8, ids, [0, 0, 0, 3], "k beyond the finish")
    for dim, dtype, why in ((256, "f16", "binary16 rows"), (384, "f32", "a width no shared scan serves")):
        other = Corpus(rlr, oracle, dim, dtype, 4100, 4, seed=0x7F00 + dim)
        try:
            col = (np.arange(4100) // 7).astype(np.uint32)
            other.ix.set_documents(col)
            other.check(range(4), 10, 2, col, [0, 0, 0, 4], why)
        finally:
            other.close()


def test_argument_rules(rlr, oracle, corpus_of):
    cp = corpus_of(256, "f32", 65)
    other = corpus_of(768, "f32", 65)
    for bad in (0, 9):
        with pytest.raises(rlr.RlrError) as ei:
            cp.ix.search_topk_grouped_batch(cp.qs[:3], 5, bad)
        assert ei.value.status == -1
    with pytest.raises(rlr.RlrError) as ei:
        cp.ix.search_topk_grouped_batch(cp.qs[:3], 0, 1)
    assert ei.value.status == -1
    with other.ix.filter_rows([1, 2, 3]) as f, pytest.raises(rlr.RlrError) as ei:
        cp.ix.search_topk_grouped_batch(cp.qs[:3], 5, 1, filter=f)          # another index's filter
    assert ei.value.status == -1
    ix = rlr.GpuIndex(256)
    try:
        ix.upload(cp.rows)
        ix.set_grouped_sharing(2)
        with ix.filter_rows([1, 2, 3]) as f:
            assert all(g[0].size == 3 for g in ix.search_topk_grouped_batch(cp.qs[:3], 5, 1, filter=f))
            ix.append(cp.rows[:2])
            with pytest.raises(rlr.RlrError) as ei:
                ix.search_topk_grouped_batch(cp.qs[:3], 5, 1, filter=f)     # stale
            assert ei.value.status == -1
        for mode in (-1, 3):
            with pytest.raises(rlr.RlrError) as ei:
                ix.set_grouped_sharing(mode)
            assert ei.value.status == -1
    finally:
        ix.close()


# ---- state ---------------------------------------------------------------------------------------------------------------------
def test_plain_and_grouped_searches_after_a_batched_call_on_the_same_context(rlr, oracle):
    n = 6000
    cp = Corpus(rlr, oracle, 256, "f32", n, 8, seed=0x7C03)
    fresh = Corpus(rlr, oracle, 256, "f32", n, 8, seed=0x7C03)
    try:
        ids = (np.arange(n) // 9).astype(np.uint32)
        for c in (cp, fresh):
            c.ix.set_documents(ids)
        want_one = fresh.ix.search_topk(fresh.qs[0], 100)
        want_many = fresh.ix.search_topk(fresh.qs, 100)
        want_grouped = fresh.ix.search_topk_grouped(fresh.qs[:3], 50, 2)
        for nq, k, m in ((8, 10, 1), (3, 100, 8), (5, 1, 3)):
            cp.ix.grouped_batch_forms(reset=True)
            cp.ix.search_topk_grouped_batch(cp.qs[:nq], k, m)
            assert cp.ix.grouped_batch_forms() == [nq, 0, 0, 0]
            r, c = cp.ix.search_topk(cp.qs[0], 100)
            assert np.array_equal(r, want_one[0]) and same_scores(c, want_one[1])
            r, c = cp.ix.search_topk(cp.qs, 100)
            assert np.array_equal(r, want_many[0]) and same_scores(c, want_many[1])
            for g, w in zip(cp.ix.search_topk_grouped(cp.qs[:3], 50, 2), want_grouped):
                assert np.array_equal(g[0], w[0]) and same_scores(g[1], w[1]) and np.array_equal(g[2], w[2])
    finally:
        cp.close()
        fresh.close()


def test_four_threads_return_what_the_serial_calls_return(corpus_of):
    cp = corpus_of(768, "f32", 4097)
    ids = id_patterns(4097)[4][1]
    cp.ix.set_documents(ids)
    sels = [list(range(i * 4, i * 4 + 5)) for i in range(4)]
    serial = [cp.ix.search_topk_grouped_batch(cp.qs[s], 50, 2) for s in sels]
    errors = []

    def work(i):
        try:
            for _ in range(10):
                got = cp.ix.search_topk_grouped_batch(cp.qs[sels[i]], 50, 2)
                for g, w in zip(got, serial[i]):
                    if not (np.array_equal(g[0], w[0]) and same_scores(g[1], w[1]) and np.array_equal(g[2], w[2])):
                        errors.append(i)
        except Exception as e:                               # noqa: BLE001 (reported below)
            errors.append(e)

    cp.ix.grouped_batch_forms(reset=True)
    threads = [threading.Thread(target=work, args=(i,)) for i in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    assert cp.ix.grouped_batch_forms() == [200, 0, 0, 0]
    for s, got in zip(sels, serial):
        for i, q in enumerate(s):
            assert np.array_equal(got[i][0], G.expect(cp.e[q], ids, 50, 2))


def test_modes_one_and_zero_return_the_bits_of_mode_two(corpus_of):
    cp = corpus_of(768, "f32", 4097)
    ids = id_patterns(4097)[1][1]
    cp.ix.set_documents(ids)
    for nq, k, m in ((3, 10, 1), (9, 10, 3)):
        cp.check(range(nq), k, m, ids, [nq, 0, 0, 0], ("mode 2", nq))
        cp.check(range(nq), k, m, ids, [0, 0, 0, nq], ("mode 1", nq), mode=1)
        cp.ix.grouped_batch_forms(reset=True)
        got = cp.check(range(nq), k, m, ids, None, ("mode 0", nq), mode=0)      # (whatever the gate decides: the same bits)
        assert len(got) == nq


# ---- the engine ----------------------------------------------------------------------------------------------------------------
def test_engine_batches_equal_the_per_query_methods(rlr, oracle):
    dim = 256
    rng = np.random.default_rng(61)
    eng = rlr.RagEngine(dim)
    try:
        for name, n in {"a.pdf": 300, "b.pdf": 200, "c.pdf": 1, "d.pdf": 40}.items():
            eng.add_document(name, [f"{name} {i}" for i in range(n)], rng.standard_normal((n, dim)).astype(np.float32))
        eng.index.set_grouped_sharing(2)
        raw = (3.0 * rng.standard_normal((5, dim))).astype(np.float32)          # not unit norm: the engine normalises
        for names in (None, ["a.pdf", "c.pdf"], ["nothing.pdf"]):
            for k, m in ((3, 1), (10, 2), (10, 8)):
                eng.index.grouped_batch_forms(reset=True)
                got = eng.search_per_document_batch(raw, k, m, documents=names)
                assert sum(eng.index.grouped_batch_forms()) == (0 if names == ["nothing.pdf"] else 5)
                for q in range(5):
                    one = eng.search_per_document(raw[q], k, m, documents=names)
                    assert [g.to_json() for g in got[q]] == [w.to_json() for w in one] and [g.row for g in got[q]] == [w.row for w in one]
                    assert all(bits(F32(g.score)) == bits(F32(w.score)) for g, w in zip(got[q], one))
            ranked = eng.rank_documents_batch(raw, 4, documents=names)
            for q in range(5):
                one = eng.rank_documents(raw[q], 4, documents=names)
                assert [(n_, r.row, r.score) for n_, r in ranked[q]] == [(n_, r.row, r.score) for n_, r in one]
        eng.index.grouped_batch_forms(reset=True)
        assert len(eng.rank_documents_batch(raw, 10)) == 5 and all(len(r) == 4 for r in eng.rank_documents_batch(raw, 10))
        assert eng.index.grouped_batch_forms()[0] == 10                         # shared chunks have run
        assert eng.search_per_document_batch(raw[:0], 3) == [] and eng.search_per_document_batch(raw, 0) == [[]] * 5
    finally:
        eng.close()
