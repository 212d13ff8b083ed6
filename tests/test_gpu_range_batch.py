"""rlr_search_range_batch on the device: every query of a batch held to the definition of tests/range_vectors.py
(`expect` over oracle.scan) AND to rlr_search_range on the same index -- rows equal, scores bit-equal, n_total equal --
and the batch forms counter says WHICH path answered: [0] behind a shared scan, [1] behind the GEMM, [2] handed back on a
device capacity, [3] by rule.  With sharing forced (mode 2) every parity case is decided on the device: n <= 8192 rows
cannot overflow a candidate list of 8192, the thresholds sit on real scores at ranks of at most 2048, and every query of
a batch has its own threshold.

Shapes, the smallest at which each path can still go wrong:
  GEMM          128-d f32 at 4097 rows (a partial 256-row tile) and 4353 (one row past a tile), 256-d binary16 at 4100,
                128-d f32 over the nomination image; 9, 16, 17, 255, 256, 257 queries (a ragged last query block, a second
                block); cap 0, 1, 64, 2048
  shared scan   256-d and 768-d f32 at 65 and 4097 rows; 2, 3, 8 queries"""
import ctypes as C
import threading

import numpy as np
import pytest

import band_vectors as B
import range_vectors as R
from conftest import bits

pytestmark = pytest.mark.gpu

F32 = np.float32
RANKS = (0, 1, 2, 7, 64, 65, 100, 333, 1024, 1025, 2047, 2048)   # hits asked of the queries of a batch, in turn
# Over the nomination image, batches of more than 128 queries take the kernel whose workgroup keeps the candidates of one
# unit (256 rows x 256 queries) in a list of 1024 before it flushes them; a unit with more marks its queries (bit 31) and
# they are handed back.  These ranks keep a unit at 256 queries x 9 hits on average x 256 / 4097 rows = about 150.
SPARSE = (0, 1, 2, 7, 16, 31, 5, 12)


def same_scores(got, want):
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    return got.shape == want.shape and bool(np.all(bits(got) == bits(want)))


class Corpus:
    """an index, its rows on the host, a pool of queries and their reference-order scores, made once"""

    def __init__(self, rlr, O, dim, dtype, n, n_queries, seed, rows=None, queries=None, image=False):
        self.O, self.dim, self.n = O, dim, n
        self.rows = O.synth_rows(n, dim, seed=seed, f16=dtype == "f16") if rows is None else rows
        self.qs = np.stack([O.normalize(O.synth_query(dim, seed=seed + 1 + i)) for i in range(n_queries)]) if queries is None else queries
        self.e = np.stack([O.scan(self.rows, q) for q in self.qs])
        self.ix = rlr.GpuIndex(dim, dtype)
        self.ix.upload(self.rows)
        if image:
            self.ix.enable_batch_image(True)
        self.ix.set_range_sharing(2)

    def taus(self, sel, allowed=None, first=0, ranks=RANKS):
        """one threshold per query, on real scores: query i of the batch gets exactly RANKS[(first + i) % len] hits (the
        rank-t score; one ulp above the best score for t = 0), fewer where the (allowed) rows run out"""
        out = []
        for i, q in enumerate(sel):
            e = self.e[q] if allowed is None else self.e[q][allowed]
            s = np.sort(e[~np.isnan(e)])[::-1]
            t = min(ranks[(first + i) % len(ranks)], s.size)
            out.append(np.nextafter(s[0], F32(np.inf)) if t == 0 else s[t - 1])
        return np.asarray(out, np.float32)

    def check(self, sel, taus, cap, forms, ctx, allowed=None, filter=None, mode=2):
        """the batch == the definition == rlr_search_range, query by query; the forms counter == `forms`; count-only too"""
        ix = self.ix
        sel = list(sel)
        ix.set_range_sharing(mode)
        ix.range_batch_forms(reset=True)
        got = ix.search_range_batch(self.qs[sel], taus, cap, filter=filter)
        counted = ix.range_batch_forms()
        ix.set_range_sharing(2)
        single = ix.search_range(self.qs[sel], taus, cap, filter=filter)
        assert len(got) == len(sel)
        for i, q in enumerate(sel):
            want_rows, want_total = R.expect(self.e[q], taus[i], cap, allowed)
            r, c, total = got[i]
            assert total == want_total, (ctx, i, taus[i], cap, total, want_total)
            assert np.array_equal(r, want_rows), (ctx, i, taus[i], cap, r[:8], want_rows[:8])
            assert same_scores(c, self.e[q][want_rows.astype(np.int64)]), (ctx, i, taus[i], cap)
            assert np.array_equal(r, single[i][0]) and same_scores(c, single[i][1]) and total == single[i][2], (ctx, i, "single")
        if forms is not None:
            assert counted == list(forms), (ctx, counted, forms)
        return got

    def close(self):
        self.ix.close()


@pytest.fixture(scope="module")
def corpus_of(rlr, oracle):
    made = {}

    def get(dim, dtype, n, n_queries=8, image=False):
        key = (dim, dtype, n, image)
        if key not in made:
            made[key] = Corpus(rlr, oracle, dim, dtype, n, n_queries, seed=0x5B00 + n + dim, image=image)
        assert made[key].qs.shape[0] >= n_queries
        return made[key]

    yield get
    for c in made.values():
        c.close()


# ---- the GEMM path ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,dtype,n,image", [(128, "f32", 4097, False), (128, "f32", 4353, False), (256, "f16", 4100, False),
                                               (128, "f32", 4097, True)])
def test_gemm_path_equals_the_definition(corpus_of, dim, dtype, n, image):
    cp = corpus_of(dim, dtype, n, 257, image)
    for nq in (9, 16, 17, 255, 256, 257):
        sel = range(nq)
        ranks = SPARSE if image and nq > 128 else RANKS
        cp.check(sel, cp.taus(sel, first=nq, ranks=ranks), 2048, [0, nq, 0, 0], (dim, dtype, n, nq))
    if image:
        # dense thresholds overflow that kernel's unit list: the marked queries are handed back, and still answered right
        cp.check(range(255), cp.taus(range(255), first=3), 2048, None, (dim, dtype, n, "dense over the image"))
        cp.ix.range_batch_forms(reset=True)
        cp.ix.search_range_batch(cp.qs[:255], cp.taus(range(255), first=3), 2048)
        forms = cp.ix.range_batch_forms()
        assert forms[2] > 0 and forms[1] + forms[2] == 255 and forms[0] == forms[3] == 0, forms
    sel = range(16)
    for cap in (0, 1, 64):
        cp.check(sel, cp.taus(sel), cap, [0, 16, 0, 0], (dim, dtype, n, "cap", cap))
    assert cp.ix.count_range_batch(cp.qs[:16], cp.taus(sel)) == [R.expect(cp.e[q], t, 0)[1] for q, t in zip(sel, cp.taus(sel))]
    # the second query block's thresholds must not reach the first: the last 200 queries take every row they may, the rest none
    taus = np.r_[[np.nextafter(cp.e[q].max(), F32(np.inf)) for q in range(57)],
                 cp.taus(range(57, 257), first=11, ranks=SPARSE if image else RANKS)].astype(np.float32)
    got = cp.check(range(257), taus, 2048, [0, 257, 0, 0], (dim, dtype, n, "two blocks"))
    assert all(g[2] == 0 for g in got[:57]) and sum(g[2] > 0 for g in got[57:]) >= 150


def test_gemm_path_serves_two_to_eight_queries_where_no_scan_is_shared(corpus_of):
    cp = corpus_of(128, "f32", 4097, 257)                                       # 128-d: no shared scan for this shape
    for nq in (2, 8):
        cp.check(range(nq), cp.taus(range(nq), first=3), 100, [0, nq, 0, 0], ("gemm small", nq))


# ---- the shared scan ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,n", [(256, 65), (256, 4097), (768, 65), (768, 4097)])
def test_shared_scan_equals_the_definition(corpus_of, dim, n):
    cp = corpus_of(dim, "f32", n, 8)
    for nq in (2, 3, 8):
        sel = range(nq)
        for cap in (0, 1, 64, 2048):
            cp.check(sel, cp.taus(sel, first=nq + cap), cap, [nq, 0, 0, 0], (dim, n, nq, cap))
    assert cp.ix.count_range_batch(cp.qs[:3], [0.0, -1.0, 0.1]) == [R.expect(cp.e[q], t, 0)[1] for q, t in zip(range(3), (0.0, -1.0, 0.1))]


# ---- filters ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,n,nq,form", [(256, 4097, 3, 0), (768, 4097, 8, 0), (128, 4097, 16, 1)])
def test_mask_filters_on_both_shared_paths(corpus_of, dim, n, nq, form):
    cp = corpus_of(dim, "f32", n, 257 if dim == 128 else 8)
    sel = range(nq)
    served = [0, 0, 0, 0]
    served[form] = nq
    best = int(np.argmax(cp.e[0]))
    allowed = np.setdiff1d(np.arange(0, n, 3), [best])                         # query 0's best hit lies just outside the mask
    with cp.ix.filter_rows(allowed) as f:
        f.set_path("scan")
        got = cp.check(sel, cp.taus(sel, allowed, first=1), 2048, served, (dim, "third"), allowed=allowed, filter=f)
        assert best not in got[0][0]
        cp.check(sel, cp.taus(sel, allowed, first=2), 0, served, (dim, "third, count"), allowed=allowed, filter=f)
        f.set_path("list")                                                      # by rule: the single path, with right answers
        cp.check(sel, cp.taus(sel, allowed, first=1), 2048, [0, 0, 0, nq], (dim, "list path"), allowed=allowed, filter=f)
    with cp.ix.filter_rows([n - 2]) as f:                                       # exactly one row
        f.set_path("scan")
        taus = np.where(np.arange(nq) % 2 == 0, cp.e[:nq, n - 2], np.nextafter(cp.e[:nq, n - 2], F32(np.inf))).astype(np.float32)
        got = cp.check(sel, taus, 5, served, (dim, "one row"), allowed=np.array([n - 2]), filter=f)
        assert [g[2] for g in got] == [1 - i % 2 for i in range(nq)]
    with cp.ix.filter_rows([]) as f:                                            # no row: RLR_OK, zero counts, nothing counted
        cp.ix.range_batch_forms(reset=True)
        got = cp.ix.search_range_batch(cp.qs[:nq], cp.taus(sel), 5, filter=f)
        assert all(g[0].size == 0 and g[2] == 0 for g in got) and sum(cp.ix.range_batch_forms()) == 0


# ---- membership inside the band, on both paths -------------------------------------------------------------------------
@pytest.mark.parametrize("f16", [False, True])
def test_membership_inside_the_band(rlr, oracle, f16):
    """band_vectors' absorption and operand_rounding rows in ONE corpus (X of the first at its row, X of the second 4096
    rows on), their two queries in one batch among fillers: tau = e(X) (X is a hit, no decoy is) and one ulp above (X is
    none either) -- the decision lies inside the band of either nomination"""
    ra, qa, fa = B.absorption(oracle, 1, f16=f16)
    rb, qb, fb = B.operand_rounding(oracle, 1, f16=f16)
    rows = np.concatenate([ra, rb])
    fill = [oracle.normalize(oracle.synth_query(768, seed=60 + i)) for i in range(7)]
    queries = np.stack([qa[0], fill[0], qb[0]] + fill[1:] + [qb[0], qa[0]])     # 11 queries; a and b at slots 0, 2, 9, 10
    cp = Corpus(rlr, oracle, 768, "f16" if f16 else "f32", rows.shape[0], 0, seed=0, rows=rows, queries=queries)
    try:
        xa, xb = fa["x"], 4096 + fb["x"]
        da, db = fa["decoys"], 4096 + fb["decoys"]
        assert (cp.e[0][da] < cp.e[0][xa]).all() and (cp.e[2][db] < cp.e[2][xb]).all()
        up = lambda v: np.nextafter(v, F32(np.inf))                            # noqa: E731
        for sel, form in (((0, 1, 2), 1 if f16 else 0), (range(11), 1)):       # 3 queries: the shared scan (f32 rows); 11: the GEMM
            sel = list(sel)
            served = [0, 0, 0, 0]
            served[form] = len(sel)
            taus = cp.taus(sel, first=4)
            taus[0], taus[2] = cp.e[0][xa], up(cp.e[2][xb])
            if len(sel) == 11:
                taus[9], taus[10] = cp.e[2][xb], up(cp.e[0][xa])
            got = cp.check(sel, taus, 2048, served, ("band", f16, len(sel)))
            assert xa in got[0][0] and not np.isin(da, got[0][0]).any()
            assert xb not in got[2][0] and not np.isin(db, got[2][0]).any()
            if len(sel) == 11:
                assert xb in got[9][0] and not np.isin(db, got[9][0]).any()
                assert xa not in got[10][0] and not np.isin(da, got[10][0]).any()
            cp.check(sel, taus, 0, served, ("band, count-only", f16, len(sel)))
    finally:
        cp.close()


# ---- capacities: form [2] for exactly the affected queries ---------------------------------------------------------------
def test_candidate_overflow_hands_back_one_query_of_sixteen(rlr, oracle):
    cp = Corpus(rlr, oracle, 128, "f32", 8449, 16, seed=0x5C01)
    try:
        taus = cp.taus(range(16), first=1)
        taus[5] = -np.inf                                                       # 8449 candidates: beyond the list of 8192
        got = cp.check(range(16), taus, 100, [0, 15, 1, 0], "overflow")
        assert got[5][2] == 8449
        got = cp.check(range(16), taus, 0, [0, 15, 1, 0], "overflow, count-only")
        assert got[5][2] == 8449
    finally:
        cp.close()


@pytest.mark.parametrize("dim,nq,form", [(128, 9, 1), (256, 3, 0)])
def test_five_thousand_identical_rows(rlr, oracle, dim, nq, form):
    rows = np.tile(oracle.synth_rows(1, dim, seed=9), (5000, 1))
    queries = np.stack([oracle.normalize(oracle.synth_query(dim, seed=70 + i)) for i in range(nq)])
    queries[1] = rows[0]
    cp = Corpus(rlr, oracle, dim, "f32", 5000, 0, seed=0, rows=rows, queries=queries)
    try:
        taus = np.full(nq, 2.0, np.float32) + np.arange(nq, dtype=np.float32)  # nobody else hits anything
        taus[1] = cp.e[1][0]
        served = [0, 0, 1, 0]
        served[form] = nq - 1
        got = cp.check(range(nq), taus, 5000, served, "identical")              # more than 2048 hits: handed back
        assert got[1][2] == 5000 and got[1][0].tolist() == list(range(5000))
        served = [0, 0, 0, 0]
        served[form] = nq
        got = cp.check(range(nq), taus, 0, served, "identical, count-only")     # stays on the device
        assert got[1][2] == 5000
    finally:
        cp.close()


# ---- numeric edges -----------------------------------------------------------------------------------------------------
def test_infinity_nan_and_zeros_in_one_batch(rlr, oracle):
    rows = oracle.synth_rows(300, 256, seed=31)
    q0 = np.zeros(256, np.float32)
    q0[0] = 1.0
    rows[[5, 6, 150], 0] = 0.0                                                  # score +0 against q0
    rows[7] = 0.0
    rows[8, 0] = -0.0
    q1 = oracle.normalize(np.abs(oracle.synth_query(256, seed=42)) + F32(0.01))  # all positive: the Inf row scores +Inf
    rows[123, 2] = np.inf
    queries = np.stack([q0, q1, q0, oracle.normalize(oracle.synth_query(256, seed=43))])
    taus = np.array([0.0, np.inf, -0.0, -np.inf], np.float32)
    cp = Corpus(rlr, oracle, 256, "f32", 300, 0, seed=0, rows=rows.copy(), queries=queries)
    try:
        assert cp.e[1][123] == np.inf and (cp.e[0][[5, 6, 7, 8, 150]] == 0.0).all()
        # (the Inf row scores NaN against q0 -- Inf x 0 -- so queries 0 and 2 see a NaN nomination and are handed back)
        got = cp.check(range(4), taus, 300, [2, 0, 2, 0], "inf and zeros")
        assert {5, 6, 7, 8, 150} <= set(got[0][0].tolist()) and {5, 6, 7, 8, 150} <= set(got[2][0].tolist())
        assert got[1][0].tolist() == [123]
        cp.check(range(4), taus, 0, None, "inf and zeros, count-only")
    finally:
        cp.close()
    rows[17, 3] = np.nan                                                        # a NaN among the allowed rows: every query goes back
    cp = Corpus(rlr, oracle, 256, "f32", 300, 0, seed=0, rows=rows, queries=queries)
    try:
        got = cp.check(range(4), taus, 300, [0, 0, 4, 0], "nan row")
        assert all(17 not in g[0] for g in got)
    finally:
        cp.close()


def test_an_operand_beyond_binary16_range_keeps_nine_queries_off_the_gemm(rlr, oracle):
    rows = oracle.synth_rows(4200, 128, seed=77)
    rows[4000, 5] = 1.0e5
    cp = Corpus(rlr, oracle, 128, "f32", 4200, 9, seed=0x5C02, rows=rows)
    try:
        got = cp.check(range(9), cp.taus(range(9), first=2), 100, [0, 0, 0, 9], "beyond binary16")
        assert any(4000 in g[0] for g in got)
    finally:
        cp.close()


# ---- state -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,nq", [(256, 3), (128, 16)])
def test_top_k_after_a_batched_range_call_on_the_same_context(rlr, oracle, dim, nq):
    cp = Corpus(rlr, oracle, dim, "f32", 6000, 16, seed=0x5C03 + dim)
    try:
        one_r, one_c = cp.ix.search_topk(cp.qs[0], 100)
        many_r, many_c = cp.ix.search_topk(cp.qs[:16], 100)
        assert np.array_equal(one_r[0], R.result_order(cp.e[0], np.arange(6000))[:100].astype(np.uint64))
        for taus, cap in ((cp.taus(range(nq)), 2048), (np.full(nq, -np.inf, np.float32), 0), (cp.taus(range(nq), first=5), 10)):
            cp.ix.search_range_batch(cp.qs[:nq], taus, cap)
            r, c = cp.ix.search_topk(cp.qs[0], 100)
            assert np.array_equal(r, one_r) and same_scores(c, one_c)
            r, c = cp.ix.search_topk(cp.qs[:16], 100)
            assert np.array_equal(r, many_r) and same_scores(c, many_c)
    finally:
        cp.close()


def test_four_threads_return_what_the_serial_calls_return(corpus_of):
    cp = corpus_of(128, "f32", 4097, 257)
    sels = [list(range(i * 20, i * 20 + 12)) for i in range(4)]
    taus = [cp.taus(s, first=i) for i, s in enumerate(sels)]
    serial = [cp.ix.search_range_batch(cp.qs[s], t, 2048) for s, t in zip(sels, taus)]
    errors = []

    def work(i):
        try:
            for _ in range(10):
                got = cp.ix.search_range_batch(cp.qs[sels[i]], taus[i], 2048)
                for g, w in zip(got, serial[i]):
                    if not (np.array_equal(g[0], w[0]) and same_scores(g[1], w[1]) and g[2] == w[2]):
                        errors.append(i)
        except Exception as e:                               # noqa: BLE001 (reported below)
            errors.append(e)

    threads = [threading.Thread(target=work, args=(i,)) for i in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for s, t, got in zip(sels, taus, serial):
        for i, q in enumerate(s):
            want_rows, want_total = R.expect(cp.e[q], t[i], 2048)
            assert np.array_equal(got[i][0], want_rows) and got[i][2] == want_total


@pytest.mark.parametrize("dim,nq", [(256, 3), (128, 16)])
def test_modes_one_and_zero_return_the_bits_of_mode_two(corpus_of, dim, nq):
    cp = corpus_of(dim, "f32", 4097, 257 if dim == 128 else 8)
    taus = cp.taus(range(nq), first=6)
    cp.check(range(nq), taus, 2048, [0, 0, 0, nq], ("mode 1", dim), mode=1)
    cp.ix.range_batch_forms(reset=True)
    cp.check(range(nq), taus, 2048, None, ("mode 0", dim), mode=0)
    cp.check(range(1), taus[:1], 2048, [0, 0, 0, 1], ("one query", dim))
    with pytest.raises(Exception):
        cp.ix.set_range_sharing(3)
    with pytest.raises(Exception):
        cp.ix.search_range_batch(cp.qs[:2], [0.5, np.nan], 5)


# ---- the engine ----------------------------------------------------------------------------------------------------------
DIM = 256


def _engine(rlr, rng, sizes):
    eng = rlr.RagEngine(DIM)
    for name, n in sizes.items():
        eng.add_document(name, [f"{name} {i}" for i in range(n)], rng.standard_normal((n, DIM)).astype(np.float32))
    eng.index.set_range_sharing(2)
    return eng


def test_engine_add_document_reports_planted_duplicates_over_shared_passes(rlr, oracle):
    rng = np.random.default_rng(53)
    eng = _engine(rlr, rng, {"a.pdf": 300, "b.pdf": 200})
    try:
        old = eng.index.fetch_rows([5, 450])
        emb = rng.standard_normal((4, DIM)).astype(np.float32)
        emb[1] = old[0] * np.float32(3.0)                                       # chunk 1 repeats row 5 of a.pdf (scaled: normalised away)
        emb[3] = old[1]                                                         # chunk 3 repeats row 450 of b.pdf
        before = len(eng)
        rows = eng.index.fetch_rows(np.arange(before))
        one_by_one = [[eng._chunks[int(r)].id for r in eng.index.search_range(oracle.normalize(e), 0.98, before)[0][0]] for e in emb]
        assert eng.duplicates_of(emb, 0.98) == one_by_one
        inside = eng.duplicates_of(emb, 0.98, documents=["b.pdf"])
        assert inside[3] == [eng._chunks[450].id] and inside[1] == []
        eng.index.range_batch_forms(reset=True)
        ids, dup = eng.add_document("new.pdf", [f"new {i}" for i in range(4)], emb, report_duplicates_above=0.98)
        forms = eng.index.range_batch_forms()
        assert forms[0] + forms[1] > 0 and sum(forms) == 4, forms               # shared passes have run
        assert len(ids) == 4 and len(eng) == before + 4 and dup == one_by_one
        for i in range(4):
            want, _ = R.expect(oracle.scan(rows, oracle.normalize(emb[i])), 0.98, before)
            assert dup[i] == [eng._chunks[int(r)].id for r in want], i
        assert eng._chunks[5].id in dup[1] and eng._chunks[450].id in dup[3]
    finally:
        eng.close()


def test_engine_duplicate_chunks_finds_planted_pairs_and_a_triple(rlr, oracle):
    rng = np.random.default_rng(54)
    a = rng.standard_normal((300, DIM)).astype(np.float32)
    b = rng.standard_normal((240, DIM)).astype(np.float32)
    b[10], b[20], b[239] = a[3], a[77] * np.float32(0.5), a[299]               # three pairs across the 256-row block edge
    a[100], b[100] = a[40], a[40]                                              # a triple: rows 40, 100, 400
    eng = rlr.RagEngine(DIM)
    try:
        eng.add_document("a.pdf", [f"a {i}" for i in range(300)], a)
        eng.add_document("b.pdf", [f"b {i}" for i in range(240)], b)
        eng.index.set_range_sharing(2)
        got = eng.duplicate_chunks(0.999)
        ids = [ch.id for ch in eng._chunks]
        want = {(3, 310), (77, 320), (299, 539), (40, 100), (40, 400), (100, 400)}
        assert {(ids.index(x), ids.index(y)) for x, y, _ in got} == want and len(got) == len(want)
        rows = eng.index.fetch_rows(np.arange(len(eng)))
        for x, y, c in got:
            assert bits(F32(c)) == bits(oracle.scan(rows[[ids.index(y)]], rows[ids.index(x)]))[0]
    finally:
        eng.close()


def test_engine_abi_batch_equals_the_single_entry_per_query(rlr, oracle):
    rng = np.random.default_rng(55)
    eng = _engine(rlr, rng, {"a.pdf": 400, "b.pdf": 70})
    try:
        N = rlr._native
        L = N.lib()
        nq, cap, dq = 5, 50, DIM + 3                                            # dq beyond the index dim: zip-truncated
        raw = (2.0 * rng.standard_normal((nq, dq))).astype(np.float32)
        mins = np.array([0.05, 0.1, -0.2, 0.12, 0.0], np.float32)
        f = eng._filter_for(["a.pdf"])
        for handle in (None, f.handle):
            hits = (N.SearchHitC * (nq * cap))()
            n_out = np.zeros(nq, np.uint32)
            n_total = np.zeros(nq, np.uint64)
            N.check(L.rlr_engine_search_range_batch(eng.index.handle, handle, raw.ctypes.data_as(N.f32p), nq, dq, mins.ctypes.data_as(N.f32p),
                                                    cap, hits, n_out.ctypes.data_as(N.u32p), n_total.ctypes.data_as(N.u64p)))
            for q in range(nq):
                one = (N.SearchHitC * cap)()
                n, total = C.c_uint32(), C.c_uint64()
                N.check(L.rlr_engine_search_range(eng.index.handle, handle, raw[q].ctypes.data_as(N.f32p), dq, float(mins[q]), cap, one,
                                                  C.byref(n), C.byref(total)))
                assert n.value == n_out[q] and total.value == n_total[q] and total.value > 0, q
                assert bytes(one)[:n.value * C.sizeof(N.SearchHitC)] == bytes(hits)[q * cap * C.sizeof(N.SearchHitC):][:n.value * C.sizeof(N.SearchHitC)]
    finally:
        eng.close()
