"""rlr_search_range on the device against the definition of tests/range_vectors.py (threshold and order over
oracle.scan): rows equal, scores bit-equal, n_total equal, count-only equal -- and the form counters say WHICH path
answered: every case is decided on the device (form 0) unless it is named here as a hand-off case:
  form 1  more hits than cap (n_total exact, the rows those of search_topk at k = cap), more than RLR_RANGE_DEVICE_MAX hits
  form 2  a row holding NaN among the allowed rows
  form 3  a list-path filter

Shapes: dim 8 f32 (generic scan) at the word, tile and workgroup edges 1, 63, 64, 65, 4095, 4096, 4097 and at 20 000
rows, 2^20 + 65 rows from fill_synthetic, 768-d f32 (fixed kernel) at 4096 rows, 256-d binary16 at 4100 rows."""
import threading

import numpy as np
import pytest

import band_vectors as B
import range_vectors as R
from conftest import bits

pytestmark = pytest.mark.gpu

F32 = np.float32
CAP = 100
SHAPES = [(8, "f32", n) for n in (1, 63, 64, 65, 4095, 4096, 4097, 20000)] + [(768, "f32", 4096), (256, "f16", 4100)]
MILLION = (1 << 20) + 65


def _query(O, dim, seed):
    return O.normalize(O.synth_query(dim, seed=seed))


def same_scores(got, want):
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    return got.shape == want.shape and bool(np.all(bits(got) == bits(want)))


def hit_counts(n):
    """the n_total a corpus of n rows is asked for: 0, 1, the finish edge, cap - 1, cap, cap + 1, n"""
    return sorted({t for t in (0, 1, 2047, 2048, 2049, CAP - 1, CAP, CAP + 1, n) if t <= n})


class Corpus:
    """an index, its rows on the host, and one query with the reference-order scores and the result order made once"""

    def __init__(self, rlr, O, dim, dtype, n, seed, synthetic=False, rows=None, q=None):
        self.O, self.dim, self.n, self.seed = O, dim, n, seed
        self.rows = O.synth_rows(n, dim, seed=seed, f16=dtype == "f16") if rows is None else rows
        self.q = _query(O, dim, seed + 1) if q is None else q
        self.e = O.scan(self.rows, self.q)
        self.order = R.result_order(self.e, np.arange(self.e.size))
        self.ix = rlr.GpuIndex(dim, dtype)
        if synthetic:
            self.ix.fill_synthetic(n, seed=seed)
        else:
            self.ix.upload(self.rows)

    def ranks_are_distinct(self, counts):
        """the precondition of thresholds placed on real scores: the rank-t and rank-(t + 1) scores differ"""
        s = self.e[self.order]
        return all(not (0 < t < self.n) or s[t - 1] != s[t] for t in counts)

    def taus_for(self, t):
        """thresholds with exactly t hits: the rank-t score (that row is included) and one ulp above the rank-(t + 1)
        score (that row is excluded); -inf for every row"""
        s = self.e[self.order]
        taus = []
        if t >= 1:
            taus.append(s[t - 1])
        if t < self.n:
            taus.append(np.nextafter(s[t], F32(np.inf)))
        if t == self.n:
            taus.append(F32(-np.inf))
        return taus

    def check(self, tau, cap, ctx, allowed=None, filter=None, form=0, count_form=None):
        """one range query == the definition; exactly one query counted, in `form`; then the count-only call"""
        ix = self.ix
        want_rows, want_total = R.expect(self.e, tau, cap, allowed)
        ix.range_forms(reset=True)
        r, c, total = ix.search_range(self.q, tau, cap, filter=filter)[0]
        forms = ix.range_forms()
        assert total == want_total, (ctx, tau, cap, total, want_total)
        assert np.array_equal(r, want_rows), (ctx, tau, cap, r[:8], want_rows[:8])
        assert same_scores(c, self.e[want_rows.astype(np.int64)]), (ctx, tau, cap)
        assert sum(forms) == 1 and forms[form] == 1, (ctx, tau, cap, forms, form)
        if cap:
            # count-only: never a capacity hand-off (nothing is fetched); the other forms as the rows call
            count_form = (0 if form == 1 else form) if count_form is None else count_form
            ix.range_forms(reset=True)
            assert ix.count_range(self.q, tau, filter=filter) == [want_total], (ctx, tau, "count-only")
            forms = ix.range_forms()
            assert sum(forms) == 1 and forms[count_form] == 1, (ctx, tau, "count-only", forms)
        return r, c, total

    def close(self):
        self.ix.close()


def make_corpus(rlr, O, dim, dtype, n, synthetic=False):
    """a corpus whose scores are distinct at every rank a threshold is placed on (another seed otherwise)"""
    for attempt in range(8):
        cp = Corpus(rlr, O, dim, dtype, n, seed=0x7A00 + n + 977 * attempt, synthetic=synthetic)
        if cp.ranks_are_distinct(hit_counts(n)):
            return cp
        cp.close()
    raise AssertionError("no seed gives distinct scores at the designed ranks")


@pytest.fixture(scope="module")
def corpus_of(rlr, oracle):
    made = {}

    def get(dim, dtype, n):
        key = (dim, dtype, n)
        if key not in made:
            made[key] = make_corpus(rlr, oracle, dim, dtype, n, synthetic=n > (1 << 20))
        return made[key]

    yield get
    for c in made.values():
        c.close()


# ---- thresholds placed on real scores -----------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,dtype,n", SHAPES)
def test_thresholds_on_real_scores(corpus_of, dim, dtype, n):
    cp = corpus_of(dim, dtype, n)
    assert cp.ranks_are_distinct(hit_counts(n))
    for t in hit_counts(n):
        for tau in cp.taus_for(t):
            assert R.expect(cp.e, tau, 0)[1] == t
            cp.check(tau, CAP, (n, t), form=1 if t > CAP else 0)             # HAND-OFF: more hits than cap
            cp.check(tau, max(n, 1), (n, t, "room for all"))                   # through the finish, or the one copy beyond it
    cp.check(F32(np.inf), CAP, (n, "tau = +inf"))
    cp.check(F32(-0.0), CAP, (n, "tau = -0"), form=1 if R.expect(cp.e, -0.0, 0)[1] > CAP else 0)


def test_a_million_rows(corpus_of):
    cp = corpus_of(8, "f32", MILLION)
    n = MILLION
    assert np.array_equal(bits(cp.ix.fetch_rows([0, n - 1])), bits(cp.rows[[0, n - 1]]))
    for t in (0, 1, CAP - 1, CAP, CAP + 1, 2047, 2048, 2049):
        for tau in cp.taus_for(t):
            cp.check(tau, 4096, (n, t))
    cp.check(cp.taus_for(CAP + 1)[0], CAP, (n, "cap + 1 hits"), form=1)        # HAND-OFF: more hits than cap
    # HAND-OFF, the one case beyond the device capacity: every row is a hit, 70 000 are wanted
    cp.check(F32(-np.inf), 70000, (n, "beyond RLR_RANGE_DEVICE_MAX"), form=1)
    # just inside it: 65 536 hits wanted and held
    t = R.DEVICE_MAX
    s = cp.e[cp.order]
    if s[t - 1] != s[t]:
        cp.check(s[t - 1], 70000, (n, "RLR_RANGE_DEVICE_MAX hits"))


@pytest.mark.parametrize("dim,dtype,n", [(8, "f32", 4097), (8, "f32", 20000), (768, "f32", 4096), (256, "f16", 4100)])
def test_capacity_answers_equal_search_topk(corpus_of, dim, dtype, n):
    cp = corpus_of(dim, dtype, n)
    plain_r, plain_c = cp.ix.search_topk(cp.q, CAP)
    tau = cp.taus_for(2049)[0]
    r, c, total = cp.check(tau, CAP, (n, "2049 hits, cap 100"), form=1)
    assert total == 2049 and np.array_equal(r, plain_r[0]) and same_scores(c, plain_c[0])
    allowed = np.arange(0, n, 3)
    with cp.ix.filter_rows(allowed) as f:
        f.set_path("scan")
        fr, fc = cp.ix.search_topk(cp.q, CAP, filter=f)
        tau = cp.e[allowed][R.result_order(cp.e[allowed], allowed)][CAP + 20]
        r, c, total = cp.check(tau, CAP, (n, "filtered, more than cap"), allowed=allowed, filter=f, form=1)
        assert total >= CAP + 21 and np.array_equal(r, fr[0]) and same_scores(c, fc[0])


# ---- rows built to err at the bound ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("maker,f16", [("absorption", False), ("absorption", True), ("operand_rounding", False),
                                       ("operand_rounding", True)])
def test_membership_inside_the_band(rlr, oracle, maker, f16):
    """band_vectors: X's exact score lies above 150 decoys' while the decoys NOMINATE above X.  tau = X's exact score
    (X is a hit, no decoy is) and one ulp above (X is none either): the decision lies inside the band on both sides"""
    rows, batch, facts = getattr(B, maker)(oracle, 1, f16=f16)
    cp = Corpus(rlr, oracle, rows.shape[1], "f16" if f16 else "f32", rows.shape[0], seed=0, rows=rows, q=batch[0])
    try:
        x, decoys = facts["x"], facts["decoys"]
        assert (cp.e[decoys] < cp.e[x]).all()
        r, _, total = cp.check(cp.e[x], 4096, (maker, f16, "tau = e(X)"))
        assert x in r and not np.isin(decoys, r).any()
        r, _, _ = cp.check(np.nextafter(cp.e[x], F32(np.inf)), 4096, (maker, f16, "tau = e(X) + 1 ulp"))
        assert x not in r and not np.isin(decoys, r).any()
        best = decoys[R.result_order(cp.e[decoys], decoys)][0]
        r, _, _ = cp.check(cp.e[best], 4096, (maker, f16, "tau = the best decoy's score"))
        assert x in r and best in r
    finally:
        cp.close()


# ---- ties ---------------------------------------------------------------------------------------------------------------
def test_duplicate_rows_come_in_ascending_row_order(rlr, oracle):
    rows = oracle.synth_rows(3000, 8, seed=77)
    dup = np.array([10, 11, 12, 300, 301, 2999])
    rows[dup] = rows[10]
    cp = Corpus(rlr, oracle, 8, "f32", 3000, seed=0, rows=rows, q=rows[10].copy())
    try:
        r, c, total = cp.check(cp.e[10], CAP, "duplicates")
        assert total == dup.size and r.tolist() == dup.tolist() and len(set(bits(c).tolist())) == 1
        cp.check(np.nextafter(cp.e[10], F32(np.inf)), CAP, "above the duplicates")
    finally:
        cp.close()


def test_five_thousand_identical_rows_are_all_hits(rlr, oracle):
    rows = np.tile(oracle.synth_rows(1, 8, seed=9), (5000, 1))
    cp = Corpus(rlr, oracle, 8, "f32", 5000, seed=10, rows=rows)
    try:
        r, _, total = cp.check(cp.e[0], 5000, "identical")                     # every tile full of hits
        assert total == 5000 and r.tolist() == list(range(5000))
        cp.check(cp.e[0], CAP, "identical, cap 100", form=1)                   # HAND-OFF: more hits than cap
        cp.check(np.nextafter(cp.e[0], F32(np.inf)), CAP, "identical, above")
    finally:
        cp.close()


def test_zero_scores_against_both_zeros(rlr, oracle):
    rows = oracle.synth_rows(200, 8, seed=31)
    q = np.zeros(8, np.float32)
    q[0] = 1.0
    rows[[5, 6, 150], 0] = 0.0                                                  # score +0 exactly
    rows[7] = 0.0
    rows[8, 0] = -0.0
    cp = Corpus(rlr, oracle, 8, "f32", 200, seed=0, rows=rows, q=q)
    try:
        assert (cp.e[[5, 6, 7, 8, 150]] == 0.0).all()
        for tau in (F32(0.0), F32(-0.0)):
            r, _, _ = cp.check(tau, 200, ("zeros", tau))
            assert {5, 6, 7, 8, 150} <= set(r.tolist())
        r, _, _ = cp.check(np.nextafter(F32(0.0), F32(1.0)), 200, "the smallest positive tau")
        assert not {5, 6, 7, 8, 150} & set(r.tolist())
    finally:
        cp.close()


# ---- non-finite values ------------------------------------------------------------------------------------------------------
def test_a_row_holding_infinity_is_a_hit(rlr, oracle):
    rows = oracle.synth_rows(500, 8, seed=41)
    q = np.abs(_query(oracle, 8, 42)) + F32(0.01)                               # all positive: the row scores +Inf, not NaN
    rows[123, 2] = np.inf
    cp = Corpus(rlr, oracle, 8, "f32", 500, seed=0, rows=rows, q=oracle.normalize(q))
    try:
        assert cp.e[123] == np.inf
        r, c, total = cp.check(F32(0.5), CAP, "inf row")
        assert r[0] == 123 and c[0] == np.inf
        r, _, total = cp.check(F32(np.inf), CAP, "tau = +inf")
        assert total == 1 and r.tolist() == [123]
        cp.check(F32(-np.inf), 500, "tau = -inf")
    finally:
        cp.close()


def test_a_row_holding_nan_is_never_a_hit_and_hands_off(rlr, oracle):
    rows = oracle.synth_rows(400, 8, seed=5)
    rows[17, 3] = np.nan
    cp = Corpus(rlr, oracle, 8, "f32", 400, seed=6, rows=rows)
    try:
        for tau in (F32(-np.inf), cp.e[cp.order[20]], F32(2.0)):
            r, _, total = cp.check(tau, 400, ("nan row", tau), form=2)          # HAND-OFF: a NaN among the allowed rows
            assert 17 not in r
        assert cp.check(F32(-np.inf), 400, "nan row", form=2)[2] == 399
        with cp.ix.filter_rows(np.r_[0:17, 18:400]) as f:                      # the NaN row masked out: decided on the device
            f.set_path("scan")
            cp.check(F32(-np.inf), 400, "nan row outside the mask", allowed=np.r_[0:17, 18:400], filter=f)
    finally:
        cp.close()


# ---- filters ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,dtype,n", [(8, "f32", 65), (8, "f32", 4097), (8, "f32", 20000), (768, "f32", 4096), (256, "f16", 4100)])
def test_with_a_filter_on_both_paths(corpus_of, dim, dtype, n):
    cp = corpus_of(dim, dtype, n)
    ix = cp.ix
    best = int(cp.order[0])
    allowed = np.setdiff1d(np.arange(0, n, 3), [best])                         # the best hit of all lies just outside the mask
    srt = cp.e[allowed][R.result_order(cp.e[allowed], allowed)]
    with ix.filter_rows(allowed) as f:
        for path, form in (("list", 3), ("scan", 0)):                          # HAND-OFF: a list-path filter, by rule
            f.set_path(path)
            for j in (0, min(10, allowed.size - 1), allowed.size - 1):
                over = path == "scan" and R.expect(cp.e, srt[j], 0, allowed)[1] > CAP   # HAND-OFF: more hits than cap
                r, _, _ = cp.check(srt[j], CAP, (n, path, j), allowed=allowed, filter=f, form=1 if over else form)
                assert best not in r
            cp.check(F32(-np.inf), n, (n, path, "all"), allowed=allowed, filter=f, form=form)
            cp.check(F32(np.inf), CAP, (n, path, "none"), allowed=allowed, filter=f, form=form)
    ids = (np.arange(n) // 5).astype(np.uint32)
    ix.set_documents(ids)
    docs = np.unique(ids)[::4]
    allowed = np.flatnonzero(np.isin(ids, docs))
    with ix.filter_documents(docs) as f:
        for path, form in (("list", 3), ("scan", 0)):
            f.set_path(path)
            cp.check(cp.e[allowed].max(), CAP, (n, "documents", path), allowed=allowed, filter=f, form=form)
            cp.check(np.median(cp.e[allowed]).astype(np.float32), n, (n, "documents", path), allowed=allowed, filter=f, form=form)
    with ix.filter_documents([0xFFFFFFF0]) as f:                               # an empty filter: RLR_OK, both counts 0, nothing counted
        ix.range_forms(reset=True)
        r, c, total = ix.search_range(cp.q, -np.inf, CAP, filter=f)[0]
        assert r.size == 0 and total == 0 and ix.count_range(cp.q, -np.inf, filter=f) == [0] and sum(ix.range_forms()) == 0


def test_argument_rules(rlr, oracle, corpus_of):
    cp = corpus_of(8, "f32", 65)
    other = corpus_of(8, "f32", 64)
    with pytest.raises(rlr.RlrError) as ei:
        cp.ix.search_range(cp.q, np.nan, 5)
    assert ei.value.status == -1
    with pytest.raises(rlr.RlrError) as ei:
        cp.ix.search_range(np.stack([cp.q, cp.q]), [0.5, np.nan], 0)
    assert ei.value.status == -1
    with other.ix.filter_rows([1, 2, 3]) as f, pytest.raises(rlr.RlrError) as ei:
        cp.ix.search_range(cp.q, 0.0, 5, filter=f)                             # another index's filter
    assert ei.value.status == -1
    ix = rlr.GpuIndex(8)
    try:
        assert ix.search_range(cp.q, -np.inf, 5)[0][2] == 0 and ix.count_range(cp.q, -np.inf) == [0]   # an empty index
        ix.upload(cp.rows)
        with ix.filter_rows([1, 2, 3]) as f:
            assert ix.search_range(cp.q, -np.inf, 5, filter=f)[0][2] == 3
            ix.append(cp.rows[:2])
            with pytest.raises(rlr.RlrError) as ei:
                ix.search_range(cp.q, -np.inf, 5, filter=f)                    # stale
            assert ei.value.status == -1
            with pytest.raises(rlr.RlrError):
                ix.count_range(cp.q, -np.inf, filter=f)
    finally:
        ix.close()


# ---- batches and concurrency ------------------------------------------------------------------------------------------------
def test_three_queries_with_three_thresholds_equal_three_calls(oracle, corpus_of):
    cp = corpus_of(8, "f32", 20000)
    qs = np.stack([_query(oracle, 8, 700 + i) for i in range(3)])
    taus = np.array([0.9, 0.2, -0.5], np.float32)
    single = [cp.ix.search_range(qs[i], taus[i], 3000)[0] for i in range(3)]
    cp.ix.range_forms(reset=True)
    batch = cp.ix.search_range(qs, taus, 3000)
    assert sum(cp.ix.range_forms()) == 3
    for i in range(3):
        want_rows, want_total = R.expect(oracle.scan(cp.rows, qs[i]), taus[i], 3000)
        assert np.array_equal(batch[i][0], want_rows) and batch[i][2] == want_total
        assert np.array_equal(batch[i][0], single[i][0]) and same_scores(batch[i][1], single[i][1]) and batch[i][2] == single[i][2]
    assert cp.ix.count_range(qs, taus) == [b[2] for b in batch]


def test_four_threads_return_what_the_serial_calls_return(oracle, corpus_of):
    cp = corpus_of(8, "f32", 20000)
    qs = [_query(oracle, 8, 900 + i) for i in range(4)]
    taus = [F32(0.8), F32(0.5), F32(0.0), F32(0.95)]
    serial = [cp.ix.search_range(qs[i], taus[i], 4096)[0] for i in range(4)]
    got, errors = [None] * 4, []

    def work(i):
        try:
            for _ in range(20):
                got[i] = cp.ix.search_range(qs[i], taus[i], 4096)[0]
                if not (np.array_equal(got[i][0], serial[i][0]) and same_scores(got[i][1], serial[i][1]) and got[i][2] == serial[i][2]):
                    errors.append(i)
        except Exception as e:                               # noqa: BLE001 (reported below)
            errors.append(e)

    threads = [threading.Thread(target=work, args=(i,)) for i in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for i in range(4):
        want_rows, want_total = R.expect(oracle.scan(cp.rows, qs[i]), taus[i], 4096)
        assert np.array_equal(serial[i][0], want_rows) and serial[i][2] == want_total


def test_a_plain_search_after_a_range_call_on_the_same_context(rlr, oracle):
    """one thread, one context: the range finish must leave the context's histogram cleared for the next query"""
    cp = Corpus(rlr, oracle, 8, "f32", 20000, seed=0x7B01)
    try:
        before_r, before_c = cp.ix.search_topk(cp.q, 100)
        for tau, cap in ((F32(0.5), 4096), (F32(-np.inf), 0), (F32(0.9), CAP)):
            cp.ix.search_range(cp.q, tau, cap)
            r, c = cp.ix.search_topk(cp.q, 100)
            assert np.array_equal(r, before_r) and same_scores(c, before_c)
            want = cp.order[:100].astype(np.uint64)
            assert np.array_equal(r[0], want)
    finally:
        cp.close()


# ---- the engine -------------------------------------------------------------------------------------------------------------
def _engine(rlr, rng, sizes):
    eng = rlr.RagEngine(8)
    for name, n in sizes.items():
        eng.add_document(name, [f"{name} {i}" for i in range(n)], rng.standard_normal((n, 8)).astype(np.float32))
    return eng


def test_engine_search_above_equals_the_definition(rlr, oracle):
    rng = np.random.default_rng(51)
    eng = _engine(rlr, rng, {"a.pdf": 400, "b.pdf": 70, "c.pdf": 1, "d.pdf": 2500})
    try:
        q_raw = (3.0 * rng.standard_normal(8)).astype(np.float32)              # not unit norm: the engine normalises it
        rows = eng.index.fetch_rows(np.arange(len(eng)))
        e = oracle.scan(rows, oracle.normalize(q_raw))
        for names in (None, ["a.pdf", "c.pdf"], ["d.pdf"], ["nothing.pdf"]):
            allowed = None if names is None else np.asarray([r for r, ch in enumerate(eng._chunks) if ch.document_name in names], np.int64)
            for min_score, limit in ((0.9, 100), (0.5, 100), (0.5, 5000), (-2.0, 10), (-2.0, 5000), (2.0, 10)):
                want_rows, want_total = R.expect(e, min_score, limit, allowed)
                got, total = eng.search_above(q_raw, min_score, limit, documents=names)
                assert total == want_total and [g.row for g in got] == want_rows.tolist(), (names, min_score, limit)
                for g in got:
                    assert bits(np.float32(g.score)) == bits(e[g.row]) and g.score == g.embedding_score == g.initial_score
                    assert g.lexical_score == 0.0 and g.document == eng._chunks[g.row].document_name
                assert eng.count_above(q_raw, min_score, documents=names) == want_total
    finally:
        eng.close()


def test_engine_similar_chunks_omits_the_chunk_itself(rlr, oracle):
    rng = np.random.default_rng(52)
    eng = _engine(rlr, rng, {"a.pdf": 300, "b.pdf": 200})
    try:
        rows = eng.index.fetch_rows(np.arange(len(eng)))
        for row in (0, 299, 300, 499):
            cid = eng._chunks[row].id
            e = oracle.scan(rows, rows[row])
            for names in (None, ["b.pdf"]):
                allowed = np.asarray([r for r, ch in enumerate(eng._chunks) if r != row and (names is None or ch.document_name in names)])
                for min_score, limit in ((0.6, 100), (0.0, 7)):
                    want_rows, want_total = R.expect(e, min_score, limit, allowed)
                    got, total = eng.similar_chunks(cid, min_score, limit, documents=names)
                    assert total == want_total and [g.row for g in got] == want_rows.tolist(), (row, names, min_score)
                    assert all(g.chunk_id != cid for g in got)
                    assert all(bits(np.float32(g.score)) == bits(e[g.row]) for g in got)
    finally:
        eng.close()


def test_engine_add_document_reports_planted_duplicates(rlr, oracle):
    rng = np.random.default_rng(53)
    eng = _engine(rlr, rng, {"a.pdf": 300, "b.pdf": 200})
    try:
        old = eng.index.fetch_rows([5, 450])
        emb = rng.standard_normal((4, 8)).astype(np.float32)
        emb[1] = old[0] * np.float32(3.0)                                       # chunk 1 repeats row 5 of a.pdf (scaled: normalised away)
        emb[3] = old[1]                                                         # chunk 3 repeats row 450 of b.pdf
        before = len(eng)
        ids, dup = eng.add_document("new.pdf", [f"new {i}" for i in range(4)], emb, report_duplicates_above=0.98)
        assert len(ids) == 4 and len(eng) == before + 4
        rows = eng.index.fetch_rows(np.arange(before))
        for i in range(4):
            want, _ = R.expect(oracle.scan(rows, oracle.normalize(emb[i])), 0.98, before)
            assert dup[i] == [eng._chunks[int(r)].id for r in want], i
        assert eng._chunks[5].id in dup[1] and eng._chunks[450].id in dup[3]
        plain = eng.add_document("other.pdf", ["x", "y"], rng.standard_normal((2, 8)).astype(np.float32))
        assert isinstance(plain, list) and len(plain) == 2 and all(isinstance(i, str) for i in plain)
        assert len(eng) == before + 6
    finally:
        eng.close()
