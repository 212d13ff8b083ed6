"""rlr_search_topk_grouped on the device against the model of tests/grouped_vectors.py (the walk of the contract over
oracle.scan): rows equal, scores bit-equal, document ids equal to the column -- and the form counters say WHICH path
answered: every case is served by the device-selected form 0 unless it is named here as a hand-off case.

Shapes: dim 8 f32 (generic scan) at the word and workgroup edges 1, 63, 64, 65, 4095, 4096, 4097 and at 20 000 rows,
2^20 + 65 rows from fill_synthetic, 768-d f32 (fixed kernel) at 4096 rows, 256-d binary16 at 4100 rows; k in 1, 10, 100;
per_doc in 1, 2, 3, 8; id patterns from document_vectors.id_patterns."""
import threading

import numpy as np
import pytest

import band_vectors as B
import document_vectors as V
import grouped_vectors as G
from conftest import bits

pytestmark = pytest.mark.gpu

KS, PER_DOC = (1, 10, 100), (1, 2, 3, 8)
COMBOS = [(k, m) for k in KS for m in PER_DOC]


def _query(O, dim, seed):
    return O.normalize(O.synth_query(dim, seed=seed))


def same_scores(got, want):
    """bit equality; a NaN equals a NaN (the library returns the canonical quiet NaN for every NaN score)"""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    return got.shape == want.shape and bool(np.all((bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want))))


class Corpus:
    """an index, its rows on the host, and one query with the reference-order scores and the result order made once"""

    def __init__(self, rlr, O, dim, dtype, n, seed, synthetic=False, rows=None, q=None):
        self.O, self.dim, self.n = O, dim, n
        self.rows = O.synth_rows(n, dim, seed=seed, f16=dtype == "f16") if rows is None else rows
        self.ix = rlr.GpuIndex(dim, dtype)
        if synthetic:
            self.ix.fill_synthetic(n, seed=seed)
        else:
            self.ix.upload(self.rows)
        self.q = _query(O, dim, seed + 1) if q is None else q
        self.rescan()

    def rescan(self):
        self.e = self.O.scan(self.rows, self.q)
        self.order = G.result_order(self.e)

    def want(self, docs, k, m, allowed=None):
        docs = np.full(self.rows.shape[0], G.DOC_NONE, np.uint32) if docs is None else np.asarray(docs, np.uint32)
        if allowed is None:
            return G.walk(self.order, docs, k, m), docs
        return G.expect(self.e, docs, k, m, allowed), docs

    def check(self, docs, k, m, ctx, allowed=None, filter=None, form=0):
        """one grouped query == the model; exactly one query counted, by (one of) `form`"""
        ix = self.ix
        ix.grouped_forms(reset=True)
        r, c, d = ix.search_topk_grouped(self.q, k, m, filter=filter)[0]
        want, docs = self.want(docs, k, m, allowed)
        assert np.array_equal(r, want), (ctx, k, m, r[:8], want[:8])
        assert same_scores(c, self.e[want.astype(np.int64)]), (ctx, k, m)
        assert np.array_equal(d, docs[want.astype(np.int64)]), (ctx, k, m)
        forms = ix.grouped_forms()
        allowed_forms = (form,) if isinstance(form, int) else form
        assert sum(forms) == 1 and any(forms[f] == 1 for f in allowed_forms), (ctx, k, m, forms, form)
        return r, c, d

    def close(self):
        self.ix.close()


@pytest.fixture(scope="module")
def corpus_of(rlr, oracle):
    made = {}

    def get(dim, dtype, n):
        key = (dim, dtype, n)
        if key not in made:
            made[key] = Corpus(rlr, oracle, dim, dtype, n, seed=0x6A00 + n, synthetic=n > (1 << 20))
        return made[key]

    yield get
    for c in made.values():
        c.close()


# ---- identities against the existing calls, and the model, over every id pattern ------------------------------------
@pytest.mark.parametrize("dim,dtype,n", [(8, "f32", n) for n in (1, 63, 64, 65, 4095, 4096, 4097, 20000)] +
                         [(768, "f32", 4096), (256, "f16", 4100)])
def test_every_id_pattern_equals_the_model(corpus_of, dim, dtype, n):
    cp = corpus_of(dim, dtype, n)
    ix = cp.ix
    plain_r, plain_c = ix.search_topk(cp.q, 100)
    patterns = V.id_patterns(n)
    small = n <= 4097 and dim == 8
    for p, (name, ids, _) in enumerate(patterns):
        ix.set_documents(ids)
        assert np.array_equal(ix.get_documents(), ids)
        # (the larger corpora: four of the twelve (k, per_doc) pairs per pattern, every pair over the patterns)
        for k, m in (COMBOS if small else [COMBOS[(p + 3 * j) % 12] for j in range(4)]):
            r, c, _ = cp.check(ids, k, m, (n, name))
            if name == "all_one_document":                   # the first min(k, per_doc) results of search_topk
                take = min(k, m, n)
                assert np.array_equal(r, plain_r[0, :take]) and same_scores(c, plain_c[0, :take]), (n, k, m)
    # every row its own document, and per_doc at or above the largest document: search_topk
    ix.set_documents(np.arange(n, dtype=np.uint32) + 5)
    for k, m in ((1, 1), (10, 3), (100, 1)):
        r, c, _ = cp.check(np.arange(n, dtype=np.uint32) + 5, k, m, (n, "own_documents"))
        assert np.array_equal(r, plain_r[0, :min(k, n)]) and same_scores(c, plain_c[0, :min(k, n)])
    ids = (np.arange(n) // 8).astype(np.uint32)
    ix.set_documents(ids)
    for k in KS:
        r, c, _ = cp.check(ids, k, 8, (n, "per_doc_covers_every_document"))
        assert np.array_equal(r, plain_r[0, :min(k, n)]) and same_scores(c, plain_c[0, :min(k, n)])


@pytest.mark.parametrize("dim,dtype,n", [(8, "f32", 65), (8, "f32", 4097), (768, "f32", 4096), (256, "f16", 4100)])
def test_an_index_without_a_column_equals_search_topk(rlr, oracle, dim, dtype, n):
    cp = Corpus(rlr, oracle, dim, dtype, n, seed=0x6B00 + n)
    try:
        plain_r, plain_c = cp.ix.search_topk(cp.q, 100)
        for k, m in ((1, 1), (10, 2), (100, 8)):
            r, c, d = cp.check(None, k, m, (n, "no_column"))
            assert np.array_equal(r, plain_r[0, :min(k, n)]) and same_scores(c, plain_c[0, :min(k, n)])
            assert (d == G.DOC_NONE).all()
    finally:
        cp.close()


def test_a_million_rows(corpus_of):
    n = (1 << 20) + 65
    cp = corpus_of(8, "f32", n)
    assert np.array_equal(bits(cp.ix.fetch_rows([0, n - 1])), bits(cp.rows[[0, n - 1]]))
    plain_r, plain_c = cp.ix.search_topk(cp.q, 100)
    r, c, _ = cp.check(None, 100, 1, "no_column")
    assert np.array_equal(r, plain_r[0]) and same_scores(c, plain_c[0])
    for ids, k, m in ((V.random_1000(n), 100, 1), (V.random_1000(n), 100, 3), ((np.arange(n) // 1000).astype(np.uint32), 100, 2),
                      (np.arange(n, dtype=np.uint32), 10, 1)):
        cp.ix.set_documents(ids)
        cp.check(ids, k, m, "2^20+65")


@pytest.mark.parametrize("dim,dtype,n", [(8, "f32", 65), (8, "f32", 4097), (8, "f32", 20000), (768, "f32", 4096), (256, "f16", 4100)])
def test_with_a_filter_on_both_paths(corpus_of, dim, dtype, n):
    cp = corpus_of(dim, dtype, n)
    ix = cp.ix
    for p, (name, ids, docs) in enumerate(V.id_patterns(n)):
        if name.startswith("run_") and not name.endswith("_at_63"):
            continue
        ix.set_documents(ids)
        allowed = np.flatnonzero(V.member_of(ids, docs))
        with ix.filter_documents(docs) as f:
            for path, form in (("list", 3), ("scan", 0)):
                f.set_path(path)
                for k, m in [COMBOS[(p + 5 * j) % 12] for j in range(2)]:
                    if allowed.size == 0:                    # an empty filter: RLR_OK, no result, no query counted
                        ix.grouped_forms(reset=True)
                        assert ix.search_topk_grouped(cp.q, k, m, filter=f)[0][0].size == 0 and sum(ix.grouped_forms()) == 0
                    else:
                        cp.check(ids, k, m, (n, name, path), allowed=allowed, filter=f, form=form)
    # a row filter that cuts across documents
    ids = (np.arange(n) // 5).astype(np.uint32)
    ix.set_documents(ids)
    allowed = np.arange(0, n, 3)
    with ix.filter_rows(allowed) as f:
        for path, form in (("list", 3), ("scan", 0)):
            f.set_path(path)
            cp.check(ids, 10, 2, (n, "every_third_row", path), allowed=allowed, filter=f, form=form)


# ---- designed cases ---------------------------------------------------------------------------------------------------
def test_duplicate_rows_inside_and_across_documents(rlr, oracle):
    rows = oracle.synth_rows(600, 8, seed=77)
    rows[[11, 12, 300, 301]] = rows[10]                      # 10, 11, 12 in one document; 300 and 301 in two others
    rows[[401, 402]] = rows[400]                             # a document of nothing but duplicates
    ids = (np.arange(600) // 10).astype(np.uint32)
    ids[401:403] = ids[400] = 900
    ids[301] = 901
    for q, lowest in ((rows[10].copy(), 10), (rows[400].copy(), 400)):
        cp = Corpus(rlr, oracle, 8, "f32", 600, seed=0, rows=rows, q=q)
        try:
            cp.ix.set_documents(ids)
            for k, m in COMBOS:
                r, _, _ = cp.check(ids, k, m, ("duplicates", lowest))
                assert r[0] == lowest                        # the lower row wins
            r, _, d = cp.check(ids, 10, 1, "duplicates")
            assert np.unique(d).size == d.size               # one row per document ...
            if lowest == 400:
                assert 401 not in r and 402 not in r         # ... and the document of duplicates gives its lowest row
            else:
                assert {10, 300, 301} <= set(r.tolist()) and 11 not in r and 12 not in r
        finally:
            cp.close()


@pytest.mark.parametrize("arrangement", ["decoys_in_x_document", "every_row_its_own_document"])
def test_absorption_corpus(rlr, oracle, arrangement):
    """band_vectors.absorption: X's exact score is the k-th best; 150 decoys score just below it and nominate above it"""
    k = 10
    rows, batch, f = B.absorption(oracle, k, dim=768, n=4096)
    cp = Corpus(rlr, oracle, 768, "f32", 4096, seed=0, rows=rows, q=batch[0])
    try:
        x, decoys = f["x"], f["decoys"]
        assert (cp.e[decoys] < cp.e[x]).all()
        ids = np.arange(4096, dtype=np.uint32) + 100
        if arrangement == "decoys_in_x_document":
            ids[decoys] = ids[x] = 7                         # the document's best by nomination is a decoy: X must come back for it
        cp.ix.set_documents(ids)
        r, _, d = cp.check(ids, k, 1, arrangement)
        assert r[k - 1] == x and not np.isin(decoys, r).any()
        if arrangement == "decoys_in_x_document":
            r, _, _ = cp.check(ids, k + 5, 3, arrangement)   # X, then the document's next two by exact score
            best = decoys[G.result_order(cp.e[decoys], decoys)][:2]
            assert r[k - 1] == x and r[k] == best[0] and r[k + 1] == best[1]
        else:
            plain_r, _ = cp.ix.search_topk(cp.q, k)
            assert np.array_equal(r, plain_r[0])
    finally:
        cp.close()


def test_document_ids_at_the_edges_and_ids_that_collide(corpus_of):
    cp = corpus_of(8, "f32", 4097)
    n = 4097
    r = np.arange(n)
    for name, ids in (("0_2^31_fffffffe", np.array([0, 1 << 31, 0xFFFFFFFE], np.uint32)[r % 3]),
                      ("differ_above_bit_20", ((r % 1000).astype(np.uint32) << 20) | 5),
                      ("differ_in_the_low_4_bits", (r % 16).astype(np.uint32) | 0xABCD0000),
                      ("consecutive", (r % 3000).astype(np.uint32))):
        cp.ix.set_documents(ids)
        for k, m in ((10, 1), (100, 2), (100, 8)):
            cp.check(ids, k, m, name)


def test_fewer_groups_than_k(corpus_of):
    cp = corpus_of(8, "f32", 4096)
    ids = (np.arange(4096) % 7).astype(np.uint32)
    cp.ix.set_documents(ids)
    for k, m in ((100, 1), (100, 3), (10, 1)):
        r, _, _ = cp.check(ids, k, m, "7_documents")
        assert r.size == min(k, 7 * m)


def test_a_nan_row_needed_to_fill_k_takes_the_exact_form(rlr, oracle):
    rows = oracle.synth_rows(40, 8, seed=5)
    rows[17, 3] = np.nan
    cp = Corpus(rlr, oracle, 8, "f32", 40, seed=6, rows=rows)
    try:
        ids = np.arange(40, dtype=np.uint32)
        cp.ix.set_documents(ids)
        r, c, _ = cp.check(ids, 40, 1, "nan_needed", form=2)
        assert r[-1] == 17 and np.isnan(c[-1]) and r.size == 40
        cp.check(ids, 10, 1, "nan_not_needed", form=0)       # the NaN row orders last: ten numbers answer
    finally:
        cp.close()


def test_five_thousand_identical_rows(rlr, oracle):
    rows = np.tile(oracle.synth_rows(1, 8, seed=9), (5000, 1))
    cp = Corpus(rlr, oracle, 8, "f32", 5000, seed=10, rows=rows)
    try:
        ids = np.arange(5000, dtype=np.uint32)
        cp.ix.set_documents(ids)
        r, _, _ = cp.check(ids, 10, 1, "identical", form=(0, 1))
        assert r.tolist() == list(range(10))
    finally:
        cp.close()


def test_argument_rules(rlr, oracle, corpus_of):
    cp = corpus_of(8, "f32", 65)
    other = corpus_of(8, "f32", 64)
    for bad in (0, 9):
        with pytest.raises(rlr.RlrError) as ei:
            cp.ix.search_topk_grouped(cp.q, 5, bad)
        assert ei.value.status == -1
    with pytest.raises(rlr.RlrError) as ei:
        cp.ix.search_topk_grouped(cp.q, 0, 1)
    assert ei.value.status == -1
    with other.ix.filter_rows([1, 2, 3]) as f, pytest.raises(rlr.RlrError) as ei:
        cp.ix.search_topk_grouped(cp.q, 5, 1, filter=f)      # another index's filter
    assert ei.value.status == -1
    ix = rlr.GpuIndex(8)
    try:
        ix.upload(cp.rows)
        with ix.filter_rows([1, 2, 3]) as f:
            assert ix.search_topk_grouped(cp.q, 5, 1, filter=f)[0][0].size == 3
            ix.append(cp.rows[:2])
            with pytest.raises(rlr.RlrError) as ei:
                ix.search_topk_grouped(cp.q, 5, 1, filter=f)  # stale
            assert ei.value.status == -1
    finally:
        ix.close()


def test_append_and_delete_documents(rlr, oracle):
    rows = oracle.synth_rows(900, 8, seed=21)
    cp = Corpus(rlr, oracle, 8, "f32", 900, seed=22, rows=rows)
    try:
        ids = (np.arange(900) // 90).astype(np.uint32)
        cp.ix.set_documents(ids)
        extra = np.tile(cp.q, (6, 1)) * np.float32(0.999)    # six rows at the top of every ranking, in no document
        cp.ix.append(extra)
        cp.rows = np.concatenate([rows, extra])
        cp.rescan()
        ids = np.concatenate([ids, np.full(6, G.DOC_NONE, np.uint32)])
        assert np.array_equal(cp.ix.get_documents(), ids)
        r, _, d = cp.check(ids, 10, 1, "appended")
        assert set(range(900, 906)) <= set(r.tolist()) and (d[:6] == G.DOC_NONE).all()
        dead = cp.ix.delete_documents([3, 4])
        keep = np.setdiff1d(np.arange(906), dead.astype(np.int64))
        cp.rows, ids = cp.rows[keep], ids[keep]
        cp.rescan()
        assert np.array_equal(cp.ix.get_documents(), ids)
        for k, m in ((10, 1), (100, 2), (100, 8)):
            cp.check(ids, k, m, "after_delete_documents")
    finally:
        cp.close()


def test_four_threads_return_what_the_serial_calls_return(rlr, oracle, corpus_of):
    cp = corpus_of(8, "f32", 20000)
    ids = V.random_1000(20000)
    cp.ix.set_documents(ids)
    qs = [_query(oracle, 8, 900 + i) for i in range(4)]
    serial = [cp.ix.search_topk_grouped(q, 100, 2)[0] for q in qs]
    got, errors = [None] * 4, []

    def work(i):
        try:
            for _ in range(20):
                got[i] = cp.ix.search_topk_grouped(qs[i], 100, 2)[0]
                if not all(np.array_equal(a, b) for a, b in zip(got[i], serial[i])):
                    errors.append(i)
        except Exception as e:                               # noqa: BLE001 (reported below)
            errors.append(e)

    cp.ix.grouped_forms(reset=True)
    threads = [threading.Thread(target=work, args=(i,)) for i in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    assert cp.ix.grouped_forms() == [80, 0, 0, 0]
    for i in range(4):
        want = G.expect(oracle.scan(cp.rows, qs[i]), ids, 100, 2)
        assert np.array_equal(serial[i][0], want)


# ---- the engine -------------------------------------------------------------------------------------------------------
def _engine_model(eng, O, q_raw, k, m, names=None):
    rows = eng.index.fetch_rows(np.arange(len(eng)))
    e = O.scan(rows, O.normalize(q_raw))
    ids = eng.index.get_documents()
    allowed = None if names is None else np.asarray([r for r, ch in enumerate(eng._chunks) if ch.document_name in names], np.int64)
    want = G.expect(e, ids, k, m, allowed)
    return [(eng._chunks[int(r)].document_name, int(r), e[int(r)]) for r in want]


def _engine_check(eng, O, q_raw, names=None):
    for k, m in ((3, 1), (10, 2), (10, 8)):
        want = _engine_model(eng, O, q_raw, k, m, names)
        got = eng.search_per_document(q_raw, k, m, documents=names)
        assert [(g.document, g.row) for g in got] == [(w[0], w[1]) for w in want], (k, m, names)
        for g, w in zip(got, want):
            assert bits(np.float32(g.score)) == bits(w[2]) and g.score == g.embedding_score == g.initial_score
            assert g.lexical_score == 0.0
    want = _engine_model(eng, O, q_raw, 10, 1, names)
    ranked = eng.rank_documents(q_raw, 10, documents=names)
    assert [(name, res.row) for name, res in ranked] == [(w[0], w[1]) for w in want]
    assert len({name for name, _ in ranked}) == len(ranked)


def test_engine_rank_documents_and_search_per_document(rlr, oracle):
    rng = np.random.default_rng(31)
    eng = rlr.RagEngine(8)
    try:
        sizes = {"a.pdf": 40, "b.pdf": 7, "c.pdf": 1, "d.pdf": 25}
        for name, n in sizes.items():
            eng.add_document(name, [f"{name} {i}" for i in range(n)], rng.standard_normal((n, 8)).astype(np.float32))
        q_raw = (3.0 * rng.standard_normal(8)).astype(np.float32)   # not unit norm: the engine normalises it
        eng.index.grouped_forms(reset=True)
        _engine_check(eng, oracle, q_raw)
        assert len(eng.rank_documents(q_raw, 10)) == 4
        _engine_check(eng, oracle, q_raw, ["a.pdf", "c.pdf"])
        _engine_check(eng, oracle, q_raw, ["nothing.pdf"])
        eng.remove_document("a.pdf")
        _engine_check(eng, oracle, q_raw)
        eng.add_document("a.pdf", [f"again {i}" for i in range(12)], rng.standard_normal((12, 8)).astype(np.float32))
        _engine_check(eng, oracle, q_raw)
        _engine_check(eng, oracle, q_raw, ["a.pdf", "d.pdf"])
        forms = eng.index.grouped_forms()
        assert forms[0] > 0 and forms[1] == forms[2] == 0       # (scoped calls over a few rows take the list path: form 3)
    finally:
        eng.close()
