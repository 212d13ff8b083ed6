"""Queries with a filter EACH (rlr_search_topk_scoped): chunks of up to 8 queries share ONE masked pass that reads the
union of their scopes once (scan_masked_scopes_kernel, then the batched select and finish of the one-filter pass); every
query that cannot join -- a list-path filter, fewer allowed rows than k, binary16 rows, other widths -- runs alone inside
its own filter.  Whatever the route, query q's result is the single-query filtered search of query q inside filters[q]:
the oracle's scan of the stored rows reduced to q's OWN scope, ordered (score desc, NaN last, row asc), cut to
min(k, rows of the scope) -- rows and score bits exact.

The indexes are created with RLR_BATCH_MIN=2 (read at creation) and the filters forced onto the masked scan, so that
corpora of a few thousand rows reach the shared pass."""
import threading

import numpy as np
import pytest

from conftest import bits
from test_gpu_filter_batch import batch_index, canon, document_ranges, expected, masks_of, model_hand_backs

pytestmark = pytest.mark.gpu

COUNTS = [2, 3, 5, 8, 9, 17]
NQ = max(COUNTS)


def scope_sets(n):
    """name -> list of ascending row arrays: the scopes one chunk of queries is spread over (query i takes scope i mod len)"""
    m = masks_of(n)
    every = np.arange(n)
    word = every // 64
    docs = [np.arange(a, a + c) for a, c in document_ranges(n)]
    return {
        "halves": [every[:n // 2], every[n // 2:]],
        "eighths": [every[i * n // 8:(i + 1) * n // 8] for i in range(8)],
        "nested": [m["all"], m["every_other"], m["one_per_word"]],
        "complement_every_other": [m["every_other"], m["not_every_other"]],
        "complement_one_per_word": [m["one_per_word"], m["not_one_per_word"]],
        "no_shared_word": [every[(word % 2 == 0) & (every % 3 == 0)], every[(word % 2 == 1) & (every % 5 != 0)]],
        "single_bits_beside_all": [m["bit63"], m["all"], m["first"], m["last"]],
        "partial_last_word": [m["last_partial_word"], every[:min(n, 640):2]],
        "one_empty": [m["every_other"], m["not_all"], m["not_every_other"]],
        "documents": docs + [np.unique(np.concatenate(docs))],
    }


def make_filters(ix, scopes):
    fs = [ix.filter_rows(rows) for rows in scopes]
    for f, rows in zip(fs, scopes):
        assert f.info()["n_allowed"] == len(rows)
        f.set_path("scan")
    return fs


def check_scoped(ix, fs, scopes, qs, e_all, k, ctx):
    """one call with the queries qs (e_all[i] = the oracle's scan for qs[i]), query i inside fs[i] / scopes[i]: every
    query held to the oracle reduced to ITS scope"""
    res = ix.search_topk_scoped(qs, k, fs)
    assert len(res) == len(qs), ctx
    for i, (r, c) in enumerate(res):
        wr, wc = expected(e_all[i], scopes[i], k)
        assert len(r) == len(wr) == min(k, len(scopes[i])), (ctx, i, len(r), len(wr))
        assert np.array_equal(r, wr), (ctx, i, r[:8], wr[:8])
        assert np.array_equal(canon(c), canon(wc)), (ctx, i)


def check_unfiltered(ix, q, e_full, ctx):
    ur, uc = ix.search_topk(q, 10)
    xr, xc = expected(e_full, np.arange(len(e_full)), 10)
    assert np.array_equal(ur[0], xr) and np.array_equal(canon(uc[0]), canon(xc)), (ctx, "unfiltered after")


def make_corpus(rlr, oracle, n, dim, dtype="f32", seed=None, nq=NQ):
    rows = oracle.synth_rows(n, dim, seed=(1900 + dim) if seed is None else seed, n_clusters=7)
    ix = batch_index(rlr, dim, dtype)
    ix.upload(rows)
    stored = ix.fetch_rows(np.arange(n))
    qs = np.stack([oracle.normalize(oracle.synth_query(dim, seed=2000 + dim + i)) for i in range(nq)]).astype(np.float32)
    e_all = np.stack([oracle.scan(stored, q) for q in qs])   # the one reference: shared by every scope, never changed
    e_all.setflags(write=False)
    return ix, stored, qs, e_all


@pytest.fixture(scope="module", params=[(2397, 256), (2397, 512), (2397, 768), (2397, 1024), (64, 768)],
                ids=lambda p: f"{p[0]}x{p[1]}f32")
def corpus(request, rlr, oracle):
    n, dim = request.param
    ix, stored, qs, e_all = make_corpus(rlr, oracle, n, dim)
    yield ix, n, qs, e_all
    ix.close()


def test_every_scope_set_query_count_and_k(corpus):
    """every scope set with every query count (2, 3, 5, 8, 9, 17) and k = 1, 10, 100, one k above the smallest scope of the
    set (ragged n_out: that query runs alone and is still exact) and one above every scope"""
    ix, n, qs, e_all = corpus
    for name, scopes in scope_sets(n).items():
        fs = make_filters(ix, scopes)
        try:
            sizes = sorted(len(s) for s in scopes)
            ks = sorted({1, 10, 100, sizes[0] + 1, sizes[-1] + 5})
            for k in ks:
                for m in COUNTS:
                    pick = [i % len(scopes) for i in range(m)]
                    check_scoped(ix, [fs[j] for j in pick], [scopes[j] for j in pick], qs[:m], e_all, k, (name, k, m))
            check_unfiltered(ix, qs[0], e_all[0], name)
        finally:
            for f in fs:
                f.close()


def test_identical_filter_objects(corpus):
    """the same filter OBJECT in every slot (and the same rows in two objects): the result of the one-filter call"""
    ix, n, qs, e_all = corpus
    rows = np.arange(n)[::2]
    fs = make_filters(ix, [rows, rows])
    try:
        for m in (2, 8, 9):
            for k in (1, 10):
                check_scoped(ix, [fs[0]] * m, [rows] * m, qs[:m], e_all, k, ("same object", m, k))
                check_scoped(ix, [fs[i % 2] for i in range(m)], [rows] * m, qs[:m], e_all, k, ("same rows", m, k))
                one_r, one_c = ix.search_topk(qs[:m], k, filter=fs[0])
                for i, (r, c) in enumerate(ix.search_topk_scoped(qs[:m], k, [fs[0]] * m)):
                    assert np.array_equal(r, one_r[i]) and np.array_equal(bits(c), bits(one_c[i])), (m, k, i)
    finally:
        for f in fs:
            f.close()


def test_one_filter_object_in_every_slot_is_the_one_filter_pass(rlr, oracle):
    """eight queries over ONE filter object through rlr_search_topk_scoped and the same eight through
    rlr_search_topk_filtered (4096 x 256 f32, k = 5, the pass forced): the two entries meet in the same shared pass --
    equal rows, cosine bits and profile deltas (one pass of eight queries, nothing handed back, no single scan, the
    filter's rows read once)"""
    n, dim, k, m = 4096, 256, 5, 8
    ix, stored, qs, e_all = make_corpus(rlr, oracle, n, dim, seed=4096, nq=m)
    ix.profile_enable(True)
    rows = np.arange(n)[::3]
    f, = make_filters(ix, [rows])
    try:
        ix.profile_read(reset=True)
        scoped = ix.search_topk_scoped(qs, k, [f] * m)
        ps = ix.profile_read(reset=True)
        one_r, one_c = ix.search_topk(qs, k, filter=f)
        pf = ix.profile_read(reset=True)
        for i, (r, c) in enumerate(scoped):
            assert np.array_equal(r, one_r[i]) and np.array_equal(bits(c), bits(one_c[i])), i
        counters = ("n_batches", "n_batch_queries", "n_batch_fallbacks", "n_searches", "n_scan_launches", "n_candidates",
                    "n_retries", "scan_bytes")
        assert [getattr(ps, c) for c in counters] == [getattr(pf, c) for c in counters], (ps, pf)
        assert ps.n_batches == 1 and ps.n_batch_queries == m and ps.n_batch_fallbacks == 0 and ps.n_searches == m, ps
        assert ps.n_scan_launches == 0 and ps.scan_bytes == len(rows) * dim * 4, ps
    finally:
        f.close()
        ix.close()


@pytest.fixture(scope="module")
def corpus768(rlr, oracle):
    ix, stored, qs, e_all = make_corpus(rlr, oracle, 2397, 768)
    ix.profile_enable(True)
    yield ix, stored, qs, e_all
    ix.close()


COUNTER_SETS = ["halves", "eighths", "nested", "complement_every_other", "no_shared_word", "documents"]


@pytest.mark.parametrize("name", COUNTER_SETS)
def test_the_shared_pass_ran_and_read_the_union_once(corpus768, name):
    """an eligible chunk of m queries is ONE pass: n_batches 1, n_batch_queries m, no single scan, as many hand-backs as
    the CPU model of the pass predicts for each query inside its own scope (none: the designs are far from every
    capacity), and scan_bytes grows by the rows of the UNION -- two disjoint halves are the matrix once, not twice"""
    ix, stored, qs, e_all = corpus768
    n, dim, k = len(stored), 768, 3
    scopes = scope_sets(n)[name]
    assert min(len(s) for s in scopes) >= k
    eps = (dim + 64) * 2.0 ** -24 * 1.0625
    fs = make_filters(ix, scopes)
    try:
        for m in (2, 3, 5, 8):
            pick = [i % len(scopes) for i in range(m)]
            predicted = 0
            for i, j in enumerate(pick):   # the CPU model first, every query with its own scope
                (n_cand, band), = model_hand_backs(stored, qs[i:i + 1], scopes[j], k, eps)
                predicted += int(not (k <= n_cand <= 4096 and band <= 1024))
            assert predicted == 0, (name, m)
            union = np.unique(np.concatenate([scopes[j] for j in pick]))
            ix.profile_read(reset=True)
            check_scoped(ix, [fs[j] for j in pick], [scopes[j] for j in pick], qs[:m], e_all, k, (name, m))
            p = ix.profile_read(reset=True)
            assert p.n_batches == 1 and p.n_batch_queries == m and p.n_batch_fallbacks == predicted, (name, m, p)
            assert p.n_scan_launches == 0 and p.n_searches == m, (name, m, p)
            assert p.scan_bytes == len(union) * dim * 4, (name, m, p.scan_bytes, len(union))
            if name == "halves":
                assert p.scan_bytes == n * dim * 4
        # 17 queries: two passes of 8 and one query alone
        pick = [i % len(scopes) for i in range(17)]
        ix.profile_read(reset=True)
        check_scoped(ix, [fs[j] for j in pick], [scopes[j] for j in pick], qs, e_all, k, (name, 17))
        p = ix.profile_read(reset=True)
        assert p.n_batches == 2 and p.n_batch_queries == 16 and p.n_batch_fallbacks == 0 and p.n_scan_launches == 1, p
        assert p.n_searches == 17, p
    finally:
        for f in fs:
            f.close()


def test_a_query_copy_outside_the_querys_own_scope_never_appears(rlr, oracle):
    """rows that ARE the query: a copy of query i lies inside scope A (rows below 1200) and another inside scope B (the
    rest).  Query i runs under one scope beside queries under the other: the pass loads the copy in the other scope --
    it is in the union -- and scores it 1.0 for query i, and it must never enter query i's result."""
    n, dim = 2397, 768
    rows = oracle.synth_rows(n, dim, seed=31, n_clusters=5)
    qs = np.stack([oracle.normalize(oracle.synth_query(dim, seed=3200 + i)) for i in range(8)]).astype(np.float32)
    copy_a = [100 + 64 * i for i in range(8)]
    copy_b = [1901 + 3 * i for i in range(8)]
    for i in range(8):
        rows[copy_a[i]] = qs[i]
        rows[copy_b[i]] = qs[i]
    ix = batch_index(rlr, dim)
    try:
        ix.upload(rows)                                  # stored as given: both rows ARE the query
        e_all = np.stack([oracle.scan(rows, q) for q in qs])
        scopes = [np.arange(0, 1200), np.arange(1200, n)]
        fs = make_filters(ix, scopes)
        ix.profile_enable(True)
        for flip in (0, 1):
            pick = [(i + flip) % 2 for i in range(8)]
            for k in (1, 10, 1000):
                ix.profile_read(reset=True)
                res = ix.search_topk_scoped(qs, k, [fs[j] for j in pick])
                p = ix.profile_read()
                assert p.n_batches == 1 and p.n_batch_queries == 8, (flip, k, p)
                for i, (r, c) in enumerate(res):
                    wr, wc = expected(e_all[i], scopes[pick[i]], k)
                    assert np.array_equal(r, wr) and np.array_equal(bits(c), bits(wc)), (flip, k, i)
                    own, other = (copy_a, copy_b) if pick[i] == 0 else (copy_b, copy_a)
                    assert r[0] == own[i] and not (set(other) & set(r.tolist())), (flip, k, i)
        for f in fs:
            f.close()
    finally:
        ix.close()


def test_mixed_routes_in_one_call(corpus768):
    """among four queries that share a pass: one whose filter was left on the list path and one whose filter holds fewer
    rows than k.  All are exact; only the four count in n_batch_queries, the other two run alone."""
    ix, stored, qs, e_all = corpus768
    n, k = len(stored), 10
    scopes = [np.arange(n)[::2], np.sort(np.random.default_rng(8).permutation(n)[:300]), np.arange(n)[1::3],
              np.array([5, 70, 71, 900, 2396])]
    fs = [ix.filter_rows(s) for s in scopes]
    try:
        assert fs[1].info()["path"] == "list"
        for j in (0, 2, 3):
            fs[j].set_path("scan")
        pick = [0, 1, 2, 3, 0, 2]
        ix.profile_read(reset=True)
        check_scoped(ix, [fs[j] for j in pick], [scopes[j] for j in pick], qs[:6], e_all, k, "mixed")
        p = ix.profile_read(reset=True)
        assert p.n_batches == 1 and p.n_batch_queries == 4 and p.n_batch_fallbacks == 0, p
        assert p.n_searches == 6 and p.n_scan_launches == 1, p      # (the 5-row filter's masked scan; the list path scans nothing)
        check_unfiltered(ix, qs[0], e_all[0], "mixed")
    finally:
        for f in fs:
            f.close()


@pytest.mark.parametrize("dim,dtype", [(1024, "f16"), (100, "f32")])
def test_unsupported_shapes_run_one_by_one(rlr, oracle, dim, dtype):
    n = 2397
    ix, stored, qs, e_all = make_corpus(rlr, oracle, n, dim, dtype, seed=61 + dim, nq=4)
    try:
        scopes = [np.arange(n)[1::2], np.arange(n)[:1200]]
        fs = make_filters(ix, scopes)
        ix.profile_enable(True)
        ix.profile_read(reset=True)
        pick = [0, 1, 0, 1]
        check_scoped(ix, [fs[j] for j in pick], [scopes[j] for j in pick], qs, e_all, 10, (dim, dtype))
        p = ix.profile_read()
        assert p.n_batches == 0 and p.n_scan_launches == 4, p
        for f in fs:
            f.close()
    finally:
        ix.close()


def test_invalid_filters_are_refused_before_any_gpu_work(rlr, oracle):
    n, dim = 300, 256
    rows = oracle.synth_rows(n + 40, dim, seed=61)
    qs = np.stack([oracle.normalize(oracle.synth_query(dim, seed=6300 + i)) for i in range(4)]).astype(np.float32)
    ix, other = batch_index(rlr, dim), batch_index(rlr, dim)
    try:
        ix.upload(rows[:n])
        other.upload(rows[:n])
        good = [ix.filter_ranges([(10, 50)]), ix.filter_ranges([(100, 80)])]
        for f in good:
            f.set_path("scan")
        res = ix.search_topk_scoped(qs, 5, [good[0], good[1], good[0], good[1]])
        assert [len(r) for r, _ in res] == [5, 5, 5, 5]
        before = ix.profile_read().n_searches
        with other.filter_rows([0, 5]) as foreign:                 # a filter of another index, in slot 2
            with pytest.raises(rlr.RlrError) as ei:
                ix.search_topk_scoped(qs, 2, [good[0], good[1], foreign, good[0]])
            assert ei.value.status == -1 and "another index" in str(ei.value)
        with pytest.raises(rlr.RlrError) as ei:                    # a null entry, in slot 3
            ix.search_topk_scoped(qs, 2, [good[0], good[1], good[0], None])
        assert ei.value.status == -1
        with ix.filter_ranges([(5, 0)]) as empty:                  # no row allowed: no result, RLR_OK
            res = ix.search_topk_scoped(qs[:3], 10, [good[0], empty, good[1]])
            assert [len(r) for r, _ in res] == [10, 0, 10]
        assert ix.profile_read().n_searches == before + 2
        before = ix.profile_read().n_searches
        ix.append(rows[n:])
        fresh = ix.filter_ranges([(10, 50)])
        fresh.set_path("scan")
        for j in range(3):                                         # a stale filter in slot j
            fs = [fresh, fresh, fresh]
            fs[j] = good[1]
            with pytest.raises(rlr.RlrError) as ei:
                ix.search_topk_scoped(qs[:3], 5, fs)
            assert ei.value.status == -1 and "stale" in str(ei.value), j
        assert ix.profile_read().n_searches == before              # nothing ran
        for f in good + [fresh]:
            f.close()
    finally:
        ix.close()
        other.close()


def test_concurrent_scoped_calls_with_different_filter_sets(rlr, oracle):
    """two threads, 8-query scoped calls with different filter sets: every result is the oracle's, and an unfiltered
    search on the same index afterwards is exact"""
    n, dim = 2397, 512
    ix, stored, qs, e_all = make_corpus(rlr, oracle, n, dim, seed=71, nq=16)
    try:
        scopes = [np.arange(n)[::2], np.arange(100, 1300), np.arange(n)[1::2], np.arange(1200, n), np.arange(7, 307)]
        fs = make_filters(ix, scopes[:4]) + [ix.filter_rows(scopes[4])]   # (the last one stays on the list path)
        sets = [[0, 1, 0, 1, 2, 2, 1, 0], [2, 3, 4, 3, 2, 4, 3, 3]]
        want = {(t, h): [expected(e_all[h * 8 + i], scopes[sets[t][i]], 25) for i in range(8)] for t in range(2) for h in range(2)}
        errors = []

        def worker(t):
            try:
                for it in range(12):
                    h = (t + it // 3) % 2
                    res = ix.search_topk_scoped(qs[h * 8:h * 8 + 8], 25, [fs[j] for j in sets[t]])
                    for i, (r, c) in enumerate(res):
                        wr, wc = want[(t, h)][i]
                        if not (np.array_equal(r, wr) and np.array_equal(canon(c), canon(wc))):
                            errors.append((t, it, i))
            except Exception as e:  # noqa: BLE001 -- reported below
                errors.append((t, repr(e)))

        ts = [threading.Thread(target=worker, args=(t,)) for t in range(2)]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        assert not errors, errors[:5]
        check_unfiltered(ix, qs[0], e_all[0], "concurrent")
        for f in fs:
            f.close()
    finally:
        ix.close()
