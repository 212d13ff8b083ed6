"""Several queries inside one row filter (rlr_search_topk_filtered with n_queries >= 2): chunks of up to 8 queries share
ONE masked pass over f32 rows of 256 / 512 / 768 / 1024 elements (scan_masked_multi_kernel, then the batched select and
finish); runs of queries on the list path share one synchronisation; every other shape runs query by query.  Whatever
the route, query q's result is the single-query filtered search of query q: the oracle's scan of the stored rows reduced
to the allowed rows, ordered (score desc, NaN last, row asc), cut to min(k, allowed rows) -- rows and score bits exact.

The indexes are created with RLR_BATCH_MIN=2 (read at creation) and the filters forced onto the masked scan, so that
corpora of a few thousand rows reach the shared pass; one test leaves both alone (the natural gate)."""
import threading

import numpy as np
import pytest

from conftest import bits

pytestmark = pytest.mark.gpu

COUNTS = [2, 3, 5, 8, 9, 17]
NQ = max(COUNTS)


def canon(a):
    """score bits with every NaN as one pattern (a NaN's payload is not part of the contract)"""
    b = bits(a).copy()
    b[np.isnan(np.ascontiguousarray(a, dtype=np.float32))] = 0x7FC00000
    return b


def expected(e_full, allowed, k):
    """allowed: ascending rows; -> (rows, scores) of the sub-corpus search mapped back to index rows"""
    allowed = np.asarray(allowed, dtype=np.uint64)
    e = e_full[allowed.astype(np.int64)]
    nan = np.isnan(e)
    order = np.lexsort((np.arange(len(e)), np.where(nan, 0.0, -e.astype(np.float64)), nan))[:k]
    return allowed[order], e[order]


def masks_of(n):
    """name -> ascending allowed rows: the masks of test_gpu_filter.py, then the complement of each"""
    every = np.arange(n)
    m = {
        "all": every,
        "first": every[:1],
        "last": every[-1:],
        "bit63": every[63:64],
        "one_per_word": np.array([w * 64 + (w * 7) % 64 for w in range((n + 63) // 64) if w * 64 + (w * 7) % 64 < n]),
        "every_other": every[::2],
        "last_partial_word": every[(n - 1) // 64 * 64:],
    }
    out = dict(m)
    for name, rows in m.items():
        keep = np.ones(n, bool)
        keep[rows] = False
        out["not_" + name] = every[keep]
    return out


def document_ranges(n):
    """three contiguous "documents" (the middle one starts inside a word and crosses into the next two)"""
    return [(3, max(1, n // 10)), (n // 3, min(65, n - n // 3 - 1)), (n - max(1, n // 7), max(1, n // 7))]


def rows_of_ranges(ranges):
    return np.unique(np.concatenate([np.arange(a, a + c) for a, c in ranges]))


def batch_index(rlr, dim, dtype="f32", batch_min="2"):
    """an index whose batch threshold is `batch_min` queries (None: the cost model)"""
    mp = pytest.MonkeyPatch()
    try:
        if batch_min is None:
            mp.delenv("RLR_BATCH_MIN", raising=False)
        else:
            mp.setenv("RLR_BATCH_MIN", batch_min)
        return rlr.GpuIndex(dim, dtype)
    finally:
        mp.undo()


def check_queries(ix, f, qs, e_all, allowed, k, ctx):
    """one call with the queries qs (e_all[i] = the oracle's scan for qs[i]); every query held to the oracle"""
    r, c = ix.search_topk(qs, k, filter=f)
    for i in range(len(qs)):
        wr, wc = expected(e_all[i], allowed, k)
        assert r.shape == (len(qs), len(wr)), (ctx, r.shape, len(wr))
        assert np.array_equal(r[i], wr), (ctx, i, r[i][:8], wr[:8])
        assert np.array_equal(canon(c[i]), canon(wc)), (ctx, i)


def check_unfiltered(ix, q, e_full, ctx):
    """hygiene: an unfiltered search on the same index finds its histograms, scores and counters as it expects them"""
    ur, uc = ix.search_topk(q, 10)
    xr, xc = expected(e_full, np.arange(len(e_full)), 10)
    assert np.array_equal(ur[0], xr) and np.array_equal(canon(uc[0]), canon(xc)), (ctx, "unfiltered after")


@pytest.fixture(scope="module", params=[(2397, 256), (2397, 512), (2397, 768), (2397, 1024), (64, 768)],
                ids=lambda p: f"{p[0]}x{p[1]}f32")
def corpus(request, rlr, oracle):
    n, dim = request.param
    rows = oracle.synth_rows(n, dim, seed=1900 + dim, n_clusters=7)
    ix = batch_index(rlr, dim)
    ix.upload(rows)
    stored = ix.fetch_rows(np.arange(n))
    qs = np.stack([oracle.normalize(oracle.synth_query(dim, seed=2000 + dim + i)) for i in range(NQ)]).astype(np.float32)
    e_all = np.stack([oracle.scan(stored, q) for q in qs])   # the one reference: shared by every mask, never changed
    e_all.setflags(write=False)
    yield ix, n, qs, e_all
    ix.close()


def test_every_mask_query_count_and_k(corpus):
    """every mask and the three-document ranges with every k and every query count (2, 3, 5, 8, 9 and 17)"""
    ix, n, qs, e_all = corpus
    cases = list(masks_of(n).items()) + [("documents", rows_of_ranges(document_ranges(n)))]
    for name, allowed in cases:
        with (ix.filter_ranges(document_ranges(n)) if name == "documents" else ix.filter_rows(allowed)) as f:
            assert f.info()["n_allowed"] == len(allowed)
            f.set_path("scan")
            for k in (1, 10, 100, len(allowed), len(allowed) + 5):
                if k == 0:
                    r, c = ix.search_topk(qs[:3], 5, filter=f)          # (not_all: no row allowed)
                    assert r.shape == (3, 0)
                    continue
                for m in COUNTS:
                    check_queries(ix, f, qs[:m], e_all, allowed, k, (name, k, m))
                    check_unfiltered(ix, qs[0], e_all[0], (name, k, m))


def model_hand_backs(stored, qs, allowed, k, eps):
    """the CPU model of the shared pass for unit rows without ties or NaN: per query, (candidates at or above the k-th
    nominated score's floor - 2 eps, rows in the band of 2 eps under the k-th nominated score).  The finish hands a query
    back when the first exceeds 8192 or falls below k, or the second exceeds 2048.  The select's floor lies at most one
    2^-13 step of the score's binade under the k-th score."""
    out = []
    for q in qs:
        nom = (stored[allowed].astype(np.float32) @ q.astype(np.float32)).astype(np.float64)
        kth = np.sort(nom)[::-1][k - 1]
        floor = kth - 2.0 ** (np.floor(np.log2(abs(kth))) - 12) - 2 * eps - eps
        out.append((int((nom >= floor).sum()), int((nom >= kth - 3 * eps).sum())))
    return out


def test_the_shared_pass_ran(rlr, oracle):
    """2397 x 768, every other row allowed: 8 queries are one shared pass and no single scan; 17 are two passes of 8 and one
    single-query masked scan"""
    n, dim, k = 2397, 768, 10
    rows = oracle.synth_rows(n, dim, seed=1900 + dim, n_clusters=7)
    ix = batch_index(rlr, dim)
    try:
        ix.upload(rows)
        stored = ix.fetch_rows(np.arange(n))
        qs = np.stack([oracle.normalize(oracle.synth_query(dim, seed=2000 + dim + i)) for i in range(NQ)]).astype(np.float32)
        e_all = np.stack([oracle.scan(stored, q) for q in qs])
        allowed = np.arange(n)[::2]
        # the CPU model first: no query of this corpus can be handed back (far from every capacity)
        eps = (dim + 64) * 2.0 ** -24 * 1.0625
        for n_cand, band in model_hand_backs(stored, qs, allowed, k, eps):
            assert k <= n_cand <= 4096 and band <= 1024, (n_cand, band)
        ix.profile_enable(True)
        with ix.filter_rows(allowed) as f:
            f.set_path("scan")
            ix.profile_read(reset=True)
            check_queries(ix, f, qs[:8], e_all, allowed, k, "8 queries")
            p = ix.profile_read(reset=True)
            assert p.n_batches == 1 and p.n_batch_queries == 8 and p.n_batch_fallbacks == 0 and p.n_scan_launches == 0, p
            assert p.n_searches == 8 and p.scan_bytes == len(allowed) * dim * 4, p
            check_queries(ix, f, qs, e_all, allowed, k, "17 queries")
            p = ix.profile_read(reset=True)
            assert p.n_batches == 2 and p.n_batch_queries == 16 and p.n_batch_fallbacks == 0 and p.n_scan_launches == 1, p
            assert p.n_searches == 17, p
    finally:
        ix.close()


def test_natural_gate_and_rows_past_131072(rlr, oracle):
    """no env override, no forced path: 140 000 x 256 with every third row allowed (46 667 >= 8192: the masked scan) and 8
    queries is a shared pass by the cost model.  Row 135 000 -- allowed, past the first 131 072 rows -- is a copy of query
    5: the winner of that slot and of no other."""
    n, dim, k = 140000, 256, 10
    rows = oracle.synth_rows(n, dim, seed=77, n_clusters=9)
    qs = np.stack([oracle.normalize(oracle.synth_query(dim, seed=7800 + i)) for i in range(8)]).astype(np.float32)
    winner = 135000
    rows[winner] = qs[5]
    ix = batch_index(rlr, dim, batch_min=None)
    try:
        ix.upload(rows)
        stored = ix.fetch_rows(np.arange(n))
        e_all = np.stack([oracle.scan(stored, q) for q in qs])
        allowed = np.arange(n)[::3]
        assert winner in allowed
        ix.profile_enable(True)
        with ix.filter_rows(allowed) as f:
            assert f.info()["path"] == "scan"
            ix.profile_read(reset=True)
            r, c = ix.search_topk(qs, k, filter=f)
            p = ix.profile_read()
            for i in range(8):
                wr, wc = expected(e_all[i], allowed, k)
                assert np.array_equal(r[i], wr) and np.array_equal(bits(c[i]), bits(wc)), i
                assert (r[i][0] == winner) == (i == 5), (i, r[i][:3])
            assert p.n_batches == 1 and p.n_batch_queries == 8 and p.n_batch_fallbacks == 0 and p.n_scan_launches == 0, p
        check_unfiltered(ix, qs[0], e_all[0], "natural gate")
    finally:
        ix.close()


@pytest.mark.parametrize("name,share", [("masked_f32_768", 0.5), ("masked_f32_768", 0.03), ("masked_f32_1024", 0.5)])
def test_every_slot_every_residue(rlr, name, share):
    """The ladder corpora of the masked scans (ladder_vectors.masked_sets): checked rows that are the only allowed row of
    their unit on every residue modulo 64, twice, and on the last, partly filled word; a checked row nominated low is
    lost (test_ladder_vectors_cpu.py).  Call s holds ladder queries s .. s + 7 (mod G): every query sits in each of the 8
    slots once.  Calls of 2 and 3 queries run the Q = 2 and Q = 4 instances.  The select behind the shared pass collects
    exactly the ladder: W = 2k candidates per query, reported as their sum per call."""
    import ladder_vectors as L
    from test_gpu_positions import assert_exact, make_index
    rows, qs, f = L.corpus(name)
    allowed = L.ladder_mask(name, share)
    G = len(qs)
    mp = pytest.MonkeyPatch()
    mp.setenv("RLR_BATCH_MIN", "2")
    try:
        ix = make_index(rlr, name)
    finally:
        mp.undo()
    try:
        ix.profile_enable(True)
        with ix.filter_rows(allowed) as flt:
            flt.set_path("scan")
            for s in range(G):
                for m in ([8] if s % 4 else [8, 2, 3]):
                    slots = [(s + i) % G for i in range(m)]
                    ix.profile_read(reset=True)
                    r, c = ix.search_topk(qs[slots], f["k"], filter=flt)
                    p = ix.profile_read()
                    for i, g in enumerate(slots):
                        assert_exact(name, g, r[i], c[i], f"{name} share {share}: call {s} of {m}, slot {i}")
                    assert p.n_batches == 1 and p.n_batch_queries == m and p.n_batch_fallbacks == 0, (s, m, p)
                    assert p.n_scan_launches == 0 and p.n_retries == 0, (s, m, p)
                    assert p.n_candidates == m * f["W"], f"call {s} of {m}: {p.n_candidates} candidates, {m} ladders of {f['W']}"
    finally:
        ix.close()


@pytest.mark.parametrize("n", [2397, 1500])
def test_non_finite_allowed_rows_are_handed_back_exactly(rlr, oracle, n):
    """the construction of test_gpu_filter.py's non-finite test at 256-d: three allowed and three masked rows hold NaN or
    Inf, every fourth row is allowed and k is every allowed row -- the threshold key is 0 and the sentinel keeps no masked
    row out.  2397 rows: all of them are candidates, more than the finish's band takes (status 1).  1500 rows: the band
    holds them, the re-scored masked rows enter the result and the host's mask test finds them.  Either way the query
    goes to the single-query filtered path and the result is the oracle's."""
    dim = 256
    rows = oracle.synth_rows(n, dim, seed=51, n_clusters=3)
    qs = np.stack([oracle.normalize(oracle.synth_query(dim, seed=5200 + i)) for i in range(5)]).astype(np.float32)
    allowed = np.arange(n)[::4]
    rows[12, 3] = np.nan
    rows[700, 0], rows[700, 1] = np.inf, -np.inf
    rows[1200, 7] = np.inf
    rows[13, 3] = np.nan
    rows[701, 0], rows[701, 1] = np.inf, -np.inf
    rows[1201, 7] = -np.inf
    ix = batch_index(rlr, dim)
    try:
        ix.upload(rows, normalize=False)
        e_all = np.stack([oracle.scan(rows, q) for q in qs])
        assert np.isnan(e_all[0][12]) and np.isnan(e_all[0][13])
        with ix.filter_rows(allowed) as f:
            f.set_path("scan")
            for k in (len(allowed), 10, len(allowed) - 2):
                ix.profile_read(reset=True)
                r, c = ix.search_topk(qs, k, filter=f)
                p = ix.profile_read()
                for i in range(len(qs)):
                    wr, wc = expected(e_all[i], allowed, k)
                    assert np.array_equal(r[i], wr), (k, i)
                    assert np.array_equal(canon(c[i]), canon(wc)), (k, i)
                    assert not (set(r[i].tolist()) & {13, 701, 1201}), (k, i)
                assert p.n_batches == 1 and p.n_batch_queries == 5, (k, p)
                if k == len(allowed):
                    assert p.n_batch_fallbacks == 5, (k, p)      # k reaches the NaN rows of every query
                check_unfiltered(ix, qs[0], e_all[0], ("non-finite", k))
    finally:
        ix.close()


def test_tie_flood_is_handed_back_exactly(rlr, oracle):
    """5000 identical allowed rows among 6000 (256-d): every query's guard band holds them all, more than the finish takes;
    the 1000 masked rows are copies of query 0, the best rows of the index"""
    n, dim = 6000, 256
    base = oracle.synth_rows(2, dim, seed=41)
    qs = np.stack([oracle.normalize(oracle.synth_query(dim, seed=4200 + i)) for i in range(3)]).astype(np.float32)
    rows = np.empty((n, dim), np.float32)
    rows[:] = base[0]
    masked = np.arange(n)[5::6]
    rows[masked] = qs[0]
    keep = np.ones(n, bool)
    keep[masked] = False
    allowed = np.arange(n)[keep]
    ix = batch_index(rlr, dim)
    try:
        ix.upload(rows)
        e_all = np.stack([oracle.scan(rows, q) for q in qs])
        with ix.filter_rows(allowed) as f:
            f.set_path("scan")
            ix.profile_read(reset=True)
            r, c = ix.search_topk(qs, 10, filter=f)
            p = ix.profile_read()
            for i in range(3):
                wr, wc = expected(e_all[i], allowed, 10)
                assert list(r[i]) == list(allowed[:10]) == list(wr), i
                assert np.array_equal(bits(c[i]), bits(wc)), i
            assert p.n_batches == 1 and p.n_batch_fallbacks == 3 and p.n_retries >= 3, p
        ur, uc = ix.search_topk(qs[0], 10)
        assert list(ur[0]) == list(masked[:10])
    finally:
        ix.close()


def test_query_copies_in_masked_rows_never_appear(rlr, oracle):
    n, dim = 2397, 768
    rows = oracle.synth_rows(n, dim, seed=31, n_clusters=5)
    qs = np.stack([oracle.normalize(oracle.synth_query(dim, seed=3200 + i)) for i in range(8)]).astype(np.float32)
    masked_copy = [130 + 64 * i for i in range(8)]
    allowed_copy = [1901 + 3 * i for i in range(8)]
    for i in range(8):
        rows[masked_copy[i]] = qs[i]
        rows[allowed_copy[i]] = qs[i]
    ix = batch_index(rlr, dim)
    try:
        ix.upload(rows)                                  # stored as given: both rows ARE the query
        e_all = np.stack([oracle.scan(rows, q) for q in qs])
        keep = np.ones(n, bool)
        keep[masked_copy] = False
        keep[5:90] = False
        allowed = np.arange(n)[keep]
        with ix.filter_rows(allowed) as f:
            f.set_path("scan")
            for k in (1, 10, 1000):
                r, c = ix.search_topk(qs, k, filter=f)
                for i in range(8):
                    wr, wc = expected(e_all[i], allowed, k)
                    assert np.array_equal(r[i], wr) and np.array_equal(bits(c[i]), bits(wc)), (k, i)
                    assert r[i][0] == allowed_copy[i] and not (set(masked_copy) & set(r[i].tolist())), (k, i)
    finally:
        ix.close()


@pytest.mark.parametrize("dim,dtype", [(1024, "f16"), (100, "f32")])
def test_unsupported_shapes_run_one_by_one(rlr, oracle, dim, dtype):
    n = 2397
    rows = oracle.synth_rows(n, dim, seed=61 + dim, n_clusters=4)
    ix = batch_index(rlr, dim, dtype)
    try:
        ix.upload(rows)
        stored = ix.fetch_rows(np.arange(n))
        qs = np.stack([oracle.normalize(oracle.synth_query(dim, seed=6200 + i)) for i in range(4)]).astype(np.float32)
        e_all = np.stack([oracle.scan(stored, q) for q in qs])
        allowed = np.arange(n)[1::2]
        ix.profile_enable(True)
        with ix.filter_rows(allowed) as f:
            f.set_path("scan")
            ix.profile_read(reset=True)
            check_queries(ix, f, qs, e_all, allowed, 10, (dim, dtype))
            p = ix.profile_read()
            assert p.n_batches == 0 and p.n_scan_launches == 4, p
    finally:
        ix.close()


def test_list_path_runs_of_queries(rlr, oracle):
    """8 queries over a 300-row filter on 2397 x 768: on the list path one run of score -> pack -> select per query and one
    synchronisation, on the forced masked scan one shared pass"""
    n, dim = 2397, 768
    rows = oracle.synth_rows(n, dim, seed=81, n_clusters=6)
    ix = batch_index(rlr, dim)
    try:
        ix.upload(rows)
        stored = ix.fetch_rows(np.arange(n))
        qs = np.stack([oracle.normalize(oracle.synth_query(dim, seed=8200 + i)) for i in range(8)]).astype(np.float32)
        e_all = np.stack([oracle.scan(stored, q) for q in qs])
        allowed = np.sort(np.random.default_rng(8).permutation(n)[:300])
        with ix.filter_rows(allowed) as f:
            assert f.info()["path"] == "list"
            for path in ("list", "scan"):
                f.set_path(path)
                for k in (1, 10, 300, 305):
                    ix.profile_read(reset=True)
                    check_queries(ix, f, qs, e_all, allowed, k, (path, k))
                    p = ix.profile_read()
                    assert p.n_batches == (1 if path == "scan" else 0) and p.n_searches == 8, (path, k, p)
                check_unfiltered(ix, qs[0], e_all[0], path)
    finally:
        ix.close()


def test_status_codes(rlr, oracle):
    n, dim = 300, 256
    rows = oracle.synth_rows(n + 40, dim, seed=61)
    qs = np.stack([oracle.normalize(oracle.synth_query(dim, seed=6300 + i)) for i in range(4)]).astype(np.float32)
    ix, other = batch_index(rlr, dim), batch_index(rlr, dim)
    try:
        ix.upload(rows[:n])
        other.upload(rows[:n])
        with other.filter_rows([0, 5]) as f:                  # a filter of another index
            with pytest.raises(rlr.RlrError) as ei:
                ix.search_topk(qs, 2, filter=f)
            assert ei.value.status == -1
        with ix.filter_ranges([(5, 0)]) as f:                 # no row allowed
            f.set_path("scan")
            r, c = ix.search_topk(qs, 10, filter=f)
            assert r.shape == (4, 0)
        old = ix.filter_ranges([(10, 50)])
        old.set_path("scan")
        assert ix.search_topk(qs, 5, filter=old)[0].shape == (4, 5)
        ix.append(rows[n:])
        with pytest.raises(rlr.RlrError) as ei:               # stale
            ix.search_topk(qs, 5, filter=old)
        assert ei.value.status == -1 and "stale" in str(ei.value)
        old.close()
    finally:
        ix.close()
        other.close()


def test_concurrent_scoped_batches(rlr, oracle):
    """four threads, 8-query calls over three filters (two on the shared pass, one on the list path): every result is the
    serial one"""
    n, dim = 2397, 512
    rows = oracle.synth_rows(n, dim, seed=71, n_clusters=9)
    ix = batch_index(rlr, dim)
    try:
        ix.upload(rows)
        qs = np.stack([oracle.normalize(oracle.synth_query(dim, seed=7200 + i)) for i in range(16)]).astype(np.float32)
        filters = [ix.filter_rows(np.arange(n)[::2]), ix.filter_ranges([(100, 1200)]), ix.filter_ranges([(7, 300)])]
        filters[0].set_path("scan")
        filters[1].set_path("scan")
        serial = {(fi, h): ix.search_topk(qs[h * 8:h * 8 + 8], 25, filter=f) for fi, f in enumerate(filters) for h in range(2)}
        errors = []

        def worker(t):
            try:
                for i in range(12):
                    fi, h = (t + i) % len(filters), (t + i // 3) % 2
                    r, c = ix.search_topk(qs[h * 8:h * 8 + 8], 25, filter=filters[fi])
                    wr, wc = serial[(fi, h)]
                    if not (np.array_equal(r, wr) and np.array_equal(bits(c), bits(wc))):
                        errors.append((t, i, fi, h))
            except Exception as e:  # noqa: BLE001 -- reported below
                errors.append((t, repr(e)))

        ts = [threading.Thread(target=worker, args=(t,)) for t in range(4)]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        assert not errors, errors[:5]
        for f in filters:
            f.close()
    finally:
        ix.close()
