"""Row filters (rlr_filter_create_*, rlr_search_topk_filtered): a filtered top-k is the reference's search over the corpus
that holds only the filter's rows, in ascending row order, mapped back to index rows -- rows and score bits exact, on
both paths (the list path and the masked scan), on every row shape the index accepts.  A row's reference-order score does
not depend on the other rows, so one oracle scan per corpus serves every mask: the expected result of a mask is that
scan reduced to the allowed rows, ordered (score desc, NaN last, row asc), cut to min(k, allowed rows)."""
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# the library's crossover between the two paths (csrc/index.hip kFilterListMax, DESIGN.md "Row filters"): filters with
# fewer allowed rows take the list path, the others the masked scan
THRESHOLD = 8192


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


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
    """name -> ascending allowed rows (the masks of the issue, then the complement of each)"""
    every = np.arange(n)
    m = {
        "all": every,
        "none": every[:0],
        "first": every[:1],
        "last": every[-1:],
        "bit63": every[63:64],
        "bit0_next": every[64:65],           # (empty when the index has a single word)
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


@pytest.fixture(scope="module", params=[(2397, 768, "f32"), (2397, 100, "f32"), (2397, 1024, "f16"), (2397, 72, "f16"),
                                        (64, 768, "f32"), (64, 100, "f32"), (64, 1024, "f16"), (64, 72, "f16")],
                ids=lambda p: f"{p[0]}x{p[1]}{p[2]}")
def corpus(request, rlr, oracle):
    n, dim, dtype = request.param
    rows = oracle.synth_rows(n, dim, seed=900 + dim, n_clusters=7)
    ix = rlr.GpuIndex(dim, dtype)
    ix.upload(rows)
    stored = ix.fetch_rows(np.arange(n))
    q = oracle.normalize(oracle.synth_query(dim, seed=77 + dim))
    e_full = oracle.scan(stored, q)          # the one reference: shared by every mask of this corpus, never changed
    yield ix, n, q, e_full
    ix.close()


def check_filtered(ix, f, q, e_full, allowed, k, ctx):
    """the filtered search on the filter's own path and on the other one, then an unfiltered search on the same index"""
    wr, wc = expected(e_full, allowed, k)
    natural = f.info()["path"]
    for path in (natural, "scan" if natural == "list" else "list"):
        f.set_path(path)
        r, c = ix.search_topk(q, k, filter=f)
        assert r.shape == (1, len(wr)), (ctx, path, r.shape, len(wr))
        assert np.array_equal(r[0], wr), (ctx, path, r[0][:8], wr[:8])
        assert np.array_equal(canon(c[0]), canon(wc)), (ctx, path)
        # hygiene: the histograms, the score array and the tail's counters are as an unfiltered search expects them
        ur, uc = ix.search_topk(q, 10)
        xr, xc = expected(e_full, np.arange(len(e_full)), 10)
        assert np.array_equal(ur[0], xr) and np.array_equal(canon(uc[0]), canon(xc)), (ctx, path, "unfiltered after")
    f.set_path(natural)


def test_masks_on_every_shape_and_both_paths(corpus):
    ix, n, q, e_full = corpus
    cases = masks_of(n)
    for name, allowed in cases.items():
        with ix.filter_rows(allowed[::-1]) as f:          # (any order; duplicates below)
            info = f.info()
            assert info["index_rows"] == n and info["n_allowed"] == len(allowed) and not info["stale"]
            assert info["path"] == ("list" if len(allowed) < THRESHOLD else "scan")
            for k in (1, 10, 300, len(allowed), len(allowed) + 5):
                if k == 0:
                    r, c = ix.search_topk(q, 0, filter=f)
                    assert r.shape[1] == 0
                    continue
                check_filtered(ix, f, q, e_full, allowed, k, (name, k))
    # ranges: three documents, overlapping ranges form a union, their complement through rows with duplicates
    ranges = document_ranges(n)
    docs = rows_of_ranges(ranges)
    with ix.filter_ranges(ranges + [ranges[0], (ranges[1][0], 1)]) as f:
        assert f.info()["n_allowed"] == len(docs)
        for k in (1, 10, 300, len(docs), len(docs) + 5):
            check_filtered(ix, f, q, e_full, docs, k, ("documents", k))
    keep = np.ones(n, bool)
    keep[docs] = False
    rest = np.arange(n)[keep]
    with ix.filter_rows(np.concatenate([rest, rest[:5]])) as f:
        assert f.info()["n_allowed"] == len(rest)
        for k in (1, 10, 300, len(rest), len(rest) + 5):
            check_filtered(ix, f, q, e_full, rest, k, ("not_documents", k))
    # the mask of every row is rlr_search_topk, bit for bit
    with ix.filter_ranges([(0, n)]) as f:
        for k in (1, 10, 300, n, n + 5):
            r, c = ix.search_topk(q, k, filter=f)
            ur, uc = ix.search_topk(q, k)
            assert np.array_equal(r, ur) and np.array_equal(bits(c), bits(uc)), k


def test_filter_arguments(corpus, rlr):
    ix, n, q, e_full = corpus
    with pytest.raises(rlr.RlrError) as ei:
        ix.filter_rows([0, n])
    assert ei.value.status == -5                                     # RLR_E_RANGE
    with pytest.raises(rlr.RlrError) as ei:
        ix.filter_ranges([(n - 1, 2)])
    assert ei.value.status == -5
    with ix.filter_ranges([(5, 0)]) as f:                            # an empty range is no row
        assert f.info()["n_allowed"] == 0
        r, c = ix.search_topk(q, 10, filter=f)
        assert r.shape == (1, 0)
    # several queries in one call run one by one
    qs = np.stack([q, -q, q])
    allowed = np.arange(n)[1::3]
    with ix.filter_rows(allowed) as f:
        r, c = ix.search_topk(qs, 7, filter=f)
        wr, wc = expected(e_full, allowed, 7)
        assert np.array_equal(r[0], wr) and np.array_equal(r[2], wr) and np.array_equal(bits(c[2]), bits(wc))
        nr, nc = expected(-e_full, allowed, 7)
        assert np.array_equal(r[1], nr) and np.array_equal(bits(c[1]), bits(nc))
    # a filter of another index is refused
    other = rlr.GpuIndex(ix.dim, ix.dtype)
    try:
        other.upload(ix.fetch_rows(np.arange(n)))
        with other.filter_rows([0]) as f:
            with pytest.raises(rlr.RlrError) as ei:
                ix.search_topk(q, 1, filter=f)
            assert ei.value.status == -1
    finally:
        other.close()


@pytest.mark.parametrize("dim,dtype", [(72, "f16"), (768, "f32")])
def test_each_path_is_chosen_on_its_side_of_the_threshold(rlr, oracle, dim, dtype):
    """n = 4 x threshold rows: threshold - 1 allowed rows take the list path, threshold the masked scan (the generic kernel
    at 72-d binary16, the fixed 768-d kernel with the query in registers)"""
    n = 4 * THRESHOLD
    rows = oracle.synth_rows(n, dim, seed=4100 + dim, n_clusters=11)
    ix = rlr.GpuIndex(dim, dtype)
    try:
        ix.upload(rows)
        stored = ix.fetch_rows(np.arange(n))
        q = oracle.normalize(oracle.synth_query(dim, seed=4200 + dim))
        e_full = oracle.scan(stored, q)
        scattered = np.sort(np.random.default_rng(5).permutation(n)[:THRESHOLD])
        for allowed, path in ((scattered[:-1], "list"), (scattered, "scan"), (np.arange(n)[n // 2 - 5:], "scan")):
            with ix.filter_rows(allowed) as f:
                assert f.info()["path"] == path, (len(allowed), f.info())
                for k in (1, 100, len(allowed)):
                    wr, wc = expected(e_full, allowed, k)
                    r, c = ix.search_topk(q, k, filter=f)
                    assert np.array_equal(r[0], wr) and np.array_equal(bits(c[0]), bits(wc)), (path, k)
                ur, uc = ix.search_topk(q, 10)
                xr, xc = expected(e_full, np.arange(n), 10)
                assert np.array_equal(ur[0], xr) and np.array_equal(bits(uc[0]), bits(xc))
    finally:
        ix.close()


def test_query_copy_in_a_masked_row_never_appears(rlr, oracle):
    n, dim = 2397, 768
    rows = oracle.synth_rows(n, dim, seed=31, n_clusters=5)
    q = oracle.normalize(oracle.synth_query(dim, seed=32))
    masked_copy, allowed_copy = 130, 1901
    rows[masked_copy] = q
    rows[allowed_copy] = q
    ix = rlr.GpuIndex(dim)
    try:
        ix.upload(rows)                                  # stored as given: both rows ARE the query
        e_full = oracle.scan(rows, q)
        keep = np.ones(n, bool)
        keep[masked_copy] = False
        keep[5:90] = False
        allowed = np.arange(n)[keep]
        with ix.filter_rows(allowed) as f:
            for path in ("list", "scan"):
                f.set_path(path)
                for k in (1, 10, len(allowed)):
                    r, c = ix.search_topk(q, k, filter=f)
                    wr, wc = expected(e_full, allowed, k)
                    assert np.array_equal(r[0], wr) and np.array_equal(bits(c[0]), bits(wc)), (path, k)
                    assert r[0][0] == allowed_copy and masked_copy not in r[0], (path, k)
        r, c = ix.search_topk(q, 2)
        assert list(r[0]) == [masked_copy, allowed_copy]  # (unfiltered: the lower row first)
    finally:
        ix.close()


def test_tie_flood_overflows_the_band_and_resolves_to_the_lowest_allowed_rows(rlr, oracle):
    """5000 identical allowed rows among 6000: the guard band holds them all, more than the one-workgroup sort takes; the
    1000 masked rows are copies of the query, the best rows of the index"""
    n, dim = 6000, 100
    base = oracle.synth_rows(2, dim, seed=41)
    q = oracle.normalize(oracle.synth_query(dim, seed=42))
    rows = np.empty((n, dim), np.float32)
    rows[:] = base[0]
    masked = np.arange(n)[5::6]
    rows[masked] = q
    keep = np.ones(n, bool)
    keep[masked] = False
    allowed = np.arange(n)[keep]
    ix = rlr.GpuIndex(dim)
    try:
        ix.upload(rows)
        e_full = oracle.scan(rows, q)
        with ix.filter_rows(allowed) as f:
            assert f.info()["n_allowed"] == 5000
            ix.profile_read(reset=True)
            for path in ("scan", "list"):
                f.set_path(path)
                r, c = ix.search_topk(q, 10, filter=f)
                wr, wc = expected(e_full, allowed, 10)
                assert list(r[0]) == list(allowed[:10]) == list(wr), path
                assert np.array_equal(bits(c[0]), bits(wc)), path
            assert ix.profile_read().n_retries >= 1      # the masked scan's band did overflow
        ur, uc = ix.search_topk(q, 10)
        assert list(ur[0]) == list(masked[:10])
    finally:
        ix.close()


def test_non_finite_rows_order_last_and_masked_ones_stay_out(rlr, oracle):
    """rows stored un-normalised; three allowed and three masked rows hold NaN or Inf components and k is every allowed
    row: the selection threshold reaches the NaN class, where a masked row's sentinel no longer keeps it out by itself"""
    n, dim = 2397, 100
    rows = oracle.synth_rows(n, dim, seed=51, n_clusters=3)
    q = oracle.normalize(oracle.synth_query(dim, seed=52))
    allowed = np.arange(n)[::2]
    rows[10, 3] = np.nan
    rows[700, 0], rows[700, 1] = np.inf, -np.inf          # Inf - Inf or a signed Inf, as the query's signs have it
    rows[1500, 7] = np.inf
    rows[11, 3] = np.nan
    rows[701, 0], rows[701, 1] = np.inf, -np.inf
    rows[1501, 7] = -np.inf
    ix = rlr.GpuIndex(dim)
    try:
        ix.upload(rows, normalize=False)
        e_full = oracle.scan(rows, q)
        assert np.isnan(e_full[10]) and np.isnan(e_full[11])
        with ix.filter_rows(allowed) as f:
            for path in ("list", "scan"):
                f.set_path(path)
                for k in (len(allowed), 10, len(allowed) - 2):
                    r, c = ix.search_topk(q, k, filter=f)
                    wr, wc = expected(e_full, allowed, k)
                    assert np.array_equal(r[0], wr), (path, k)
                    assert np.array_equal(canon(c[0]), canon(wc)), (path, k)
                    assert not (set(r[0].tolist()) & {11, 701, 1501}), (path, k)
                ur, uc = ix.search_topk(q, 10)
                xr, xc = expected(e_full, np.arange(n), 10)
                assert np.array_equal(ur[0], xr) and np.array_equal(canon(uc[0]), canon(xc)), path
    finally:
        ix.close()


def test_a_mutated_index_makes_its_filters_stale(rlr, oracle):
    n, dim = 300, 72
    rows = oracle.synth_rows(n + 40, dim, seed=61)
    q = oracle.normalize(oracle.synth_query(dim, seed=62))
    ix = rlr.GpuIndex(dim)
    try:
        ix.upload(rows[:n])
        old = ix.filter_ranges([(10, 50)])
        assert ix.search_topk(q, 5, filter=old)[0].shape == (1, 5)
        ix.append(rows[n:])
        assert old.info()["stale"]
        with pytest.raises(rlr.RlrError) as ei:
            ix.search_topk(q, 5, filter=old)
        assert ei.value.status == -1 and "stale" in str(ei.value)
        stored = ix.fetch_rows(np.arange(n + 40))
        fresh = ix.filter_ranges([(10, 50), (n, 40)])
        allowed = rows_of_ranges([(10, 50), (n, 40)])
        r, c = ix.search_topk(q, 20, filter=fresh)
        wr, wc = expected(oracle.scan(stored, q), allowed, 20)
        assert np.array_equal(r[0], wr) and np.array_equal(bits(c[0]), bits(wc))
        ix.delete_rows([0, 11, 12])                       # renumbers every row behind them
        with pytest.raises(rlr.RlrError) as ei:
            ix.search_topk(q, 5, filter=fresh)
        assert ei.value.status == -1
        stored = ix.fetch_rows(np.arange(n + 37))
        again = ix.filter_ranges([(9, 48)])
        r, c = ix.search_topk(q, 48, filter=again)
        wr, wc = expected(oracle.scan(stored, q), np.arange(9, 57), 48)
        assert np.array_equal(r[0], wr) and np.array_equal(bits(c[0]), bits(wc))
        for f in (old, fresh, again):
            f.close()
    finally:
        ix.close()


def test_concurrent_filtered_and_unfiltered_searches(rlr, oracle):
    """eight threads, four filters (two per path) and unfiltered searches in one process: every result is the serial one"""
    n, dim = 3 * THRESHOLD, 72
    rows = oracle.synth_rows(n, dim, seed=71, n_clusters=9)
    ix = rlr.GpuIndex(dim)
    try:
        ix.upload(rows)
        qs = [oracle.normalize(oracle.synth_query(dim, seed=720 + i)) for i in range(4)]
        filters = [ix.filter_rows(np.arange(n)[::2]), ix.filter_ranges([(100, THRESHOLD + 37)]),
                   ix.filter_ranges([(7, 300)]), ix.filter_rows(np.arange(n)[5::97]), None]
        assert [f.info()["path"] for f in filters[:4]] == ["scan", "scan", "list", "list"]
        serial = {(fi, qi): ix.search_topk(qs[qi], 25, filter=f) for fi, f in enumerate(filters) for qi in range(4)}
        errors = []

        def worker(t):
            try:
                for i in range(50):
                    fi, qi = (t + i) % len(filters), (t * 3 + i) % 4
                    r, c = ix.search_topk(qs[qi], 25, filter=filters[fi])
                    wr, wc = serial[(fi, qi)]
                    if not (np.array_equal(r, wr) and np.array_equal(bits(c), bits(wc))):
                        errors.append((t, i, fi, qi))
            except Exception as e:  # noqa: BLE001 -- reported below
                errors.append((t, repr(e)))

        ts = [threading.Thread(target=worker, args=(t,)) for t in range(8)]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        assert not errors, errors[:5]
        for f in filters[:4]:
            f.close()
    finally:
        ix.close()
