"""Every nomination path at the numeric edges its guard band has to cover: f32 operands beyond binary16 range, binary16
subnormals against operands of a very different size, f32 subnormal and signed-zero scores, scores at the edge of f32
overflow (+-Inf, NaN from Inf - Inf), and the recorded row norms across mutations.

Each corpus is built element by element, run through every path that can serve it, and checked against the oracle's
left-to-right scan: the same rows in the same order, scores equal as bit patterns.  The profile counters prove which
path ran: a call whose operands leave binary16 range must not nominate in binary16 (n_f16_range_fallbacks), every
other call must run where the test sent it."""
import numpy as np
import pytest

from conftest import bits

pytestmark = pytest.mark.gpu

DIM = 768
N = 4096                      # the batched paths need at least 4096 rows
S24 = np.float32(2.0 ** -24)  # binary16's subnormal spacing
PATHS = ("scan", "multi", "gemm", "image", "image_scan", "q8", "f16_scan", "f16_gemm", "shards3")


def oracle_topk(O, rows, q, k):
    e = O.scan(rows, q)
    key = np.where(np.isnan(e), -np.inf, e)
    order = np.lexsort((np.arange(len(e)), -key.astype(np.float64)))[:k]
    return order.astype(np.uint64), e[order]


def beyond_f16(a):
    return bool((np.abs(np.asarray(a, np.float32)) > 65504).any())


def filler(O, n, seed, scale=1.0):
    """ordinary unit-norm rows, scaled"""
    return (O.synth_rows(n, DIM, seed=seed, n_clusters=5) * np.float32(scale)).astype(np.float32)


def pad_batch(O, qs, nq, scale=1.0):
    """the case's queries followed by ordinary ones (of the same order of norm) up to nq"""
    extra = [(O.normalize(O.synth_query(DIM, seed=7000 + i)) * np.float32(scale)).astype(np.float32)
             for i in range(max(0, nq - len(qs)))]
    return np.stack(list(qs) + extra).astype(np.float32)


def check(O, rows, qs, r, c, k, ctx):
    for i in range(len(qs)):
        wr, wc = oracle_topk(O, rows, qs[i], k)
        assert np.array_equal(r[i], wr), f"{ctx} query {i}: rows differ: got {r[i][:5]} want {wr[:5]}"
        assert np.array_equal(bits(c[i]), bits(wc)), f"{ctx} query {i}: scores differ: got {c[i][:5]} want {wc[:5]}"


def run_path(rlr, O, monkeypatch, path, rows, qs, k):
    """search `qs` (top-k each) through `path`, check against the oracle, assert that the path ran"""
    f16_index = path.startswith("f16")
    ref_rows = O.round_f16(rows) if f16_index else rows
    ctx = dict(path=path, k=k)
    if path == "shards3":
        mi = rlr.MultiGpuIndex(DIM, [0, 0, 0], "f32")
        try:
            mi.upload(rows)
            r, c = mi.search_topk(qs, k)
            check(O, ref_rows, qs, r, c, k, ctx)
        finally:
            mi.close()
        return
    batched = path in ("multi", "gemm", "image", "f16_gemm")
    if batched:
        monkeypatch.setenv("RLR_BATCH_MIN", "2")   # read when the index is created
    else:
        monkeypatch.setenv("RLR_BATCH_MIN", "100000")
    ix = rlr.GpuIndex(DIM, "f16" if f16_index else "f32")
    try:
        ix.upload(rows)
        if path == "image":
            ix.enable_batch_image(True)
        elif path == "image_scan":
            ix.enable_batch_image(True, single_query=True)
        elif path == "q8":
            ix.enable_batch_image(False, q8=True)
        ix.profile_enable(True)
        # binary16 nomination is safe for this call only if no stored f32 row and no query leaves binary16 range
        rows_out = not f16_index and beyond_f16(rows)
        if batched:
            batches = [qs] if path != "multi" else [qs[i:i + 8] for i in range(0, len(qs), 8)]
            for b in batches:
                ix.profile_read(reset=True)
                r, c = ix.search_topk(b, k)
                p = ix.profile_read()
                check(O, ref_rows, b, r, c, k, ctx)
                f16_safe = not rows_out and not beyond_f16(b)
                if path == "multi":                # 2..8 queries over f32 rows: the shared f32 scan, whatever the range
                    assert 2 <= len(b) <= 8
                    assert p.n_batches == 1 and p.n_f16_range_fallbacks == 0, (ctx, p)
                elif f16_safe:
                    assert p.n_batches == 1 and p.n_f16_range_fallbacks == 0, (ctx, p)
                    # >= 16 queries over f32 rows without an image count as such: the GEMM streamed the f32 rows
                    want_without = 1 if path == "gemm" else 0
                    assert p.n_batches_without_image == want_without, (ctx, p)
                else:                              # the single-query pipelines over the f32 / f16 rows instead
                    assert p.n_batches == 0 and p.n_f16_range_fallbacks == len(b), (ctx, p)
                    assert p.n_scan_launches == len(b), (ctx, p)
        else:
            for i in range(len(qs)):
                ix.profile_read(reset=True)
                r, c = ix.search_topk(qs[i], k)
                p = ix.profile_read()
                check(O, ref_rows, qs[i:i + 1], r, c, k, dict(ctx, query=i))
                assert p.n_batches == 0 and p.n_scan_launches == 1, (ctx, p)
                f16_safe = not rows_out and not beyond_f16(qs[i])
                if path == "image_scan":
                    fell_back = not f16_safe
                    assert p.n_f16_range_fallbacks == int(fell_back), (ctx, i, p)
                    assert p.scan_bytes == len(rows) * DIM * (4 if fell_back else 2), (ctx, i, p)
                elif path == "q8":
                    assert p.n_f16_range_fallbacks == 0 and p.scan_bytes == len(rows) * DIM, (ctx, i, p)
                else:
                    assert p.n_f16_range_fallbacks == 0, (ctx, i, p)
                    assert p.scan_bytes == len(rows) * DIM * (2 if f16_index else 4), (ctx, i, p)
    finally:
        ix.close()


def run_all(rlr, O, monkeypatch, rows, qs, ks, paths=PATHS):
    for k in ks:
        for path in paths:
            run_path(rlr, O, monkeypatch, path, rows, qs, k)


# ---------------------------------------------------------------- binary16 overflow
def overflow_rows(O):
    """rows whose f32 elements binary16 cannot hold, against a query with q[0] = 2, q[1] = 1, q[2] = 0.5, q[3] = 0.3"""
    rows = filler(O, N, seed=8101)
    rows[100] = 0
    rows[100, 0], rows[100, 1] = 70000.0, -70000.0  # exact 70000 (the best); binary16: Inf * 2 - Inf * 1 = NaN
    rows[101] = 0
    rows[101, 2] = 1.0e5                            # exact 50000; binary16 +Inf
    rows[102] = 0
    rows[102, 3] = 65520.0                          # half-way from 65504 to 65536: rounds (to even) to Inf
    rows[103] = 0
    rows[103, 3] = 65504.0                          # binary16's largest finite value
    rows[104] = 0
    rows[104, 3] = 65519.0                          # rounds down to 65504 in binary16
    rows[105] = 0
    rows[105, 4], rows[105, 5] = -9.0e5, 9.0e5      # -Inf + Inf in binary16 for the ordinary queries below
    rows[106] = rows[100] * np.float32(-1.0)        # the worst row
    return rows


def overflow_query(O):
    q = (O.normalize(O.synth_query(DIM, seed=8102)) * np.float32(0.01)).astype(np.float32)
    q[0], q[1], q[2], q[3] = 2.0, 1.0, 0.5, 0.3
    return q


@pytest.mark.parametrize("k", [1, 10, 100])
def test_f32_rows_beyond_binary16_range(rlr, oracle, monkeypatch, k):
    rows = overflow_rows(oracle)
    qs = pad_batch(oracle, [overflow_query(oracle)], 16)
    wr, _ = oracle_topk(oracle, rows, qs[0], 3)
    assert list(wr) == [100, 101, 102]
    run_all(rlr, oracle, monkeypatch, rows, qs, [k], paths=[p for p in PATHS if not p.startswith("f16")])


@pytest.mark.parametrize("k", [1, 10, 100])
def test_queries_beyond_binary16_range(rlr, oracle, monkeypatch, k):
    rows = filler(oracle, N, seed=8201)
    qa = oracle.normalize(rows[17].copy())
    qa[5] = 1.0e5                                   # one element past binary16's range
    qb = oracle.normalize(rows[33].copy())
    qb[9] = -65520.0                                # rounds to -Inf in binary16
    qc = oracle.normalize(rows[44].copy())
    qc[2] = 65504.0                                 # the largest finite binary16: binary16 paths stay on
    base = pad_batch(oracle, [], 15)
    run_all(rlr, oracle, monkeypatch, rows, np.concatenate([qa[None], base]), [k])
    run_all(rlr, oracle, monkeypatch, rows, np.concatenate([qb[None], base]), [k], paths=("gemm", "image_scan", "f16_gemm"))
    run_all(rlr, oracle, monkeypatch, rows, np.concatenate([qc[None], base]), [k], paths=("gemm", "image", "image_scan", "f16_gemm"))


# ---------------------------------------------------------------- binary16 subnormals
def tiny_rows(O, sign):
    """rows A (every element 1.49 * 2^-24: binary16 rounds it down to 2^-24) and 150 decoys B (two thirds of the elements
    just above 1.5 * 2^-24: rounded up to 2^-23) -- A's exact score is the best, every B nominates above it"""
    rng = np.random.default_rng(8301)
    rows = filler(O, N, seed=8302, scale=1e-9)      # exact scores far below A's, zero in binary16
    rows[50] = np.float32(1.49) * S24
    for j in range(150):
        nz = 500 + j % 13                           # 500..512 non-zero elements
        b = np.zeros(DIM, np.float32)
        b[rng.permutation(DIM)[:nz]] = np.float32(1.51 - 0.0005 * (j % 17)) * S24
        rows[200 + j] = b
    rows[50:350] *= np.float32(sign)
    return rows


@pytest.mark.parametrize("qnorm", [1e2, 1e4, 1e6])
@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_binary16_subnormal_rows_against_large_queries(rlr, oracle, monkeypatch, qnorm, sign):
    rows = tiny_rows(oracle, sign)
    q = np.full(DIM, np.float32(qnorm / np.sqrt(DIM)) * np.float32(sign), np.float32)
    qs = pad_batch(oracle, [q], 16, scale=qnorm)
    wr, _ = oracle_topk(oracle, rows, q, 1)
    assert wr[0] == 50
    run_all(rlr, oracle, monkeypatch, rows, qs, [1, 10, 100])


@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_binary16_subnormal_queries_against_large_rows(rlr, oracle, monkeypatch, sign):
    """the mirror case: a query whose elements binary16 stores as subnormals (norm 2.5e-6) against rows of norm 6e5 --
    the product of the norms is about 1, so only a band that grows with the larger norm alone keeps A"""
    rng = np.random.default_rng(8401)
    half = rng.permutation(DIM)
    lo, hi = half[: DIM // 2], half[DIM // 2:]
    q = np.zeros(DIM, np.float32)
    q[lo] = np.float32(1.49) * S24                  # rounds down to 2^-24
    q[hi] = np.float32(1.51) * S24                  # rounds up to 2^-23
    rows = filler(oracle, N, seed=8402)
    X = np.float32(30000.0)
    rows[60] = 0
    rows[60, lo] = X                                # A: exact 384 * 1.49 * 2^-24 * X
    for j in range(150):                            # B: exact 384 * 1.51 * 2^-24 * X * (1 - v) < A, nominated ~2 x A
        b = np.zeros(DIM, np.float32)
        b[hi] = X * np.float32(1.0 - 0.014 - 0.0001 * j)
        rows[300 + j] = b
    rows[60:450] *= np.float32(sign)               # (negative rows against a negative query: the same products)
    q *= np.float32(sign)
    qs = pad_batch(oracle, [q], 16, scale=2.5e-6)
    wr, _ = oracle_topk(oracle, rows, q, 1)
    assert wr[0] == 60
    run_all(rlr, oracle, monkeypatch, rows, qs, [1, 10, 100])


def test_binary16_subnormal_row_on_f16_index(rlr, oracle, monkeypatch):
    """an f16-typed index holding a row of binary16 subnormals (exact there) and rows of them in every pattern"""
    rows = filler(oracle, N, seed=8501, scale=1e-3)
    rng = np.random.default_rng(8502)
    for j in range(64):
        rows[10 + j] = (rng.integers(-1023, 1024, DIM) * S24).astype(np.float32)   # every binary16 subnormal
    rows[9] = np.float32(1023) * S24               # the largest subnormal everywhere
    q = np.full(DIM, np.float32(500.0), np.float32)
    qs = pad_batch(oracle, [q, -q], 16, scale=1e4)
    run_all(rlr, oracle, monkeypatch, rows, qs, [1, 10, 100], paths=("f16_scan", "f16_gemm", "scan", "gemm"))


# ---------------------------------------------------------------- f32 subnormals on the exact path
def test_f32_subnormal_elements_and_scores(rlr, oracle, monkeypatch):
    """rows of f32 subnormals (multiples of 2^-149: distinct scores one ulp apart, +-0), products that underflow into
    subnormals, a subnormal query against ordinary rows: the re-score must not flush, the select must order every
    subnormal and the two zeros like the oracle"""
    rng = np.random.default_rng(8601)
    tiny = np.float32(2.0 ** -149)
    rows = (rng.integers(-3, 4, (N, DIM)) * tiny).astype(np.float32)   # every score a subnormal (or zero)
    rows[::7] *= np.float32(1e3)                                      # ... some larger, still subnormal
    rows[5] = 0.0
    rows[6] = -0.0
    rows[7] = tiny
    rows[8] = -tiny
    rows[11] = np.float32(1e-39)
    rows[12] = np.float32(-1e-39)
    q = np.ones(DIM, np.float32)
    q[::2] = -1.0
    q2 = np.full(DIM, np.float32(0.5), np.float32)                    # products 2^-150 * n: round to even
    q3 = np.full(DIM, np.float32(1e-3), np.float32)                   # 1e-39 * 1e-3 underflows to the subnormal grid
    run_all(rlr, oracle, monkeypatch, rows, pad_batch(oracle, [q, q2, q3, -q], 16, scale=1.0), [1, 10, 300])
    # a subnormal query against ordinary rows: subnormal products, normal sums
    rows2 = filler(oracle, N, seed=8602)
    qs = np.stack([np.float32(1e-39) * np.sign(rows2[3]).astype(np.float32), np.full(DIM, np.float32(1e-45), np.float32)])
    run_all(rlr, oracle, monkeypatch, rows2, pad_batch(oracle, list(qs), 16, scale=1e-39), [1, 100])


# ---------------------------------------------------------------- scores near f32 overflow
def test_scores_near_f32_overflow(rlr, oracle, monkeypatch):
    """dot products at +-3.4e38: the reference's left-to-right sum overflows where another order would not, and the
    reverse; +-Inf scores rank like the oracle's, a NaN from Inf - Inf orders last"""
    rows = filler(oracle, N, seed=8701)
    big = np.float32(2e38)
    def row(**el):
        r = np.zeros(DIM, np.float32)
        for i, v in el.items():
            r[int(i[1:])] = v
        return r
    rows[20] = row(e0=big, e1=big, e2=-big)                       # left to right: +Inf; pairwise from the end: 2e38
    rows[21] = row(e0=-big, e1=-big, e2=big)                      # -Inf
    rows[22] = row(e0=big, e1=-big, e2=big, e700=big)             # 2e38, then +Inf at the end
    rows[23] = row(e0=np.float32(1.7e38), e1=np.float32(1.6e38))  # 3.3e38: finite, the largest finite score here
    rows[24] = row(e0=np.float32(1.7e38), e1=np.float32(1.7e38))  # 3.4e38 + rounding: overflows to +Inf
    rows[25] = row(e0=big, e1=big, e10=np.float32(-1e38))         # +Inf + (-1e38 * 10 = -Inf) = NaN
    rows[26] = row(e0=np.float32(3e38), e767=np.float32(-3e38))   # 0 exactly
    rows[27] = row(e0=np.float32(3.4e38))                          # f32 max region, finite
    rows[28] = -rows[27]
    q = np.ones(DIM, np.float32)
    q[10] = 10.0
    q2 = q.copy()
    q2[0] = -1.0                                                  # flips which rows overflow
    run_all(rlr, oracle, monkeypatch, rows, pad_batch(oracle, [q, q2], 16, scale=27.7), [1, 10, 100])


# ---------------------------------------------------------------- band bookkeeping across mutations
@pytest.mark.parametrize("mode", ["plain", "image", "image_scan"])
def test_recorded_row_norms_follow_mutations(rlr, oracle, monkeypatch, mode):
    """append a huge row (beyond binary16 range) and a long one (norm 6e5), delete them, replace the corpus with
    upload(normalize=True): exact after every step, binary16 nomination off exactly while a huge row may be stored"""
    monkeypatch.setenv("RLR_BATCH_MIN", "2")
    rows = filler(oracle, N, seed=8801)
    ix = rlr.GpuIndex(DIM)
    try:
        ix.upload(rows)
        if mode != "plain":
            ix.enable_batch_image(True, single_query=(mode == "image_scan"))
        qs = pad_batch(oracle, [], 16)

        def step(cur, want_fallback, qset=qs):
            ix.profile_read(reset=True)
            r, c = ix.search_topk(qset, 10)
            check(oracle, cur, qset, r, c, 10, dict(mode=mode, n=len(cur)))
            p = ix.profile_read()
            assert (p.n_f16_range_fallbacks > 0) == want_fallback, (mode, p)
            r1, c1 = ix.search_topk(qset[0], 10)
            check(oracle, cur, qset[:1], r1, c1, 10, dict(mode=mode, single=True))

        step(rows, False)
        huge = np.zeros((1, DIM), np.float32)
        huge[0, :8] = np.float32(1e5) * np.sign(qs[0, :8])         # the best row for query 0
        ix.append(huge)
        cur = np.concatenate([rows, huge])
        step(cur, True)
        ix.delete_rows([N])
        step(rows, True)                                          # (a deleted huge row keeps the f32 path: conservative)
        # a query whose elements are binary16 subnormals, and a long row appended after the upload: the band must use
        # the appended row's norm
        tq = np.zeros(DIM, np.float32)
        tq[::2] = np.float32(1.49) * S24
        tq[1::2] = np.float32(1.51) * S24
        longr = np.zeros((151, DIM), np.float32)
        longr[0, ::2] = 30000.0
        for j in range(1, 151):
            longr[j, 1::2] = np.float32(30000.0 * (1.0 - 0.014 - 0.0001 * j))
        ix.upload(rows, normalize=True)                           # normalised rows: nothing beyond binary16 range
        norm_rows = np.stack([oracle.normalize(r) for r in rows])
        step(norm_rows, False)
        ix.append(longr)
        tqs = pad_batch(oracle, [tq], 16, scale=2.5e-6)
        step(np.concatenate([norm_rows, longr]), False, tqs)
    finally:
        ix.close()


# ---------------------------------------------------------------- unit-norm data: the bands do not move
def test_unit_norm_bands_unchanged(rlr, oracle, monkeypatch):
    """unit-norm rows and queries: every binary16 path serves the batch with no query handed back"""
    rows = oracle.synth_rows(20000, DIM, seed=8901, n_clusters=9)
    qs = np.stack([oracle.normalize(oracle.synth_query(DIM, seed=8902 + i)) for i in range(32)])
    for path in ("gemm", "image"):
        monkeypatch.setenv("RLR_BATCH_MIN", "2")
        ix = rlr.GpuIndex(DIM)
        try:
            ix.upload(rows)
            if path == "image":
                ix.enable_batch_image(True)
            ix.profile_read(reset=True)
            r, c = ix.search_topk(qs, 100)
            p = ix.profile_read()
            check(oracle, rows, qs, r, c, 100, dict(path=path))
            assert p.n_batches == 1 and p.n_batch_fallbacks == 0 and p.n_f16_range_fallbacks == 0, (path, p)
        finally:
            ix.close()
