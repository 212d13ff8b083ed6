"""On-device normalisation and the binary16 store (sumsq_kernel, sqrt_rn, ref_scale, scale_store_kernel; the chunk loop
of ingest()) at their rounding edges: the stored rows, read back with fetch_rows, are the oracle's `normalize` -- then its
binary16 rounding for binary16 storage -- bit for bit.  No tolerances; NaNs compare as one pattern.  The input rows come
from ingest_vectors.py, and test_ingest_vectors_cpu.py proves without a GPU what they hit and that a root one ulp off, a
directed divide or a wrong tie rule in the store would change them."""
import functools

import numpy as np
import pytest

import ingest_vectors as V
from ingest_vectors import bits, canon

pytestmark = pytest.mark.gpu

STAGING_BYTES = 64 << 20          # ingest() stages an upload in chunks of this many bytes of f32 rows (csrc/index.hip)


@functools.lru_cache(maxsize=None)
def _expected(dim, f16, edges=True):
    from oracle import oracle as O
    want = V.oracle_rows(O, V.corpus(dim, edges), f16=f16)
    want.setflags(write=False)
    return want


def assert_rows(got, want, ctx):
    same = canon(got) == canon(want)
    if not same.all():
        r, c = np.argwhere(~same)[0]
        raise AssertionError(f"{ctx}: {int((~same).sum())} elements in {int((~same).any(axis=1).sum())} rows differ; first "
                             f"at row {r} col {c}: got {bits(got)[r, c]:#010x} want {bits(want)[r, c]:#010x}")


def check_search(O, ix, want, dim, k=300):
    """one search over the stored rows: the oracle's scan of the expected rows, in its order, score bits equal.  The
    kernels read whole 16-byte units of a row, so this also holds the pad columns to zero."""
    q = O.normalize(O.synth_query(dim, seed=4100 + dim))
    r, c = ix.search_topk(q, k)
    wr, wc = V.ranking(O.scan(want, q), k)
    assert r.shape == (1, len(wr))
    assert np.array_equal(r[0], wr), (dim, r[0][:8], wr[:8])
    assert np.array_equal(canon(c[0]), canon(wc)), dim


@pytest.mark.parametrize("dim,dtype", [(8, "f32"), (768, "f32"), (3, "f32"), (101, "f32"),
                                       (1024, "f16"), (72, "f16"), (100, "f16"), (7, "f16")])
def test_upload_normalize_hard_vectors(rlr, oracle, dim, dtype):
    """(a) hard roots at three scales, (b) hard quotients (dims with room for them), (c) the class edges: rows that stay
    as given (norm^2 <= 1e-20, NaN -- in binary16 with Inf where an entry exceeds 65504) among rows that are scaled"""
    rows = V.corpus(dim)
    want = _expected(dim, dtype == "f16")
    ix = rlr.GpuIndex(dim, dtype)
    try:
        ix.upload(rows, normalize=True)
        assert len(ix) == len(rows)
        assert_rows(ix.fetch_rows(np.arange(len(rows))), want, (dim, dtype))
        check_search(oracle, ix, want, dim)
    finally:
        ix.close()


def test_binary16_store_conversion_table(rlr, oracle):
    """(d): every binary16 pattern, every tie between two patterns and its f32 neighbours, 2^-25, 65504 .. 65520, FLT_MAX,
    +-Inf, NaN and f32 subnormals, stored as given into a binary16 index"""
    rows, _kind, _lower = V.f16_table(768)
    ix = rlr.GpuIndex(768, "f16")
    try:
        ix.upload(rows, normalize=False)
        assert_rows(ix.fetch_rows(np.arange(len(rows))), oracle.round_f16(rows), "binary16 table")
    finally:
        ix.close()


@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_append_normalize_behind_existing_rows(rlr, oracle, dtype):
    """rows stored as given, then two normalising appends of (a) + (b) -- the second grows the allocation --, then a
    deletion from each part: earlier rows and survivors keep their bits"""
    dim, f16 = 768, dtype == "f16"
    first = (np.random.default_rng(31).standard_normal((300, dim)) * 3).astype(np.float32)
    hard, hard_want = V.corpus(dim, edges=False), _expected(dim, f16, edges=False)
    # the first append: every fourth row of (a) and the rows of (b); the second: all of (a) + (b)
    some = np.union1d(np.arange(0, len(hard), 4), np.arange(len(hard) - 4, len(hard)))
    want = np.concatenate([oracle.round_f16(first) if f16 else first, hard_want[some], hard_want])
    n1, n2 = 300 + len(some), 300 + len(some) + len(hard)
    assert n1 <= 1024 < n2                                  # (a first allocation holds 1024 rows)
    ix = rlr.GpuIndex(dim, dtype)
    try:
        ix.upload(first, normalize=False)
        assert ix.append(hard[some], normalize=True) == 300
        assert_rows(ix.fetch_rows(np.arange(n1)), want[:n1], (dtype, "after the first append"))
        assert ix.append(hard, normalize=True) == n1
        assert len(ix) == n2
        assert_rows(ix.fetch_rows(np.arange(n2)), want, (dtype, "after the second append"))
        dead = np.array([0, 7, 299, 300, 301, n1 - 1, n1, n1 + 1, 1023, 1024, 1500, n2 - 1])
        ix.delete_rows(dead)
        keep = np.setdiff1d(np.arange(n2), dead)
        assert len(ix) == len(keep)
        assert_rows(ix.fetch_rows(np.arange(len(keep))), want[keep], (dtype, "after delete_rows"))
    finally:
        ix.close()


@functools.lru_cache(maxsize=None)
def _chunk_case(dim):
    """N(0, 9) rows that cross the staging chunk by 300, the hard rows of (a) in the 64 rows on either side of the
    boundary, and their normalised reference (shared by the storage types; not to be written to)"""
    boundary = STAGING_BYTES // (dim * 4)
    n = boundary + 300
    rows = np.random.default_rng(dim).standard_normal((n, dim), dtype=np.float32)
    rows *= np.float32(3)
    hard = np.concatenate([V.hard_root_rows(dim, s)[0] for s in (0, -20, 20)])
    pick = np.linspace(0, len(hard) - 1, 128).astype(np.int64)
    rows[boundary - 64:boundary + 64] = hard[pick]
    want = V.normalize_rows(rows)
    rows.setflags(write=False)
    want.setflags(write=False)
    return boundary, rows, want


@pytest.mark.parametrize("dim,dtype", [(768, "f32"), (768, "f16"), (100, "f32")])
def test_upload_normalize_across_the_staging_chunk(rlr, oracle, dim, dtype):
    """one upload that ingest() splits: every row of both chunks against the vectorised reference (held to the oracle by
    test_ingest_vectors_cpu.py)"""
    boundary, rows, want = _chunk_case(dim)
    assert boundary == {768: 21845, 100: 167772}[dim] and len(rows) == boundary + 300
    # the reference is the oracle's on the rows around the boundary
    edge = slice(boundary - 70, boundary + 70)
    assert np.array_equal(bits(V.oracle_rows(oracle, rows[edge])), bits(want[edge]))
    if dtype == "f16":
        want = oracle.round_f16(want)
    ix = rlr.GpuIndex(dim, dtype)
    try:
        ix.upload(rows, normalize=True)
        assert len(ix) == len(rows)
        assert_rows(ix.fetch_rows(np.arange(len(rows))), want, (dim, dtype))
    finally:
        ix.close()


@pytest.mark.parametrize("n,dim,dtype,n_clusters", [(20000, 96, "f32", 0), (20000, 96, "f32", 5),
                                                    (5000, 1024, "f16", 0), (5000, 1024, "f16", 5)])
def test_fill_synthetic_at_more_norms(rlr, oracle, n, dim, dtype, n_clusters):
    """the generator's rows go through the same ref_scale: 25 000 more roots than the 900 of the parity test"""
    ix = rlr.GpuIndex(dim, dtype)
    try:
        ix.fill_synthetic(n, seed=77, row0=12345, n_clusters=n_clusters)
        want = oracle.synth_rows(n, dim, seed=77, row0=12345, n_clusters=n_clusters, f16=(dtype == "f16"))
        assert_rows(ix.fetch_rows(np.arange(n)), want, (n, dim, dtype, n_clusters))
    finally:
        ix.close()


def test_multi_shard_upload_normalize(rlr, oracle):
    """rlr_multi_upload(normalize_on_device=1) over three shards of one device, a row count that is no multiple of 3"""
    dim = 768
    hard = V.corpus(dim, edges=False)
    n_extra = 500 + int((len(hard) + 500) % 3 == 0)
    extra = (np.random.default_rng(53).standard_normal((n_extra, dim)) * 3).astype(np.float32)
    rows = np.concatenate([hard, extra])
    assert len(rows) % 3 != 0
    want = np.concatenate([_expected(dim, False, edges=False), V.oracle_rows(oracle, rows[len(hard):])])
    mi = rlr.MultiGpuIndex(dim, [0, 0, 0], "f32")
    try:
        mi.upload(rows, normalize=True)
        assert len(mi) == len(rows)
        assert_rows(mi.fetch_rows(np.arange(len(rows))), want, "three shards")
        for seed in (4201, 4202):
            q = oracle.normalize(oracle.synth_query(dim, seed=seed))
            r, c = mi.search_topk(q, 300)
            wr, wc = V.ranking(oracle.scan(want, q), 300)
            assert np.array_equal(r[0], wr), (seed, r[0][:8], wr[:8])
            assert np.array_equal(canon(c[0]), canon(wc)), seed
    finally:
        mi.close()


def test_host_normalize_hard_vectors(rlr, oracle):
    """rlr.normalize (the engine normalises queries with it) on (a) and (c)"""
    for dim in (8, 768, 3, 101):
        rows = V.corpus(dim)
        got = np.stack([rlr.normalize(r) for r in rows])
        assert_rows(got, _expected(dim, False), ("host", dim))
