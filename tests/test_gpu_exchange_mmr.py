"""The device code of the cross-shard MMR exchange at the shapes several GPUs produce, on one: the LDS greedy loop behind
single pools of 1025..4096 candidates, both ends of the winner-row exchange (rlr_gather_rows_device ->
rlr_mmr_select_staged) over matrices the tests build themselves, the second pass of the batched implementation's chunk
loop, and rlr_multi_mmr_select* with several shards on the one device.  Everything bit for bit against oracle.mmr (the
full drains against its Gram-based restatement, which test_mmr_restatement_cpu.py pins to it)."""
import importlib
import time

import numpy as np
import pytest

import mmr_restatement as R
from conftest import bits

pytestmark = pytest.mark.gpu

N = importlib.import_module("rust-local-rag_amd._native")


def make_index(rlr, rows, dtype="f32"):
    ix = rlr.GpuIndex(rows.shape[1], dtype)
    ix.upload(rows)
    return ix


def stored_rows(oracle, rows, dtype):
    return oracle.round_f16(rows) if dtype == "f16" else rows


def check_pool(oracle, emb, sc, k, lam, order, mmr, where):
    wo, wm = oracle.mmr(emb, sc, k, lam)
    assert np.array_equal(order, wo), where
    assert np.array_equal(bits(mmr[1:]), bits(wm[1:])), where


# ---------------------------------------------------------------- a. large single pools: mmr_greedy_kernel
_POOLS = {}


def big_pool(oracle, P, dim):
    """(f32 rows, pool) shared by the dtypes and lambdas of one (P, dim): duplicated rows inside the pool"""
    if (P, dim) not in _POOLS:
        rows = oracle.synth_rows(P + 50, dim, seed=7100 + P + dim, n_clusters=6)
        rows[10:20] = rows[3]
        pool = np.random.default_rng([P, dim]).permutation(P + 50)[:P].astype(np.uint64)
        assert np.isin(np.arange(10, 20), pool).sum() >= 2
        _POOLS[(P, dim)] = (rows, pool)
    return _POOLS[(P, dim)]


@pytest.mark.parametrize("dtype", ["f32", "f16"])
@pytest.mark.parametrize("dim", [96, 70])
@pytest.mark.parametrize("P", [1025, 1088, 2048, 2049, 4095, 4096])
def test_mmr_single_pool_of_1025_to_4096(rlr, oracle, P, dim, dtype):
    """every lambda regime over the LDS greedy loop and the 32 x 32-tile Gram behind it (dim 70: its scalar dim % 4 path);
    k <= 100 (<= 64 above 2048 candidates) keeps the oracle's literal loop near a second per case"""
    rows, pool = big_pool(oracle, P, dim)
    stored = stored_rows(oracle, rows, dtype)
    emb = stored[pool.astype(np.int64)]
    ix = make_index(rlr, stored, dtype)
    rng = np.random.default_rng([P, dim, dtype == "f16"])
    try:
        for lam, kk in ((0.3, 100 if P <= 2049 else 64), (0.0, 40), (1.0, 25)):
            sc = R.awkward_scores(rng, P)
            o, m = ix.mmr_select(pool, sc, kk, lam)
            assert len(o) == kk
            check_pool(oracle, emb, sc, kk, lam, o, m, (P, dim, dtype, lam, kk))
    finally:
        ix.close()


@pytest.mark.parametrize("P,dtype,nonfinite", [(1025, "f16", False), (4096, "f32", True)])
def test_mmr_single_pool_full_drain(rlr, oracle, P, dtype, nonfinite):
    """k = P: the loop runs until `remaining` is empty (finite relevance throughout) or until no finite candidate is left"""
    dim = 96
    rows, pool = big_pool(oracle, P, dim)
    stored = stored_rows(oracle, rows, dtype)
    sc = R.awkward_scores(np.random.default_rng(P), P, nonfinite)
    wo, wm = R.mmr_from_gram(R.gram(oracle, stored[pool.astype(np.int64)]), sc, P, 0.3)
    assert (len(wo) == P) == (not nonfinite) and len(wo) >= P - 4
    ix = make_index(rlr, stored, dtype)
    try:
        t0 = time.perf_counter()
        o, m = ix.mmr_select(pool, sc, P, 0.3)
        print("full drain P=%d %s: %.2f s on the device" % (P, dtype, time.perf_counter() - t0))
        assert np.array_equal(o, wo)
        assert np.array_equal(bits(m[1:]), bits(wm[1:]))
    finally:
        ix.close()


def test_mmr_single_pool_of_4097_is_refused(rlr, oracle):
    ix = make_index(rlr, oracle.synth_rows(64, 8, seed=1))
    try:
        with pytest.raises(N.RlrError) as e:
            ix.mmr_select(np.zeros(4097, np.uint64), np.zeros(4097, np.float32), 5, 0.3)
        assert e.value.status == N.RLR_E_INVALID
    finally:
        ix.close()


# ---------------------------------------------------------------- b. the two row gathers
def device_filled(torch, shape, dtype, bits_value):
    """a device tensor pre-set to a pattern no row holds (copied from the host: no fill kernel of torch's to load)"""
    return torch.from_numpy(np.full(shape, bits_value, dtype=dtype)).cuda()


def row_lists(rng, n_rows):
    """lengths 1, 255, 256, 257: repeats, reversed order, first and last row"""
    yield np.array([n_rows - 1], np.uint64)
    yield np.array([0], np.uint64)
    yield np.arange(n_rows - 1, n_rows - 256, -1).astype(np.uint64)                                  # 255, reversed
    yield np.concatenate([[0, n_rows - 1, 0, n_rows - 1], rng.integers(0, n_rows, 252)]).astype(np.uint64)   # 256, repeats
    yield np.concatenate([rng.permutation(n_rows)[:255], [n_rows - 1, 0]]).astype(np.uint64)       # 257


def check_gathers(rlr, torch, ix, want, lists):
    dim, dtype = ix.dim, ix.dtype
    esize = 4 if dtype == "f32" else 2
    rb = ix.row_bytes()
    assert rb == (dim * esize + 15) // 16 * 16
    for rows in lists:
        n = rows.size
        host = ix.fetch_rows(rows)
        assert np.array_equal(bits(host), bits(want[rows.astype(np.int64)])), (dim, dtype, n)
        raw = device_filled(torch, n * rb, np.uint8, 0xA5)
        dense = device_filled(torch, (n, dim), np.int32, 0x7FC00000)
        torch.cuda.synchronize()
        ix.gather_rows_device(rows, raw.data_ptr())
        ix.fetch_rows_device(rows, dense.data_ptr())
        assert np.array_equal(dense.cpu().numpy().view(np.uint32), bits(host)), (dim, dtype, n)
        got = raw.cpu().numpy().reshape(n, rb)[:, :dim * esize]
        if dtype == "f32":
            assert np.array_equal(np.ascontiguousarray(got).view(np.uint32), bits(host)), (dim, dtype, n)
        else:
            halves = np.ascontiguousarray(got).view(np.float16)
            assert np.array_equal(bits(halves.astype(np.float32)), bits(host)), (dim, dtype, n)
            assert np.array_equal(np.ascontiguousarray(got).view(np.uint16),
                                  host.astype(np.float16).view(np.uint16)), (dim, dtype, n)    # as stored


@pytest.mark.parametrize("dtype,dim", [("f32", 3), ("f32", 5), ("f32", 96), ("f32", 770),
                                       ("f16", 7), ("f16", 72), ("f16", 200), ("f16", 768), ("f16", 1026)])
def test_row_gathers_at_padded_pitches(rlr, oracle, dtype, dim):
    import torch
    n_rows = 700
    rows = oracle.synth_rows(n_rows, dim, seed=8200 + dim)
    rows[0, 0], rows[n_rows - 1, dim - 1] = -0.0, 6.0e-8                     # a sign bit and a binary16 subnormal at the corners
    want = stored_rows(oracle, rows, dtype)
    ix = make_index(rlr, rows, dtype)
    try:
        check_gathers(rlr, torch, ix, want, row_lists(np.random.default_rng(dim), n_rows))
    finally:
        ix.close()


def test_row_gathers_beyond_one_grid(rlr, oracle):
    """6000 rows of 768-d f32: more 16-byte units (and more elements) than the 4096 x 256 threads of the capped grid, so
    the kernels' grid-stride loops take further turns"""
    import torch
    n_rows, dim, n = 300, 768, 6000
    rows = oracle.synth_rows(n_rows, dim, seed=8300)
    ix = make_index(rlr, rows)
    assert n * (ix.row_bytes() // 16) > 4096 * 256
    lst = np.random.default_rng(6).integers(0, n_rows, n).astype(np.uint64)
    lst[:2], lst[-2:] = [0, n_rows - 1], [n_rows - 1, 0]
    try:
        check_gathers(rlr, torch, ix, rows, [lst])
    finally:
        ix.close()


# ---------------------------------------------------------------- c. rlr_mmr_select_staged over a matrix built here
def stage(torch, stored, dtype, row_bytes):
    """the rows at `row_bytes` pitch in device memory, every pad element a NaN: no sum may read one"""
    n, dim = stored.shape
    if dtype == "f32":
        m = np.full((n, row_bytes // 4), 0x7FC00000, np.uint32)
        m[:, :dim] = bits(stored)
    else:
        m = np.full((n, row_bytes // 2), 0x7E00, np.uint16)
        m[:, :dim] = stored.astype(np.float16).view(np.uint16)
        assert np.array_equal(bits(m[:, :dim].view(np.float16).astype(np.float32)), bits(stored))
    t = torch.from_numpy(m.view(np.uint8).reshape(-1)).cuda()
    torch.cuda.synchronize()
    return t


def staged_setup(rlr, oracle, torch, dim, dtype, n_staged, seed):
    rows = oracle.synth_rows(n_staged, dim, seed=seed, n_clusters=5)
    rows[7:12] = rows[2]
    stored = stored_rows(oracle, rows, dtype)
    ix = make_index(rlr, stored, dtype)                      # the same rows in an index: rlr_mmr_select_batch must agree
    mat = stage(torch, stored, dtype, ix.row_bytes())
    return stored, ix, mat


@pytest.mark.parametrize("dtype", ["f32", "f16"])
@pytest.mark.parametrize("dim,P,k", [(70, 300, 60), (768, 200, 24)])
@pytest.mark.parametrize("nq", [3, 9, 20])
def test_mmr_staged_batches(rlr, oracle, nq, dim, P, k, dtype):
    """3 / 9 / 20 pools: each Gram tile shape, and at 20 binary16 pools the matrix-core Gram, over the staged matrix"""
    import torch
    n_staged, lam = 500, 0.3
    stored, ix, mat = staged_setup(rlr, oracle, torch, dim, dtype, n_staged, 8400 + dim)
    rng = np.random.default_rng([nq, dim, dtype == "f16"])
    slots = rng.integers(0, n_staged, (nq, P)).astype(np.uint64)             # repeats inside a pool
    slots[1] = rng.permutation(n_staged)[:P]                                 # a permutation
    slots[2, : P // 2] = slots[2, P // 2: 2 * (P // 2)]                      # every row of the first half twice
    slots[0, :2] = [n_staged - 1, 0]
    sizes = np.full(nq, P, np.uint32)
    sizes[0], sizes[2] = P - 1, 2 * (P // 2)
    if nq > 3:
        sizes[3], sizes[4], sizes[5], sizes[nq - 1] = 0, 1, 17, P - 3
    sc = np.stack([R.awkward_scores(rng, P) for _ in range(nq)])
    try:
        order, mmr, n = ix.mmr_select_staged(mat.data_ptr(), n_staged, slots, sc, sizes, k, lam)
        ob, mb, nb = ix.mmr_select_batch(slots, sc, sizes, k, lam)
        assert np.array_equal(n, nb)
        for q in range(nq):
            s = int(sizes[q])
            if s == 0:
                assert n[q] == 0, q
                continue
            emb = stored[slots[q, :s].astype(np.int64)]
            check_pool(oracle, emb, sc[q, :s], k, lam, order[q, : n[q]], mmr[q, : n[q]], (nq, dim, dtype, q))
            assert np.array_equal(order[q, : n[q]], ob[q, : nb[q]]) and np.array_equal(bits(mmr[q, 1: n[q]]), bits(mb[q, 1: nb[q]]))
    finally:
        ix.close()


@pytest.mark.parametrize("dtype", ["f32", "f16"])
@pytest.mark.parametrize("size,P", [(1500, 1500), (4096, 4096), (800, 2048)])
def test_mmr_staged_single_pool(rlr, oracle, size, P, dtype):
    """n_queries == 1: pools of 1025..4096 slots take the single-pool kernels over the staged matrix, and so does a small
    pool in a slot list wider than 1024 -- one pool does not use the stride P"""
    import torch
    dim, n_staged, k, lam = 70, 2500, 40, 0.3
    stored, ix, mat = staged_setup(rlr, oracle, torch, dim, dtype, n_staged, 8500)
    rng = np.random.default_rng([size, P, dtype == "f16"])
    slots = rng.integers(0, n_staged, (1, P)).astype(np.uint64)
    slots[0, :2] = [n_staged - 1, 0]
    slots[0, size:] = n_staged + 5                          # beyond the pool: never looked at, whatever they hold
    sc = R.awkward_scores(rng, P)[None, :]
    try:
        order, mmr, n = ix.mmr_select_staged(mat.data_ptr(), n_staged, slots, sc, [size], k, lam)
        assert n[0] == k
        emb = stored[slots[0, :size].astype(np.int64)]
        check_pool(oracle, emb, sc[0, :size], k, lam, order[0, :k], mmr[0, :k], (size, P, dtype))
        if size <= 1024:
            ob, mb, nb = ix.mmr_select_batch(slots[:, :size], sc[:, :size], [size], k, lam)
        else:
            ob, mb = ix.mmr_select(slots[0, :size], sc[0, :size], k, lam)
            ob, mb, nb = ob[None, :], mb[None, :], [len(ob)]
        assert nb[0] == k and np.array_equal(ob[0, :k], order[0, :k]) and np.array_equal(bits(mb[0, 1:k]), bits(mmr[0, 1:k]))
    finally:
        ix.close()


def test_mmr_staged_refusals(rlr, oracle):
    import torch
    dim, n_staged = 70, 100
    stored, ix, mat = staged_setup(rlr, oracle, torch, dim, "f16", n_staged, 8600)
    rng = np.random.default_rng(3)
    try:
        for nq, P, sizes in ((4, 50, [50, 50, 50, 50]), (1, 2000, [2000]), (1, 2048, [800])):
            slots = rng.integers(0, n_staged, (nq, P)).astype(np.uint64)
            slots[nq - 1, sizes[-1] - 1] = n_staged                      # one slot past the matrix, inside the pool
            with pytest.raises(N.RlrError) as e:
                ix.mmr_select_staged(mat.data_ptr(), n_staged, slots, np.zeros((nq, P), np.float32), sizes, 5, 0.3)
            assert e.value.status == N.RLR_E_RANGE, (nq, P)
        for nq, P, sizes in ((1, 2048, [2049]), (2, 2048, [800, 800]), (1, 4097, [4097]), (3, 50, [50, 51, 50])):
            slots = rng.integers(0, n_staged, (nq, P)).astype(np.uint64)
            with pytest.raises(N.RlrError) as e:
                ix.mmr_select_staged(mat.data_ptr(), n_staged, slots, np.zeros((nq, P), np.float32), sizes, 5, 0.3)
            assert e.value.status == N.RLR_E_INVALID, (nq, P)
    finally:
        ix.close()


# ---------------------------------------------------------------- d. two passes of the batched implementation
TWO_PASS = dict(nq=770, P=1024, dim=8, k=5, lam=0.5, n_rows=3000)


@pytest.fixture(scope="module")
def two_pass_case(oracle):
    """770 pools of up to 1024: 765 fit the 3 GB workspace of one pass, so a second pass of 5 follows (its own Gram tile);
    ragged sizes, pools 764..769 -- either side of the seam -- all different"""
    c = TWO_PASS
    nq, P = c["nq"], c["P"]
    rows = oracle.synth_rows(c["n_rows"], c["dim"], seed=8700, n_clusters=7)
    rng = np.random.default_rng(87)
    pools = np.stack([rng.permutation(c["n_rows"])[:P] for _ in range(nq)]).astype(np.uint64)
    sizes = np.full(nq, P, np.uint32)
    sizes[[0, 1, 2, 400]] = [1000, 0, 1, 513]
    sizes[764:770] = [1024, 1001, 977, 64, 1023, 500]
    sc = (rng.standard_normal((nq, P)) * 0.2).astype(np.float32)
    sc[:, 5] = sc[:, 9]
    sc[765, 3], sc[768, 4], sc[3, 6] = np.nan, np.inf, -0.0
    t0 = time.perf_counter()
    want = [oracle.mmr(rows[pools[q, :sizes[q]].astype(np.int64)], sc[q, :sizes[q]], c["k"], c["lam"]) for q in range(nq)]
    print("oracle, 770 pools: %.2f s" % (time.perf_counter() - t0))
    return rows, pools, sizes, sc, want


@pytest.mark.parametrize("form", ["batch", "values", "staged"])
def test_mmr_batch_second_pass(rlr, two_pass_case, form):
    import torch
    c = TWO_PASS
    rows, pools, sizes, sc, want = two_pass_case
    nq, P, k, lam = c["nq"], c["P"], c["k"], c["lam"]
    ix = make_index(rlr, rows)
    t0 = time.perf_counter()
    try:
        if form == "batch":
            order, mmr, n = ix.mmr_select_batch(pools, sc, sizes, k, lam)
        elif form == "values":
            vals = device_filled(torch, (nq * P, c["dim"]), np.int32, 0x7FC00000)
            torch.cuda.synchronize()
            ix.fetch_rows_device(pools.ravel(), vals.data_ptr())
            order, mmr, n = ix.mmr_select_values(vals.data_ptr(), sc, sizes, k, lam)
            del vals
        else:
            mat = stage(torch, rows, "f32", ix.row_bytes())
            order, mmr, n = ix.mmr_select_staged(mat.data_ptr(), rows.shape[0], pools, sc, sizes, k, lam)
    finally:
        ix.close()                                          # (the ~3 GB workspace goes with it)
        torch.cuda.empty_cache()
    print("nq = 770 through %s: %.2f s" % (form, time.perf_counter() - t0))
    for q in range(nq):
        wo, wm = want[q]
        assert n[q] == len(wo), (form, q, n[q], len(wo))
        assert np.array_equal(order[q, : n[q]], wo), (form, q)
        assert np.array_equal(bits(mmr[q, 1: n[q]]), bits(wm[1:])), (form, q)


# ---------------------------------------------------------------- e. rlr_multi_mmr_select* with the shards on one GPU
MULTI_ROWS, MULTI_DIM = 21000, 70


@pytest.fixture(scope="module")
def multi_corpus(oracle):
    rows = oracle.synth_rows(MULTI_ROWS, MULTI_DIM, seed=8800, n_clusters=9)
    rows[15:20] = rows[MULTI_ROWS - 3]                       # duplicates on the first and the last shard
    return rows


@pytest.mark.parametrize("n_shards", [3, 5])
def test_multi_mmr_one_large_pool(rlr, oracle, multi_corpus, n_shards):
    """one pool of 4096 global rows: spread over all shards, then wholly on the last one (the owner, shard 0, holds none)"""
    rows = multi_corpus
    P, k, lam = 4096, 40, 0.3
    mi = rlr.MultiGpuIndex(MULTI_DIM, [0] * n_shards)
    mi.upload(rows)
    rng = np.random.default_rng(n_shards)
    per = (MULTI_ROWS + n_shards - 1) // n_shards
    last0 = per * (n_shards - 1)
    assert MULTI_ROWS - last0 >= P
    spanning = rng.permutation(MULTI_ROWS)[:P].astype(np.uint64)
    spanning[:4] = [MULTI_ROWS - 3, 15, 0, MULTI_ROWS - 1]
    assert len(set((spanning // per).tolist())) == n_shards
    on_last = (last0 + rng.permutation(MULTI_ROWS - last0)[:P]).astype(np.uint64)
    try:
        assert np.array_equal(bits(mi.fetch_rows(on_last[:50])), bits(rows[on_last[:50].astype(np.int64)]))
        for name, pool in (("spanning", spanning), ("last shard", on_last)):
            sc = R.awkward_scores(rng, P)
            o, m = mi.mmr_select(pool, sc, k, lam)
            assert len(o) == k
            check_pool(oracle, rows[pool.astype(np.int64)], sc, k, lam, o, m, (n_shards, name))
        st = mi.stats()
        assert st["n_mmr_exchanges"] == 2 and st["n_mmr_host_bounces"] == 0, st
    finally:
        mi.close()


def test_multi_mmr_binary16_batch_of_sixty(rlr, oracle, multi_corpus):
    """60 pools of 300 over three shards: 20 per owner, so each owner's matrix-core Gram runs over its receive buffer"""
    stored = oracle.round_f16(multi_corpus)
    nq, P, k, lam = 60, 300, 30, 0.3
    mi = rlr.MultiGpuIndex(MULTI_DIM, [0, 0, 0], "f16")
    mi.upload(stored)
    rng = np.random.default_rng(60)
    pools = np.stack([rng.permutation(MULTI_ROWS)[:P] for _ in range(nq)]).astype(np.uint64)
    pools[0, :3] = [MULTI_ROWS - 3, 15, 16]
    sizes = np.full(nq, P, np.uint32)
    sizes[[4, 5, 6, 7]] = [0, 1, 33, 299]
    sc = np.stack([R.awkward_scores(rng, P) for _ in range(nq)])
    try:
        order, mmr, n = mi.mmr_select_batch(pools, sc, sizes, k, lam)
        for q in range(nq):
            s = int(sizes[q])
            if s == 0:
                assert n[q] == 0, q
            else:
                check_pool(oracle, stored[pools[q, :s].astype(np.int64)], sc[q, :s], k, lam, order[q, : n[q]], mmr[q, : n[q]], q)
        st = mi.stats()
        assert st["n_mmr_exchanges"] == 1 and st["n_mmr_host_bounces"] == 0, st
    finally:
        mi.close()
