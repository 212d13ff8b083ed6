"""The exchange step's merge kernel (rlr_merge_topk) on what 1..16 ranks deliver: every vector of merge_vectors.py -- all
k output slots and the counts, bit for bit against the numpy reference merge that test_merge_vectors_cpu.py holds to the
torch merge -- the argument rejections, and the packed lists of real searches over 16 shards on the one GPU."""
import ctypes as C

import numpy as np
import pytest

import merge_vectors as V
from conftest import bits

pytestmark = pytest.mark.gpu

RLR_OK, RLR_E_INVALID = 0, -1
SENTINEL_ROW, SENTINEL_BITS, SENTINEL_N = 0x1234567812345678, 0x5A5A5A5A, 0x0BADF00D


def merge(rlr, gathered_t, world, nq, k, bases, stream=None):
    """rlr_merge_topk over a device tensor; outputs pre-set to sentinels so that an untouched slot shows"""
    rows = np.full((max(nq, 1), max(k, 1)), SENTINEL_ROW, np.uint64)
    cos = np.full((max(nq, 1), max(k, 1)), SENTINEL_BITS, np.uint32)
    n = np.full(max(nq, 1), SENTINEL_N, np.uint32)
    bases = np.ascontiguousarray(bases, dtype=np.uint64)
    st = rlr.lib().rlr_merge_topk(0, C.c_void_p(gathered_t.data_ptr()), world, nq, k, bases.ctypes.data_as(C.POINTER(C.c_uint64)),
                                  rows.ctypes.data_as(C.POINTER(C.c_uint64)), cos.ctypes.data_as(C.POINTER(C.c_float)),
                                  n.ctypes.data_as(C.POINTER(C.c_uint32)), C.c_void_p(stream) if stream else None)
    return st, rows, cos, n


def untouched(rows, cos, n):
    return (rows == SENTINEL_ROW).all() and (cos == SENTINEL_BITS).all() and (n == SENTINEL_N).all()


@pytest.mark.parametrize("world,k", V.SHAPES)
def test_merge_kernel_on_every_vector(rlr, world, k):
    import torch
    side = torch.cuda.Stream()
    for nq in V.NQS:
        for variant in V.VARIANTS:
            if variant == "marker" and nq != 5:
                continue
            g, bases = V.make_vector(world, k, nq, variant)
            want_rows, want_bits, want_n, defined = V.expected(world, k, nq, variant)
            g_t = torch.from_numpy(g.view(np.int64)).cuda()
            torch.cuda.synchronize()
            for stream in (None, side.cuda_stream):
                st, rows, cos, n = merge(rlr, g_t, world, nq, k, bases, stream)
                where = (world, k, nq, variant, "null stream" if stream is None else "side stream")
                assert st == RLR_OK, where
                assert np.array_equal(n, want_n), (where, n, want_n)
                for q in range(nq):
                    if not defined[q]:
                        continue
                    assert np.array_equal(rows[q], want_rows[q]), (where, q)
                    assert np.array_equal(cos[q], want_bits[q]), (where, q)


def test_merge_rejections_leave_the_outputs_untouched(rlr):
    import torch
    g_t = torch.zeros(16 * 2 * 513, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    ok16 = np.arange(16, dtype=np.uint64) * 1000
    for world, nq, k, bases in ((0, 1, 4, ok16), (17, 1, 4, np.arange(17, dtype=np.uint64)), (1, 1, 8193, ok16), (3, 1, 2731, ok16),
                                (16, 2, 513, ok16), (2, 2, 4, [0, 2 ** 32 - 1]), (2, 2, 4, [2 ** 32 - 1, 0]), (1, 1, 4, [2 ** 40])):
        st, rows, cos, n = merge(rlr, g_t, world, nq, k, bases)
        assert st == RLR_E_INVALID, (world, nq, k)
        assert untouched(rows, cos, n), (world, nq, k)
    for world, nq, k in ((4, 0, 4), (4, 2, 0), (0, 0, 0), (17, 3, 0)):           # nothing to do: RLR_OK, nothing written
        st, rows, cos, n = merge(rlr, g_t, world, nq, k, ok16)
        assert st == RLR_OK and untouched(rows, cos, n), (world, nq, k)
    for world, k, bases in ((16, 512, ok16), (1, 8192, [2 ** 32 - 2])):           # the limits themselves are accepted
        st, rows, cos, n = merge(rlr, g_t, world, 2, k, bases)
        assert st == RLR_OK and (n == 0).all() and (rows == V.PAD_ROW).all() and (cos == V.PAD_BITS).all()


def test_rows_of_negative_zeros_score_plus_zero(rlr):
    """the merge vectors hold no -0.0 score because no search can emit one: the reference sum starts at +0.0, and +0.0 +
    (-0.0) is +0.0.  Rows of -0.0 elements against a positive query, every pipeline, host and packed results."""
    import torch
    dim, n, k = 128, 40, 10
    rows = np.full((n, dim), -0.0, np.float32)
    assert np.signbit(rows).all()
    for dtype in ("f32", "f16"):
        ix = rlr.GpuIndex(dim, dtype)
        ix.upload(rows)
        assert np.array_equal(bits(ix.fetch_rows(np.arange(n))), np.full((n, dim), 0x80000000, np.uint32))
        for nq in (1, 3, 16):
            qs = np.abs(np.random.default_rng(nq).standard_normal((nq, dim))).astype(np.float32) + np.float32(0.01)
            qs /= np.linalg.norm(qs, axis=1, keepdims=True).astype(np.float32)
            r, c = ix.search_topk(qs, k)
            assert np.array_equal(r, np.tile(np.arange(k, dtype=np.uint64), (nq, 1))), (dtype, nq)
            assert (bits(c) == 0).all(), (dtype, nq, bits(c))
            out = torch.zeros((nq, k), dtype=torch.int64, device="cuda")
            ix.search_topk_device(qs, k, out.data_ptr())
            torch.cuda.synchronize()
            assert np.array_equal(out.cpu().numpy().view(np.uint64), np.tile(V.pack(np.zeros(k, np.float32), np.arange(k)), (nq, 1)))
        assert (bits(ix.score_rows(qs[0], np.arange(n))) == 0).all()
        ix.close()


# ---------------------------------------------------------------- real searches, 16 shards on the one GPU
E2E_SHARDS, E2E_ROWS, E2E_DIM, E2E_K, E2E_SMALL = 16, 4100, 128, 512, (5, 30)


@pytest.fixture(scope="module")
def e2e_corpus(oracle):
    """16 shards of 4100 rows (binary16-representable copy for the binary16 index), a cross-shard duplicate of row 11, and
    16 queries; query 0 is row 11 itself"""
    n = E2E_SHARDS * E2E_ROWS
    rows = oracle.synth_rows(n, E2E_DIM, seed=9100, n_clusters=12)
    rows[3 * E2E_ROWS + 7] = rows[11]
    qs = np.stack([oracle.normalize(rows[11])] + [oracle.normalize(oracle.synth_query(E2E_DIM, seed=9200 + i)) for i in range(15)])
    out = {}
    for dtype in ("f32", "f16"):
        stored = rows if dtype == "f32" else oracle.round_f16(rows)
        out[dtype] = (stored, np.stack([oracle.scan(stored, q) for q in qs]))
    return qs, out


def ranking(e, k):
    """(score desc, NaN last, row asc) -> (rows, scores) of the k best"""
    key = np.where(np.isnan(e), -np.inf, e).astype(np.float64)
    order = np.lexsort((np.arange(len(e)), -key))[:k]
    return order.astype(np.uint64), e[order]


@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_sixteen_shards_searched_and_merged(rlr, e2e_corpus, dtype):
    import torch
    qs_all, per_dtype = e2e_corpus
    stored, e_all = per_dtype[dtype]
    k, world = E2E_K, E2E_SHARDS
    shards = []
    for r in range(world):
        ix = rlr.GpuIndex(E2E_DIM, dtype)
        ix.upload(stored[r * E2E_ROWS:(r + 1) * E2E_ROWS])
        shards.append(ix)
    small = rlr.GpuIndex(E2E_DIM, dtype)                        # shard 5 cut to 30 rows: k exceeds the rows, zero tails
    small.upload(stored[E2E_SMALL[0] * E2E_ROWS:E2E_SMALL[0] * E2E_ROWS + E2E_SMALL[1]])
    try:
        for small_shard in (False, True):
            sizes = np.full(world, E2E_ROWS, np.int64)
            if small_shard:
                sizes[E2E_SMALL[0]] = E2E_SMALL[1]
            bases = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.uint64)
            keep = np.concatenate([np.arange(r * E2E_ROWS, r * E2E_ROWS + sizes[r]) for r in range(world)])
            for nq in (1, 3, 16):                              # the single, shared-scan and batched pipelines
                qs = qs_all[:nq]
                gathered = torch.zeros((world, nq, k), dtype=torch.int64, device="cuda")
                for r in range(world):
                    ix = small if (small_shard and r == E2E_SMALL[0]) else shards[r]
                    ix.search_topk_device(qs, k, gathered[r].data_ptr())
                torch.cuda.synchronize()
                g = gathered.cpu().numpy().view(np.uint64)
                for r in range(world):
                    for q in range(nq):
                        lr, ls = ranking(e_all[q, r * E2E_ROWS:r * E2E_ROWS + sizes[r]], k)
                        want = np.zeros(k, np.uint64)
                        want[:lr.size] = V.pack(ls, lr)
                        assert np.array_equal(g[r, q], want), (dtype, small_shard, nq, r, q)
                st, rows, cos, n = merge(rlr, gathered, world, nq, k, bases)
                assert st == RLR_OK and (n == k).all()
                for q in range(nq):
                    wr, ws = ranking(e_all[q][keep], k)
                    assert np.array_equal(rows[q], wr), (dtype, small_shard, nq, q)
                    assert np.array_equal(cos[q], bits(ws)), (dtype, small_shard, nq, q)
                if not small_shard:
                    assert list(rows[0][:2]) == [11, 3 * E2E_ROWS + 7]      # the duplicate: lower global row first
    finally:
        for ix in shards + [small]:
            ix.close()
