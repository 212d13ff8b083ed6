"""Every branch of the greedy MMR chain, mmr_greedy_lazy_kernel<J> (J = 1, 2, 5, 8, 16) and mmr_greedy_kernel (csrc/exact.hip),
on the designed pools of tests/greedy_vectors.py: every (lane, register slot) as a lone winner and as the winner of a tie
that position decides against the index, ties of 2 / 3 / 64+ holders and replays that start from earlier ones, zeros of both
signs, the floor of the running maximum, the overflow recount (lambda outside [0, 1]), every way the loop ends, and ragged
batches.  test_greedy_vectors_cpu.py proves that the pools reach those states and that the rows' Gram matrix is exact in any
order and storage, so a difference here is the chain's.  Picks, count and logged bits must equal the traced restatement's;
element 0 of the logged values is NaN on both sides."""
import functools
import importlib

import numpy as np
import pytest

import greedy_vectors as V
from conftest import bits

pytestmark = pytest.mark.gpu
N = importlib.import_module("rust-local-rag_amd._native")
DTYPES = ("f32", "f16")


@functools.lru_cache(maxsize=None)
def want(name, P):
    """(plan, (order, logged, n), traces): computed once per process and shared by every test of the plan"""
    pl, g = V.plan(name, P), V.corpus_gram()
    traces = V.trace_plan(pl, g)
    exp = V.expected(pl, g, traces)
    for a in exp:
        a.setflags(write=False)
    return pl, exp, traces


def open_index(rlr, dtype):
    ix = rlr.GpuIndex(V.DIM, dtype)
    ix.upload(V.corpus())
    return ix


def run_batch(pl, call):
    """every (k, lambda) group of the plan in one call(pool_rows, rel, sizes, k, lam) -> (order [Q, W], logged [Q, W], n [Q])"""
    W = V.width(pl)
    order, logged, n = np.zeros((pl.Q, W), np.uint32), np.zeros((pl.Q, W), np.float32), np.zeros(pl.Q, np.uint32)
    for qs, k, lam in pl.calls():
        o, m, c = call(pl.pool_rows[qs], pl.rel[qs], pl.sizes[qs], k, lam)
        assert (c <= W).all(), (pl.name, pl.P, k, c.max())
        order[qs], logged[qs], n[qs] = o[:, :W], m[:, :W], c
    return order, logged, n


def run_single(pl, ix):
    """pool by pool through mmr_select, each pool cut to its size"""
    W = V.width(pl)
    order, logged, n = np.zeros((pl.Q, W), np.uint32), np.zeros((pl.Q, W), np.float32), np.zeros(pl.Q, np.uint32)
    for q in range(pl.Q):
        s = int(pl.sizes[q])
        o, m = ix.mmr_select(pl.pool_rows[q, :s], pl.rel[q, :s], int(pl.k[q]), float(pl.lam[q]))
        assert o.size <= W
        order[q, : o.size], logged[q, : m.size], n[q] = o, m, o.size
    return order, logged, n


def compare(name, P, got, what):
    pl, (want_order, want_logged, want_n), traces = want(name, P)
    order, logged, n = got
    col = np.arange(want_order.shape[1])[None, :]
    live = col < want_n[:, None]                                   # columns beyond a pool's count hold nothing
    bad = (n != want_n) | ((order != want_order) & live).any(axis=1)
    bad |= ((bits(logged) != bits(want_logged)) & live)[:, 1:].any(axis=1)
    bad |= (want_n > 0) & ~np.isnan(np.where(want_n > 0, logged[:, 0], np.nan))
    if bad.any():
        lines = []
        for q in np.flatnonzero(bad)[:12]:
            lines.append(f"{V.describe(pl, q, traces[q][2])}: picks {order[q, : n[q]].tolist()} want "
                         f"{want_order[q, : want_n[q]].tolist()}, logged {[hex(x) for x in bits(logged[q, 1: n[q]])]} want "
                         f"{[hex(x) for x in bits(want_logged[q, 1: want_n[q]])]}")
        states = sorted({pl.state[q] for q in np.flatnonzero(bad)})
        raise AssertionError(f"{what}: {int(bad.sum())} of {pl.Q} pools of {name} at stride {P} (J = {V.greedy_j(P)}) differ, "
                             f"states {states}\n" + "\n".join(lines))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("P", V.STRIDES)
@pytest.mark.parametrize("name", V.BATCH_PLANS)
def test_batch(rlr, oracle, name, P, dtype):
    pl = want(name, P)[0]
    ix = open_index(rlr, dtype)
    try:
        compare(name, P, run_batch(pl, ix.mmr_select_batch), ("batch", dtype))
    finally:
        ix.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("P", V.STRIDES + (V.SINGLE,))
@pytest.mark.parametrize("name", V.SINGLE_PLANS)
def test_single_pool(rlr, oracle, name, P, dtype):
    """rlr_mmr_select: the register-resident kernel without `sizes`, and mmr_greedy_kernel at stride 1030"""
    pl = want(name, P)[0]
    ix = open_index(rlr, dtype)
    try:
        compare(name, P, run_single(pl, ix), ("single", dtype))
    finally:
        ix.close()


@pytest.mark.parametrize("P", V.STRIDES)
@pytest.mark.parametrize("source", ["values", "staged"])
def test_values_and_staged(rlr, oracle, source, P):
    """tie_forms of every J over dense f32 values in device memory (rlr_mmr_select_values) and over a staged matrix
    (rlr_mmr_select_staged)"""
    import torch
    rows = V.corpus()
    pl = want("tie_forms", P)[0]
    ix = open_index(rlr, "f32")
    try:
        if source == "staged":
            m = np.full((rows.shape[0], ix.row_bytes() // 4), 0x7FC00000, np.uint32)
            m[:, : rows.shape[1]] = bits(rows)
            mat = torch.from_numpy(m.view(np.uint8).reshape(-1)).cuda()
            torch.cuda.synchronize()

            def call(pool_rows, rel, sizes, k, lam):
                return ix.mmr_select_staged(mat.data_ptr(), rows.shape[0], pool_rows, rel, sizes, k, lam)
        else:
            vals = torch.from_numpy(np.full((pl.Q * P, V.DIM), 0x7FC00000, np.int32)).cuda()
            torch.cuda.synchronize()

            def call(pool_rows, rel, sizes, k, lam):
                ix.fetch_rows_device(pool_rows.ravel(), vals.data_ptr())
                return ix.mmr_select_values(vals.data_ptr(), rel, sizes, k, lam)
        compare("tie_forms", P, run_batch(pl, call), source)
    finally:
        ix.close()


def test_a_batch_of_stride_1025_is_refused_and_writes_nothing(rlr, oracle):
    """include/rlr_gpu.h: pool_sizes[q] <= P <= 1024 for the batch; a bad argument is RLR_E_INVALID"""
    P, Q = 1025, 2
    ix = open_index(rlr, "f32")
    try:
        pool_rows = np.zeros((Q, P), np.uint64)
        rel = np.ones((Q, P), np.float32)
        sizes = np.full(Q, P, np.uint32)
        order = np.full((Q, P), 0xDEADBEEF, np.uint32)
        mmr = np.full((Q, P), -7.0, np.float32)
        n = np.full(Q, 0xDEADBEEF, np.uint32)
        st = ix._L.rlr_mmr_select_batch(ix.handle, pool_rows.ctypes.data_as(N.u64p), rel.ctypes.data_as(N.f32p),
                                        sizes.ctypes.data_as(N.u32p), Q, P, 5, 0.5, order.ctypes.data_as(N.u32p),
                                        mmr.ctypes.data_as(N.f32p), n.ctypes.data_as(N.u32p))
        assert st == N.RLR_E_INVALID
        assert (order == 0xDEADBEEF).all() and (mmr == -7.0).all() and (n == 0xDEADBEEF).all()
        with pytest.raises(N.RlrError) as e:
            ix.mmr_select_batch(pool_rows, rel, sizes, 5, 0.5)
        assert e.value.status == N.RLR_E_INVALID
        o, m = ix.mmr_select(pool_rows[0, :1024], rel[0, :1024], 3, 0.5)   # the index still serves
        assert o.tolist() == [0, 1023, 1022]                              # equal rows and scores: position 0 every time
    finally:
        ix.close()
