"""Every entry of the MMR Gram matrix, read back through the greedy loop and held to the reference-order dot product bit
for bit: gram_tiled_kernel<R, SRC, GK> in its four shapes and three sources and gram_mfma_f32_kernel (csrc/exact.hip).
The matrix never leaves the device; tests/gram_vectors.py builds pools of which each makes the greedy kernel log one entry,
-G[a][b] / 2, exactly (test_gram_vectors_cpu.py proves that, the coverage of every tile class and that the rows tell a
faulty sum from the right one).  Here every pool's picks and logged bits must equal mmr_from_gram's over the oracle's matrix.

Shapes (gram_vectors.SHAPES): the smallest that reach each instance with a full block on both sides of the diagonal where
the rule allows it, a ragged last block, one staged chunk and several, and widths on the scalar path (dim % 4 != 0, and
dim % 8 != 0 for the matrix cores).  Every pool of a call has its own layout of the rows, and every call has exactly the
pool count its instance is chosen by.

A side effect: a and b are winners, so in the plans that read every ordered pair (33, 37, 70, 100 and 130 slots) every
candidate position (lane, register slot j) of mmr_greedy_lazy_kernel<1>, <2> and <5> wins somewhere; <5> and <8> also run at
180 and 325 slots on the sampled blocks, mmr_greedy_kernel at 1030.  No shape here reaches <16> (pools above 512), and the
winners here are always alone at the maximum: every (lane, j) of every J, <16> included, as a lone winner and as the winner
of a tie, and the chain's other branches, are test_gpu_greedy.py's (on the pools of tests/greedy_vectors.py)."""
import numpy as np
import pytest

import gram_vectors as V
import mmr_restatement as R
from conftest import bits

pytestmark = pytest.mark.gpu


def open_index(rlr, rows, dtype):
    ix = rlr.GpuIndex(rows.shape[1], dtype)
    ix.upload(rows)
    return ix


def run(plan, call):
    """the plan's calls through call(pool_rows, rel, sizes, k, lam) -> (order [Q, k], logged [Q, k], n [Q])"""
    order = np.zeros((plan.Q, plan.k), np.uint32)
    logged = np.zeros((plan.Q, plan.k), np.float32)
    n = np.zeros(plan.Q, np.uint32)
    for sl in plan.calls():
        o, m, c = call(plan.pool_rows[sl], plan.rel[sl], plan.sizes[sl], plan.k, plan.lam)
        order[sl], logged[sl], n[sl] = o[:, : plan.k], m[:, : plan.k], c
    return order, logged, n


def single(ix):
    def call(pool_rows, rel, sizes, k, lam):
        o, m = ix.mmr_select(pool_rows[0], rel[0], k, lam)
        order, logged = np.zeros((1, k), np.uint32), np.zeros((1, k), np.float32)
        order[0, : o.size], logged[0, : m.size] = o, m
        return order, logged, [o.size]
    return call


def compare(plan, g, got, what):
    """picks, logged bits and count of every pool against the reference's loop over the reference-order matrix"""
    want_order, want_logged, want_n = V.expected(plan, g)
    order, logged, n = got
    bad = (n != want_n) | (order != want_order).any(axis=1) | (bits(logged[:, 1:]) != bits(want_logged[:, 1:])).any(axis=1)
    if bad.any():
        lines = []
        for q in np.flatnonzero(bad)[:12]:
            a, b = int(plan.a[q]), int(plan.b[q])
            lines.append(f"entry ({a}, {b}) = rows ({plan.pool_rows[q, a]}, {plan.pool_rows[q, b]}), pool {q % plan.pools} of its pass "
                         f"(call {q // plan.pools}, size {plan.sizes[q]}): picks {order[q, : n[q]].tolist()} want "
                         f"{want_order[q, : want_n[q]].tolist()}, logged {[hex(x) for x in bits(logged[q, 1: n[q]])]} want "
                         f"{[hex(x) for x in bits(want_logged[q, 1: want_n[q]])]}")
        a, b = plan.a[bad], plan.b[bad]
        raise AssertionError(f"{what}: {int(bad.sum())} of {plan.Q} pools differ; rows of the entries {np.unique(a)[:40].tolist()}, "
                             f"columns {np.unique(b)[:40].tolist()}\n" + "\n".join(lines))


@pytest.mark.parametrize("name,dim,dtype", V.cases())
def test_every_read_entry_is_the_reference_dot(rlr, oracle, name, dim, dtype):
    s = V.shape(name)
    assert V.gram_instance(dtype, s["pools"], s["P"])[0] == s["instance"]
    rows, g = V.corpus_and_gram(s["P"], dim, dtype == "f16")
    ix = open_index(rlr, rows, dtype)
    try:
        for plan in V.shape_plans(name):
            call = single(ix) if s["pools"] == 1 else ix.mmr_select_batch
            compare(plan, g, run(plan, call), (name, dim, dtype, plan.k))
    finally:
        ix.close()


def stage(torch, ix, stored):
    """the f32 rows at the index' row pitch in device memory, every pad element a NaN: no sum may read one"""
    m = np.full((stored.shape[0], ix.row_bytes() // 4), 0x7FC00000, np.uint32)
    m[:, : stored.shape[1]] = bits(stored)
    t = torch.from_numpy(m.view(np.uint8).reshape(-1)).cuda()
    torch.cuda.synchronize()
    return t


@pytest.mark.parametrize("source", ["values", "staged"])
def test_the_64_block_kernel_over_dense_values_and_over_a_staged_matrix(rlr, oracle, source):
    """gram_tiled<4, 0, 64> (rlr_mmr_select_values: the pools' rows as dense f32 values in device memory) and
    gram_tiled<4, 1, 64> through the d_matrix list (rlr_mmr_select_staged), every ordered pair of 130 slots"""
    import torch
    s, dim = V.shape("r4_64"), 132
    rows, g = V.corpus_and_gram(s["P"], dim, False)
    ix = open_index(rlr, rows, "f32")
    try:
        if source == "staged":
            mat = stage(torch, ix, rows)

            def call(pool_rows, rel, sizes, k, lam):
                return ix.mmr_select_staged(mat.data_ptr(), rows.shape[0], pool_rows, rel, sizes, k, lam)
        else:
            vals = torch.from_numpy(np.full((s["pools"] * s["P"], dim), 0x7FC00000, np.int32)).cuda()
            torch.cuda.synchronize()

            def call(pool_rows, rel, sizes, k, lam):
                ix.fetch_rows_device(pool_rows.ravel(), vals.data_ptr())
                return ix.mmr_select_values(vals.data_ptr(), rel, sizes, k, lam)
        for plan in V.shape_plans("r4_64"):
            compare(plan, g, run(plan, call), (source, plan.k))
    finally:
        ix.close()


def test_ragged_pools_in_one_batch(rlr, oracle):
    """stride 130, pools of 129, 65 and 33 candidates mixed in every call: entries up to each size, three picks each"""
    rows, g = V.corpus_and_gram(130, 132, False)
    plan = V.ragged_plan(130, (129, 65, 33), 256)
    ix = open_index(rlr, rows, "f32")
    try:
        got = run(plan, ix.mmr_select_batch)
        assert (got[2] == 3).all()
        compare(plan, g, got, "ragged")
    finally:
        ix.close()


@pytest.mark.parametrize("dtype,pools,T", [("f32", 256, 64), ("f16", 12, 64), ("f16", 256, 32)])
def test_entries_that_are_not_positive_read_zero(rlr, oracle, dtype, pools, T):
    """a negative dot, a row holding NaN or Inf (gram_entry stores -inf), an exact zero: the third pick logs +0.0, at
    positions of every tile class of the 64-block kernel (f32 and binary16 rows) and of the matrix-core kernel"""
    rows, special = V.class_corpus(oracle, 130, 132, dtype == "f16")
    plan = V.class_plan(130, T, pools, 130, special)
    assert V.gram_instance(dtype, pools, 130)[1] == T
    g = R.gram(oracle, rows)
    ix = open_index(rlr, rows, dtype)
    try:
        got = run(plan, ix.mmr_select_batch)
        assert (bits(got[1][: plan.n_special, 2]) == 0).all() and (got[2] == 3).all()
        compare(plan, g, got, ("not positive", dtype, pools))
    finally:
        ix.close()
