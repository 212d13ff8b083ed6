"""The width ladder (width_vectors.py) checked without a GPU: the restated dispatch rules give the thresholds worked out by
hand from the LDS budgets; the ladder holds every (kernel, cpb) class of every path, both neighbours of every class boundary
and every way through the two chains' loops; and the corpora are such that a re-score with one of the modelled faults
computes other score bits than the oracle on the stated share of the checked (row, query) pairs, at every ladder width.
Each sensitivity case prints the shares it measured (pytest -s shows them; DESIGN.md records the range)."""
import numpy as np
import pytest

import width_vectors as W
from conftest import bits
from test_gpu_parity import oracle_topk

DTYPES = ("f32", "f16")
ALL_WIDTHS = {t: sorted({w for p in W.LADDER for w in W.LADDER[p][t]}) for t in DTYPES}
N_CHECK = 64 + W.N_SPECIAL     # 64 rows of the construction x 4 queries per width


# ---------------------------------------------------------------- the restated rules
def test_thresholds_worked_out_by_hand():
    """q = 4 * q_floats bytes of query, q + 16 per product row: cpb rows fit while (cpb + 1) q + 16 cpb <= budget"""
    for budget, last in ((56 * 1024, {8: 1584, 4: 2864, 2: 4776, 1: 7160}), (60 * 1024, {8: 1696, 4: 3064, 2: 5112, 1: 7672})):
        for cpb, w in last.items():
            assert (cpb + 1) * 4 * w + 16 * cpb <= budget < (cpb + 1) * 4 * (w + 8) + 16 * cpb
            assert W.staged_cpb(w, budget) == cpb and W.staged_cpb(w + 8, budget) == cpb // 2
            assert W.staged_cpb(w - 7, budget) == cpb and W.staged_cpb(w + 1, budget) == cpb // 2   # by q_floats, not by dim
    for t in DTYPES:
        assert W.form("tail", 1584, t) == ("tail_stage_kernel", 8) and W.form("tail", 1592, t) == ("tail_stage_kernel", 4)
        assert W.form("tail", 7160, t) == ("tail_stage_kernel", 1) and W.form("tail", 7168, t) == ("rescore_staged_kernel", 1)
        assert W.form("tail", 7672, t) == ("rescore_staged_kernel", 1) and W.form("tail", 7680, t) == ("rescore_kernel", 0)
        assert W.form("split", 768, t) == ("rescore_staged_kernel", 8) and W.form("split", 8192, t) == ("rescore_kernel", 0)
        assert W.form("score_rows", 5120, t) == ("score_rows_staged_kernel", 1)
        assert W.form("score_rows_small", 768, t) == ("score_rows_kernel", 0) and W.form("big", 768, t) == ("rescore_kernel", 0)
        assert W.form("batch", 7552, t) == ("batch_rescore_kernel", 1) and W.form("batch", 7680, t) == ("batch_finish_kernel", 0)
        assert W.form("hybrid_batch", 100, t) == ("score_rows_batch_kernel", 0)
    assert not W.legal("batch", 100) and W.legal("batch", 8192) and not W.legal("split", 8193)


def test_the_pitch_rule():
    """f32 rows are ceil(dim / 4) units wide, the staged product loop reads ceil(dim / 8) * 8 floats: dim % 8 in 1..4 is refused;
    binary16 rows are ceil(dim / 8) units of eight: never"""
    for d in range(1, 200):
        assert W.pitch_fits(d, "f32") == (d % 8 not in (1, 2, 3, 4)), d
        assert W.pitch_fits(d, "f16"), d
    assert W.form("split", 100, "f32") == ("rescore_kernel", 0) and W.form("split", 101, "f32") == ("rescore_staged_kernel", 8)
    assert W.form("tail", 100, "f32") == ("rescore_kernel", 0) and W.form("tail", 100, "f16") == ("tail_stage_kernel", 8)
    assert W.form("score_rows", 1596, "f32") == ("score_rows_kernel", 0)


# ---------------------------------------------------------------- coverage
@pytest.mark.parametrize("ladder", list(W.LADDER))
@pytest.mark.parametrize("dtype", DTYPES)
def test_ladder_holds_every_class_and_both_sides_of_every_boundary(ladder, dtype):
    widths = W.LADDER[ladder][dtype]
    assert all(W.legal(p, w) for p in W.LADDER_PATHS[ladder] for w in widths)
    for path in W.LADDER_PATHS[ladder]:
        assert {W.form(path, w, dtype) for w in widths} == W.classes(path, dtype), path
        for lo, hi in W.boundaries(path, dtype):
            assert lo in widths and hi in widths, (path, lo, hi)
    assert W.MAX_DIM in widths and min(widths) == (128 if ladder == "batch" else 1)


@pytest.mark.parametrize("dtype", DTYPES)
def test_ladder_takes_every_way_through_the_two_chains(dtype):
    """over all widths a path stages (or does not), the routes through chain_sum_lds (dot_ref_row) that exist are in the ladder"""
    for ladder, path in (("single", "tail"), ("single", "split"), ("score_rows", "score_rows")):
        widths = W.LADDER[ladder][dtype]
        staged = lambda w: W.form(path, w, dtype)[1] > 0
        every = range(1, W.MAX_DIM + 1)
        assert {W.chain_route(w) for w in widths if staged(w)} == {W.chain_route(w) for w in every if staged(w)}, path
        assert {W.row_route(w, dtype) for w in widths if not staged(w)} == {W.row_route(w, dtype) for w in every if not staged(w)}, path
    # the paths that never stage see every route of dot_ref_row at the score_rows widths (list lengths up to 64)
    assert {W.row_route(w, dtype) for w in W.LADDER["score_rows"][dtype]} == {W.row_route(w, dtype) for w in range(1, W.MAX_DIM + 1)}
    # the chain's pipeline edges by number of units: no prologue, epilogue only, one pass, one pass with the reload
    units = {w // 4 for w in W.LADDER["single"][dtype] if W.form("split", w, dtype)[1] > 0}
    assert {0, 1, 3} & units and {4, 5, 7} & units and {8, 11} & units and 12 in units and 16 in units


def test_f32_ladder_has_the_staged_scalar_tail_and_the_narrow_pitch_twins():
    single = W.LADDER["single"]["f32"]
    assert {w % 8 for w in single if W.form("split", w, "f32")[1] > 0} >= {0, 5, 7}
    for lo, _ in W.boundaries("tail", "f32"):
        assert lo + 4 in single and W.form("tail", lo + 4, "f32") == ("rescore_kernel", 0)
    assert {w % 8 for w in W.LADDER["single"]["f16"]} == set(range(8))


# ---------------------------------------------------------------- the corpora
@pytest.mark.parametrize("dim,f16", [(1, False), (7, False), (21, False), (103, False), (1592, False), (5, True), (100, True), (203, True)])
def test_the_numpy_chain_is_the_oracles_scan(oracle, dim, f16):
    rows, qs, want = W.case(N_CHECK, dim, f16)
    got = W.variant_scores(rows, qs, 8 if f16 else 4, models=())["reference"]
    assert np.array_equal(W.pattern_bits(got), W.pattern_bits(want))
    real = slice(W.N_SPECIAL, None)
    assert np.array_equal(bits(got[:, real]), bits(want[:, real])) and (want[:, real] > 0).all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_last_element_and_last_unit_stay_positive(oracle, dtype):
    """the construction's promise, on the rows as stored: the product of the last element and the sum of the products of the
    last aligned 16-byte unit are at least 0.1 / dim for every pair"""
    unit = 8 if dtype == "f16" else 4
    for dim in ALL_WIDTHS[dtype]:
        rows, qs, _ = W.case(N_CHECK, dim, dtype == "f16")
        x = rows[W.N_SPECIAL:].astype(np.float64)
        p = x[None, :, :] * qs[:, None, :].astype(np.float64)
        assert (p[:, :, -1] >= 0.1 / dim).all(), dim
        assert (p[:, :, (dim - 1) // unit * unit:].sum(axis=2) >= 0.1 / dim).all(), dim
        assert (p[:, :, -min(dim, 8):] > 0).all(), dim


@pytest.mark.parametrize("dtype", DTYPES)
def test_special_rows_rank_where_the_oracle_puts_them(oracle, dtype):
    """NaN last, ties by row (oracle_topk); the zero row scores +0.0 below every row of the construction; +Inf in the last
    column gives an infinite score of the sign of the query's last element"""
    for dim in (1, 2, 13, 100, 1592):
        rows, qs, scores = W.case(N_CHECK, dim, dtype == "f16")
        assert not rows[W.ZERO_ROW].any() and np.isnan(rows[W.NAN_ROW, -1]) and rows[W.INF_ROW, -1] == np.inf
        for q, e in zip(qs, scores):
            r, c = W.topk(e, N_CHECK)
            wr, wc = oracle_topk(oracle, rows, q, N_CHECK)
            assert np.array_equal(r, wr) and np.array_equal(W.pattern_bits(c), W.pattern_bits(wc))
            assert r[-1] == W.NAN_ROW and np.isnan(c[-1]) and not np.isnan(c[:-1]).any()
            assert bits(e[W.ZERO_ROW:W.ZERO_ROW + 1])[0] == 0
            assert np.isinf(e[W.INF_ROW]) and np.sign(e[W.INF_ROW]) == np.sign(q[-1])
            at = {int(x): i for i, x in enumerate(r)}
            assert at[W.INF_ROW] == (0 if q[-1] > 0 else N_CHECK - 2)
            assert at[W.ZERO_ROW] == N_CHECK - (2 if q[-1] > 0 else 3)
    rows, qs, scores = W.case(N_CHECK, 1, False)           # one column: every row of the construction is the same vector
    assert len(set(bits(scores[0, W.N_SPECIAL:]).tolist())) == 1


# ---------------------------------------------------------------- sensitivity
@pytest.mark.parametrize("dtype,dim", [(t, w) for t in DTYPES for w in ALL_WIDTHS[t]])
def test_every_fault_model_changes_the_score_bits(oracle, dtype, dim):
    rows, qs, want = W.case(N_CHECK, dim, dtype == "f16")
    real = slice(W.N_SPECIAL, None)
    v = W.variant_scores(rows[real], qs, 8 if dtype == "f16" else 4)
    ref = bits(v.pop("reference"))
    assert np.array_equal(ref, bits(want[:, real]))
    assert set(v) == {m for m in W.MODELS if dim >= W.FROM_DIM[m]}
    shares = {m: float((bits(s) != ref).mean()) for m, s in v.items()}
    print(dtype, dim, " ".join(f"{m}={x:.2f}" for m, x in shares.items()))
    for m, x in shares.items():
        assert x >= W.MIN_SHARE[m], (m, x)
