"""tests/range_batch_vectors.py held to itself: the restated batched device path equals the definition on every designed
case and on random batches behind both passes, reports the designed status per query, and every planted defect breaks
the designed case named for it (a defect no case catches would say nothing about the device)."""
import numpy as np
import pytest

import range_batch_vectors as V
import range_vectors as R
from conftest import bits

F32 = np.float32


def same(got, want):
    """(rows, scores, n_total) of every query: rows equal, scores bit-equal, totals equal"""
    return len(got) == len(want) and all(
        np.array_equal(g[0], w[0]) and g[0].dtype == np.uint64 and np.array_equal(bits(g[1]), bits(w[1])) and g[2] == w[2]
        for g, w in zip(got, want))


def wanted(case):
    return V.definition(case["exact"], case["taus"], case["cap"], case.get("allowed"))


@pytest.mark.parametrize("name", [n for n in V.CASES if n != "nan_tau"])
def test_the_restatement_equals_the_definition_on_every_designed_case(name):
    case = V.CASES[name]()
    assert np.all(np.abs(case["nominated"] - case["exact"])[~np.isnan(case["nominated"])] <= F32(case["eps"]))
    got = V.run(case)
    assert same(got, wanted(case)), name
    assert [g[3] for g in got] == V.STATUS[name], name


def test_a_nan_threshold_refuses_the_whole_call():
    with pytest.raises(ValueError):
        V.run(V.CASES["nan_tau"]())


@pytest.mark.parametrize("defect", V.DEFECTS)
def test_every_planted_defect_breaks_its_designed_case(defect):
    name = V.BROKEN_BY[defect]
    case = V.CASES[name]()
    if name == "nan_tau":
        got = V.run(case, defect=defect)                     # the defect answers where the call must be refused
        assert len(got) == 2 and got[1][2] == 2              # (every row of query 1 counted against -inf)
        return
    got = V.run(case, defect=defect)
    assert not (same(got, wanted(case)) and [g[3] for g in got] == V.STATUS[name]), (defect, name)
    assert not same(got, wanted(case)), (defect, name, "the answer itself must be wrong, not only the status")


@pytest.mark.parametrize("defect", V.DEFECTS)
def test_a_defect_leaves_the_cases_designed_for_others_alone_or_wrong_but_never_raises(defect):
    for name, make in V.CASES.items():
        if name == "nan_tau":
            continue
        V.run(make(), defect=defect)


def test_the_defect_list_and_the_case_table_agree():
    assert set(V.BROKEN_BY) == set(V.DEFECTS) and len(V.DEFECTS) == 8
    assert set(V.BROKEN_BY.values()) <= set(V.CASES)
    assert set(V.STATUS) == set(V.CASES) - {"nan_tau"}


def test_per_query_bounds_are_the_single_path_bounds():
    taus = np.array([0.9, -0.3, 0.0, -0.0, np.inf, -np.inf], np.float32)
    for (lo, hi), t in zip(V.per_query_bounds(taus, 1e-4), taus):
        want = R.bounds(t, F32(2e-4))
        assert np.array_equal(bits([lo, hi]), bits(want))
        assert lo <= t <= hi
    lo, hi = V.per_query_bounds([np.inf], np.inf)[0]         # tau and the band both infinite: a bound that is no number
    assert np.isnan(lo)
    e = np.array([[0.1, np.inf, -0.5]], np.float32)
    got = V.device_path(e, e, np.inf, [np.inf], 5, path="gemm")
    assert same(got, V.definition(e, [np.inf], 5)) and got[0][0].tolist() == [1]


def test_the_capacities_and_the_mark():
    rng = np.random.default_rng(5)
    e = rng.uniform(-1, 1, (3, 40)).astype(np.float32)
    a = (e + rng.uniform(-1, 1, e.shape).astype(np.float32) * F32(0.9e-4)).astype(np.float32)
    taus = np.array([-0.5, 0.0, 0.9], np.float32)
    lists = V.gemm_lists(a, taus, 1e-4, cand_cap=16, marked=(2,))
    assert lists[0][1] > 16 and lists[0][0].size == 16        # the count runs on, the list stops
    assert lists[2][1] & V.MARK
    got = V.device_path(a, e, 1e-4, taus, 8, path="gemm", cand_cap=16, marked=(2,))
    assert [g[3] for g in got] == [1, 1 if lists[1][1] > 16 else 0, 1]
    assert same(got, V.definition(e, taus, 8))
    got = V.device_path(a, e, 1e-4, taus, 40, path="gemm", finish_max=4)        # rows wanted: the hit capacity hands back
    assert [g[3] for g in got] == [2, 2, 0 if got[2][2] <= 4 else 2] and same(got, V.definition(e, taus, 40))
    got = V.device_path(a, e, 1e-4, taus, 0, path="gemm", finish_max=4)         # count-only: never
    assert [g[3] for g in got] == [0, 0, 0] and same(got, V.definition(e, taus, 0))


@pytest.mark.parametrize("path", ["gemm", "scan"])
@pytest.mark.parametrize("cap", [0, 1, 7, 500])
def test_random_batches_equal_the_definition(path, cap):
    rng = np.random.default_rng(11 + cap)
    for trial in range(20):
        nq, n = int(rng.integers(1, 9)), int(rng.integers(1, 300))
        e = rng.uniform(-1, 1, (nq, n)).astype(np.float32)
        e[:, rng.integers(0, n)] = e[:, rng.integers(0, n)]                     # a tie here and there
        a = (e + rng.uniform(-1, 1, e.shape).astype(np.float32) * F32(0.9e-4)).astype(np.float32)
        pool = np.sort(e.ravel())
        taus = np.r_[pool[rng.integers(0, pool.size, nq - 1)], [rng.choice([-np.inf, np.inf, 0.0, -0.0])]].astype(np.float32)[:nq]
        allowed = None if trial % 3 else np.flatnonzero(rng.random(n) < 0.5)
        got = V.device_path(a, e, 1e-4, taus, cap, allowed=allowed, path=path)
        assert same(got, V.definition(e, taus, cap, allowed)), (path, cap, trial)
        assert all(g[3] == 0 for g in got)
