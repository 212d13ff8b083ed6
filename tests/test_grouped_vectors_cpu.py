"""tests/grouped_vectors.py held to itself: the model against its second statement, the restated fast path against the
model on random cases with nomination errors up to the band, and every planted defect against the designed case that
must expose it.  No GPU: tests/test_gpu_grouped.py holds the device to the same model."""
import numpy as np
import pytest

import grouped_vectors as G


def _random_case(rng):
    n = int(rng.integers(1, 120))
    pattern = rng.integers(0, 4)
    if pattern == 0:
        docs = rng.integers(0, 6, n).astype(np.uint32)                       # few documents, scattered
    elif pattern == 1:
        docs = (np.arange(n) // int(rng.integers(1, 9))).astype(np.uint32)   # runs
    elif pattern == 2:
        docs = np.where(rng.random(n) < 0.4, G.DOC_NONE, rng.integers(0, 4, n)).astype(np.uint32)
    else:
        docs = None
    # a coarse grid makes ties (inside and across documents) common
    e = (rng.integers(-8, 9, n) / 8.0).astype(np.float32)
    if rng.random() < 0.3:
        e[rng.integers(0, n)] = np.nan
    return e, docs, int(rng.integers(1, 40)), int(rng.integers(1, 9))


def test_the_walk_is_the_top_k_of_the_union_of_the_group_tops():
    rng = np.random.default_rng(1)
    short = 0
    for _ in range(400):
        e, docs, k, m = _random_case(rng)
        allowed = None if rng.random() < 0.5 else np.flatnonzero(rng.random(e.size) < 0.6)
        got, want = G.expect(e, docs, k, m, allowed), G.expect_union(e, docs, k, m, allowed)
        assert np.array_equal(got, want), (e, docs, k, m, allowed)
        short += got.size < min(k, e.size if allowed is None else allowed.size)
    assert short > 20          # the groups ran out before k in a fair share of them


def test_the_order_is_score_descending_row_ascending_nan_last_zeros_equal():
    e = np.array([0.0, np.nan, -0.0, 1.0, -1.0, 1.0], np.float32)
    assert G.expect(e, None, 6, 1).tolist() == [3, 5, 0, 2, 4, 1]
    assert G.expect(e, [7] * 6, 6, 8).tolist() == [3, 5, 0, 2, 4, 1]
    assert G.expect(e, [7] * 6, 6, 2).tolist() == [3, 5]
    assert G.expect(e, None, 3, 1, allowed=[1, 2, 4]).tolist() == [2, 4, 1]


def test_the_restated_fast_path_is_the_model_within_the_band():
    rng = np.random.default_rng(2)
    for _ in range(400):
        e, docs, k, m = _random_case(rng)
        e = np.nan_to_num(e, nan=0.25).astype(np.float32)
        # errors of up to 0.99 eps on a grid of 0.6 eps: nominated order differs from exact order all over
        e = (e * np.float32(0.6 * G.EPS * 8)).astype(np.float32)
        a = (e.astype(np.float64) + rng.uniform(-0.99, 0.99, e.size) * G.EPS).astype(np.float32)
        want = G.expect(e, docs, k, m)
        assert np.array_equal(G.fast_path(a, e, docs, k, m, G.EPS), want)
        for harmless in G.HARMLESS:                       # a lower threshold: more candidates, the same answer
            assert np.array_equal(G.fast_path(a, e, docs, k, m, G.EPS, defect=harmless), want), harmless


@pytest.mark.parametrize("name", sorted(G.CASES))
def test_designed_cases_pass_without_a_defect(name):
    a, e, docs, k, m, eps = G.CASES[name]()
    assert np.abs(a.astype(np.float64) - e.astype(np.float64)).max() <= eps
    assert np.array_equal(G.fast_path(a, e, docs, k, m, eps), G.expect(e, docs, k, m))
    assert np.array_equal(G.expect(e, docs, k, m), G.expect_union(e, docs, k, m))


@pytest.mark.parametrize("defect", G.DEFECTS)
def test_every_defect_changes_the_answer_of_its_designed_case(defect):
    assert set(G.BROKEN_BY) == set(G.DEFECTS)
    for name in G.BROKEN_BY[defect]:
        a, e, docs, k, m, eps = G.CASES[name]()
        assert not np.array_equal(G.fast_path(a, e, docs, k, m, eps, defect=defect), G.expect(e, docs, k, m)), (defect, name)


def test_nominated_and_exact_order_disagree_inside_a_group():
    a, e, docs, k, m, eps = G.CASES["decoy_document"]()
    g = np.flatnonzero(docs == 5)
    by_nomination, by_exact = g[G.result_order(a[g], g)], g[G.result_order(e[g], g)]
    assert by_exact[0] == 3 and by_nomination[0] != 3 and by_nomination[-1] == 3
    assert 3 in G.expect(e, docs, k, m).tolist()
