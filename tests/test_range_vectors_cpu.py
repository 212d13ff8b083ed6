"""tests/range_vectors.py held to itself: the restated device path against the definition on the designed cases and on
seeded corpora whose nominations are perturbed by up to 0.99 eps, the bounds against exact arithmetic, and the mutation
proof -- every planted defect is caught by the designed case named for it.  No GPU: tests/test_gpu_range.py holds the
device to the same definition."""
from fractions import Fraction

import numpy as np
import pytest

import range_vectors as R

F32 = np.float32


def _same(got, want):
    return np.array_equal(got[0], want[0]) and got[1] == want[1]


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_designed_cases_equal_the_definition(name):
    a, e, eps, tau, cap, allowed = R.CASES[name]()
    mask = R._allowed_mask(e.size, allowed)
    ok = mask & ~np.isnan(a)
    assert (np.abs(a[ok].astype(np.float64) - e[ok].astype(np.float64)) <= eps).all(), "the case leaves its own band"
    rows, n_total, form = R.device_path(a, e, eps, tau, cap, allowed)
    assert _same((rows, n_total), R.expect(e, tau, cap, allowed)), name
    want_form = {"more_hits_than_cap": 1, "nan_nomination": 2}.get(name, 0)
    assert form == want_form, (name, form)
    # count-only agrees with the rows call
    rows0, n0, form0 = R.device_path(a, e, eps, tau, 0, allowed)
    assert rows0.size == 0 and n0 == n_total and form0 == (2 if want_form == 2 else 0)


def test_every_planted_defect_is_caught_by_its_designed_case():
    assert set(R.BROKEN_BY) == set(R.DEFECTS)
    caught = {}
    for defect in R.DEFECTS:
        for name in sorted(R.CASES):
            a, e, eps, tau, cap, allowed = R.CASES[name]()
            got = R.device_path(a, e, eps, tau, cap, allowed, defect=defect)
            if not _same(got[:2], R.expect(e, tau, cap, allowed)):
                caught.setdefault(defect, []).append(name)
    for defect in R.DEFECTS:
        print(f"{defect}: caught by {caught.get(defect, [])}")
        assert caught.get(defect), f"no designed case catches the planted defect {defect}"
        for name in R.BROKEN_BY[defect]:
            assert name in caught[defect], (defect, name, caught[defect])


def test_the_definition_on_the_ieee_edges():
    e = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 1.0], np.float32)
    assert R.expect(e, -np.inf, 10)[1] == 5                                   # every row with a number for a score
    assert R.expect(e, np.inf, 10)[0].tolist() == [1]                         # +Inf is a hit of tau = +Inf
    assert R.expect(e, 0.0, 10)[0].tolist() == [1, 5, 3, 4]                   # -0 >= +0; key order puts +0 first
    assert R.expect(e, -0.0, 10)[1] == 4
    assert R.expect(e, 0.0, 2)[0].tolist() == [1, 5] and R.expect(e, 0.0, 2)[1] == 4
    assert R.expect(e, 0.0, 0)[0].size == 0 and R.expect(e, 0.0, 0)[1] == 4


@pytest.mark.parametrize("tau", [0.5, -0.5, 0.0, -0.0, 1e-30, 3.0e38, -3.0e38, np.inf, -np.inf, 0.7, 1.0 - 2.0 ** -24])
@pytest.mark.parametrize("two_eps", [0.0, 2e-4, 1e-7, 1e-45, 1.0, 3.0e38])
def test_bounds_lie_outside_the_real_margins(tau, two_eps):
    lo, hi = R.bounds(tau, two_eps)
    if np.isfinite(tau):
        t, m = Fraction(float(F32(tau))), Fraction(float(F32(two_eps)))
        assert lo == -np.inf or Fraction(float(lo)) <= t - m
        assert hi == np.inf or Fraction(float(hi)) >= t + m
    elif tau == np.inf:
        assert hi == np.inf and lo >= F32(3.4e38)                             # inf - band = inf, stepped down once
    else:
        assert lo == -np.inf and hi <= F32(-3.4e38)


@pytest.mark.parametrize("seed", range(6))
def test_seeded_corpora_equal_the_definition(seed):
    rng = np.random.default_rng(900 + seed)
    n, eps = 5000, 1.0e-4
    e = rng.uniform(-1.0, 1.0, n).astype(np.float32)
    e[rng.integers(0, n, 200)] = e[rng.integers(0, n, 200)]                   # ties
    a = (e.astype(np.float64) + rng.uniform(-0.99, 0.99, n) * eps).astype(np.float32)
    assert (np.abs(a.astype(np.float64) - e.astype(np.float64)) <= eps).all()
    order = R.result_order(e, np.arange(n))
    masks = [None, rng.random(n) < 0.3, np.arange(0, n, 7)]
    for allowed in masks:
        for j in (0, 1, 99, 100, 101, 2047, 2048, 2049, n - 1):
            t_in = e[order[j]]
            for tau in (t_in, np.nextafter(t_in, F32(np.inf)), F32(-np.inf), F32(np.inf)):
                for cap in (0, 100, n):
                    rows, n_total, form = R.device_path(a, e, eps, tau, cap, allowed)
                    want = R.expect(e, tau, cap, allowed)
                    assert _same((rows, n_total), want), (seed, j, tau, cap)
                    assert form == (1 if cap and want[1] > cap else 0)


def test_a_nomination_at_the_edge_of_the_band_is_still_decided_right():
    """|a - e| = eps exactly (in f64, then rounded to f32) on both sides of tau, for taus across binades"""
    eps = 1.0e-4
    for tau in (F32(0.98), F32(0.5), F32(0.7), F32(1e-3), F32(-0.25)):
        e = np.array([tau, np.nextafter(tau, F32(-np.inf)), tau, np.nextafter(tau, F32(-np.inf))], np.float32)
        a = np.array([float(tau) - eps, float(tau) - eps, float(tau) + eps, float(tau) + eps]).astype(np.float32)
        for cap in (0, 10):
            rows, n_total, _ = R.device_path(a, e, eps, tau, cap)
            assert _same((rows, n_total), R.expect(e, tau, cap)), (tau, cap)
