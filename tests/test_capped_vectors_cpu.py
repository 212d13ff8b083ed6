"""tests/capped_vectors.py held to itself and to the oracle, on the CPU: the definition equals the reference's search and
search_with_diversity when every row is its own document; the restated device path equals the definition wherever it
says "decided" -- on the designed cases and on seeded corpora with nominations perturbed inside the band -- and reports
the hand-off where the case is built for one; every planted defect breaks the case named for it."""
import numpy as np
import pytest

import capped_vectors as V
import grouped_vectors as G
from conftest import bits


def _lex(rng, n, n_lex):
    rows = np.sort(rng.choice(n, size=min(n_lex, n), replace=False)).astype(np.uint64)
    return rows, (rng.random(rows.size) * 7.0 + 0.01).astype(np.float32)


# ---- the definition against the oracle -------------------------------------------------------------------------------
@pytest.mark.parametrize("n,dim,n_lex", [(1, 8, 0), (40, 8, 0), (40, 8, 7), (300, 16, 25), (300, 16, 150), (7, 8, 7)])
def test_every_row_its_own_document_is_the_reference(oracle, n, dim, n_lex):
    O = oracle
    rng = np.random.default_rng(1000 + n + n_lex)
    rows = O.synth_rows(n, dim, seed=0x7C00 + n)
    q_raw = O.synth_query(dim, seed=0x7D00 + n)
    q = O.normalize(q_raw)
    lr, ls = _lex(rng, n, n_lex)
    lex = list(zip(lr.tolist(), ls.tolist()))
    docs = np.arange(n, dtype=np.uint32) + 3
    for w_e, w_l in ((0.7, 0.3), (0.3, 0.7), (1.0, 0.0)):
        for top_k in (1, 5, 100):
            for stage in (0, 1):
                want = O.search(rows, q_raw, top_k, w_e, w_l, lex, stage=stage)
                for d, m in ((docs, 1), (docs, 3), (None, 1)):
                    got = V.define_search(O, rows, q, d, lr, ls, w_e, w_l, top_k, m, stage=stage)
                    assert np.array_equal(got["rows"], want[0]), (top_k, stage, w_e)
                    assert np.array_equal(bits(got["comb"]), bits(want[1]))
                    assert np.array_equal(bits(got["cos"]), bits(want[2]))
                    assert np.array_equal(bits(got["lexn"]), bits(want[3]))
            for lam in (0.3, 1.0):
                want = O.search_with_diversity(rows, q_raw, top_k, lam, w_e, w_l, lex)
                got = V.define_search(O, rows, q, docs, lr, ls, w_e, w_l, top_k, 2, diversity=lam)
                assert np.array_equal(got["rows"], want[0]), (top_k, lam, w_e)
                assert np.array_equal(bits(got["comb"]), bits(want[1])) and np.array_equal(bits(got["cos"]), bits(want[2]))
                assert np.array_equal(bits(got["lexn"]), bits(want[3]))


def test_without_lexical_pairs_the_rows_are_the_grouped_rows(oracle):
    O = oracle
    rows = O.synth_rows(500, 8, seed=0x7E00)
    e = O.scan(rows, O.normalize(O.synth_query(8, seed=0x7E01)))
    docs = (np.arange(500) % 37).astype(np.uint32)
    docs[::11] = V.DOC_NONE
    for k, m in ((1, 1), (10, 2), (100, 3), (100, 8)):
        got = V.define(e, docs, [], [], 1.0, 0.0, k, m)
        assert np.array_equal(got["rows"], G.expect(e, docs, k, m))
        allowed = np.arange(0, 500, 3)
        got = V.define(e, docs, [], [], 1.0, 0.0, k, m, allowed=allowed)
        assert np.array_equal(got["rows"], G.expect(e, docs, k, m, allowed))


def test_need_of():
    assert V.need_of(1000, 5) == 5 and V.need_of(3, 5) == 3 and V.need_of(1000, 0) == 1
    assert V.need_of(1000, 5, stage=1) == 15 and V.need_of(7, 5, stage=1) == 7
    assert V.need_of(1000, 5, diversify=True) == 15 and V.need_of(1000, 100, diversify=True) == 300
    assert V.need_of(12, 5, diversify=True) == 12 and V.need_of(1000, 1, diversify=True) == 11


# ---- the designed cases ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(V.CASES))
def test_designed_case(name):
    c = V.CASES[name]()
    want = V.run_define(c)
    status, got = V.run_device(c)
    assert status == c["status"], (name, status)
    if status == 0:
        assert V.same(got, want), (name, got["rows"], want["rows"])
    # the inputs stay inside what the finish holds: a hand-off here is never a capacity hand-off
    assert status != 1 and c["need"] <= V.NEED_MAX and c["lex_rows"].size <= V.LEX_CAP


def test_what_the_designed_cases_show():
    c = V.CASES["lexical_displaces_best_cosine"]()
    assert V.run_define(c)["rows"][0] == 2 and 0 not in V.run_define(c)["rows"]
    c = V.CASES["lexical_row_of_a_full_document"]()
    r = V.run_define(c)
    assert 5 not in r["rows"] and 6 in r["rows"] and (r["docs"] == 7).sum() == 2
    c = V.CASES["mth_place_by_a_far_lexical_row"]()
    r = V.run_define(c)
    assert r["rows"].tolist()[:4] == [41, 0, 1, 40] and (r["docs"] == 3).sum() == 2
    c = V.CASES["rounding_tie_outside_the_band"]()
    r = V.run_define(c)
    assert r["rows"][-1] == 0 and bits(r["comb"][-1]) == bits(np.float32(0.3) * c["e"][9])  # the tie, won by the lower row
    assert c["e"][0] < c["e"][9] and V.run_device(c, "boundary_ignored")[1]["rows"][-1] == 9
    c = V.CASES["signed_zero_combined"]()
    r = V.run_define(c)
    assert r["rows"].tolist() == [0, 2, 4, 6] and bits(r["comb"][:3]).tolist() == [0x80000000] * 3
    c = V.CASES["fewer_documents_than_need"]()
    assert V.run_define(c)["rows"].size == 6
    c = V.CASES["nan_row_needed"]()
    r = V.run_define(c)
    assert r["rows"][-1] == 1 and np.isnan(r["comb"][-1])
    c = V.CASES["lexical_rows_outside_the_filter"]()
    r = V.run_define(c)
    assert not np.isin([1, 3], r["rows"]).any() and bits(r["lexn"][r["rows"] == 4]) == bits(np.float32(2.0) / np.float32(8.0))


@pytest.mark.parametrize("defect", V.DEFECTS)
def test_every_defect_breaks_its_case(defect):
    assert set(V.BROKEN_BY) == set(V.DEFECTS)
    for name in V.BROKEN_BY[defect]:
        c = V.CASES[name]()
        status, got = V.run_device(c, defect)
        broken = status != c["status"] or (status == 0 and not V.same(got, V.run_define(c)))
        assert broken, (defect, name)


# ---- the proof, numerically: wherever the device path says "decided" it equals the definition --------------------------
@pytest.mark.parametrize("seed", range(6))
def test_perturbed_nominations_inside_the_band(oracle, seed):
    O = oracle
    rng = np.random.default_rng(4000 + seed)
    n = (70, 400, 1500, 4097, 400, 1500)[seed]
    rows = O.synth_rows(n, 8, seed=0x7F00 + seed)
    e = O.scan(rows, O.normalize(O.synth_query(8, seed=0x7F80 + seed)))
    eps = 2.0e-3                                             # a wide band: nominated and exact order disagree often
    a = (e.astype(np.float64) + rng.uniform(-0.99 * eps, 0.99 * eps, n)).astype(np.float32)
    decided = 0
    for docs in (None, (np.arange(n) % 13).astype(np.uint32), rng.integers(0, max(n // 9, 2), n).astype(np.uint32),
                 np.where(np.arange(n) % 4 == 0, V.DOC_NONE, np.arange(n) // 20).astype(np.uint32)):
        for n_lex in (0, 1, 50):
            lr, ls = _lex(rng, n, n_lex)
            for need, m, w_e, w_l in ((1, 1, 0.7, 0.3), (5, 2, 0.7, 0.3), (15, 1, 0.3, 0.7), (100, 3, 1.0, 0.0), (300, 8, 0.5, 0.5)):
                for allowed in (None, np.arange(0, n, 3)):
                    status, got = V.device_path(a, e, docs, lr, ls, w_e, w_l, need, m, eps, allowed)
                    assert status in (0, 2)
                    if status == 0:
                        decided += 1
                        want = V.define(e, docs, lr, ls, w_e, w_l, need, m, allowed)
                        assert V.same(got, want), (seed, need, m, n_lex, got["rows"][:8], want["rows"][:8])
    assert decided > 60                                      # the rule hands off where it must, not everywhere


def test_by_rule():
    e = np.linspace(0.9, 0.1, 30).astype(np.float32)
    args = dict(nominated=e, exact=e, docs=None, lex_rows=[3], lex_scores=[1.0], need=5, per_doc=1, eps=V.EPS)
    assert V.device_path(w_e=0.7, w_l=0.3, **args)[0] == 0
    for w_e, w_l in ((0.0, 0.3), (-0.5, 0.3), (float("nan"), 0.3), (float("inf"), 0.3), (0.7, -0.1), (0.7, float("nan"))):
        assert V.device_path(w_e=w_e, w_l=w_l, **args)[0] == 3
    args["lex_scores"] = [-1.0]
    assert V.device_path(w_e=0.7, w_l=0.3, **args)[0] == 3
    big = np.linspace(0.9, 0.1, 5000).astype(np.float32)
    assert V.device_path(big, big, None, [], [], 0.7, 0.3, V.NEED_MAX + 1, 1, V.EPS)[0] == 3
    assert V.device_path(big, big, None, np.arange(V.LEX_CAP + 1), np.ones(V.LEX_CAP + 1), 0.7, 0.3, 5, 1, V.EPS)[0] == 3
