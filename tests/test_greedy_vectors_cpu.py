"""The designed pools of greedy_vectors.py, proved on the CPU before test_gpu_greedy.py relies on them:
  * the traced restatement is mmr_from_gram bit for bit on every pool, and the oracle's literal loop on the strides up to 130;
  * every plan reaches the state of the chain it is named for (from the trace: a condition, no pool is dropped to meet it);
  * the rows are exact: the Gram matrix is the same bits with the additions reversed, from the binary16-rounded rows, and in
    exact arithmetic;
  * each planted defect of the restatement changes the picks or the logged bits of a pool of the plan aimed at it."""
import functools

import numpy as np
import pytest

import greedy_vectors as V
import mmr_restatement as R
from conftest import bits

ALL_STRIDES = V.STRIDES + (V.SINGLE,)


@functools.lru_cache(maxsize=None)
def summary(name, P):
    pl = V.plan(name, P)
    return pl, V.states(pl, V.corpus_gram())


def same(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and bool(((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))).all())


def slots_of(P):
    return {(c % 64, c // 64) for c in range(1, P)}


# ---------------------------------------------------------------- the restatement
@pytest.mark.parametrize("P", ALL_STRIDES)
def test_traced_restatement_is_the_restatement_and_the_oracle_loop(oracle, P):
    g, rows = V.corpus_gram(), V.corpus()
    for pl in V.plans(P):
        _, st = summary(pl.name, P)
        for q, (order, logged, picks, broke) in enumerate(st["traces"]):
            s, k, lam = int(pl.sizes[q]), int(pl.k[q]), pl.lam[q]
            wo, wm = R.mmr_from_gram(V.PoolGram(g, pl.pool_rows[q, :s]), pl.rel[q, :s], k, lam)
            assert np.array_equal(order, wo) and same(logged, wm), (pl.name, P, q, pl.state[q])
            assert len(picks) == max(order.size - 1, 0)
            assert (broke is not None) == (0 < order.size < min(max(k, 1), s)), (pl.name, P, q, pl.state[q])
            do, dm = V.with_defect(None, g, pl.pool_rows[q], pl.rel[q], s, k, lam, P)
            assert np.array_equal(order, do) and same(logged, dm), (pl.name, P, q, pl.state[q])
            if P <= 130 and s:
                oo, om = oracle.mmr(rows[pl.pool_rows[q, :s].astype(np.int64)], pl.rel[q, :s], k, float(lam))
                assert np.array_equal(order, oo) and same(logged[1:], om[1:]) and np.isnan(om[0]), (pl.name, P, q, pl.state[q])


def test_expected_is_the_trace(oracle):
    pl, st = summary("ragged", 128)
    order, logged, n = V.expected(pl, V.corpus_gram(), st["traces"])
    assert order.shape == (pl.Q, V.width(pl)) and V.width(pl) == 6
    for q, (o, m, _, _) in enumerate(st["traces"]):
        assert n[q] == o.size and np.array_equal(order[q, : n[q]], o) and same(logged[q, : n[q]], m)
    assert sorted(set(pl.sizes.tolist())) == sorted(V.ragged_sizes(128)) and (pl.sizes == 0).sum() == 3
    assert (n[pl.sizes == 0] == 0).all() and (n[pl.sizes == 1] == 1).all()
    assert len(pl.calls()) == 1                                   # one batch call


# ---------------------------------------------------------------- the rows
def test_the_gram_matrix_does_not_depend_on_the_order_or_the_storage(oracle):
    rows, g = V.corpus(), V.corpus_gram()
    cp = V.corpus_spec()
    fin = cp.finite()
    assert rows.shape[1] == V.DIM and (~fin).sum() == 2
    assert np.array_equal(bits(oracle.round_f16(rows[fin])), bits(rows[fin]))       # on the binary16 grid
    assert same(R.gram(oracle, oracle.round_f16(rows)), g)
    assert same(R.gram(oracle, np.ascontiguousarray(rows[:, ::-1])), g)             # the additions in reversed order
    exact = cp.exact_gram()[np.ix_(fin, fin)]
    assert np.array_equal(g[np.ix_(fin, fin)].astype(np.float64), exact)            # no entry was rounded at all
    assert not np.isfinite(g[~fin]).any() and not np.isfinite(g[:, ~fin]).any()     # the NaN / Inf rows: non-finite throughout
    assert np.isposinf(g[~fin]).any() and np.isneginf(g[~fin]).any() and np.isnan(g[~fin]).any()
    nz = (rows[fin] != 0).sum(axis=1)
    assert nz.max() <= 2
    m, e = np.frexp(np.abs(rows[fin][rows[fin] != 0]))
    assert (m == 0.5).all()                                                          # signed powers of two


# ---------------------------------------------------------------- coverage
@pytest.mark.parametrize("P", V.STRIDES)
def test_slot_sweep_makes_every_slot_a_lone_winner(oracle, P):
    pl, st = summary("slot_sweep", P)
    assert pl.Q == P - 1 and st["aimed_fast"] == slots_of(P) and not st["aimed_tie"]
    for q, (order, _, picks, broke) in enumerate(st["traces"]):
        c = q + 1
        assert pl.aim[q] == (1, c) and order.size == 3 and order[1] == c and broke is None
        p = picks[0]
        assert p.holders == 1 and p.lane_mates == 0 and p.nan_neighbours and p.n_rem == P - 1


@pytest.mark.parametrize("P", V.STRIDES)
def test_tie_sweep_makes_every_slot_a_tie_winner_and_half_of_them_against_the_index(oracle, P):
    pl, st = summary("tie_sweep", P)
    assert st["aimed_tie"] == slots_of(P)
    against = 0
    for q, (order, _, picks, _) in enumerate(st["traces"]):
        pick, c = pl.aim[q]
        assert pick == 2 and order.size == 3 and order[2] == c, (q, order)
        assert picks[0].holders == 1                                       # pick 2 is no tie: pick 3's replay is the first
        p = picks[1]
        assert p.holders == 2 and p.idx == c and p.replayed == 0
        if pl.state[q] in ("tie_first", "tie_second"):
            assert p.moved and p.idx > p.lowest_idx and p.pos < p.lowest_idx    # the higher index holds the lower position
            assert p.pos == (0 if pl.state[q] == "tie_first" else 1)
            against += 1
        else:
            assert not p.moved and p.idx == p.lowest_idx
    assert 2 * against >= pl.Q and set(st["pools"]) == {"tie_first", "tie_second", "tie_own"}


@pytest.mark.parametrize("P", ALL_STRIDES)
def test_tie_forms(oracle, P):
    pl, st = summary("tie_forms", P)
    by = {}
    for q, t in enumerate(st["traces"]):
        by.setdefault(pl.state[q], []).append(t)
    assert all(int(pl.k[q]) >= 6 for q in range(pl.Q))
    assert by["two_holders"][0][2][0].holders == 2 and by["two_holders"][0][2][0].moved
    three = by["three_holders"][0][2]
    assert three[0].holders == 3 and three[1].holders == 2 and three[1].moved and three[1].replayed == 1
    many = by["many_holders"][0][2]
    assert len(many) == 7 and many[0].holders == P - 1 >= min(64, P - 1) and all(p.holders > 1 and p.pos == 0 for p in many)
    assert [p.replayed for p in many] == list(range(7))                    # every replay after the first is incremental
    if P > 64:                                                             # J = 1 has one slot per lane
        for _, _, picks, _ in by["same_lane"]:
            a, b = picks[0].holder_idx
            assert picks[0].holders == 2 and a % 64 == b % 64
        assert len(by["same_lane"]) == (2 if P > 128 else 1)
    fl = by["first_last_lane"][0][2][0]
    assert fl.holders == 2 and {c % 64 for c in fl.holder_idx} == {0 if P > 64 else 1, 63}
    p245 = by["picks_2_4_5"][0][2]
    assert [p.holders > 1 for p in p245] == [True, False, True, True, False, False]
    assert [p.replayed for p in p245 if p.holders > 1] == [0, 1, 3] and p245[2].holders == 3 and p245[2].moved
    order, _, last, broke = by["last_pick"][0]
    assert order.size == 6 and last[-1].holders == 2 and all(p.holders == 1 for p in last[:-1]) and broke is None
    order, _, drain, _ = by["two_left"][0]
    assert order.size == P and drain[-2].n_rem == 2 and drain[-2].holders == 2 and drain[-1].n_rem == 1
    assert all(p.holders == 1 for p in drain[:-2])
    replays = [p.replayed for t in st["traces"] for p in t[2] if p.holders > 1]
    assert 0 in replays and max(replays) > 0


@pytest.mark.parametrize("P", ALL_STRIDES)
def test_zeros(oracle, P):
    pl, st = summary("zeros", P)
    seen, mixed, lam_zero = set(), set(), {0.0: set(), 1.0: set()}
    for q, (order, logged, picks, _) in enumerate(st["traces"]):
        p = picks[0]
        assert p.zero and bits(logged[1]) == (0x80000000 if p.zero < 0 else 0), (q, pl.state[q])
        if p.holders == 1:
            seen.add(p.zero)
        elif p.zero_signs == {1, -1}:
            mixed.add((pl.state[q], p.zero, p.moved))
        if float(pl.lam[q]) in lam_zero:
            lam_zero[float(pl.lam[q])] |= {x.zero for x in picks}
    assert seen == {1, -1}
    assert {(s, z) for s, z, _ in mixed} >= {("mixed_minus_wins", -1), ("mixed_plus_wins", 1)}
    assert {m for _, _, m in mixed} == {True, False}                        # decided at its own position and at a moved one
    assert lam_zero[0.0] >= {1, -1} and lam_zero[1.0] >= {1, -1}


@pytest.mark.parametrize("P", ALL_STRIDES)
def test_maxsim(oracle, P):
    pl, st = summary("maxsim", P)
    g = V.corpus_gram()
    for q, (order, logged, picks, _) in enumerate(st["traces"]):
        s = pl.state[q]
        rows = pl.pool_rows[q].astype(np.int64)
        if s == "all_negative":
            read = [g[rows[a], rows[b]] for a in order[:2] for b in (2, P - 1, 7) if a != b]
            assert max(read) < 0 and np.array_equal(logged[1:], [2.0, 1.5])
        elif s.endswith("_row_pick"):
            assert order.tolist()[:4] == [0, 6, 9, P - 2] and not np.isfinite(g[rows[6]][rows]).any()
            assert np.array_equal(logged[1:4], [4.0, 1.75, 0.875])           # 1 - max(1/4, 1/8) / 2: slot 0 and slot 9 only
        elif s.endswith("_row_first"):
            assert order.tolist()[:3] == [0, 9, P - 2] and np.array_equal(logged[1:3], [2.0, 0.9375])
        elif s in ("rising", "falling"):
            t = [float(g[rows[a], rows[8]]) for a in order[:3]]
            assert t == ([0.25, 0.5, 1.5] if s == "rising" else [1.5, 0.5, 0.25]) and order[3] == 8 and logged[3] == 3.25
    assert set(pl.state) == {"all_negative", "nan_row_pick", "nan_row_first", "inf_row_pick", "inf_row_first", "rising", "falling"}


@pytest.mark.parametrize("P", ALL_STRIDES)
def test_overflow(oracle, P):
    pl, st = summary("overflow", P)
    got = {}
    for q, (order, logged, picks, broke) in enumerate(st["traces"]):
        got.setdefault(pl.state[q], []).append((order, picks, broke))
        assert np.isfinite(logged[1:]).all()
        assert abs(float(pl.lam[q])) == V.BIG_LAM
    for order, picks, broke in got["recount_pick"]:
        assert picks[1].plus_inf == 1 and picks[1].holders == 1 and order[2] == 9 and broke is None
    order, picks, _ = got["recount_tie"][0]
    assert picks[1].plus_inf == 1 and picks[1].holders == 2 and order.tolist() == [0, 4, 3, 9]
    order, picks, broke = got["recount_then_break"][0]
    assert order.size == 4 and [p.plus_inf for p in picks] == [0, 1, 1] and broke == V.End(P - 4, 1, 1, 0)
    order, picks, broke = got["all_inf_break"][0]
    assert order.size == 2 and broke == V.End(P - 2, 2, 2, 0)
    order, picks, broke = got["mirror_minus_inf"][0]
    assert order.size == 4 and picks[1].minus_inf == 1 and picks[1].plus_inf == 0 and broke is None
    assert got["mirror_break"][0][2] == V.End(P - 2, 2, 0, 2) and got["mirror_break"][0][0].size == 2
    order, picks, broke = got["mirror_t0_overflow"][0]
    assert order.tolist() == [0, 2, 9] and broke == V.End(P - 3, 1, 1, 0) and picks[0].nonfinite == 1
    lams = {float(x) for x in pl.lam}
    assert min(lams) < 0 and max(lams) > 1


@pytest.mark.parametrize("P", ALL_STRIDES)
def test_ends(oracle, P):
    pl, st = summary("ends", P)
    want = dict(size_1=(5, 1), size_2=(5, 2), size_2_nan=(5, 1), k_0=(0, 1), k_1=(1, 1), k_P=(P, P), k_P_plus_7=(P + 7, P),
                all_non_finite=(5, 1), run_out=(10, 3), run_out_sooner=(10, 2), t0_overflow=(5, 2), t0_overflow_only=(5, 1))
    assert set(pl.state) == set(want)
    for q, (order, _, picks, broke) in enumerate(st["traces"]):
        assert (int(pl.k[q]), order.size) == want[pl.state[q]], pl.state[q]
        if pl.state[q] in ("size_2_nan", "all_non_finite", "run_out", "run_out_sooner", "t0_overflow", "t0_overflow_only"):
            assert broke is not None
        if pl.state[q].startswith("t0_overflow"):
            assert broke[1:] == (2, 1, 1) and float(pl.lam[q]) == -1.0     # 2 * (+-FLT_MAX): both infinities, from t0 alone
    assert sorted(pl.sizes.tolist())[:4] == [1, 1, 2, 2]


# ---------------------------------------------------------------- planted defects
# defect -> the plans that must notice it (at every stride they exist at; the dropped slot: where J is odd)
AIMED = (
    ("tie_lowest_index", ("tie_sweep", "tie_forms", "ragged")),
    ("tie_stale_positions", ("tie_sweep", "tie_forms")),
    ("zero_logged_plus", ("zeros",)),
    ("zeros_ordered_by_bits", ("zeros",)),
    ("max_sim_from_minus_inf", ("maxsim",)),
    ("max_sim_takes_non_finite", ("maxsim",)),
    ("infinite_selectable", ("overflow",)),
    ("continues_past_no_finite", ("ends", "overflow")),
    ("odd_j_last_slot_dropped", ("slot_sweep", "tie_sweep")),
    ("slot_0_needs_finite_score", ("ends", "slot_sweep")),
    ("sizes_ignored", ("ragged",)),
)


def noticed(defect, pl, st):
    g = V.corpus_gram()
    hit = []
    for q, (order, logged, _, _) in enumerate(st["traces"]):
        o, m = V.with_defect(defect, g, pl.pool_rows[q], pl.rel[q], int(pl.sizes[q]), int(pl.k[q]), pl.lam[q], pl.P)
        if not (np.array_equal(o, order) and same(m, logged)):
            hit.append(q)
    return hit


@pytest.mark.parametrize("defect,names", AIMED)
def test_every_planted_defect_is_noticed(oracle, defect, names):
    assert {d for d, _ in AIMED} == set(V.DEFECTS)
    for name in names:
        for P in ALL_STRIDES:
            if P > 1024 and name not in V.SINGLE_PLANS:
                continue
            if defect == "odd_j_last_slot_dropped" and V.greedy_j(P) % 2 == 0:
                continue
            pl, st = summary(name, P)
            hit = noticed(defect, pl, st)
            assert hit, (defect, name, P)
            if defect == "odd_j_last_slot_dropped":                        # every pool whose winner sits in that slot
                J = V.greedy_j(P)
                assert {q for q in range(pl.Q) if pl.aim[q][1] // 64 == J - 1} <= set(hit)
            if defect == "tie_lowest_index" and name == "tie_sweep":
                assert set(hit) == {q for q in range(pl.Q) if pl.state[q] != "tie_own"}
            if defect == "sizes_ignored":
                assert set(hit) >= {q for q in range(pl.Q) if 1 < pl.sizes[q] < P and pl.state[q] != "all_tie"}
