"""tests/pool_vectors.py does what it says, without a GPU: the rows' cosines and Gram entries are exact, the restatement
equals the C oracle on every case it predicts status 0 for, every plan reaches the state each case is labelled with, the
statuses are the ones the plans promise, and every planted defect changes what at least one case expects."""
import collections

import numpy as np
import pytest

import pool_vectors as V
from pool_vectors import bits

E0 = np.zeros(V.DIM, np.float32)
E0[0] = 1.0
ALL = [(e, nm) for e, names in (("hybrid", V.HYBRID_PLANS), ("diverse", V.DIVERSE_PLANS)) for nm in names]
CORPORA = sorted({c.corpus for c in V.cases()})


def each(entry, name):
    for i, c in enumerate(V.plan(entry, name)):
        for mode in c.modes:
            yield i, c, mode, V.want(entry, name, i, mode)


@pytest.mark.parametrize("name", CORPORA)
def test_cosines_are_exact_in_any_order_and_storage(oracle, name):
    """one non-zero product per cosine (the query is e_0): oracle.scan returns cos[r] bit for bit; a corpus that binary16
    cases use survives the rounding to binary16 unchanged; every row has at most one element beside element 0"""
    cp = V.corpus(name)
    rows = cp.rows()
    assert np.array_equal(bits(oracle.scan(rows, E0)), bits(cp.cos))
    assert (np.count_nonzero(rows[:, 1:], axis=1) <= 1).all()
    uses_f16 = any("f16" in c.dtypes for c in V.cases() if c.corpus == name)
    assert uses_f16 <= cp.f16
    if cp.f16:
        assert np.array_equal(bits(oracle.round_f16(rows)), bits(rows))


def test_gram_entries_of_every_diversified_pool_are_exact(oracle):
    """rows without an extra element: the entry is ONE rounded product (the other fifteen terms are zeros) -- equal to the
    reference-order dot product; pools that hold extra elements: the two products and their sum are exact in f32 (and the
    rows are binary16 numbers, so the same holds for a binary16 index)"""
    import mmr_restatement as R
    seen = 0
    for c in V.cases():
        if not c.diversify:
            continue
        for mode in c.modes[:1]:
            e = V.expected(c, mode)
            if e.status:
                continue
            cp = V.corpus(c.corpus)
            # the pool, not only the picks: the chain reads the Gram row of every pick against every candidate
            pool = V.expected(V.Case(c.entry, c.plan, c.state, c.corpus, c.need, c.w_e, c.w_l, zip(c.lex_rows, c.lex_scores),
                                     k=c.need, diversify=1, lam=1.0), mode)
            rows = np.unique(pool.rows.astype(np.int64))
            g = cp.gram(rows)
            assert np.array_equal(bits(R.gram(oracle, cp.rows()[rows])), bits(g)), c.describe()
            if cp.col[rows].any():
                a, b = cp.cos[rows].astype(np.float64), cp.val[rows].astype(np.float64)
                same = cp.col[rows][:, None] == cp.col[rows][None, :]
                p0, p1 = np.outer(a, a), np.where(same, np.outer(b, b), 0.0)
                for x in (p0, p1, p0 + p1):
                    assert np.array_equal(x.astype(np.float32).astype(np.float64), x), c.describe()
            seen += 1
    assert seen >= 20


@pytest.mark.parametrize("entry,name", ALL)
def test_restatement_equals_the_oracle_on_every_status_0_case(oracle, entry, name):
    checked = 0
    for i, c in enumerate(V.plan(entry, name)):
        e = V.want(entry, name, i, c.modes[0])
        if e.status:
            continue
        cp = V.corpus(c.corpus)
        rows = cp.rows()
        need = min(c.need, cp.n)
        lex = [(int(r), float(s)) for r, s in zip(c.lex_rows, c.lex_scores)] or None
        wr, wc, we, wl = oracle.search(rows, E0, -(-need // 3), float(c.w_e), float(c.w_l), lex=lex, stage=1)
        wr, wc, we, wl = wr[:need], wc[:need], we[:need], wl[:need]
        if c.diversify:
            order, _ = oracle.mmr(rows[wr.astype(np.int64)], wc, max(c.k, 1), float(c.lam))
            wr, wc, we, wl = wr[order], wc[order], we[order], wl[order]
            if need == max(3 * c.k, c.k + 10) and 0 < c.lam <= 1 and cp.n >= need:
                dr, dc, de, dl = oracle.search_with_diversity(rows, E0, c.k, float(c.lam), float(c.w_e), float(c.w_l), lex=lex)
                assert np.array_equal(dr, wr) and np.array_equal(bits(dc), bits(wc)) and np.array_equal(bits(dl), bits(wl))
        what = c.describe()
        assert e.n == wr.size and np.array_equal(e.rows, wr), what
        assert np.array_equal(bits(e.comb), bits(wc)) and np.array_equal(bits(e.cos), bits(we)), what
        assert np.array_equal(bits(e.lex), bits(wl)), what
        checked += 1
    assert checked >= 1 or name == "overflow"


@pytest.mark.parametrize("entry,name", ALL)
def test_statuses_are_the_promised_ones_and_the_band_stays_small(entry, name):
    """hash, reach, arith, zeros, classes and sizes: status 0 in every case and mode (the refused sizes of the gate aside,
    which list their status) -- a condition, not a measurement; boundary, chains and overflow list every status.  Outside
    the overflow plans at most 256 rows beyond the fetch lie within 2^-10 of the fetch-th cosine (the nomination band is
    about 2 * rlr_default_guard_eps(16) = 2^-16.6 wide), so the candidate list never overflows and the status is the
    restatement's to predict."""
    for i, c, mode, e in each(entry, name):
        what = (c.describe(), mode)
        if c.expect is not None:
            assert e.status == c.expect[mode], what
        else:
            assert e.status == 0, what
        if entry == "hybrid" and name in V.STATUS_0_PLANS:
            assert e.status == 0 or c.state == "gate_refused", what
        if name in ("boundary", "chains", "overflow"):
            assert c.expect is not None and set(c.expect) == set(c.modes), what
        if name != "overflow" and not e.info.get("gate"):
            assert e.info["near"] + e.info["tied_beyond"] <= 256, what
            if c.entry == "diverse" and e.info["fetch"] <= V.FROM_CANDIDATES_MAX:
                assert e.info["fetch"] + 256 <= 1024


def test_every_code_form_of_pool_prepare_is_reached():
    """fetch <= 512 (pool_prepare_kernel<true> / the fused tail) and fetch > 512 (sort_emit + pool_prepare_kernel<false>) in
    every plan of rlr_search_diverse"""
    for name in V.DIVERSE_PLANS:
        f = [V.fetch_of(c, "tail0", V.corpus(c.corpus).n)[0] for c in V.plan("diverse", name)]
        assert min(f) <= 512 < max(f), name
    # both sides of the boundary rule in each form
    for small in (True, False):
        sides = {c.state for c in V.plan("diverse", "boundary")
                 if (V.fetch_of(c, "tail0", V.corpus(c.corpus).n)[0] <= 512) == small}
        assert sides == {"one_ulp_above", "equal"}, (small, sides)


def test_hash_plan_reaches_its_chains():
    st = {}
    for i, c, mode, e in each("hybrid", "hash"):
        if c.state != "gate_refused":
            st[c.state, mode] = V.hash_state(c, mode)
    one = st["one_bucket", "default"]
    assert one["longest_run"] >= 16 and one["longest_probe"] >= 15 and not one["wraps"] and one["walkers"] >= 4
    assert one["fetched_lex"] == 16
    w = st["wrap_all_fetched", "default"]
    assert w["wraps"] and w["longest_run"] == 128 and w["fetched_lex"] == 128 and w["unfetched_lex"] == 0
    assert w["fetched_lex_wrapped"] >= 100                       # whoever is stored last in the wrapped chain is a fetched row
    assert w["walkers"] >= 100 and w["longest_walk"] >= 64        # rows of buckets 0..119 walk to the end of the chain
    p = st["wrap_partly_fetched", "default"]
    assert p["wraps"] and p["fetched_lex"] >= 5 and p["unfetched_lex"] >= 64
    for mode in V.HYBRID_MODES:
        assert st["gate_max_need_1", mode]["unfetched_lex"] == 2043
        g = st["gate_max_need_1024", mode]
        assert g["fetched_lex"] + g["unfetched_lex"] == 1532 and g["wraps"] and g["fetched_lex"] >= 128
    d = st["dense_table", "default"]
    assert d["wraps"] and d["longest_run"] >= 128
    refused = [c for c in V.plan("hybrid", "hash") if c.state == "gate_refused"]
    assert sorted((c.need, c.n_lex) for c in refused) == [(1, 2044), (1024, 1533)]
    for c in V.plan("hybrid", "hash") + V.plan("hybrid", "sizes"):
        if c.state in ("gate_max_need_1", "gate_max_need_1024", "slots_full"):
            assert (c.need + 2 * c.n_lex + 8 == 4096) == (c.state == "slots_full" or c.need == 1024), c.describe()
            assert c.need + 2 * c.n_lex + 8 <= 4096


def test_reach_plan_reaches_its_states():
    st = {c.state: V.hash_state(c, "default") for c in V.plan("hybrid", "reach")}
    assert st["all_inside"]["unfetched_lex"] == 0 and st["all_inside"]["fetched_lex"] == 25
    assert st["none_inside"]["fetched_lex"] == 0 and st["none_inside"]["unfetched_lex"] >= 20
    assert st["half_inside"]["fetched_lex"] == 10 and st["half_inside"]["unfetched_lex"] == 10
    assert st["n_lex_0"]["fetched_lex"] == st["n_lex_0"]["unfetched_lex"] == 0
    c = next(c for c in V.plan("hybrid", "reach") if c.state == "lex_is_last_fetched")
    for mode in V.HYBRID_MODES:
        cp = V.corpus(c.corpus)
        assert int(cp.head[V.fetch_of(c, mode, cp.n)[0] - 1]) in set(c.lex_rows.tolist())


def test_arith_plan_holds_the_triples_and_pairs_that_tell_the_forms_apart():
    """reported rows whose combined score differs under a contracted fma(w_e, cos, t1), and reported lexical scores that
    differ under lex * (1 / max_lex): both in every `fma_and_division` case"""
    for i, c, mode, e in each("hybrid", "arith"):
        if c.state == "fma_and_division":
            f, d = V.expected(c, mode, "fma"), V.expected(c, mode, "recip_division")
            assert (bits(f.comb) != bits(e.comb)).sum() >= 3 or not np.array_equal(f.rows, e.rows), c.describe()
            assert (bits(d.lex) != bits(e.lex)).sum() >= 3 or not np.array_equal(d.rows, e.rows), c.describe()
        if c.state == "nan_lexical":
            assert np.isnan(e.lex[-3:]).all() and np.isnan(e.comb[-3:]).all() and e.rows[-3:].tolist() == [3, 5, 11]
            assert not np.isnan(e.comb[:-3]).any()
        if c.state == "max_lex_epsilon":
            assert c.max_lex == V.EPS
        if c.state == "negative_w_l":
            assert c.w_l < 0
        if c.state == "negative_lexical":
            assert (c.lex_scores < 0).sum() >= 3 and (e.lex < 0).any()


def test_zeros_plans_cut_inside_a_class_of_both_signs():
    for entry in ("hybrid", "diverse"):
        states = collections.Counter()
        for i, c, mode, e in each(entry, "zeros"):
            cp = V.corpus(c.corpus)
            with np.errstate(all="ignore"):
                l = np.zeros(cp.n, np.float32)
                l[c.lex_rows.astype(np.int64)] = c.lex_scores / c.max_lex
                comb = (c.w_e * cp.cos + c.w_l * l).astype(np.float32)
            zero = np.flatnonzero(comb == 0)
            rank_lo, rank_hi = int((comb > 0).sum()), int((comb > 0).sum()) + zero.size
            assert rank_lo < min(c.need, cp.n) < rank_hi, c.describe()           # the cut falls inside the class of zeros
            signs = np.signbit(comb[zero])
            states["both" if signs.any() and not signs.all() else "minus" if signs.all() else "plus"] += 1
            if signs.any() and not signs.all():
                # interleaved by row: ordering -0 below +0 changes the pool
                assert not V.same(e, V.expected(c, mode, "neg_zero_below")), c.describe()
            if c.state == "minus_w_l":
                assert signs.any() and not signs.all() and np.signbit(c.w_l)
            if c.state == "cancellation":
                assert zero.size == 4 and not signs.any()
        assert states["both"] >= 4 and states["plus"] >= 1, (entry, states)


def test_classes_plan_walks_one_two_and_more_digits():
    """the digit walk of lds_kth_key64 over the keys of every case: 1, 2 and >= 3 passes occur, it ends both by `done` above the last digit
    and at `shift == 0`, and between need and need + 32 keys reach key_lo in every case"""
    passes, ends = collections.Counter(), collections.Counter()
    for i, c, mode, e in each("hybrid", "classes"):
        keys, n_cand = V.slot_keys(c, mode)
        need = min(c.need, V.corpus(c.corpus).n)
        if n_cand <= need:
            continue
        key_lo, n_pass, end, reach = V.kth_trace(keys, need)
        assert need <= reach <= need + V.KTH_SLACK, (c.describe(), mode, reach)
        passes[min(n_pass, 3)] += 1
        ends[end] += 1
    assert passes[1] and passes[2] and passes[3], passes
    assert ends["done"] and ends["shift0"], ends
    big = [c for c in V.plan("hybrid", "classes") if c.state.startswith("one_score")]
    assert max(c.n_lex for c in big) == 2043 and any(c.n_lex == 1500 and 1 < c.need < 1500 for c in big)


def test_every_hybrid_case_keeps_the_select_within_its_slack():
    for c in V.cases("hybrid"):
        for mode in c.modes:
            e = V.expected(c, mode)
            if e.info.get("gate") or e.status == 1:
                continue
            keys, n_cand = V.slot_keys(c, mode)
            need = min(c.need, V.corpus(c.corpus).n)
            assert n_cand == e.info["n_cand"]
            if n_cand > need:
                assert need <= V.kth_trace(keys, need)[3] <= need + V.KTH_SLACK, c.describe()


def test_boundary_cases_stand_on_the_side_they_name():
    for entry, name in (("hybrid", "boundary"), ("diverse", "boundary"), ("diverse", "chains")):
        for i, c, mode, e in each(entry, name):
            c_need, c_tail = e.info["c_need"], e.info["c_tail"]
            up, down = np.nextafter(c_tail, np.float32(np.inf)), np.nextafter(c_tail, np.float32(-np.inf))
            if c.state.startswith("one_ulp_above"):
                assert e.status == 0 and (c_need == up or mode == "full"), (c.describe(), mode)
            if c.state in ("equal", "chain_reaches_last") or (c.state == "equal_from_outside" and mode == "default"):
                assert c_need == c_tail and e.status == 2, (c.describe(), mode)
            if c.state == "one_ulp_below" and mode == "default":
                assert c_need == down and e.status == 2, (c.describe(), mode)
            if c.state == "chain_stops_before":
                cp = V.corpus(c.corpus)
                assert e.status == 0 and c_need > c_tail
                # the pool's end is the chain: distinct cosines, one combined score, ordered by row and NOT by cosine
                pool = V.expected(V.Case(c.entry, c.plan, c.state, c.corpus, c.need, c.w_e, c.w_l, k=c.need, diversify=0
                                         if entry == "hybrid" else 1, lam=1.0), mode)
                tail = np.sort(pool.rows.astype(np.int64))[-57:] if entry == "diverse" else pool.rows.astype(np.int64)[-57:]
                assert np.unique(cp.cos[tail]).size == 57
            if c.state == "chains_of_two" and c.corpus != "chain16":
                cp = V.corpus(c.corpus)
                chain = cp.head[int(c.corpus[5:]):][:64]
                assert np.unique((np.float32(0.7) * cp.cos[chain]).astype(np.float32)).size == 45
    modes_differ = [c for c in V.plan("hybrid", "boundary") if c.expect["default"] != c.expect["full"]]
    assert len(modes_differ) >= 3


def test_emit_plan_spans_three_greedy_kernels_and_reorders():
    strides = set()
    for i, c, mode, e in each("hybrid", "emit"):
        strides.add(c.need)
        if c.n_lex:
            assert (e.lex != 0).any() and not V.same(e, V.expected(c, mode, "lex_pool_order")), c.describe()
        assert not np.array_equal(e.info["picks"], np.arange(e.n)), c.describe()
    assert {60, 120, 300} <= strides                                # J = 1, 2, 5 of the register-resident greedy kernel


# which plan has to notice which planted defect (entry, plan)
NOTICED_BY = {
    "fma": ("hybrid", "arith"),
    "recip_division": ("hybrid", "arith"),
    "neg_zero_below": ("diverse", "zeros"),
    "boundary_ge": ("hybrid", "boundary"),
    "tail_from_largest": ("hybrid", "reach"),
    "flag_ignored": ("hybrid", "reach"),
    "probe_no_wrap": ("hybrid", "hash"),
    "drop_unfetched": ("hybrid", "reach"),
    "ties_desc": ("hybrid", "classes"),
    "nan_first": ("hybrid", "arith"),
    "cut_need_plus_1": ("hybrid", "sizes"),
    "lex_pool_order": ("hybrid", "emit"),
}


@pytest.mark.parametrize("defect", V.DEFECTS)
def test_every_planted_defect_is_noticed(defect):
    entry, name = NOTICED_BY[defect]
    seen = [c.describe() for i, c, mode, e in each(entry, name) if not V.same(e, V.expected(c, mode, defect))]
    assert seen, f"no case of {entry}/{name} notices the planted defect {defect}"
    print(f"{defect}: noticed by {len(seen)} case(s) of {entry}/{name}, first {seen[0]}")


def test_neg_zero_defect_is_noticed_by_both_entries():
    for entry in ("hybrid", "diverse"):
        assert any(not V.same(e, V.expected(c, mode, "neg_zero_below")) for i, c, mode, e in each(entry, "zeros")), entry


def test_defect_table_is_complete():
    assert set(NOTICED_BY) == set(V.DEFECTS) and len(V.DEFECTS) == 12


def test_text_batch_queries_reach_their_states_and_equal_the_oracle(oracle):
    """the batch of test_gpu_pool.py: the BM25 pairs of oracle/lexical.py put the queries into the states they name, one
    query fails the boundary rule and every other one is status 0 and equals the C oracle"""
    o = V.text_oracle()
    rows = V.corpus("text").rows()
    seen = {}
    for state, text, axis in V.TEXT_QUERIES:
        pairs = V.text_pairs(o, text)
        c = V.text_case(state, axis, pairs)
        e = V.expected(c, "batch")
        seen[state] = (len(pairs), c.n_lex, e.status)
        assert e.info["near"] + e.info["tied_beyond"] <= 256
        q = np.zeros(V.DIM, np.float32)
        q[axis] = 1.0
        assert np.array_equal(bits(oracle.scan(rows, q)), bits(V.corpus(c.corpus).cos))
        if e.status == 0:
            wr, wc, we, wl = oracle.search(rows, q, V.TEXT_TOP_K, lex=pairs or None, stage=1)
            assert np.array_equal(e.rows, wr) and np.array_equal(bits(e.comb), bits(wc)) and np.array_equal(bits(e.lex), bits(wl))
            assert np.array_equal(bits(e.cos), bits(we))
    assert seen == {"unknown_token": (0, 0, 0), "one_row": (1, 1, 0), "more_rows_than_the_limit": (50, 50, 0),
                    "all_rows_outside_the_index": (5, 0, 0), "boundary_rule_fails": (1, 1, 2)}
    assert sum(1 for t in V.text_rows() if t == "many") > 5 * V.TEXT_TOP_K
