"""The Gram readout plans (gram_vectors.py) checked without a GPU: on the reference-order Gram matrix every pool picks
[0, a, b] (or [0, b]) and logs exactly -G[a][b] / 2; the read pairs cover every residue pair of every tile class of the
instance the shape reaches; and the rows are such that a kernel with one of the modelled faults computes other bits -- a
condition on the inputs, met by the reference alone -- and that every changed entry changes what its pool logs.
Each sensitivity test prints the fractions it measured (pytest -s shows them; DESIGN.md records them)."""
import numpy as np
import pytest

import gram_vectors as V
import mmr_restatement as R
from conftest import bits

T_OF = {r[3]: r[4] for r in V.GRAM_RULES}
# one case per corpus and set of read pairs (the single-pool form of the 37-slot shape reads the pairs of the batched one)
CORPORA = [c for c in V.cases() if c[0] != "r1_384_single"]


def setup(name, dim, dtype):
    s = V.shape(name)
    rows, g = V.corpus_and_gram(s["P"], dim, dtype == "f16")
    return s, rows, g, V.shape_plans(name)


# ---------------------------------------------------------------- the restated rules
def test_every_shape_reaches_the_instance_it_names():
    for s in V.SHAPES:
        for dtype in s["dtypes"]:
            assert s["pools"] <= V.pools_per_pass(s["P"]) or s["pools"] == 1
            assert V.gram_instance(dtype, s["pools"], s["P"])[0] == s["instance"], (s["name"], dtype)
    assert 8 <= V.shape("r4_64_f16")["pools"] < 16           # from 16 pools a binary16 pass is the matrix-core kernel's
    assert min(d for s in V.SHAPES for d in s["dims"]) >= 132   # the widths the sensitivity floors were set at
    reached = {next(j for lim, j in V.GREEDY_J if s["P"] <= lim) for s in V.SHAPES if s["P"] <= 1024}
    assert reached == {1, 2, 5, 8}


def test_rule_thresholds():
    assert V.gram_instance("f32", 1, 496)[0] == "gram_tiled<1,384>" and V.gram_instance("f32", 1, 497)[0] == "gram_tiled<1,128>"
    assert V.gram_instance("f16", 15, 40)[0] == "gram_tiled<4,64>" and V.gram_instance("f16", 16, 40)[0] == "gram_mfma_f32_kernel"
    assert V.gram_instance("f32", 7, 40)[0] == "gram_tiled<1,384>" and V.gram_instance("f32", 8, 40)[0] == "gram_tiled<4,64>"
    assert V.gram_instance("f32", 1, 864)[0] == "gram_tiled<1,128>" and V.gram_instance("f32", 1, 865)[0] == "gram_tiled<2,64>"
    assert V.pools_per_pass(33) == 4096 and V.pools_per_pass(1024) == 765 and V.pools_per_pass(4096) == 64


# ---------------------------------------------------------------- the two restatements the rest relies on
@pytest.mark.parametrize("dim,f16", [(132, False), (390, False), (140, True), (1024, True)])
def test_the_numpy_chain_is_the_oracles_dot(oracle, dim, f16):
    rows, g = V.corpus_and_gram(37, dim, f16)
    ia, ib = np.divmod(np.arange(38 * 38), 38)
    assert np.array_equal(bits(V.variant_dots(rows, ia, ib, "reference", 4)), bits(g[ia, ib]))
    assert np.array_equal(bits(g), bits(g.T))                  # dot(i, j) == dot(j, i) bitwise: one matrix serves both orders


def loop_pool(g, plan, q, override=None):
    s = int(plan.sizes[q])
    pr = plan.pool_rows[q, :s].astype(np.int64)
    gp = g[pr][:, pr].copy()
    if override is not None:
        gp[plan.a[q], plan.b[q]] = override[q]
    return R.mmr_from_gram(gp, plan.rel[q, :s], plan.k, plan.lam)


@pytest.mark.parametrize("name", ["r1_384", "r2_64", "mfma_70", "single_1030"])
def test_the_batched_loop_is_the_restatement(oracle, name):
    """mmr_batch against mmr_from_gram pool by pool: on the true matrix, with an entry raised, lowered past another,
    made negative, NaN and -inf, and for ragged pools"""
    s = V.shape(name)
    rows, g = V.corpus_and_gram(s["P"], s["dims"][0], False)
    rng = np.random.default_rng(5)
    plans = V.shape_plans(name) + ([V.ragged_plan(130, (129, 65, 33), 64)] if name == "r1_384" else [])
    for plan in plans:
        if plan.P == 130:
            rows, g = V.corpus_and_gram(130, 132, False)
        sample = np.arange(plan.Q) if plan.Q <= 1300 else rng.choice(plan.Q, 150, replace=False)
        true = V.read_entries(plan, g)
        for ov in (None, true * np.float32(1.5), -true, np.full(plan.Q, np.nan, np.float32), np.full(plan.Q, -np.inf, np.float32)):
            order, logged, n = V.expected(plan, g, None if ov is None else (plan.a, plan.b, ov))
            for q in (sample if ov is None else sample[:100]):
                wo, wl = loop_pool(g, plan, q, ov)
                assert n[q] == len(wo) == plan.k, (name, q)
                assert np.array_equal(order[q, : n[q]], wo) and np.array_equal(bits(logged[q, 1: n[q]]), bits(wl[1:])), (name, q)


# ---------------------------------------------------------------- what every pool reads
def check_reads(plan, g):
    order, logged, n = V.expected(plan, g)
    entry = V.read_entries(plan, g)
    assert np.isfinite(entry).all() and (entry >= 2.0 ** -100).all()
    assert (n == plan.k).all()
    assert (order[:, 0] == 0).all() and np.array_equal(order[:, -1], plan.b)
    if plan.k == 3:
        assert np.array_equal(order[:, 1], plan.a) and (logged[:, 1] == 2.0).all()
    assert np.array_equal(bits(np.float32(-2.0) * logged[:, -1]), bits(entry))
    return entry


@pytest.mark.parametrize("name,dim,dtype", V.cases())
def test_every_pool_reads_its_entry(oracle, name, dim, dtype):
    s, rows, g, plans = setup(name, dim, dtype)
    assert rows.shape == (s["P"] + 1, dim) and not rows[0].any()
    for plan in plans:
        assert plan.Q % s["pools"] == 0 and plan.pools == s["pools"]
        three = plan.k == 3
        assert (plan.pool_rows[:, 0] == 0).all() == three    # the zero row in slot 0, or a real one
        srt = np.sort(plan.pool_rows[:, 1:].astype(np.int64), axis=1)
        assert (np.diff(srt, axis=1) > 0).all() and (srt[:, 0] >= 1).all()     # distinct real rows
        assert len({r.tobytes() for r in plan.pool_rows}) == plan.Q             # no two pools share a layout
        fin = np.isfinite(plan.rel)
        assert (fin.sum(axis=1) == plan.k - 1).all()
        check_reads(plan, g)
    entry = np.concatenate([V.read_entries(p, g) for p in plans])
    ra, rb = corpus_pairs(plans)
    n_pairs = np.unique(np.stack([np.minimum(ra, rb), np.maximum(ra, rb)]), axis=1).shape[1]
    print(f"{name} {dim} {dtype}: {entry.size} reads, entries {entry.min():.3f}..{entry.max():.3f}, "
          f"bit-distinct {np.unique(bits(entry)).size / n_pairs:.4f}")


def corpus_pairs(plans):
    ra = np.concatenate([p.pool_rows[np.arange(p.Q), p.a] for p in plans]).astype(np.int64)
    rb = np.concatenate([p.pool_rows[np.arange(p.Q), p.b] for p in plans]).astype(np.int64)
    return ra, rb


def test_ragged_and_class_plans_read_what_they_say(oracle):
    rows, g = V.corpus_and_gram(130, 132, False)
    plan = V.ragged_plan(130, (129, 65, 33), 256)
    assert set(plan.sizes.tolist()) == {129, 65, 33} and all(len(set(plan.sizes[c].tolist())) == 3 for c in plan.calls())
    check_reads(plan, g)
    for s in (129, 65, 33):                                   # the last slot of every size, as row and as column
        assert ((plan.sizes == s) & (plan.a == s - 1)).any() and ((plan.sizes == s) & (plan.b == s - 1)).any()
    for f16, T in ((False, 64), (True, 64), (True, 32)):
        crows, special = V.class_corpus(oracle, 130, 132, f16)
        cplan = V.class_plan(130, T, 256, 130, special)
        cg = R.gram(oracle, crows)
        order, logged, n = V.expected(cplan, cg)
        sp = slice(0, cplan.n_special)
        entry = V.read_entries(cplan, cg)[sp]
        assert not (np.isfinite(entry) & (entry > 0)).any()    # nothing a maximum over the finite values would take from +0.0
        assert np.isnan(entry).any() and np.isinf(entry).any() and (entry < 0).any() and (entry == 0).any()
        assert (n[sp] == 3).all() and np.array_equal(order[sp, 1], cplan.a[sp]) and np.array_equal(order[sp, 2], cplan.b[sp])
        assert (bits(logged[sp, 2]) == 0).all()                # +0.0
        a, b = cplan.a[sp], cplan.b[sp]
        for cname, pred in V.tile_classes(130, T).items():     # four positions x five kinds x both slots
            assert pred(a, b).sum() >= 4 * 10, cname


# ---------------------------------------------------------------- coverage
@pytest.mark.parametrize("name", [s["name"] for s in V.SHAPES])
def test_read_pairs_cover_every_residue_of_every_tile_class(name):
    s = V.shape(name)
    P, T = s["P"], T_OF[s["instance"]]
    plans = V.shape_plans(name)
    a = np.concatenate([p.a for p in plans])
    b = np.concatenate([p.b for p in plans])
    oa, ob = V.observable_pairs(P)
    if P <= V.EVERY_PAIR_MAX:                                  # simply every ordered pair, row 0 through the two-pick form
        assert set(zip(a.tolist(), b.tolist())) == set(zip(oa.tolist(), ob.tolist()))
        assert plans[1].k == 2 and set(plans[1].b.tolist()) == set(range(1, P))
    if P > 1024:                                               # the ragged last rows x every column residue, both orders
        lo = (P - 1) // T * T
        for r in range(lo, P):
            assert {x % T for x in b[a == r].tolist()} == set(range(T)), r
            assert {x % T for x in a[b == r].tolist()} == set(range(T)), r
        return
    nb = (P + T - 1) // T
    full = T * T
    for cname, pred in V.tile_classes(P, T, mfma=s["instance"] == "gram_mfma_f32_kernel").items():
        got = V.residues(a[pred(a, b)], b[pred(a, b)], T)
        want = V.residues(oa[pred(oa, ob)], ob[pred(oa, ob)], T)
        assert got == want, (name, cname, sorted(want - got)[:8])
        rag = P - (nb - 1) * T
        # what "every observable residue pair" comes to once a class has a column block besides the one that holds slot 0:
        # all T x T (less the diagonal in diagonal blocks), rag x T in the ragged blocks
        if nb >= 4:
            full_count = {"diagonal": full - T, "lower": full, "upper": full, "ragged_row": rag * T, "ragged_col": rag * T,
                          "ragged_diagonal": rag * (rag - 1)}
            assert cname not in full_count or len(got) == full_count[cname], (name, cname, len(got))
        if cname in ("lower", "upper", "pair_second"):          # (two blocks: no full block off the diagonal, and the second tile
            assert len(got) > 0 or nb < 3, (name, cname)         # row's own entries are one ragged row's diagonal)
        elif cname == "unpaired_row":
            assert (len(got) > 0) == (nb % 2 == 1), (name, cname)
        elif cname == "ragged_diagonal":
            assert len(got) == rag * (rag - 1), (name, cname)    # (one ragged row: its only entry there is the diagonal)
        else:
            assert len(got) > 0, (name, cname)
    if s["instance"] == "gram_mfma_f32_kernel" and nb % 2:      # the unpaired tile row exists and is read whole
        pred = V.tile_classes(P, T, mfma=True)["unpaired_row"]
        assert pred(a, b).sum() >= rag * (rag - 1)


# ---------------------------------------------------------------- fault sensitivity
def unit_of(dtype):
    return 8 if dtype == "f16" else 4


@pytest.mark.parametrize("name,dim,dtype", CORPORA)
def test_entry_faults_change_every_entry_and_every_log(oracle, name, dim, dtype):
    """(i) one ulp up or down, (ii) the entry of another slot of the pool's own matrix, wherever that slot exists: the pool
    then logs something else.  (Two entries of a matrix can hold the same bits -- 1 to 16 pairs in 10 000 per corpus -- and an
    entry replaced by an equal one is no fault: at most one replacement in a thousand may meet that.)"""
    s, rows, g, plans = setup(name, dim, dtype)
    n_same = n_applies = 0
    for plan in plans:
        entry = V.read_entries(plan, g)
        want = V.expected(plan, g)
        faults = [(np.nextafter(entry, np.float32(np.inf)), np.ones(plan.Q, bool)),
                  (np.nextafter(entry, np.float32(-np.inf)), np.ones(plan.Q, bool))]
        faults += [V.shifted_entries(plan, g, da, db) for da, db in V.SHIFTS]
        for val, applies in faults:
            same = applies & (bits(val) == bits(entry))
            n_same, n_applies = n_same + int(same.sum()), n_applies + int(applies.sum())
            applies = applies & ~same
            got = V.expected(plan, g, (plan.a, plan.b, np.where(applies, val, entry)))
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[2], want[2])
            assert np.array_equal(bits(got[1][:, -1]) != bits(want[1][:, -1]), applies)
    assert n_same <= 0.001 * n_applies, (n_same, n_applies)


@pytest.mark.parametrize("name,dim,dtype", CORPORA)
def test_summation_faults_change_the_entries_and_the_logs(oracle, name, dim, dtype):
    """(iii) omitted last element / last aligned unit: every read entry; (iv) four interleaved chains, (v) a partial sum per
    64-column chunk, (vi) reversed order: at least 0.70 of them; (vii) fused steps (f32 rows): at least 0.30.  With the faulty
    matrix in place of the true one, the plan's pools disagree with the expectation exactly where the entry changed."""
    s, rows, g, plans = setup(name, dim, dtype)
    ra, rb = corpus_pairs(plans)
    lo, hi = np.minimum(ra, rb), np.maximum(ra, rb)
    pairs = np.unique(np.stack([lo, hi]), axis=1)
    ia, ib = pairs[0], pairs[1]
    assert np.array_equal(bits(V.variant_dots(rows, ia, ib, "reference", unit_of(dtype))), bits(g[ia, ib]))
    floors = dict(drop_last=1.0, drop_unit=1.0, four_chains=0.70, chunk64=0.70, reversed=0.70, fused=0.30)
    report = []
    for model in V.CHAIN_MODELS:
        if model == "fused" and dtype == "f16":
            continue
        bad = g.copy()
        bad[ia, ib] = bad[ib, ia] = V.variant_dots(rows, ia, ib, model, unit_of(dtype))
        frac = []
        for plan in plans:
            entry, wrong = V.read_entries(plan, g), V.read_entries(plan, bad)
            changed = bits(entry) != bits(wrong)
            frac.append(changed)
            want, got = V.expected(plan, g), V.expected(plan, bad)
            assert np.array_equal(bits(got[1][:, -1]) != bits(want[1][:, -1]), changed), model
        f = float(np.concatenate(frac).mean())
        report.append(f"{model} {f:.3f}")
        assert f >= floors[model], (name, dim, dtype, model, f)
    print(f"{name} {dim} {dtype}: " + ", ".join(report))
