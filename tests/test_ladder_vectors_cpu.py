"""The ladder corpora (ladder_vectors.py) checked without a GPU, for every corpus test_gpu_positions.py uses.  Each path's
nominations are modelled as in test_band_vectors_cpu.py -- the binary64 dot of the operands for the f32 scans, of the
binary16-rounded operands for the matrix-core batch and the image, of the dequantised rows for the 8-bit copy -- and the
select is band_vectors.select.  Proved per corpus:
  1  the oracle's top-k of every ladder query is its checked set, on the requested rows; every modelled nomination lies
     within eps of the true score; the k-th lies in edge's bin; the model collects exactly W = 2k candidates
  2  lower the nomination of ANY one checked row by 5 eps: the modelled result differs from the oracle's
  3  omit any one aligned 16-byte unit of a checked row's operand (f32 rows 4 elements, binary16 operands 8, 8-bit codes
     16), or exchange any two units that differ: the row is lost.  Where the band is wider than one unit, the smallest
     run of units that is caught is measured and bounded, and the share of differing pairs whose exchange is caught has
     a floor per family (the 8-bit copy's from the binomial count of differing signs)
  4  lower every checked row of a query that shares one 8-row group, one 64-row span or one 256-row tile by 5 eps
     together: the result still differs
The shard corpus is proved under the select its path runs: every shard selects with the full k among its own rows, then
the results are merged (sharded_select) -- which is why each of its ladders lives inside one shard.  The masks of the
masked-scan tests are proved to leave each `alone` checked row the only allowed row of its unit.
Each test prints what it measured (pytest -s): the smallest multiple of eps that is caught on every checked row, the
smallest run of units, the share of unit pairs whose exchange is caught.

Measured (smallest fault caught on every checked row, in eps | run of 16-byte units omitted | differing pairs exchanged):
  f32 scans, f32 rows       128-d .. 1536-d 4.0-4.25 | 1 | all
  f32 scans, binary16 rows  72-d .. 1536-d 4.0-4.25 | 1 | 0.997-0.9998 (the rest differ in a remainder element only)
  binary16 operands         768-d f32 rows 4.0 | 1 | 0.98      1024-d binary16 rows 4.0 | 1 | 0.9996
  8-bit copy                128-d 4.0 | 1 | all      400-d 4.0 | 2 | 0.99      768-d 4.0 | 2 | 0.82"""
import numpy as np
import pytest

import ladder_vectors as L

UNIT_ELEMS = {"scan": {"f32": 4, "f16": 8}, "binary16": {"f32": 8, "f16": 8}, "q8": {"q8": 16}}
FAULT = 5.0                    # eps: what the construction promises to catch (ladder_vectors.py's header)


def bin_below(edge):
    return float(L.bin_floor(np.nextafter(edge, 0.0)))


def not_collected(others_desc, new, k, band):
    """a row of the oracle's top-k nominated at `new` (array) next to the other W - 1 rungs: is it left out of the
    candidates?  The k-th nominated score is the k-th of (others + new); the rest of the top-k was collected before and
    the floor only moves down, so the result differs from the oracle's exactly when this row is not collected."""
    kth = np.maximum(others_desc[k - 1], np.minimum(new, others_desc[k - 2])) if k > 1 else np.maximum(others_desc[0], new)
    return new < L.bin_floor(kth) - band


def sharded_select(nominated, exact, rows, bounds, k, band):
    """the result of MultiGpuIndex as a model: every shard [bounds[i], bounds[i + 1]) selects its own top-k with the full k
    among ITS rows -- where it holds fewer than k rungs its k-th nominated score is a filler row's (below 0.6, many bins
    down) and everything it holds is collected --, then the shards' results are merged by (exact desc, row asc).
    nominated / exact / rows: the rungs of one query, rows ascending.  -> indices into them"""
    kept = []
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        loc = np.flatnonzero((rows >= lo) & (rows < hi))
        if len(loc) >= k:
            kept += list(loc[L.select(nominated[loc], exact[loc], k, band)])
        else:
            kept += list(loc)
    kept = np.array(sorted(kept))
    return kept[np.lexsort((kept, -exact[kept].astype(np.float64)))[:k]]


def analyse(O, name):
    rows, qs, f = L.corpus(name)
    k, W, edge, eps, fam, kind, dim = f["k"], f["W"], f["edge"], f["eps"], f["family"], f["kind"], f["dim"]
    band = 2.0 * eps
    n = len(rows)
    assert rows.shape == (n, dim) and n == f["n"] and n % 8 and n % 64 and n % 256
    per = UNIT_ELEMS[fam][kind]
    assert dim % per == 0
    U = dim // per
    # norms: the unit band applies
    rn = float(np.sqrt((rows.astype(np.float64) ** 2).sum(axis=1).max()))
    qn = float(np.linalg.norm(qs.astype(np.float64), axis=1).max())
    assert rn * qn <= 1.0001 and rn + qn <= 2.0001, (name, rn, qn)
    if kind == "f16":
        assert np.array_equal(rows.view(np.uint32), L.to_f16(rows).view(np.uint32))
    # every row outside a query's ladder: below the bin under edge, minus the band, with the model's error to spare
    cross = rows @ qs.T
    for g in range(f["G"]):
        cross[f["rungs"][g], g] = -np.inf
    assert float(cross.max()) + 2.0 * eps < min(L.OTHERS_BELOW, bin_below(edge) - band), (name, float(cross.max()))
    del cross
    stats = dict(min_eps=0.0, units=1, pairs_differ=0, pairs_caught=0)
    multiples = np.arange(0.25, 8.01, 0.25)
    caught_at = np.ones(len(multiples), bool)
    run_needed = 1
    for g in range(f["G"]):
        idx = np.sort(f["rungs"][g])
        q = qs[g]
        e = O.scan(rows[idx], q)
        mr, mq = L.model_operands(rows[idx], q, fam, kind)
        nom = mr @ mq
        true = L.true_dot(rows[idx], q)
        # ---- 1
        top = idx[np.lexsort((idx, -e.astype(np.float64)))[:k]]
        assert set(top) == set(f["checked"][g]), (name, g)
        assert np.abs(nom - true).max() <= eps, (name, g, np.abs(nom - true).max() / eps)
        assert np.abs(e.astype(np.float64) - true).max() <= eps
        assert true.min() >= edge + 1.2 * eps and true.max() <= edge + 2.05 * eps, (name, g)
        assert L.bin_floor(np.sort(nom)[::-1][k - 1]) == edge, (name, g)
        assert int((nom >= edge - band).sum()) == W and nom.max() < edge + 0.125
        want = L.select(nom, e, k, band)
        assert np.array_equal(idx[want], top), (name, g)
        is_checked = np.isin(idx, f["checked"][g])
        if L.SPECS[name][5] == "shards":                      # the path selects per shard: the proof must too
            bounds = [0] + L.shard_cuts(n) + [n]
            assert len({int(np.searchsorted(bounds, r, side="right")) for r in idx}) == 1, "a ladder split over shards"
            assert np.array_equal(sharded_select(nom, e, idx, bounds, k, band), want)
            for j in np.flatnonzero(is_checked):
                low = nom.copy()
                low[j] -= FAULT * eps
                assert not np.array_equal(sharded_select(low, e, idx, bounds, k, band), want), (name, g, idx[j])
        for j in np.flatnonzero(is_checked):
            others = np.sort(np.delete(nom, j))[::-1]
            # ---- 2
            low = nom.copy()
            low[j] -= FAULT * eps
            got = L.select(low, e, k, band)
            assert not np.array_equal(got, want), (name, g, idx[j], "a nomination 5 eps low went unnoticed")
            assert not_collected(others, low[j:j + 1], k, band)[0]            # (the shortcut used below agrees)
            caught_at &= not_collected(others, nom[j] - multiples * eps, k, band)
            # ---- 3
            X, Q = mr[j].reshape(U, per), mq.reshape(U, per)
            M = X @ Q.T                                       # M[u, v]: unit u of the row against unit v of the query
            P = np.diag(M)
            run = 1
            while True:                                       # omit `run` consecutive units, from every start
                drop = np.convolve(P, np.ones(run), mode="valid")
                if not_collected(others, nom[j] - drop, k, band).all():
                    break
                run += 1
                assert run <= 4, (name, g, idx[j], "omitting four 16-byte units went unnoticed")
            run_needed = max(run_needed, run)
            drop2 = P[:, None] + P[None, :] - M - M.T         # exchange units u and v
            differ = (X[:, None, :] != X[None, :, :]).any(axis=2)
            gone = not_collected(others, nom[j] - drop2, k, band)
            assert gone[differ & (drop2 >= FAULT * eps)].all(), (name, g, idx[j])
            stats["pairs_differ"] += int(differ.sum())
            stats["pairs_caught"] += int((gone & differ).sum())
        # ---- 4
        for size in (8, 64, 256):
            for unit in np.unique(f["checked"][g] // size):
                low = nom.copy()
                low[is_checked & (idx // size == unit)] -= FAULT * eps
                assert not np.array_equal(L.select(low, e, k, band), want), (name, g, size, unit)
            assert np.bincount(idx // size).max() <= k
    assert caught_at[multiples >= FAULT].all()
    stats["min_eps"] = float(multiples[np.flatnonzero(~caught_at).max() + 1]) if (~caught_at).any() else float(multiples[0])
    stats["units"] = run_needed
    share = stats["pairs_caught"] / max(stats["pairs_differ"], 1)
    print(f"{name}: eps {eps:.3e}; caught on every checked row from {stats['min_eps']:.2f} eps; {run_needed} unit(s) of "
          f"{per} elements omitted; {share:.4f} of the differing unit pairs exchanged")
    return stats, share


def test_positions_cover_what_the_gpu_tests_claim():
    """every residue modulo 256 twice -- once in rows a wave reaches in its first trip, once behind 32 768 rows (131 072
    for the packed scans) --, every row of the ragged last tile, row 0 and row n - 1; the sampled batch's checked rows
    behind the sample and its lower rungs inside; the shards' on both sides of each cut"""
    for name, (dim, n, kind, fam, k, lay) in L.SPECS.items():
        pos, lower = L.layout(name)
        flat = pos.ravel()
        assert len(np.unique(flat)) == flat.size
        tail0 = n - n % 256
        assert n - 1 in flat and (lay in ("shards", "masked") or set(range(tail0, n)) <= set(flat))
        if lay == "shards":
            bounds = [0] + L.shard_cuts(n) + [n]
            assert len(lower) == len(pos) == 21
            for g in range(len(pos)):                         # a whole ladder inside one shard
                lo, hi = lower[g]
                assert (lo, hi) in list(zip(bounds[:-1], bounds[1:])) and ((pos[g] >= lo) & (pos[g] < hi)).all()
            for lo, hi in zip(bounds[:-1], bounds[1:]):      # both sides of every cut, the whole ragged tile of each shard
                assert set(range(lo, lo + 32)) | set(range(hi - 192, hi)) <= set(flat)
                assert (hi - lo) % 256 <= 192 and (hi - lo) % 8 and (hi - lo) % 64
            continue
        if lay == "masked":
            alone, full = L.masked_sets(n)
            assert set(alone) | set(full) <= set(flat)
            assert set(alone[:64] % 64) == set(alone[64:128] % 64) == set(range(64)) and (alone[64:128] >= 8192).all()
            assert set(alone % 16) == set(range(16)) and {0, 63} <= set(alone % 64)
            assert (alone[128:] >= n - n % 64).all() and n - 1 in alone and len(alone) == 132
            continue
        if lay == "sampled":
            assert flat.min() >= L.SAMPLE and lower == (0, L.SAMPLE)
            assert set(flat[flat < tail0] % 256) == set(range(256))
            continue
        assert 0 in flat
        first = flat[flat < 256]
        assert set(first) == set(range(256))
        far = 131072 if lay == "residues_long" else 32768 if lay == "residues" else 2048
        later = flat[(flat >= far) & (flat < tail0)]
        assert set(later % 256) == set(range(256)), name
        if lay == "shards":
            for c in L.shard_cuts(n):
                assert set(range(c - 24, c + 24)) <= set(flat)
        # condition 4's premise: no 8-row group, 64-row span or 256-row tile holds more than k of a query's rows
        for g in range(len(pos)):
            assert np.bincount(pos[g] // 8).max() <= k // 2


@pytest.mark.parametrize("name", [s for s in L.SPECS if L.SPECS[s][5] == "masked"])
@pytest.mark.parametrize("share", [0.5, 0.03])
def test_masks_leave_checked_rows_alone_in_their_unit(name, share):
    """the masks of the masked-scan tests: each `alone` row is the only allowed row of its 16-row unit (so of its 8-row
    unit), at every unit position 0..15, on both sides of mask-word edges and in the partly filled last word, whose other
    bits are clear but for the four; the units of `full` are all ones; every rung is allowed; dense / sparse as intended"""
    rows, qs, f = L.corpus(name)
    n = len(rows)
    allowed = L.ladder_mask(name, share)
    allow = np.zeros(n, bool)
    allow[allowed] = True
    alone, full = L.masked_sets(n)
    checked = set(f["checked"].ravel())
    assert set(alone) <= checked and set(full) <= checked and allow[f["rungs"].ravel()].all()
    seen = set()
    for r in alone:
        u = r // 16
        assert allow[u * 16:(u + 1) * 16].sum() == 1 and allow[r], r
        seen.add(r % 16)
    assert seen == set(range(16))
    last = allow[n - n % 64:]
    assert last.sum() == 4 and len(last) == 59
    edge_rows = [r for r in alone if r % 64 in (0, 63)]
    assert {r % 64 for r in edge_rows} == {0, 63} and len(edge_rows) >= 4     # the first and the last bit of a mask word
    assert allow[:256].all()
    assert (len(allowed) * 4 >= n) == (share >= 0.25)


@pytest.mark.parametrize("name", [s for s in L.SPECS if L.SPECS[s][3] == "scan"])
def test_f32_arithmetic_ladders(oracle, name):
    """f32 rows: every exchange of two units that differ is caught.  Binary16 rows: all but the pairs that differ only in
    the size of a remainder element under equal signs (the query's elements all have one size: such a pair scores the same)"""
    stats, share = analyse(oracle, name)
    assert stats["units"] == 1 and (share == 1.0 if L.SPECS[name][2] == "f32" else share >= 0.99)


@pytest.mark.parametrize("name", [s for s in L.SPECS if L.SPECS[s][3] == "binary16"])
def test_binary16_operand_ladders(oracle, name):
    stats, share = analyse(oracle, name)
    assert stats["units"] == 1 and share >= 0.9


@pytest.mark.parametrize("name", [s for s in L.SPECS if L.SPECS[s][3] == "q8"])
def test_8_bit_ladders(oracle, name):
    rows, qs, f = L.corpus(name)
    deq, delta, scale = L.q8_model(rows[np.sort(f["rungs"].ravel())])
    codes = np.rint(np.abs(deq) / scale[:, None].astype(np.float64))
    assert (codes.max(axis=1) == 127).all() and (codes < 127).mean() > 0.5       # two magnitudes below the largest code
    d, s = L.q8_stats(rows)
    assert f["eps"] == pytest.approx(L.q8_eps(f["dim"], d, s, float(np.linalg.norm(qs[0].astype(np.float64)))), rel=1e-6)
    stats, share = analyse(oracle, name)
    assert stats["units"] <= (3 if f["dim"] == 768 else 2)   # eps is 6 to 7e-3 here: a unit of 16 codes carries 0.75 * 16 / dim
    # Exchanging two units whose sign patterns differ in h of 16 places lowers the score by about 4 h * 0.75 / dim; a row is
    # lost from about 4 eps.  h is Binomial(16, 1/2) for random patterns: the share of differing pairs caught must reach
    # P(h >= h0 + 1), h0 = ceil(eps * dim / 0.75) (one place to spare for the unequal magnitudes).
    from math import ceil, comb
    h0 = ceil(f["eps"] * f["dim"] / 0.75) + 1
    floor = sum(comb(16, h) for h in range(h0, 17)) / 2.0 ** 16
    print(f"    exchange floor P(h >= {h0}) = {floor:.4f}")
    assert share >= floor, (name, share, floor)
