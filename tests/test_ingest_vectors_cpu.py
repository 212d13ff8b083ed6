"""The ingestion test vectors (ingest_vectors.py) checked without a GPU: they hit the rounding edges they claim to hit, a
subtly wrong kernel (a root one ulp off, a divide that rounds toward or away from zero, a binary16 store that truncates or
rounds ties upward) would change them, and the vectorised reference the GPU tests use for large inputs is the oracle's
`normalize` bit for bit.  Each test prints the coverage it observed (pytest -s shows it)."""
from fractions import Fraction

import numpy as np

import ingest_vectors as V
from ingest_vectors import F32, bits, canon


def mantissa(x):
    """positive float -> (m, e) with x == m * 2^e and 2^23 <= m < 2^24"""
    fr = Fraction(float(x))
    e = 0
    while fr >= 1 << 24:
        fr, e = fr / 2, e + 1
    while fr < 1 << 23:
        fr, e = fr * 2, e - 1
    assert fr.denominator == 1
    return fr.numerator, e


def root_boundary_distance(x):
    """distance of sqrt(x) from the nearest rounding boundary of a 24-bit root, in ulp of the root (exact up to the
    second order of that distance: |x - b^2| / (2 b ulp) for the boundary b)"""
    m, e = mantissa(np.sqrt(F32(x)))
    best = None
    for b in (2 * m - 1, 2 * m + 1):                      # the boundaries around the root, in units of 2^(e - 1)
        d = abs(Fraction(float(x)) / Fraction(2) ** (2 * (e - 1)) - b * b) / (2 * b * 2)
        best = d if best is None or d < best else best
    return best


# ---------------------------------------------------------------- (a)
def test_hard_root_rows_are_exact_hard_and_tell_a_wrong_root(oracle):
    targets = V.hard_root_targets()
    assert len({t[0] for t in targets}) == 600
    rows8, x = V.hard_root_rows(8)
    assert len(rows8) == len(targets)
    parity = (bits(x) >> 23) & 1
    n_even, n_odd = int((parity == 0).sum()), int((parity == 1).sum())
    near = np.array([root_boundary_distance(v) < Fraction(1, 1024) for v in x])
    near_even, near_odd = int((near & (parity == 0)).sum()), int((near & (parity == 1)).sum())
    worst_near = max(float(root_boundary_distance(v)) for v in x[near])
    print(f"hard roots: {len(x)} rows from 600 M; biased exponent even {n_even}, odd {n_odd}; within 2^-10 ulp of a "
          f"boundary: even {near_even}, odd {near_odd} (the farthest of those {worst_near:.3g} ulp)")
    assert n_even >= 200 and n_odd >= 200
    # both 24-bit neighbours of a hard M^2 are rows; only the nearer one is next to the boundary (the other lies about a
    # third of an ulp off), and where the exponent is odd only one of the two is a sum of exact squares: about half
    assert near_even >= 100 and near_odd >= 100
    for dim in (8, 768, 3, 101):
        for scale in (0, -20, 20):
            rows, xs = V.hard_root_rows(dim, scale)
            assert rows.shape[1] == dim and (dim == 3 or len(rows) == len(targets))
            assert len(rows) >= 400
            assert (np.count_nonzero(rows, axis=1) <= 4).all()
            got = np.array([oracle.dot(r, r) for r in rows], dtype=np.float32)
            assert np.array_equal(bits(got), bits(xs)), (dim, scale)
            assert np.array_equal(bits(V.seq_sumsq(rows)), bits(xs)), (dim, scale)
            if dim != 3:
                assert np.array_equal(bits(xs), bits(x * F32(4.0) ** scale))
            y, lo, hi = V.root_neighbours(xs)
            want = V.oracle_rows(oracle, rows)
            assert np.array_equal(bits(want), bits(rows / y[:, None])), (dim, scale)
            told_lo = (bits(rows / lo[:, None]) != bits(want)).any(axis=1)
            told_hi = (bits(rows / hi[:, None]) != bits(want)).any(axis=1)
            print(f"hard roots dim {dim} scale 2^{scale}: {len(rows)} rows; a root one ulp low changes "
                  f"{int(told_lo.sum())}, one ulp high {int(told_hi.sum())}")
            assert told_lo.all() and told_hi.all(), (dim, scale)


# ---------------------------------------------------------------- (b)
def directed_quotients(v, y):
    """|v| / y rounded toward zero and away from zero, as f32 (exact arithmetic; normal quotients only)"""
    q = Fraction(abs(float(v))) / Fraction(float(y))
    e = 0
    while q >= 1 << 24:
        q, e = q / 2, e + 1
    while q < 1 << 23:
        q, e = q * 2, e - 1
    down = q.numerator // q.denominator
    up = down + (0 if q.denominator == 1 else 1)
    s = -1.0 if v < 0 else 1.0
    return F32(s * float(Fraction(down) * Fraction(2) ** e)), F32(s * float(Fraction(up) * Fraction(2) ** e))


def test_hard_quotient_rows_are_absorbed_hard_and_tell_a_directed_divide(oracle):
    rows = V.hard_quotient_rows(768)
    assert rows.shape == (4, 768)
    heads = {r[:V.HEAD].tobytes() for r in rows}
    assert len(heads) == 4
    want = V.oracle_rows(oracle, rows)
    for i, row in enumerate(rows):
        head_sum = oracle.dot(row[:V.HEAD], row[:V.HEAD])
        assert F32(oracle.dot(row, row)) == F32(head_sum)        # every tail square is absorbed
        y = np.sqrt(F32(head_sum))
        tail = row[V.HEAD:]
        assert (tail > 0).sum() >= 100 and (tail < 0).sum() >= 100
        n_hard, worst, n_rz, n_ra = 0, Fraction(0), 0, 0
        for c, v in enumerate(tail):
            q = Fraction(abs(float(v))) / Fraction(float(y)) * (1 << 38)      # in units of the boundaries' last bit
            assert (1 << 24) <= q < (1 << 25)
            m_odd = 2 * (q.numerator // (2 * q.denominator)) + 1              # the odd integer of q's unit interval pair
            d = abs(q - m_odd) / 2                                             # in ulp of the 24-bit quotient
            if d < Fraction(1, 1024):
                n_hard += 1
                worst = max(worst, d)
                rz, ra = directed_quotients(v, y)
                n_rz += int(bits(rz)[0] != bits(want[i, V.HEAD + c])[0])
                n_ra += int(bits(ra)[0] != bits(want[i, V.HEAD + c])[0])
        print(f"hard quotients row {i}: {n_hard} of {len(tail)} tail entries within 2^-10 ulp of a boundary (the farthest "
              f"{float(worst):.3g} ulp); a divide rounding toward zero changes {n_rz}, away from zero {n_ra}")
        assert n_hard >= 500
        assert n_rz >= n_hard / 4 and n_ra >= n_hard / 4
        assert n_rz + n_ra == n_hard                       # (no quotient is exact: one of the two directions is wrong)
    for dim in (72, 100, 101, 1024):
        r = V.hard_quotient_rows(dim)
        s = V.seq_sumsq(r)
        assert np.array_equal(bits(s), bits(V.seq_sumsq(r[:, :V.HEAD]))), dim


# ---------------------------------------------------------------- (c)
def test_class_edge_rows_hit_every_class(oracle):
    for dim in (3, 7, 8, 72, 100, 101, 768, 1024):
        rows, names = V.class_edge_rows(dim)
        want = V.oracle_rows(oracle, rows)
        by = {n: (rows[i], want[i]) for i, n in enumerate(names)}
        s = V.seq_sumsq(rows)
        sb = {n: int(bits(s[i:i + 1])[0]) for i, n in enumerate(names)}
        if dim != 3:                                       # (three squares do not reach every one of the three values)
            assert {"below_threshold", "at_threshold", "above_threshold"} <= set(names)
        assert sum(n.endswith("threshold") for n in names) >= 2
        for n, off in (("below_threshold", -1), ("at_threshold", 0), ("above_threshold", 1)):
            if n in by:
                assert sb[n] == V.THRESHOLD_BITS + off
                raw, out = by[n]
                assert np.array_equal(bits(raw), bits(out)) == (off <= 0), (dim, n)
        for n in ("zero", "negative_zero", "nan_stays_as_given"):
            raw, out = by[n]
            assert np.array_equal(bits(raw), bits(out)), (dim, n)
        raw, out = by["nan_stays_as_given"]
        assert np.isnan(raw).sum() == 1 and (np.abs(raw[1:]) > 65504).any()
        raw, out = by["unit"]
        assert np.array_equal(bits(raw), bits(out)) and np.count_nonzero(raw) == 1
        tiny = F32(2.0 ** -126)
        for n, first in (("subnormal_dividends_norm_3", 1), ("subnormal_dividends_norm_3_of_three", 3)):
            raw, out = by[n]
            assert sb[n] == int(bits(F32(9.0))[0]) and (np.abs(raw[first:]) < tiny).all()
            assert (np.abs(out)[np.abs(raw) < tiny] < tiny).all() and not np.array_equal(bits(raw), bits(out))
        raw, out = by["subnormal_and_underflowing_quotients"]
        a = np.abs(out[1:])
        assert np.isfinite(s[names.index("subnormal_and_underflowing_quotients")])
        assert ((a > 0) & (a < F32(2.0 ** -126))).any() and (a == 0).any()
        assert np.array_equal(np.signbit(out), np.signbit(raw))             # the sign of a zero quotient is the dividend's
        raw, out = by["sum_of_squares_overflows"]
        assert np.isfinite(raw).all() and np.isinf(s[names.index("sum_of_squares_overflows")])
        assert (out == 0).all() and np.array_equal(np.signbit(out), np.signbit(raw))
        for n in ("one_inf", "negative_inf"):
            raw, out = by[n]
            assert np.isnan(out[0]) and (out[1:] == 0).all()
            assert np.array_equal(np.signbit(out[1:]), np.signbit(raw[1:]))
        if dim >= 7:
            z = by["subnormal_and_underflowing_quotients"][1]
            assert (np.signbit(z) & (z == 0)).any() and (~np.signbit(z) & (z == 0)).any()


# ---------------------------------------------------------------- (d)
def test_f16_table_holds_every_pattern_and_every_tie(oracle):
    rows, kind, lower = V.f16_table()
    assert rows.shape[1] == 768 and 253_952 < rows.size < 253_952 + 2 * 768
    want = oracle.round_f16(rows)
    # an independent statement of round-to-nearest-even: numpy's binary16 cast
    with np.errstate(over="ignore"):
        assert np.array_equal(canon(want), canon(rows.astype(np.float16).astype(np.float32)))
    for sign in (False, True):
        side = np.signbit(rows) == sign
        for k in range(4):
            assert np.array_equal(np.sort(lower[(kind == k) & side]), np.arange(0x7C00)), (sign, k)
    widened = V.f16_widen(lower)
    widened_next = V.f16_widen(lower + 1)
    wmag = np.abs(want)
    exact, tie, below, above = (kind == 0), (kind == 1), (kind == 2), (kind == 3)
    assert np.array_equal(bits(want[exact]), bits(rows[exact]))
    even, odd = tie & (lower % 2 == 0), tie & (lower % 2 == 1)
    print(f"binary16 table: {rows.size} values in {rows.shape[0]} rows; ties with an even lower neighbour "
          f"{int(even.sum())}, with an odd one {int(odd.sum())}")
    assert even.sum() == 2 * 15872 and odd.sum() == 2 * 15872
    assert np.array_equal(wmag[even], widened[even]) and np.array_equal(wmag[below], widened[below])
    up = np.where(lower + 1 == 0x7C00, np.inf, widened_next).astype(np.float32)
    assert np.array_equal(wmag[odd], up[odd]) and np.array_equal(wmag[above], up[above])
    # what a wrong conversion would change: truncation every `above` and every odd tie, ties-upward every even tie
    assert (wmag[above] != widened[above]).all() and (wmag[odd] != widened[odd]).all()
    assert (wmag[even] != up[even]).all()
    extras = rows[kind == 4]
    for v in (2.0 ** -25, 2.0 ** -26, 65504.0, 65519.996, 65520.0, 3.4028234663852886e38):
        assert (extras == F32(v)).any() and (extras == -F32(v)).any()
    assert (bits(extras) == 0x33000001).any() and np.isinf(extras).any() and np.isnan(extras).any()
    assert ((np.abs(extras) > 0) & (np.abs(extras) < F32(2.0 ** -126))).any()
    e = {float(v): float(w) for v, w in zip(extras, want[kind == 4]) if not np.isnan(v)}
    assert e[2.0 ** -25] == 0.0 and e[float(V.from_bits([0x33000001])[0])] == 2.0 ** -24 and e[2.0 ** -26] == 0.0
    assert e[65504.0] == 65504.0 and e[float(F32(65519.996))] == 65504.0 and e[65520.0] == np.inf
    assert e[float(F32(3.4028234663852886e38))] == np.inf


# ---------------------------------------------------------------- the vectorised reference
def test_vectorised_reference_is_the_oracle(oracle):
    for dim in (3, 7, 8, 72, 100, 101, 768, 1024):
        rows = V.corpus(dim)
        assert np.array_equal(canon(V.normalize_rows(rows)), canon(V.oracle_rows(oracle, rows))), dim
    rng = np.random.default_rng(4)
    for n, dim in ((22145, 768), (3000, 100)):
        rows = (rng.standard_normal((n, dim)) * 3).astype(np.float32)
        assert np.array_equal(bits(V.normalize_rows(rows)), bits(V.oracle_rows(oracle, rows))), (n, dim)
