"""Input rows for the ingestion tests (test_ingest_vectors_cpu.py proves what they hit, test_gpu_ingest.py feeds them to
`upload / append(normalize=True)`): rows whose norm, whose element / norm quotients and whose binary16 conversion sit at
the rounding edges that random rows practically never reach.  Everything here is deterministic and exact by
construction; the only floating-point reference is the oracle (and `normalize_rows`, its vectorised twin for inputs too
large for a per-row call, which the CPU test holds to the oracle bit for bit).

  (a) hard_root_rows      norm^2 = the f32 next to M^2 for an odd 25-bit M: sqrt lies next to a rounding boundary
  (b) hard_quotient_rows  elements v with v / norm next to an odd 25-bit m: the divide lies next to a rounding boundary
  (c) class_edge_rows     the 1e-20 threshold and its neighbours, zeros, subnormals, overflow, Inf, NaN
  (d) f16_table           every binary16 pattern, every tie between two patterns and the f32 values on either side
"""
import functools
import math

import numpy as np

F32 = np.float32
HEAD = 16                      # (b): the leading entries that fix a row's norm
MIN_QUOTIENT_DIM = 2 * HEAD    # (b) needs room for a tail behind the head


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def canon(a):
    """f32 bit patterns with every NaN as one pattern (a NaN's payload is not part of the contract)"""
    a = np.ascontiguousarray(a, dtype=np.float32)
    b = a.view(np.uint32).copy()
    b[np.isnan(a)] = 0x7FC00000
    return b


def from_bits(u):
    return np.asarray(u, dtype=np.uint32).view(np.float32)


# ---------------------------------------------------------------- the references
def seq_sumsq(rows):
    """per row: the f32 sum of squares in column order, one rounded multiply and one rounded add per element"""
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    cols = np.ascontiguousarray(rows.T)
    s = np.zeros(rows.shape[0], dtype=np.float32)
    with np.errstate(all="ignore"):
        for c in range(cols.shape[0]):
            p = cols[c] * cols[c]
            s = s + p
    return s


def normalize_rows(rows):
    """`normalize` of every row, vectorised over rows: a column loop of f32 multiply and add, np.sqrt, a divide"""
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    s = seq_sumsq(rows)
    with np.errstate(all="ignore"):
        scaled = rows / np.sqrt(s)[:, None]
    return np.where((s > F32(1e-20))[:, None], scaled, rows)


def oracle_rows(O, rows, f16=False):
    """the oracle's normalize, row by row, then its binary16 rounding for binary16 storage"""
    want = np.stack([O.normalize(r) for r in np.ascontiguousarray(rows, dtype=np.float32)])
    return O.round_f16(want) if f16 else want


def ranking(e, k):
    """the reference's order of the scores e: descending, NaN last, equal scores by ascending row"""
    nan = np.isnan(e)
    order = np.lexsort((np.arange(len(e)), np.where(nan, 0.0, -e.astype(np.float64)), nan))[:k]
    return order.astype(np.uint64), e[order]


# ---------------------------------------------------------------- sums of squares
_TWO_LIMIT = 1 << 16


@functools.lru_cache(maxsize=None)
def _two_squares():
    tab = {}
    top = math.isqrt(_TWO_LIMIT) + 1
    for c in range(top):
        for d in range(c + 1):
            tab.setdefault(c * c + d * d, (c, d))
    return tab


def square_decompositions(X, terms=4):
    """yields (a, b, c, d) with a^2 + b^2 + c^2 + d^2 == X, largest a first; terms == 3: d == 0 only"""
    tab = _two_squares()
    if terms < 4:
        t = X
        while t and t % 4 == 0:
            t //= 4
        if t % 8 == 7:
            return                        # (Legendre: 4^a (8 b + 7) is no sum of three squares)
    for a in range(math.isqrt(X), -1, -1):
        r = X - a * a
        b0 = math.isqrt(r)
        for b in range(b0, max(b0 - 64, -1), -1):
            r2 = r - b * b
            if r2 >= _TWO_LIMIT:
                break
            if terms < 4:
                c = math.isqrt(r2)
                if c * c == r2:
                    yield (a, b, c, 0)
                continue
            cd = tab.get(r2)
            if cd is not None:
                yield (a, b, cd[0], cd[1])


def _place(dim, parts, unit_exp, rng):
    """a zero row with the integers `parts` * 2^unit_exp at scattered columns"""
    row = np.zeros(dim, dtype=np.float32)
    cols = np.sort(rng.choice(dim, size=len(parts), replace=False))
    for c, a in zip(cols, rng.permutation(len(parts))):
        row[c] = math.ldexp(parts[a], unit_exp)
    return row


# ---------------------------------------------------------------- (a) hard square roots
@functools.lru_cache(maxsize=None)
def hard_root_targets(n_m=600):
    """[(M, X, e, dist)]: x = X * 2^e (X < 2^24, e even) is a 24-bit neighbour of M^2 for one of the n_m odd 25-bit M
    whose square lies closest to such an x; dist = |x - M^2|.  sqrt(x) then lies |dist| / (4 M) ulp from the rounding
    boundary M.  An x with an odd exponent and an odd mantissa is no sum of exact f32 squares and is left out."""
    M = np.arange((1 << 24) + 1, 1 << 25, 2, dtype=np.uint64)
    sq = M * M
    sh = np.where(sq >= np.uint64(1 << 49), 26, 25).astype(np.uint64)
    ulp = np.uint64(1) << sh
    rem = sq & (ulp - np.uint64(1))
    dist = np.minimum(rem, ulp - rem)
    out = []
    for i in np.argsort(dist, kind="stable")[:n_m]:
        m = int(M[i])
        s = m * m
        e0 = 26 if s >= (1 << 49) else 25
        for X in ((s >> e0), (s >> e0) + 1):
            e, x = e0, X << e0
            if X == 1 << 24:
                X, e = X >> 1, e + 1
            if e % 2:
                if X % 2:
                    continue
                X, e = X // 2, e + 1
            out.append((m, X, e, abs(x - s)))
    return tuple(out)


def root_neighbours(x):
    """the correctly rounded f32 root of the f32 array x, and its lower and upper f32 neighbours"""
    y = np.sqrt(np.asarray(x, dtype=np.float32))
    return y, np.nextafter(y, F32(0)), np.nextafter(y, F32(np.inf))


def _sensitive(row, x):
    """does a root one ulp off, on either side, change a stored element of the normalised row?"""
    y, lo, hi = root_neighbours(F32(x))
    good = bits(row / y)
    return bool((bits(row / lo) != good).any() and (bits(row / hi) != good).any())


@functools.lru_cache(maxsize=None)
def _hard_root_base(dim, seed=11):
    rng = np.random.default_rng(seed)
    rows, xs = [], []
    for (_m, X, e, _d) in hard_root_targets():
        unit = (e - 50) // 2
        best = None
        for n_try, parts in enumerate(square_decompositions(X, terms=min(dim, 4))):
            row = _place(dim, parts[:min(dim, 4)], unit, rng)
            if best is None:
                best = row
            if _sensitive(row, math.ldexp(X, 2 * unit)):
                best = row
                break
            if n_try >= 8:
                break
        if best is None:
            continue                      # (dim 3: X is no sum of three squares)
        rows.append(best)
        xs.append(math.ldexp(X, 2 * unit))
    return np.stack(rows).astype(np.float32), np.array(xs, dtype=np.float32)


def hard_root_rows(dim, scale_exp=0):
    """-> (rows [n, dim], x [n]): row i holds three (dim 3) or four integers * 2^k at scattered columns of a zero row, so
    that its sequential f32 sum of squares is exactly x[i], a hard_root_targets value brought to [1/4, 1) * 4^scale_exp.
    Of the decompositions of a target, the first whose stored elements tell a root one ulp off is taken."""
    assert dim >= 3
    rows, xs = _hard_root_base(dim)
    return rows * F32(2.0 ** scale_exp), xs * F32(4.0 ** scale_exp)


# ---------------------------------------------------------------- (b) hard quotients
def _head(seed):
    rng = np.random.default_rng(seed)
    scale = (1.0, 3.0, 1.0e-3, 50.0, 0.25, 7.0e2)[seed % 6]
    return (rng.standard_normal(HEAD) * scale).astype(np.float32)


_MAX_TAIL = 1024


@functools.lru_cache(maxsize=None)
def _quotient_candidates(seed):
    """-> (head, [v]): the head of that seed and the _MAX_TAIL hardest dividends under its norm, hardest first"""
    head = _head(seed)
    y = float(np.sqrt(seq_sumsq(head[None, :])[0]))
    fr, ex = math.frexp(y)
    Y, ey = int(fr * (1 << 24)), ex - 24
    assert math.ldexp(Y, ey) == y
    ms = np.arange((1 << 24) + 1, 1 << 25, 2, dtype=np.uint64)
    P = ms * np.uint64(Y)
    sh = np.where(P >= np.uint64(1 << 48), 25, 24).astype(np.uint64)
    ulp = np.uint64(1) << sh
    rem = P & (ulp - np.uint64(1))
    dist = np.minimum(rem, ulp - rem)
    dist[rem == 0] = np.iinfo(np.uint64).max              # (an exact quotient is no hard one)
    pick = np.argpartition(dist, _MAX_TAIL)[:_MAX_TAIL]
    pick = pick[np.lexsort((pick, dist[pick]))]
    out = []
    for i in pick:
        p, s = int(P[i]), int(sh[i])
        V = ((p + (1 << (s - 1))) >> s) << s
        out.append(math.ldexp(V, ey - 38))
    return head, tuple(out)


@functools.lru_cache(maxsize=None)
def hard_quotient_rows(dim, n_rows=4, seed=23):
    """-> rows [n_rows, dim]: columns 0..15 are generic and fix the norm y = Y * 2^ey; behind them, in mixed order and with
    mixed signs, sit the dim - 16 values v = V * 2^(ey - 38) with V the 24-bit value next to m * Y for the odd 25-bit m
    whose product with Y lies closest to one.  v / y = (V / Y) * 2^-38 then lies next to the rounding boundary m * 2^-38,
    and v^2 < y^2 * 2^-26 is absorbed by the running sum of squares, which ends on the head's."""
    assert MIN_QUOTIENT_DIM <= dim <= HEAD + _MAX_TAIL
    n_tail = dim - HEAD
    rows = []
    for r in range(n_rows):
        rng = np.random.default_rng(seed * 1000 + r)
        head, cand = _quotient_candidates(seed + r)
        tail = np.array(cand[:n_tail], dtype=np.float64)[rng.permutation(n_tail)]
        tail *= np.where(rng.integers(0, 2, n_tail) == 1, -1.0, 1.0)
        row = np.concatenate([head.astype(np.float64), tail])
        assert np.array_equal(row.astype(np.float32).astype(np.float64), row)
        rows.append(row.astype(np.float32))
    return np.stack(rows)


# ---------------------------------------------------------------- (c) class edges of normalize
THRESHOLD_BITS = int(np.array([1e-20], dtype=np.float32).view(np.uint32)[0])

_SUBNORMAL_BITS = (0x00000001, 0x00000002, 0x00000003, 0x00000005, 0x007FFFFF, 0x00400000, 0x002AAAAB, 0x00555555,
                   0x00000FFF, 0x00700001, 0x00123457, 0x0000FFFF)
# dividends under a norm of 2^60: quotients in the f32 subnormal range (exact, inexact, ties) and below it
_TINY = (2.0 ** -90, 1.5 * 2.0 ** -90, 2.0 ** -80, 2.0 ** -100, 3 * 2.0 ** -88, 2.0 ** -89, 3 * 2.0 ** -90, 5 * 2.0 ** -91,
         2.0 ** -126, float(np.float32(1.2345678e-26)), float(np.float32(6.54321e-27)), 2.0 ** -91,
         float(np.float32(2.0 ** -66) - np.float32(2.0 ** -89)))


def _cycle(dim, first, values, neg_every=2):
    row = np.zeros(dim, dtype=np.float32)
    row[0] = first
    for c in range(1, dim):
        v = values[(c - 1) % len(values)]
        row[c] = -v if ((c - 1) // len(values) + c) % neg_every else v
    return row


def _threshold_row(dim, xbits, rng):
    """a row whose sequential sum of squares is the f32 with the bit pattern xbits (next to 1e-20f), or None"""
    x = float(from_bits([xbits])[0])
    fr, ex = math.frexp(x)
    X, e = int(fr * (1 << 24)), ex - 24
    while X % 2 == 0 and e % 2:
        X, e = X // 2, e + 1
    if e % 2:
        return None
    for parts in square_decompositions(X, terms=min(dim, 4)):
        return _place(dim, parts[:min(dim, 4)], e // 2, rng)
    return None


@functools.lru_cache(maxsize=None)
def class_edge_rows(dim):
    """-> (rows [n, dim], names): one row per class of `normalize`'s behaviour (see the names)"""
    assert dim >= 3
    rng = np.random.default_rng(dim)
    rows, names = [], []

    def add(name, row):
        if row is not None:
            rows.append(np.asarray(row, dtype=np.float32))
            names.append(name)

    for name, xb in (("below_threshold", THRESHOLD_BITS - 1), ("at_threshold", THRESHOLD_BITS),
                     ("above_threshold", THRESHOLD_BITS + 1)):
        add(name, _threshold_row(dim, xb, rng))
    add("zero", np.zeros(dim, dtype=np.float32))
    add("negative_zero", np.full(dim, -0.0, dtype=np.float32))
    unit = np.zeros(dim, dtype=np.float32)
    unit[dim // 2] = 1.0
    add("unit", unit)
    add("negative_unit_with_negative_zeros", np.where(np.arange(dim) == 0, F32(-1.0), F32(-0.0)))
    sub = [float(v) for v in from_bits(list(_SUBNORMAL_BITS))]
    add("subnormal_dividends_norm_3", _cycle(dim, 3.0, sub))
    r = _cycle(dim, 1.0, sub)
    r[1], r[2] = 2.0, -2.0
    add("subnormal_dividends_norm_3_of_three", r)
    add("subnormal_and_underflowing_quotients", _cycle(dim, 2.0 ** 60, _TINY))
    add("sum_of_squares_overflows", _cycle(dim, 1.0e20, (1.5e20, 0.75e20, 3.0e19, 0.0, 1.0, 2.0 ** -149)))
    add("one_inf", _cycle(dim, np.inf, (1.0, 0.0, 1.0e30, 3.4e38, 2.0 ** -149)))
    add("negative_inf", _cycle(dim, -np.inf, (2.0, 0.0)))
    add("nan_stays_as_given", _cycle(dim, np.nan, (1.0e5, 7.0e4, 65520.0, 65504.0, 0.5, 2.0 ** -25, 0.0, 65519.996)))
    return np.stack(rows), tuple(names)


# ---------------------------------------------------------------- a corpus of (a) + (b) + (c)
@functools.lru_cache(maxsize=None)
def corpus(dim, edges=True):
    """(a) at three scales, (b) where the row has room for it, (c) on request; the rows are not to be written to"""
    parts = [hard_root_rows(dim, s)[0] for s in (0, -20, 20)]
    if dim >= MIN_QUOTIENT_DIM:
        parts.append(hard_quotient_rows(dim))
    if edges:
        parts.append(class_edge_rows(dim)[0])
    out = np.concatenate(parts)
    out.setflags(write=False)
    return out


# ---------------------------------------------------------------- (d) the binary16 conversion table
def f16_widen(h):
    """exact f32 value of the binary16 patterns h (0x7C00 stands for 65536 here: the end of the last rounding interval)"""
    h = np.asarray(h, dtype=np.uint32)
    e, m = (h >> 10) & 0x1F, h & 0x3FF
    mag = np.where(e == 0, m * 2.0 ** -24, (1024 + m) * 2.0 ** (e.astype(np.float64) - 25))
    return np.where(h & 0x8000, -mag, mag).astype(np.float32)


F16_EXTRAS = np.concatenate([
    np.array([2.0 ** -25, 2.0 ** -26, 65504.0, 65519.996, 65520.0, np.inf, np.nan], dtype=np.float32),
    from_bits([0x33000001, 0x7F7FFFFF, 0x00000001, 0x007FFFFF, 0x00400000, 0x7FA00001]),
])


@functools.lru_cache(maxsize=None)
def f16_table(width=768):
    """-> (rows [n, width], kind, lower): for every finite binary16 magnitude h and both signs the widened value (kind 0),
    the midpoint to the next pattern (1) and that midpoint's lower (2) and upper (3) f32 neighbour; then F16_EXTRAS with
    both signs (kind 4) and zero padding (kind 5).  kind and lower (the pattern h of an entry) have the rows' shape."""
    h = np.arange(0x7C00, dtype=np.uint32)
    lo, hi = f16_widen(h).astype(np.float64), f16_widen(h + 1).astype(np.float64)
    mid64 = 0.5 * (lo + hi)
    mid = mid64.astype(np.float32)
    assert np.array_equal(mid.astype(np.float64), mid64)
    pos = np.stack([lo.astype(np.float32), mid, np.nextafter(mid, F32(0)), np.nextafter(mid, F32(np.inf))], axis=1)
    kinds = np.broadcast_to(np.arange(4, dtype=np.uint8), pos.shape)
    lows = np.broadcast_to(h[:, None], pos.shape)
    vals = np.concatenate([pos.ravel(), -pos.ravel(), F16_EXTRAS, -F16_EXTRAS])
    kind = np.concatenate([kinds.ravel(), kinds.ravel(), np.full(2 * len(F16_EXTRAS), 4, np.uint8)])
    lower = np.concatenate([lows.ravel(), lows.ravel(), np.zeros(2 * len(F16_EXTRAS), np.uint32)])
    pad = -len(vals) % width
    vals = np.concatenate([vals, np.zeros(pad, np.float32)]).astype(np.float32)
    kind = np.concatenate([kind, np.full(pad, 5, np.uint8)])
    lower = np.concatenate([lower, np.zeros(pad, np.uint32)])
    return vals.reshape(-1, width), kind.reshape(-1, width), lower.reshape(-1, width)
