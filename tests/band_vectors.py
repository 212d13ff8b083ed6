"""Corpora for the guard-band tests (test_band_vectors_cpu.py proves what they reach, test_gpu_guard_bands.py runs them
through every nomination path): rows whose nomination errors are coherent -- all in one direction and as large as the
arithmetic of the path allows -- where random rows leave them one to two orders of magnitude below the band.

Every builder returns (rows, queries, facts).  The corpus is ordinary filler (oracle.synth_rows) plus
  X   one winner row (facts["x"]): its reference-order score is the k-th best;
  C   k - 1 champion rows far above everything else, so that X sits exactly at rank k;
  D   150 decoy rows whose reference-order scores are all slightly BELOW X's and whose nominated scores are as far
      ABOVE X's as the path permits.
|row| * |query| stays below 1.0001 for every row, so the library applies its unit-norm band (scale 1, norm sum 2).
X, C and D lie in the first third of the rows: three shards leave them on one shard.

The select behind every nomination collects from (floor of the k-th nominated score's radix bin) - band, not from the
k-th nominated score itself (bins: a quarter of a binade, select_dev.h), so each corpus puts a bin floor `facts["edge"]`
just below its best decoy's nominated score and above X's: with X and the decoys inside one bin no band would be needed.

  (a) absorption        summation order of the f32 scans: X's terms round up in the left-to-right sum, D's are dropped
  (b) operand_rounding  binary16 rounding of both operands (f32 rows) or of the query alone (binary16 rows)
  (c) q8_rounding       8-bit rounding at 0.49 of a step on every element, parallel to the query
"""
import numpy as np

F32 = np.float32
ULP = 2.0 ** -24               # the f32 spacing in [0.5, 1)
U10 = 2.0 ** -10               # the binary16 spacing relative to the bottom of a binade
X_ROW, D_ROW, C_ROW, N_DECOYS = 50, 200, 400, 150


def to_f16(a):
    """round to nearest even onto the binary16 grid (the CPU test holds this to oracle.round_f16)"""
    return np.asarray(a, dtype=np.float32).astype(np.float16).astype(np.float32)


def true_dot(rows, q):
    """binary64 dot products of f32 operands: every product is exact, the sum good to ~1e-13"""
    return np.asarray(rows, np.float64) @ np.asarray(q, np.float64)


def bin_floor(v):
    """lower edge of the quarter-binade bin of a positive score (the first radix digit of the select)"""
    e = np.floor(np.log2(v))
    return np.floor(v / 2.0 ** e * 4.0) / 4.0 * 2.0 ** e


def f32_with_product(other, target):
    """the f32 r next to target / other whose rounded f32 product with `other` is exactly `target`"""
    other, target = F32(other), F32(target)
    r = F32(float(target) / float(other))
    cands = [r]
    lo = hi = r
    for _ in range(4):
        lo, hi = np.nextafter(lo, F32(0)), np.nextafter(hi, F32(2))
        cands += [lo, hi]
    for c in cands:
        if F32(c * other) == target:
            return F32(c)
    raise AssertionError("no f32 factor reaches the target product")


def _assemble(O, n, dim, seed, q, x, decoys, k, f16):
    """filler + X + decoys + (k - 1) champions (the query's direction plus a little noise, unit norm)"""
    rows = O.synth_rows(n, dim, seed=seed, n_clusters=5)
    rng = np.random.default_rng(seed + 1)
    rows[X_ROW] = x
    rows[D_ROW:D_ROW + len(decoys)] = decoys
    unit = np.asarray(q, np.float64) / np.linalg.norm(np.asarray(q, np.float64))
    for i in range(k - 1):
        c = unit + rng.standard_normal(dim) * (0.05 / np.sqrt(dim))
        rows[C_ROW + i] = O.normalize(c.astype(np.float32))
    if f16:
        built = np.r_[X_ROW, D_ROW:D_ROW + len(decoys)]       # on the grid by construction
        keep = rows[built].copy()
        rows = to_f16(rows)
        assert np.array_equal(rows[built].view(np.uint32), keep.view(np.uint32))
    return np.ascontiguousarray(rows, dtype=np.float32)


def _facts(rows, q, k, edge, **more):
    rn = float(np.sqrt((np.asarray(rows, np.float64) ** 2).sum(axis=1).max()))
    qn = float(np.linalg.norm(np.asarray(q, np.float64)))
    f = dict(x=X_ROW, decoys=np.arange(D_ROW, D_ROW + N_DECOYS), champions=np.arange(C_ROW, C_ROW + k - 1), k=k,
             edge=float(edge), row_norm_max=rn, query_norm=qn, norm_product=rn * qn, norm_sum=rn + qn)
    f.update(more)
    return f


# ---------------------------------------------------------------- (a) summation order
T_HI, T_LO = 0.502, 0.498      # a term of (b + T) ulps: the left-to-right sum adds b + 1 for T_HI, b for T_LO


def absorption(O, k=1, dim=768, n=4096, f16=False, span=N_DECOYS):
    """One leading product S in [0.5, 1) and dim - 1 terms next to half an ulp of it.  X: every term T_HI ulps -- the
    reference's running sum rounds each one up to a whole ulp (S + m), a sum in parallel partials keeps S + 0.502 m.
    D_j: every term 1 + T_LO ulps (the reference adds 1, the truth 1.498) except drop_j = 1 + j % span terms of T_LO
    (dropped by the reference): reference S + m - drop_j < X's, truth S + 1.498 m - drop_j, about m - drop_j ulps ABOVE X.
    S is aimed so that the best decoy's true score lies `margin` ulps above the bin floor 0.75.
    f16: the rows lie on the binary16 grid (tiny elements 2^-14 (1 + j / 1024)), the query carries the precision; f32:
    the query is oracle.normalize(facts["raw_query"]), so the engine's entry points can be fed the raw one."""
    m = dim - 1
    edge = 0.75
    margin = 16 + dim // 48                                  # above the few ulps a lane's chain loses on the device
    s_ulps = int(round(edge / ULP)) - int(round(m * (1.0 + T_LO) - 1)) + margin
    S = F32(s_ulps * ULP)
    assert float(S) == s_ulps * ULP
    if f16:
        raw = None
        r0 = F32(0.875)
        x_t = F32(2.0 ** -14 * 1275 / 1024)
        qi = F32(T_HI * ULP / float(x_t))
        d_lo, d_hi = to_f16(float(x_t) * T_LO / T_HI), to_f16(float(x_t) * (1.0 + T_LO) / T_HI)
        q = np.full(dim, qi, np.float32)
        q[0] = f32_with_product(r0, S)
    else:
        raw = np.full(dim, np.sqrt(0.25 / m), np.float32)
        raw[0] = np.sqrt(0.75)
        q = O.normalize(raw)
        qi = q[1]
        assert (q[1:] == qi).all()
        r0 = f32_with_product(q[0], S)
        x_t, d_lo, d_hi = (F32(t * ULP / float(qi)) for t in (T_HI, T_LO, 1.0 + T_LO))
    rng = np.random.default_rng(4100 + dim)
    x = np.full(dim, x_t, np.float32)
    x[0] = r0
    decoys = np.full((N_DECOYS, dim), d_hi, np.float32)
    decoys[:, 0] = r0
    drops = 1 + np.arange(N_DECOYS) % span
    for j in range(N_DECOYS):
        decoys[j, 1 + rng.choice(m, size=drops[j], replace=False)] = d_lo
    rows = _assemble(O, n, dim, 4200 + dim + (1 if f16 else 0), q, x, decoys, k, f16)
    return rows, q[None].copy(), _facts(rows, q, k, edge, raw_query=raw, lead=float(S), drops=drops, dim=dim)


# ---------------------------------------------------------------- (b) binary16 operand rounding
def operand_rounding(O, k=1, f16=False):
    """768-d.  The dimensions split at random into halves M and P.  The query is 2^e (1 + 0.49 * 2^-10) on M (binary16
    rounds it DOWN by almost half a step at the bottom of its binade, where that is 2^-11 relative) and
    2^e (1 + 0.51 * 2^-10) on P (rounded UP).  X lives on M, the decoys on P; f32 rows carry the same two mantissas, so
    both roundings push X's nominated score down and D's up; binary16 rows are powers of two and only the query
    rounds.  Exponents: 42 query elements of a half at 2^-4 and 342 at 2^-5 (norm^2 0.997); the rows' are chosen so that
    X's nominated score is 639/1024 (f16: 639.5/1024) and the decoys' just above the bin floor 640/1024.  One element of
    D_j is lowered until its exact score is a little below X's (more with j)."""
    dim, half = 768, 384
    rng = np.random.default_rng(5100)
    perm = rng.permutation(dim)
    M, P = perm[:half], perm[half:]
    qexp = np.array([-4] * 42 + [-5] * 342)
    if f16:
        xexp = np.array([-4] * 172 + [-5] * 211 + [-6])
    else:
        xexp = np.array([-4] * 171 + [-5] * 213)
    assert len(xexp) == half and (2.0 ** (qexp + xexp)).sum() * 1024 == (639.5 if f16 else 639.0)
    down, up = 1.0 + 0.49 * U10, 1.0 + 0.51 * U10
    q = np.zeros(dim, np.float32)
    q[M] = 2.0 ** qexp * down
    q[P] = 2.0 ** qexp * up
    x = np.zeros(dim, np.float32)
    x[M] = 2.0 ** xexp * (1.0 if f16 else down)
    d = np.zeros(dim, np.float32)
    d[P] = 2.0 ** xexp * (1.0 if f16 else up)
    tw = P[300]                                              # an element of 2^-5 against a query element of 2^-5
    excess = float(true_dot(d, q) - true_dot(x, q))          # the untouched decoy's exact score lies above X's
    decoys = np.tile(d, (N_DECOYS, 1))
    if f16:
        step = 2.0 ** -16                                    # the binary16 spacing below 2^-5
        n0 = int(np.ceil(excess / (float(q[tw]) * step))) + 3
        decoys[:, tw] = d[tw] - (n0 + np.arange(N_DECOYS)) * step
    else:
        cut = excess + 1.5e-6 + 2.0e-7 * np.arange(N_DECOYS)
        decoys[:, tw] = (float(d[tw]) - cut / float(q[tw])).astype(np.float32)
    rows = _assemble(O, 4096, dim, 5200 + (1 if f16 else 0), q, x, decoys, k, f16)
    return rows, q[None].copy(), _facts(rows, q, k, 640.0 / 1024.0, dim=dim, M=M, P=P)


# ---------------------------------------------------------------- (c) the 8-bit copy
Q8_STEP = 2.0 ** -8            # the row scale of X and of every decoy: their largest element is 127 steps


def q8_model(rows):
    """the 8-bit copy as q8.hip's header states it: per row s = max|x| / 127 (1 for a zero row), k = round-to-even(x / s)
    clamped to +-127, in f32 -> (dequantised rows s * k in binary64, error norms |x - s k|, scales)"""
    rows = np.asarray(rows, np.float32)
    m = np.abs(rows).max(axis=1)
    s = np.where(m == 0, F32(1.0), m / F32(127.0)).astype(np.float32)
    kq = np.clip(np.rint(rows / s[:, None]), -127.0, 127.0)
    deq = s[:, None].astype(np.float64) * kq.astype(np.float64)
    delta = np.sqrt(((rows.astype(np.float64) - deq) ** 2).sum(axis=1))
    return deq, delta, s


def q8_rounding(O, k=1):
    """768-d.  The query is c * g with signs g.  X = g * step * (k_i + 0.49): every element rounds DOWN in magnitude by
    0.49 of a step, the error vector is parallel to the query and Cauchy-Schwarz holds with equality.  D = g * step *
    (k_i + 0.51): rounds UP by 0.49.  Element 0 of both is exactly 127 steps and pins the scale.  One element of D_j is
    lowered by (15.44 + 0.02 j) steps, which puts its exact score a little below X's.  k_i in 2..4 keeps the rows short
    (norm 0.62) and their error norm (0.053) far above the filler's (0.008): X and D own the index's delta_max.  c is
    chosen so that the best decoy's nominated score is three steps' worth above the bin floor 0.4375."""
    dim = 768
    rng = np.random.default_rng(6100)
    g = rng.choice(np.array([-1.0, 1.0]), size=dim)
    ki = rng.integers(2, 5, size=dim).astype(np.float64)
    tw = 5
    xs = ki + 0.49
    ds = ki + 0.51
    xs[0] = ds[0] = 127.0
    cuts = 0.02 * (dim - 1) + 0.1 + 0.02 * np.arange(N_DECOYS)
    edge = 0.4375
    k_top = 127.0 + (ki[1:] + 1.0).sum() - (ki[tw] + 1.0) + np.rint(ds[tw] - cuts[0])   # the best decoy, in steps
    c = F32(edge / (Q8_STEP * (k_top - 3.0)))
    assert float(c) * np.sqrt(dim) < 1.0, "the query would be longer than 1: raise the k_i"
    q = (g * float(c)).astype(np.float32)
    x = (g * Q8_STEP * xs).astype(np.float32)
    decoys = np.tile((g * Q8_STEP * ds).astype(np.float32), (N_DECOYS, 1))
    decoys[:, tw] = (g[tw] * Q8_STEP * (ds[tw] - cuts)).astype(np.float32)
    rows = _assemble(O, 4096, dim, 6200, q, x, decoys, k, False)
    return rows, q[None].copy(), _facts(rows, q, k, edge, dim=dim)


# ---------------------------------------------------------------- the select, as a model
def select(nominated, exact, k, band, bins=True):
    """rows the pipeline returns when `nominated` are its nomination scores: everything at or above (the bin floor of)
    the k-th nominated score minus `band` is re-scored (`exact`), the best k by (exact desc, row asc) are returned"""
    kth = np.sort(nominated)[::-1][k - 1]
    lo = (bin_floor(kth) if bins else kth) - band
    cand = np.flatnonzero(nominated >= lo)
    order = np.lexsort((cand, -exact[cand].astype(np.float64)))[:k]
    return cand[order]
