"""Corpora for the position tests (test_ladder_vectors_cpu.py proves what they catch, test_gpu_positions.py runs them
through every nominating kernel): rows that lose their place in the top-k as soon as their nomination is a few eps low,
placed on chosen rows -- where the corpora of band_vectors.py always put the winner on row 50 and query slot 0.

One query per class g: q_g = s_g / sqrt(dim), s_g a random +-1 pattern (no tiled blocks: two aligned 16-byte units of a
pattern repeat only by chance).  Class g owns a LADDER of W = 2k rows parallel to q_g whose true scores are spread
over [edge + 1.25 eps, edge + 2 eps], `edge` the floor of a quarter-binade bin of the select (0.75) and eps the eps of the
path under test.  The best k of them by the oracle's score are the CHECKED rows of q_g -- its top-k -- and go to the rows
the caller names; the other k (the lower rungs, scores up to edge + 1.6 eps) go anywhere.  Every other row scores below
0.6 for every query: far under (the floor of the bin below edge) - band.

A path is exact when a top-k row's nomination is at most eps under its true score; the select collects from
edge - 2 eps.  A checked row nominated 5 eps low falls from <= edge + 2 eps (+ eps of legitimate error) to
< edge - 2 eps: it is not collected, while the lower rungs keep the k-th nominated score -- and the floor -- in
edge's bin, and the result differs from the oracle's.

kind  "f32"  every element of a rung has one magnitude beta / sqrt(dim)
      "f16"  rows on the binary16 grid: one grid magnitude plus four elements of descending size that carry the
             remainder (one magnitude alone moves the score in steps of several eps)
      "q8"   three magnitudes (1 : 0.7 : 0.45), so that the 8-bit codes are not all +-127
|row| * |query| <= 1.0001: the unit-norm bands apply.  Upload the rows as built.
"""
import functools

import numpy as np

from band_vectors import bin_floor, q8_model, select, to_f16, true_dot  # noqa: F401  (re-exported for the tests)

F32 = np.float32
EDGE = 0.75
CHECKED_SPAN = (1.65, 2.0)     # true scores of the checked rungs, in eps above edge
LOWER_SPAN = (1.25, 1.6)       # ... of the lower rungs
OTHERS_BELOW = 0.6             # every row outside a query's ladder scores below this


# ---------------------------------------------------------------- the bands, as specified
def scan_eps(dim):
    """f32 scans (and the shared scans): (dim + 64) * 2^-24 * 1.0625 for unit-norm operands"""
    return (dim + 64) * 2.0 ** -24 * 1.0625


def binary16_eps(dim, f16_rows):
    """binary16 nomination (the matrix-core batch, the scan over the image): operand rounding 2^-10 (2^-11 over binary16
    rows) * 1.001, two accumulations of (dim + 64) * 2^-24, the subnormal term 2^-25 sqrt(dim) * 2, all * 1.0625"""
    op = 2.0 ** -11 if f16_rows else 2.0 ** -10
    return (op * 1.001 + 2.0 * (dim + 64) * 2.0 ** -24 + 2.0 ** -25 * np.sqrt(dim) * 2.0) * 1.0625


def q8_eps(dim, delta_max, scale_max, query_norm):
    """the 8-bit copy: delta_max * |q| + 32 roundings * 2^-24 * 256 sqrt(dim) |q| * the largest row scale * 1.0625 + the
    scan's eps"""
    qn = query_norm * 1.0001 + 1e-30
    return delta_max * 1.001 * qn + 32.0 * 2.0 ** -24 * 256.0 * np.sqrt(dim) * qn * scale_max * 1.0625 + scan_eps(dim)


# ---------------------------------------------------------------- pieces
def patterns(n_classes, dim, rng):
    """+-1 patterns whose pairwise correlation stays below 0.3 (another class' rungs score below 0.3 then)"""
    out = []
    while len(out) < n_classes:
        s = rng.choice(np.array([-1.0, 1.0]), size=dim)
        if all(abs(float(s @ t)) <= 0.3 * dim for t in out):
            out.append(s)
    return np.stack(out)


def f16_floor(x):
    """the largest binary16 value <= x (x >= 0)"""
    h = np.float16(x)
    if float(h) > x:
        h = np.nextafter(h, np.float16(0))
    return float(h)


def rung_magnitudes(total, dim, kind, rng):
    """dim magnitudes (f32) whose binary64 sum is `total` as nearly as the kind's grid allows"""
    if kind == "f32":
        return np.full(dim, F32(total / dim), np.float32)
    if kind == "f16":
        fine = rng.choice(dim, size=4, replace=False)
        m = np.full(dim, f16_floor(total / (dim - 2.5)), np.float64)
        m[fine] = 0.0
        rest = total - m.sum()                               # about 1.5 elements' worth
        for j, i in enumerate(fine):
            m[i] = f16_floor(rest * (0.5 if j == 0 else 1.0))
            rest -= m[i]
        assert 0.0 <= rest < 2.0 ** -23
        return m.astype(np.float32)
    if kind == "q8":
        w = rng.choice(np.array([1.0, 0.7, 0.45]), size=dim)
        w[rng.integers(dim)] = 1.0
        return (w * (total / w.sum())).astype(np.float32)
    raise ValueError(kind)


def ladder(O, dim, n, positions, eps, kind="f32", seed=0, lower_range=None, edge=EDGE, avoid=()):
    """-> (rows f32 [n, dim], queries f32 [G, dim], facts).  positions: int [G, k], the rows of each class' checked set
    (distinct).  lower_range: (lo, hi) the lower rungs are drawn from (default: every row), or one (lo, hi) per class;
    avoid: rows no lower rung may take.  facts: checked [G, k] (the rows of `positions`, as given), rungs [G, 2k] (checked
    first), k, W, edge, eps, kind, dim."""
    positions = np.asarray(positions, np.int64)
    G, k = positions.shape
    assert len(np.unique(positions)) == positions.size and positions.min() >= 0 and positions.max() < n
    rng = np.random.default_rng(9000 + seed)
    rows = rng.standard_normal((n, dim), dtype=np.float32) * F32(0.5 / np.sqrt(dim))     # filler: norm ~0.5, scores ~0.02
    if kind == "f16":
        rows = to_f16(rows)
    qe = float(F32(1.0 / np.sqrt(dim)))
    S = patterns(G, dim, rng)
    queries = (S * qe).astype(np.float32)
    ranges = lower_range if lower_range is not None else (0, n)
    ranges = [tuple(ranges)] * G if np.ndim(ranges) == 1 else [tuple(r) for r in ranges]
    taken = np.union1d(positions.ravel(), np.asarray(avoid, np.int64))
    lower = np.empty((G, k), np.int64)
    for g, (lo, hi) in enumerate(ranges):
        lower[g] = rng.choice(np.setdiff1d(np.arange(lo, hi), taken), size=k, replace=False)
        taken = np.union1d(taken, lower[g])
    betas = np.r_[edge + np.linspace(*CHECKED_SPAN, k)[::-1] * eps, edge + np.linspace(*LOWER_SPAN, k)[::-1] * eps]
    rungs = np.empty((G, 2 * k), np.int64)
    for g in range(G):
        vec = np.stack([S[g] * rung_magnitudes(b / qe, dim, kind, rng) for b in betas]).astype(np.float32)
        e = O.scan(vec, queries[g])
        # the oracle's own order decides which k are checked; built with a gap of 0.05 eps, so the split is strict
        order = np.lexsort((np.arange(2 * k), -e.astype(np.float64)))
        assert e[order[k - 1]] > e[order[k]], "the reference-order scores of the two halves touch: widen the gap"
        where = np.empty(2 * k, np.int64)
        where[order[:k]] = rng.permutation(positions[g])      # (score order and row order unrelated)
        where[order[k:]] = lower[g]
        rows[where] = vec
        rungs[g] = np.r_[positions[g], lower[g]]
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    return rows, queries, dict(checked=positions, rungs=rungs, k=k, W=2 * k, edge=float(edge), eps=float(eps), kind=kind,
                               dim=dim, G=G)


def q8_stats(rows, chunk=8192):
    """(largest |x - s k|, largest row scale) of the 8-bit copy of `rows`, a slice at a time"""
    d = s = 0.0
    for i in range(0, len(rows), chunk):
        _, delta, scale = q8_model(rows[i:i + chunk])
        d, s = max(d, float(delta.max())), max(s, float(scale.max()))
    return d, s


def q8_ladder(O, dim, n, positions, seed=0):
    """the ladder at the 8-bit copy's eps, which depends on the corpus (the largest |x - s k| and row scale): built at the
    filler's eps, then again at the eps of the result (the filler owns delta_max, so the second pass changes nothing)"""
    eps = None
    for _ in range(3):
        rows, queries, f = ladder(O, dim, n, positions, eps if eps else 4.0 * scan_eps(dim), "q8", seed)
        qn = float(np.linalg.norm(queries.astype(np.float64), axis=1).max())
        new = q8_eps(dim, *q8_stats(rows), qn)
        if eps is not None and abs(new - eps) <= 1e-6 * eps:
            break
        eps = new
    f["eps"] = float(new)
    return rows, queries, f


# ---------------------------------------------------------------- positions
def residue_slots(n, first=0, later=None, extra=()):
    """rows that cover every residue modulo 256 twice (from `first` and from `later`, by default the last whole tile),
    every row of the ragged last tile, row 0 and row n - 1, plus `extra`"""
    tail0 = n - n % 256
    later = tail0 - 256 if later is None else later
    assert first % 256 == 0 and later % 256 == 0 and first + 256 <= later and later + 256 <= tail0 < n
    return np.unique(np.r_[first:first + 256, later:later + 256, tail0:n, 0, n - 1, np.asarray(extra, np.int64)])


def deal(slots, k, n, seed=0, G=None, pad_range=None, avoid=()):
    """slots -> positions [G, k]: slot i goes to class i % G (neighbouring rows to different classes: no 8-row group holds
    two checked rows of one query while G >= 8); padded to G * k with random unused rows of pad_range"""
    slots = np.asarray(slots, np.int64)
    G = G if G is not None else -(-len(slots) // k)
    assert G * k >= len(slots)
    rng = np.random.default_rng(9500 + seed)
    lo, hi = pad_range if pad_range is not None else (0, n)
    pad = rng.choice(np.setdiff1d(np.arange(lo, hi), np.union1d(slots, np.asarray(avoid, np.int64))),
                     size=G * k - len(slots), replace=False)
    allp = np.r_[slots, pad]
    return np.stack([allp[g::G] for g in range(G)])


# ---------------------------------------------------------------- the corpora of test_gpu_positions.py
N_SCAN = 36923        # 144 whole tiles + 59 rows (n mod 8 = 3, mod 64 = 59, mod 256 = 59); rows >= 32768 lie in a later trip
N_LONG = 135037       # 527 tiles + 125 rows (mod 8 = 5, mod 64 = 61): a second sweep of the packed scans, a sampled batch
N_GEMM = 4411         # 17 tiles + 59 rows: the smallest corpus the batch takes, materialised
N_GEMM8 = 8507        # 33 tiles + 59 rows: room for 300 ladders of 16
SAMPLE = 65536

# name -> (dim, n, kind, eps family, k, layout)
SPECS = {
    "scan_f32_768": (768, N_SCAN, "f32", "scan", 32, "residues"),
    "scan_f32_256": (256, N_SCAN, "f32", "scan", 32, "residues"),
    "scan_f32_1024": (1024, N_SCAN, "f32", "scan", 32, "residues"),
    "scan_f32_1536": (1536, N_SCAN, "f32", "scan", 32, "residues"),
    "scan_f16_1024": (1024, N_SCAN, "f16", "scan", 32, "residues"),
    "scan_f16_1536": (1536, N_SCAN, "f16", "scan", 32, "residues"),
    "packed_f32_128": (128, N_LONG, "f32", "scan", 32, "residues_long"),
    "packed_f16_256": (256, N_LONG, "f16", "scan", 32, "residues_long"),
    "long_f32_256": (256, N_LONG, "f32", "scan", 32, "residues_long"),
    "generic_f32_200": (200, N_SCAN, "f32", "scan", 32, "residues"),
    "generic_f16_72": (72, N_SCAN, "f16", "scan", 32, "residues"),
    "image_768": (768, N_SCAN, "f32", "binary16", 32, "residues"),
    "q8_768": (768, N_SCAN, "q8", "q8", 32, "residues"),
    "q8_128": (128, N_LONG, "q8", "q8", 32, "residues_long"),
    "q8_400": (400, N_SCAN, "q8", "q8", 32, "residues"),
    "gemm_768_q17": (768, N_GEMM, "f32", "binary16", 36, ("batch", 17)),
    "gemm_768_q128": (768, N_GEMM, "f32", "binary16", 8, ("batch", 128)),
    "gemm_768_q300": (768, N_GEMM8, "f32", "binary16", 8, ("batch", 300)),
    "gemm_f16_1024_q17": (1024, N_GEMM, "f16", "binary16", 36, ("batch", 17)),
    "sampled_768": (768, N_LONG, "f32", "binary16", 32, "sampled"),
    "shards_768": (768, N_GEMM, "f32", "scan", 32, "shards"),
    "masked_f32_768": (768, N_SCAN, "f32", "scan", 32, "masked"),
    "masked_f32_1024": (1024, N_SCAN, "f32", "scan", 32, "masked"),
    "masked_f16_72": (72, N_SCAN, "f16", "scan", 32, "masked"),
}


def shard_cuts(n, parts=3):
    """first row of every shard but the first: contiguous shards of ceil(n / parts) rows (multi.cpp: set_bases)"""
    per = -(-n // parts)
    return [min(n, g * per) for g in range(1, parts)]


def masked_sets(n):
    """-> (alone, full): checked rows of the masked-scan corpora.  `alone`: one row per 16-row unit, the only allowed row
    of that unit -- every residue modulo 64 (both sides of every mask-word edge, every position of an 8-row and a 16-row
    unit) once from row 1024 on and once from row 20 480 on (a later trip of the dense shape), and four rows of the last,
    partly filled word, one per unit, row n - 1 among them.  `full`: rows 0..255, every row of their units allowed."""
    r = np.arange(64)
    tail0 = n - n % 64
    last = np.array([tail0 + 2, tail0 + 31, tail0 + 37, n - 1])
    assert n % 64 > 48 and len(np.unique(last // 16)) == 4
    return np.r_[1024 + 129 * r, 20480 + 129 * r, last], np.arange(256)


def ladder_mask(name, share, seed=11):
    """allowed rows of a masked-scan test: every rung; every row of the units of `full`; nothing else in the unit of an
    `alone` row; every other row with probability `share`"""
    dim, n, kind, fam, k, lay = SPECS[name]
    assert lay == "masked"
    positions, _ = layout(name)
    rows, qs, f = corpus(name)
    alone, full = masked_sets(n)
    allow = np.random.default_rng(seed).random(n) < share
    for u in np.unique(full // 16):
        allow[u * 16:(u + 1) * 16] = True
    for u in np.unique(alone // 16):
        allow[u * 16:(u + 1) * 16] = False
    allow[f["rungs"].ravel()] = True
    return np.flatnonzero(allow)


def layout(name):
    """-> (positions [G, k], lower_range or None) of a corpus"""
    dim, n, kind, fam, k, lay = SPECS[name]
    seed = sorted(SPECS).index(name)
    if lay == "residues":
        return deal(residue_slots(n), k, n, seed), None
    if lay == "residues_long":                               # the later tile lies in the second sweep of a 131 072-row grid
        return deal(residue_slots(n, later=131072 + 256), k, n, seed), None
    if lay == "sampled":                                     # checked rows behind the sample, lower rungs inside it
        tail0 = n - n % 256
        slots = np.unique(np.r_[SAMPLE:SAMPLE + 256, tail0 - 256:tail0, tail0:n])
        return deal(slots, k, n, seed, pad_range=(SAMPLE, n)), (0, SAMPLE)
    if lay == "shards":
        # Every shard runs its own top-k with the full k, so a ladder lives in ONE shard: its checked rows on the shard's
        # first 32 and last 192 rows (both sides of each cut, the whole ragged last tile of 1471 or 1469 rows), its lower
        # rungs anywhere in the same shard.  Seven classes per shard.
        bounds = [0] + shard_cuts(n) + [n]
        pos, ranges = [], []
        for lo, hi in zip(bounds[:-1], bounds[1:]):
            p = deal(np.r_[lo:lo + 32, hi - 192:hi], k, n, seed, pad_range=(lo, hi))
            pos.append(p)
            ranges += [(lo, hi)] * len(p)
        return np.concatenate(pos), ranges
    if lay == "masked":
        alone, full = masked_sets(n)
        units = np.unique(alone // 16)
        avoid = (units[:, None] * 16 + np.arange(16)).ravel()
        avoid = avoid[avoid < n]
        return deal(np.r_[full, alone], k, n, seed, avoid=avoid), None
    assert lay[0] == "batch"
    return deal(residue_slots(n, later=256 * 8), k, n, seed, G=lay[1]), None


@functools.lru_cache(maxsize=4)
def corpus(name):
    """-> (rows, queries, facts) of SPECS[name], read-only"""
    from oracle import oracle as O
    dim, n, kind, fam, k, lay = SPECS[name]
    positions, lower_range = layout(name)
    seed = sorted(SPECS).index(name)
    if fam == "q8":
        rows, qs, f = q8_ladder(O, dim, n, positions, seed)
    else:
        eps = scan_eps(dim) if fam == "scan" else binary16_eps(dim, kind == "f16")
        avoid = ()
        if lay == "masked":                                  # no lower rung inside the unit of a checked row that stands alone
            units = np.unique(masked_sets(n)[0] // 16)
            avoid = (units[:, None] * 16 + np.arange(16)).ravel()
        rows, qs, f = ladder(O, dim, n, positions, eps, kind, seed, lower_range, avoid=avoid)
    f["family"], f["name"], f["n"] = fam, name, n
    rows.setflags(write=False)
    qs.setflags(write=False)
    return rows, qs, f


# ---------------------------------------------------------------- the model of a path's nominations
def model_operands(rows, q, family, kind):
    """the operands whose binary64 dot product models a path's nominated score: the f32 scans and the shared scans use
    the operands themselves, binary16 nomination rounds both (binary16 rows are on the grid already), the 8-bit copy
    dequantises the rows"""
    if family == "scan":
        return np.asarray(rows, np.float64), np.asarray(q, np.float64)
    if family == "binary16":
        return to_f16(rows).astype(np.float64), to_f16(q).astype(np.float64)
    if family == "q8":
        return q8_model(rows)[0], np.asarray(q, np.float64)
    raise ValueError(family)
