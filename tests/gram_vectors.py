"""Pools that read single entries of the MMR Gram matrix back through the greedy loop (test_gram_vectors_cpu.py proves what
they read, test_gpu_gram_positions.py runs them through every Gram kernel of csrc/exact.hip).

The P x P matrix of pairwise dot products never leaves the device; the suite saw it only as the running maximum of a winner's
similarities.  The reference's loop (rag_engine.rs:767-839) takes pool slot 0 first whatever its score, never picks a candidate
whose relevance is not finite and logs (1 - lambda) * rel - lambda * max_sim.  So, with lambda = 0.5:

  three picks   slot 0 holds an all-zero row, rel[a] = 4, rel[b] = 0, every other relevance NaN, k = 3.  The picks are
                [0, a, b] and the third logged value is 0 - 0.5 * max(0, G[a][b]) = -G[a][b] / 2, exact (a power-of-two scaling of
                a value of at least 2^-100) whenever G[a][b] > 0;
  two picks     any row in slot 0, rel[b] = 0, the rest NaN, k = 2: the picks are [0, b], the second logged value -G[0][b] / 2.

One pool reads one entry, exactly as the greedy kernel reads it: G[last pick][candidate], row a, column b.  NEVER observable,
by any greedy run: column 0 (slot 0 is never a candidate), the diagonal (a pick is no longer a candidate) and the magnitude
of an entry that is not positive (max(0, .) hides it; it reads +0.0, like a non-finite one, which gram_entry stores as -inf).
No plan claims those.  None of them can change a result either: the loop does not read them.

Rows: normalize(u + g / sqrt(dim)), u a random +-1/sqrt(dim) pattern common to all rows, g standard normal: every dot
product is positive (0.2 .. 0.75) and every one is a sum of terms of both signs, so that the order of the additions and
the rounding of each product show in the last bits.  In the last eight columns u g is kept at or above -0.5 (the element keeps u's sign): the products
of the last element and of the last aligned 16-byte unit are then positive and at least 0.1 / dim each, so a sum that
omits them differs on EVERY pair (fault model iii), not on most.  Corpus row 0 is the all-zero row.

numpy only; the oracle is passed in, as in mmr_restatement.py."""
import functools

import numpy as np

import mmr_restatement as R

F32 = np.float32
LAM = 0.5
REL_A, REL_B = F32(4.0), F32(0.0)


# ---------------------------------------------------------------- rows
def corpus(O, n_real, dim, f16, seed=0):
    """-> rows f32 [1 + n_real, dim]: row 0 all zero, then n_real rows as the module docstring says (on the binary16 grid if f16)"""
    rng = np.random.default_rng([7300 + seed, n_real, dim, int(f16)])
    u = rng.choice(np.array([-1.0, 1.0]), size=dim)
    g = rng.standard_normal((n_real, dim))
    g[:, -8:] = u[-8:] * np.maximum(u[-8:] * g[:, -8:], -0.5)   # u (u + g) = 1 + u g >= 0.5
    raw = ((u + g) / np.sqrt(dim)).astype(np.float32)
    rows = np.zeros((1 + n_real, dim), np.float32)
    for i in range(n_real):
        rows[1 + i] = O.normalize(raw[i])
    if f16:
        rows = O.round_f16(rows)
    return rows


@functools.lru_cache(maxsize=None)
def _corpus_cached(n_real, dim, f16):
    from oracle import oracle as O
    rows = corpus(O, n_real, dim, f16)
    g = R.gram(O, rows)
    rows.setflags(write=False)
    g.setflags(write=False)
    return rows, g


def corpus_and_gram(n_real, dim, f16):
    """(rows, G) with G = mmr_restatement.gram(oracle, rows): computed once per process, shared and read-only"""
    return _corpus_cached(int(n_real), int(dim), bool(f16))


# ---------------------------------------------------------------- which kernel a pass runs
# launch_gram_rows / launch_gram_src (csrc/exact.hip), restated: the first row that matches names the instance.  `blocks16` is
# ceil(P / 16) * (ceil(P / 16) + 1) / 2 * pools, the 16 x 16 blocks of a pass.  launch_gram (dense f32 values) is
# launch_gram_src without the first row.
#   (rows dtype, pools per pass at least, blocks16 at most) -> (instance, block side T)
GRAM_RULES = (
    ("f16", 16, None, "gram_mfma_f32_kernel", 32),
    (None, 8, None, "gram_tiled<4,64>", 64),
    (None, 1, 512, "gram_tiled<1,384>", 16),
    (None, 1, 1536, "gram_tiled<1,128>", 16),
    (None, 1, None, "gram_tiled<2,64>", 32),
)
# launch_mmr_greedy: the register-resident greedy kernel's J by the pool stride (above 1024: one pool, mmr_greedy_kernel)
GREEDY_J = ((64, 1), (128, 2), (320, 5), (512, 8), (1024, 16))


def gram_instance(dtype, pools, P):
    nb1 = (P + 15) // 16
    blocks16 = nb1 * (nb1 + 1) // 2 * pools
    for dt, min_pools, max_blocks, name, T in GRAM_RULES:
        if (dt is None or dt == dtype) and pools >= min_pools and (max_blocks is None or blocks16 <= max_blocks):
            return name, T
    raise AssertionError("no rule")


def pools_per_pass(P):
    """mmr_batch_impl (csrc/index_fused.hip): a call is cut into passes of this many pools; the Gram instance is chosen per pass"""
    per_query = P * P + 3 * P + 2
    return max(64, min(4096, (3 << 30) // 4 // per_query))


# ---------------------------------------------------------------- the shapes (the table of DESIGN.md)
# name, instance, P, dims, dtypes, pools per call (1: rlr_mmr_select, one pool)
SHAPES = (
    dict(name="r1_384_single", instance="gram_tiled<1,384>", P=37, dims=(388, 772, 390), dtypes=("f32", "f16"), pools=1),
    dict(name="r1_384", instance="gram_tiled<1,384>", P=37, dims=(388, 772, 390), dtypes=("f32", "f16"), pools=7),
    dict(name="r1_128", instance="gram_tiled<1,128>", P=180, dims=(132, 260), dtypes=("f32", "f16"), pools=7),
    dict(name="r2_64", instance="gram_tiled<2,64>", P=325, dims=(132,), dtypes=("f32", "f16"), pools=7),
    dict(name="r4_64", instance="gram_tiled<4,64>", P=130, dims=(132, 134), dtypes=("f32",), pools=256),
    dict(name="r4_64_f16", instance="gram_tiled<4,64>", P=130, dims=(132, 134), dtypes=("f16",), pools=12),
    dict(name="mfma_33", instance="gram_mfma_f32_kernel", P=33, dims=(136, 140, 1024), dtypes=("f16",), pools=256),
    dict(name="mfma_70", instance="gram_mfma_f32_kernel", P=70, dims=(136, 140, 1024), dtypes=("f16",), pools=256),
    dict(name="mfma_100", instance="gram_mfma_f32_kernel", P=100, dims=(136, 140, 1024), dtypes=("f16",), pools=256),
    dict(name="single_1030", instance="gram_tiled<2,64>", P=1030, dims=(132,), dtypes=("f32", "f16"), pools=1),
)
EVERY_PAIR_MAX = 130


def shape(name):
    return next(s for s in SHAPES if s["name"] == name)


def cases(names=None):
    """(shape name, dim, dtype) of every corpus the shapes use"""
    return [(s["name"], d, t) for s in SHAPES if names is None or s["name"] in names for d in s["dims"] for t in s["dtypes"]]


# ---------------------------------------------------------------- tile classes
def tile_classes(P, T, mfma=False):
    """name -> predicate over slot arrays (a, b): the classes of T x T blocks a Gram kernel treats differently.  The tiled
    kernels compute the blocks on and below the diagonal and store every entry twice (`lower`: read where it was computed;
    `upper`: the mirror store); the matrix-core kernel computes the blocks on and above it in pairs of tile rows (2p, 2p + 1),
    one wave per pair and column block: an entry belongs to the tile row min(block of a, block of b).  (The pair's block
    below the diagonal, (2p + 1, 2p), is computed a second time by the wave's other half and stored over the same words.)"""
    nb = (P + T - 1) // T
    last = nb - 1 if P % T else nb                        # the ragged block (none when T divides P)
    cls = {
        "diagonal": lambda a, b: (a // T == b // T) & (a // T != last),
        "lower": lambda a, b: (a // T > b // T) & (a // T != last),
        "upper": lambda a, b: (a // T < b // T) & (b // T != last),
        "ragged_row": lambda a, b: (a // T == last) & (b // T != last),
        "ragged_col": lambda a, b: (b // T == last) & (a // T != last),
        "ragged_diagonal": lambda a, b: (a // T == last) & (b // T == last),
    }
    if mfma:
        tr = lambda a, b: np.minimum(a // T, b // T)       # the tile row that computes the entry (its mirror included)
        paired = lambda a, b: tr(a, b) // 2 * 2 + 1 < nb
        cls["pair_first"] = lambda a, b: (tr(a, b) % 2 == 0) & paired(a, b)
        cls["pair_second"] = lambda a, b: tr(a, b) % 2 == 1
        cls["unpaired_row"] = lambda a, b: (tr(a, b) % 2 == 0) & ~paired(a, b)
    return cls


def observable_pairs(P):
    """every (a, b) a greedy run can read: a != b, b != 0"""
    a, b = np.divmod(np.arange(P * P), P)
    keep = (a != b) & (b != 0)
    return a[keep], b[keep]


def residues(a, b, T):
    return set(zip((a % T).tolist(), (b % T).tolist()))


# ---------------------------------------------------------------- which pairs a shape reads
def _block_pairs(P, T, ba, bb):
    a = np.arange(ba * T, min(P, (ba + 1) * T))
    b = np.arange(bb * T, min(P, (bb + 1) * T))
    a, b = np.repeat(a, b.size), np.tile(b, a.size)
    keep = (a != b) & (b != 0)
    return a[keep], b[keep]


def read_pairs(P, T, rng):
    """the ordered slot pairs (a, b) a shape reads, row 0 included (those go through the two-pick form).
    P <= 130: every observable pair.  Above: whole blocks of every tile class -- with the first, the second and the last
    full block among them -- plus four pairs of every block; P > 1024 (one pool, a call per entry): the rows of the
    ragged last block against one column of every residue modulo T, both orders."""
    if P <= EVERY_PAIR_MAX:
        return observable_pairs(P)
    nb = (P + T - 1) // T
    lo = (nb - 1) * T
    if P > 1024:
        rag = np.arange(lo, P)
        cols = rng.integers(0, nb - 1, T) * T + np.arange(T)
        cols[cols == 0] = T                                  # residue 0, but not slot 0
        a, b = np.repeat(rag, T), np.tile(cols, rag.size)
        return np.r_[a, b], np.r_[b, a]
    f = nb - 2                                               # the last full block
    blocks = [(0, 0), (1, 1), (f, f), (1, 0), (2, 1), (f, 1), (0, 1), (1, 2), (1, f),
              (nb - 1, 1), (nb - 1, f), (1, nb - 1), (f, nb - 1), (nb - 1, nb - 1)]
    parts = [_block_pairs(P, T, ba, bb) for ba, bb in dict.fromkeys(blocks)]
    for ba in range(nb):
        for bb in range(nb):
            a, b = _block_pairs(P, T, ba, bb)
            pick = rng.choice(a.size, size=min(4, a.size), replace=False)
            parts.append((a[pick], b[pick]))
    ab = np.unique(np.stack([np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])], axis=1), axis=0)
    return ab[:, 0], ab[:, 1]


# ---------------------------------------------------------------- readout plans
class Plan:
    """Q pools of stride P for calls of `pools` pools each (Q is a multiple of it) with one k.
    pool_rows [Q, P] corpus rows by slot, rel [Q, P], sizes [Q], a / b [Q]: the entry pool q reads (slots)."""

    def __init__(self, P, k, pools, pool_rows, rel, sizes, a, b):
        self.P, self.k, self.pools, self.lam = P, k, pools, LAM
        self.pool_rows, self.rel, self.sizes, self.a, self.b = pool_rows, rel, sizes, a, b
        self.Q = pool_rows.shape[0]

    def calls(self):
        return [slice(s, s + self.pools) for s in range(0, self.Q, self.pools)]


def build_plan(P, a, b, k, pools, n_real, rng, sizes=None):
    """One pool per pair.  Every pool lays the corpus out by a permutation of its own (three picks: the zero row stays in
    slot 0): a pass reuses the workspace of the pass before, and with one layout an entry that is never stored would
    still hold that pass's correct value.  The pairs are padded (re-reading pairs at random under new layouts) to a
    multiple of `pools`, so that every call, and every pass of it, has exactly the pool count its Gram instance is chosen by."""
    assert pools <= pools_per_pass(P) and n_real >= P
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    sizes = np.full(a.size, P, np.uint32) if sizes is None else np.asarray(sizes, np.uint32)
    pad = -a.size % pools
    if pad:
        again = rng.integers(0, a.size, pad)
        a, b, sizes = np.r_[a, a[again]], np.r_[b, b[again]], np.r_[sizes, sizes[again]]
    Q = a.size
    assert (a < sizes).all() and (b < sizes).all() and (b != 0).all() and (a != b).all()
    perm = rng.permuted(np.tile(np.arange(1, n_real + 1), (Q, 1)), axis=1)[:, :P]
    if k == 3:
        assert (a != 0).all()
        perm[:, 0] = 0
    else:
        assert k == 2 and (a == 0).all()
    rel = np.full((Q, P), np.nan, np.float32)
    q = np.arange(Q)
    if k == 3:
        rel[q, a] = REL_A
    rel[q, b] = REL_B
    return Plan(P, k, pools, np.ascontiguousarray(perm, dtype=np.uint64), rel, sizes, a, b)


def plans_for(P, T, pools, seed=0):
    """[three-pick plan, two-pick plan] that together read read_pairs(P, T); the corpus needs P real rows"""
    rng = np.random.default_rng([7400 + seed, P, T, pools])
    a, b = read_pairs(P, T, rng)
    three = a != 0
    out = [build_plan(P, a[three], b[three], 3, pools, P, rng)]
    if (~three).any():
        out.append(build_plan(P, a[~three], b[~three], 2, pools, P, rng))
    return out


def ragged_plan(P, pool_sizes, pools, n_random=600):
    """a three-pick plan over pools of stride P and sizes `pool_sizes`, mixed within every call: per size s the pairs that
    touch its last slot s - 1 and n_random others inside it"""
    rng = np.random.default_rng([7450, P, pools])
    aa, bb, ss = [], [], []
    for s in pool_sizes:
        a, b = observable_pairs(s)
        a, b = a[a != 0], b[a != 0]
        edge = (a == s - 1) | (b == s - 1)
        keep = np.r_[np.flatnonzero(edge), rng.choice(np.flatnonzero(~edge), n_random, replace=False)]
        aa.append(a[keep]); bb.append(b[keep]); ss.append(np.full(keep.size, s))
    a, b, s = np.concatenate(aa), np.concatenate(bb), np.concatenate(ss)
    mix = rng.permutation(a.size)
    return build_plan(P, a[mix], b[mix], 3, pools, P, rng, s[mix])


def shape_plans(name):
    s = shape(name)
    return plans_for(s["P"], dict((r[3], r[4]) for r in GRAM_RULES)[s["instance"]], s["pools"])


# ---------------------------------------------------------------- the reference's loop over many pools at once
def mmr_batch(gc, pool_rows, rel, k, lam, override=None):
    """mmr_restatement.mmr_from_gram for Q pools of one size at once (test_gram_vectors_cpu.py pins it to that function pool
    by pool): gc is the corpus' Gram matrix, pool q's is gc[pool_rows[q]][:, pool_rows[q]].
    override = (a [Q], b [Q], value [Q]): pool q's own entry [a][b] replaced (the entry fault models).
    -> (order u32 [Q, k], logged f32 [Q, k], n [Q]); order / logged are valid up to n."""
    pr = np.ascontiguousarray(pool_rows, dtype=np.int64)
    rel = np.ascontiguousarray(rel, dtype=np.float32)
    Q, P = rel.shape
    ar = np.arange(Q)
    base = (ar * P)[:, None]
    lam = F32(lam)
    one_minus = F32(1.0) - lam
    order = np.zeros((Q, k), np.uint32)
    logged = np.full((Q, k), np.nan, np.float32)
    n = np.ones(Q, np.uint32)
    rem = np.tile(np.arange(P), (Q, 1))
    n_rem = P - 1
    rem[:, 0] = rem[:, n_rem]
    max_sim = np.zeros((Q, P), np.float32)
    fin = np.isfinite(rel)
    alive = np.ones(Q, bool)
    last = np.zeros(Q, np.int64)
    step = 1
    with np.errstate(all="ignore"):
        while step < k and n_rem > 0:
            c = rem[:, :n_rem].copy()
            at_c = base + c                                    # flat positions of the candidates' slots
            sim = gc[pr[ar, last][:, None], pr.reshape(-1)[at_c]]
            if override is not None:
                oa, ob, ov = override
                sim = np.where((last == oa)[:, None] & (c == ob[:, None]), np.asarray(ov, np.float32)[:, None], sim)
            ms = max_sim.reshape(-1)[at_c]
            ms = np.where(np.isfinite(sim), np.maximum(ms, sim), ms)
            max_sim.reshape(-1)[at_c] = ms
            m = one_minus * rel.reshape(-1)[at_c] - lam * ms
            ok = fin.reshape(-1)[at_c] & np.isfinite(m)
            alive &= ok.any(axis=1)
            at = np.argmax(np.where(ok, m, -np.inf), axis=1)
            pick = c[ar, at]
            order[alive, step] = pick[alive]
            logged[alive, step] = m[ar, at][alive]
            n[alive] += 1
            last = pick
            n_rem -= 1
            rem[ar, at] = rem[ar, n_rem]
            step += 1
    return order, logged, n


def expected(plan, gc, override=None):
    """(order [Q, k], logged [Q, k], n [Q]) of every pool of the plan, pools of one size together"""
    order = np.zeros((plan.Q, plan.k), np.uint32)
    logged = np.full((plan.Q, plan.k), np.nan, np.float32)
    n = np.zeros(plan.Q, np.uint32)
    for s in np.unique(plan.sizes):
        at = np.flatnonzero(plan.sizes == s)
        ov = None if override is None else tuple(np.asarray(x)[at] for x in override)
        order[at], logged[at], n[at] = mmr_batch(gc, plan.pool_rows[at, :s], plan.rel[at, :s], plan.k, plan.lam, ov)
    return order, logged, n


def read_entries(plan, gc):
    """the entries the plan's pools read: gc at (row in slot a, row in slot b)"""
    q = np.arange(plan.Q)
    pr = plan.pool_rows.astype(np.int64)
    return gc[pr[q, plan.a], pr[q, plan.b]]


# ---------------------------------------------------------------- fault models
# (ii): the entry of another slot, as an index that is off by one, by a tile's thread row or by an accumulator register
SHIFTS = ((1, 0), (-1, 0), (0, 1), (0, -1), (16, 0), (-16, 0), (0, 32), (0, -32), (0, 64), (0, -64))
CHAIN_MODELS = ("drop_last", "drop_unit", "four_chains", "chunk64", "reversed", "fused")


def _chain(xt, yt, cols, fused=False):
    """s = s + fl(x * y) over `cols` in that order, in f32 (fused: fl(s + x * y), the product exact in binary64)"""
    s = np.zeros(xt.shape[1], np.float32)
    for k in cols:
        if fused:
            s = (s.astype(np.float64) + xt[k].astype(np.float64) * yt[k].astype(np.float64)).astype(np.float32)
        else:
            s = s + xt[k] * yt[k]
    return s


def variant_dots(rows, ia, ib, model, unit):
    """the dot products of corpus rows ia[i] . ib[i] as a kernel with fault `model` would sum them; "reference" is the
    strict left-to-right chain of rounded products, which the CPU test holds to the oracle bit for bit.
    unit = elements per aligned 16-byte unit of the stored rows (4: f32, 8: binary16)."""
    xt = np.ascontiguousarray(rows[ia].T)
    yt = np.ascontiguousarray(rows[ib].T)
    dim = xt.shape[0]
    if model == "reference":
        return _chain(xt, yt, range(dim))
    if model == "drop_last":                                 # (iii) the last element omitted
        return _chain(xt, yt, range(dim - 1))
    if model == "drop_unit":                                 # (iii) the last aligned 16-byte unit omitted
        return _chain(xt, yt, range((dim - 1) // unit * unit))
    if model == "four_chains":                               # (iv) four interleaved partial chains, combined at the end
        p = [_chain(xt, yt, range(j, dim, 4)) for j in range(4)]
        return (p[0] + p[1]) + (p[2] + p[3])
    if model == "chunk64":                                   # (v) one partial sum per 64-column chunk, added at the end
        s = np.zeros(xt.shape[1], np.float32)
        for k0 in range(0, dim, 64):
            s = s + _chain(xt, yt, range(k0, min(dim, k0 + 64)))
        return s
    if model == "reversed":                                  # (vi)
        return _chain(xt, yt, range(dim - 1, -1, -1))
    if model == "fused":                                     # (vii) f32 rows only: binary16 products are exact
        return _chain(xt, yt, range(dim), fused=True)
    raise ValueError(model)


def shifted_entries(plan, gc, da, db):
    """(ii) per pool: the entry of slot (a + da, b + db) of its own matrix, and whether that slot exists"""
    a2, b2 = plan.a + da, plan.b + db
    ok = (a2 >= 0) & (b2 >= 0) & (a2 < plan.sizes) & (b2 < plan.sizes)
    q = np.arange(plan.Q)
    pr = plan.pool_rows.astype(np.int64)
    val = gc[pr[q, np.where(ok, a2, 0)], pr[q, np.where(ok, b2, 0)]]
    return val, ok


# ---------------------------------------------------------------- entries that must read +0.0
def class_corpus(O, n_real, dim, f16):
    """the corpus of (n_real, dim) plus rows whose similarities are not positive -> (rows, special)
    special["neg"]: the negative of real row 1 (every dot with a real row is negative); ["nan"] / ["inf"]: a real row with
    one element NaN / +Inf; ["zero"]: the all-zero row (row 0; every dot exactly +0.0); ["e0"], ["e1"]: two unit vectors
    with disjoint support (the dot is a sum of exact zeros)."""
    base, _ = corpus_and_gram(n_real, dim, f16)
    extra = np.zeros((5, dim), np.float32)
    extra[0] = -base[1]
    extra[1] = base[2]
    extra[1, dim // 3] = np.nan
    extra[2] = base[3]
    extra[2, dim - 1] = np.inf
    extra[3, 5] = 1.0
    extra[4, dim - 2] = 1.0
    n = base.shape[0]
    return np.vstack([base, extra]), dict(neg=n, nan=n + 1, inf=n + 2, zero=0, e0=n + 3, e1=n + 4)


def class_plan(P, T, pools, n_real, special):
    """three-pick pools over class_corpus whose read entry is non-positive or non-finite: at four positions of every tile
    class (first, last and two random pairs of it) x {negative, NaN row, Inf row, zero row, disjoint supports}, the
    special row in slot a and again in slot b."""
    rng = np.random.default_rng([7500, P, T])
    oa, ob = observable_pairs(P)
    keep = oa != 0
    oa, ob = oa[keep], ob[keep]
    pos = []
    for name, pred in tile_classes(P, T).items():
        at = np.flatnonzero(pred(oa, ob))
        if at.size:
            pos += [at[0], at[-1], *rng.choice(at, 2)]
    kinds = ("neg", "nan", "inf", "zero", "e0")
    a = np.repeat(oa[pos], 2 * len(kinds))
    b = np.repeat(ob[pos], 2 * len(kinds))
    plan = build_plan(P, a, b, 3, pools, n_real, rng)
    for q in range(a.size):                                  # (the padding pools stay ordinary reads)
        kind = kinds[q % len(kinds)]
        at_a = (q // len(kinds)) % 2 == 0
        plan.pool_rows[q, plan.a[q] if at_a else plan.b[q]] = special[kind]
        if kind == "e0":
            plan.pool_rows[q, plan.b[q] if at_a else plan.a[q]] = special["e1"]
    plan.n_special = a.size
    return plan
