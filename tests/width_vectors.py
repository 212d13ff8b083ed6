"""Row widths at which the reference-order re-score changes form, and corpora whose score bits show what a re-score did
wrong (test_width_vectors_cpu.py proves both without a GPU; test_gpu_widths.py runs every path at every width).

Every score the library returns is dot_product (rag_engine.rs:1777-1779): s = s + fl(x_i * q_i), left to right.  Two
routines compute it on the device, and which one a call gets depends on the row width alone:

  dot_ref_row (csrc/exact_dot.h)   one lane per row; groups of four 16-byte units in flight (16 f32 / 32 binary16
                                   elements), then element by element;
  staged_reference_dot + chain_sum_lds (csrc/staged_dot.h)   the products of `cpb` rows staged in LDS by all threads, one
                                   chain per row over the f32 products: a prologue that needs 4 units (of 4 products), a
                                   loop of 8 units that reloads when 12 are left, an epilogue of 4, then element by element.

`form(path, dim, dtype)` restates the dispatch, `LADDER` lists the widths derived from it and from the structure of the two
chains.  numpy only; the oracle is passed in, as in gram_vectors.py.

Rows and queries: normalize((u + g) / sqrt(dim)) as in gram_vectors.corpus -- one +-1 pattern u for rows and queries alike,
g standard normal -- so every score is positive while its terms have both signs.  In the last eight columns u g is drawn
uniformly from [-0.4, 0.6] (the element keeps u's sign and a bounded size): the product of the last element, and the sum over the last
16-byte unit, are then positive and at least 0.1 / dim for every (row, query) pair.  Every corpus starts with three rows that
are not of that kind: row 0 all zero, row 1 a real row with +Inf in its last column, row 2 a real row with NaN there (in that
order: a score of -Inf then ranks in front of the NaN by value and by row alike)."""
import functools

import numpy as np

F32 = np.float32
KIB = 1024
MAX_DIM = 8192                     # rlr_index_create (csrc/index_internal.h: kMaxDim)
LDS_SORT_CAP = 4096                # kLdsSortCap (csrc/index_internal.h): a larger k takes big_query's one-lane re-score
SCORE_ROWS_STAGED_MIN = 65         # launch_score_rows (csrc/exact.hip): `fits && n > 64`
N_SPECIAL = 3
ZERO_ROW, INF_ROW, NAN_ROW = 0, 1, 2


# ---------------------------------------------------------------- the dispatch, restated
def q_floats(dim):
    """the query (and a product row) in LDS: dim rounded up to 8 floats"""
    return (dim + 7) & ~7


def pitch16(dim, dtype):
    """rlr_index_create (csrc/index.hip): ix->pitch16 = (dim * elem + 15) / 16"""
    return (dim * (2 if dtype == "f16" else 4) + 15) // 16


def pitch_fits(dim, dtype):
    """`pitch16 * (dtype == RLR_F16 ? 8u : 4u) < ((dim + 7) & ~7u)` refuses the staged form: tail_shape (csrc/tail.hip),
    launch_rescore_staged, batch_rescore_fits, launch_batch_rescore, launch_score_rows (csrc/exact.hip).  The staged
    product loop reads q_floats(dim) elements of a row; f32 rows with dim % 8 in 1..4 are four floats narrower."""
    return pitch16(dim, dtype) * (8 if dtype == "f16" else 4) >= q_floats(dim)


def staged_cpb(dim, budget):
    """`cpb = 8; while (cpb > 1 && q_bytes + cpb * row_bytes > budget) cpb >>= 1;` then the same test once more: the rows
    staged per workgroup, 0 when not even one fits.  q_bytes = q_floats * 4, row_bytes = q_bytes + 16."""
    q_bytes = q_floats(dim) * 4
    row_bytes = q_bytes + 16
    cpb = 8
    while cpb > 1 and q_bytes + cpb * row_bytes > budget:
        cpb >>= 1
    return cpb if q_bytes + cpb * row_bytes <= budget else 0


# path -> (LDS budget, staged kernel, kernel when the staged form is refused, where the rule is written)
RULES = {
    "tail": (56 * KIB, "tail_stage_kernel", None, "tail_shape, csrc/tail.hip; refused: enqueue_query_rest (csrc/index.hip) takes `split`"),
    "split": (60 * KIB, "rescore_staged_kernel", "rescore_kernel", "launch_rescore_staged / launch_rescore, csrc/exact.hip"),
    "score_rows": (60 * KIB, "score_rows_staged_kernel", "score_rows_kernel", "launch_score_rows with n > 64, csrc/exact.hip"),
    "batch": (60 * KIB, "batch_rescore_kernel", "batch_finish_kernel",
              "batch_rescore_fits / launch_batch_rescore, csrc/exact.hip; launch_batch_finish, csrc/gemm.hip"),
}
# paths that never stage: the kernel, where
UNSTAGED = {
    "score_rows_small": ("score_rows_kernel", "launch_score_rows with n <= 64, csrc/exact.hip"),
    "big": ("rescore_kernel", "big_query with k > kLdsSortCap (`second_level` false), csrc/index.hip"),
    "hybrid_batch": ("score_rows_batch_kernel", "launch_score_rows_batch, csrc/exact.hip"),
}
PATHS = tuple(RULES) + tuple(UNSTAGED)


def legal(path, dim):
    """batch_eligible (csrc/index.hip) takes `dim % 128 == 0` only"""
    return 1 <= dim <= MAX_DIM and (path != "batch" or dim % 128 == 0)


def form(path, dim, dtype):
    """-> (kernel, cpb): the kernel that computes the returned scores of `path` at this width and the rows it stages per
    group (0: one lane per row, dot_ref_row)"""
    assert legal(path, dim) and dtype in ("f32", "f16"), (path, dim, dtype)
    if path in UNSTAGED:
        return UNSTAGED[path][0], 0
    budget, staged, fallback, _ = RULES[path]
    cpb = staged_cpb(dim, budget) if pitch_fits(dim, dtype) else 0
    if path == "batch":
        # batch_rescore_fits asks for one row (`2 * q_bytes + 16 <= 60 KiB`): the same bound as cpb >= 1 above
        assert (cpb >= 1) == (pitch_fits(dim, dtype) and 2 * q_floats(dim) * 4 + 16 <= budget)
    if cpb:
        return staged, cpb
    return form("split", dim, dtype) if fallback is None else (fallback, 0)


def classes(path, dtype):
    """every (kernel, cpb) `form` returns for the path over its legal widths"""
    return {form(path, d, dtype) for d in range(1, MAX_DIM + 1) if legal(path, d)}


def grid_step(path):
    return 128 if path == "batch" else 8


def boundaries(path, dtype):
    """[(w, w + step)]: neighbouring widths of the path's grid (multiples of 8: whole units of both dtypes, so that only the
    LDS budget decides; multiples of 128 for the batch) with different forms"""
    step = grid_step(path)
    return [(w, w + step) for w in range(step, MAX_DIM, step) if form(path, w, dtype) != form(path, w + step, dtype)]


# ---------------------------------------------------------------- the chains' own edges
def chain_route(dim):
    """the way chain_sum_lds (csrc/staged_dot.h) takes through its loops at this width, passes and reloads counted up to two:
    (prologue, loop passes, reloads, epilogue, scalar tail: 0 none / 1 elements only / 2 whole units too)"""
    units = dim // 4
    u = passes = reloads = 0
    while u + 8 <= units:
        reloads += u + 12 <= units
        passes += 1
        u += 8
    epilogue = u + 4 <= units
    if epilogue:
        u += 4
    tail = dim - 4 * u
    return units >= 4, min(passes, 2), min(reloads, 2), epilogue, 0 if tail == 0 else 1 if tail < 4 else 2


def row_route(dim, dtype):
    """the same for dot_ref_row (csrc/exact_dot.h): (groups of four units, up to two; whole units left; elements behind them)"""
    epu = 8 if dtype == "f16" else 4
    full = dim // epu
    return min(full // 4, 2), full % 4 > 0, dim % epu > 0


def chain_widths(dtype):
    """widths at which chain_sum_lds or dot_ref_row takes another way through its loops"""
    w = {1, 2, 3, 4, 5, 7, 8, 9}              # every remainder of 4; dim % 8 on both sides of the f32 pitch rule (1..4 | 5..7, 0)
    w |= {12, 13, 15}                         # three units: the longest chain without a prologue, remainders 0, 1, 3
    for b in (16, 32, 48, 64):                # 4 / 8 / 12 / 16 units: prologue + epilogue, one loop pass, the reload, two passes
        w |= {b - 1, b, b + 1}                #   (and dot_ref_row's groups of four f32 units)
    w |= {80}                                 # 20 units: two passes, both reloads, the epilogue, nothing left
    if dtype == "f32":
        w |= {20, 21}                         # five units: a whole unit behind the epilogue is left to the scalar tail
        w |= {71}                             # 17 units: two passes, the second without its reload, then a unit and 3 elements
        w |= {101, 103}                       # several passes, then dim % 8 = 5 / 7: the staged chain's scalar tail (100 is unstaged)
        w |= {26, 36, 43}                     # dot_ref_row, narrow pitch: one / two groups, then whole units, with and without elements
    else:
        w |= {23, 24, 25, 39, 40, 72}         # 3 / 5 / 9 units of eight: dot_ref_row<F16>'s group of four with a remainder of units
        w |= {83, 99}                         # two passes with / without the epilogue, then 3 elements
        w |= {100, 203}                       # several passes, dim % 8 = 4 / 3: an odd width of the staged product loop
        w |= {7678, 7684, 7688}               # too wide to stage: dot_ref_row<F16> with units, elements, or both behind its groups
    return w


def threshold_widths(path, dtype):
    return {w for pair in boundaries(path, dtype) for w in pair}


def _single(dtype):
    w = chain_widths(dtype) | threshold_widths("tail", dtype) | threshold_widths("split", dtype) | {MAX_DIM}
    if dtype == "f32":                        # the last staged width of every fused-tail class, moved into the narrow-pitch class
        w |= {lo + 4 for lo, _ in boundaries("tail", "f32")}
    return tuple(sorted(w))


# path -> dtype -> widths.  "single": rlr_search_topk in every tail mode (the `tail` and `split` rules); "score_rows":
# rlr_score_rows, both kernels; "batch": the batched pipeline
LADDER = {
    "single": {t: _single(t) for t in ("f32", "f16")},
    "score_rows": {t: tuple(sorted(chain_widths(t) | threshold_widths("score_rows", t) | {MAX_DIM})) for t in ("f32", "f16")},
    "batch": {t: tuple(sorted({128, MAX_DIM} | threshold_widths("batch", t))) for t in ("f32", "f16")},
}
# which rules of `form` a ladder has to cover
LADDER_PATHS = {"single": ("tail", "split"), "score_rows": ("score_rows", "score_rows_small"), "batch": ("batch",)}

N_SINGLE = 8 * 25 + 3      # a ragged last group for every cpb
N_BATCH = 4096 + 3         # batch_eligible wants 4096 rows
N_BIG = 4200               # k just above kLdsSortCap needs that many rows


# ---------------------------------------------------------------- corpora
def _raw(rng, u, n, dim):
    g = rng.standard_normal((n, dim), dtype=np.float32)
    t = min(8, dim)
    g[:, -t:] = u[-t:] * rng.uniform(-0.4, 0.6, (n, t)).astype(np.float32)   # u (u + g) = 1 + u g in [0.6, 1.6]
    return ((u + g) / F32(np.sqrt(dim))).astype(np.float32)


def _pattern(dim, seed):
    return np.random.default_rng([8100 + seed, dim]).choice(np.array([-1.0, 1.0], np.float32), size=dim)


def corpus(O, n, dim, f16, seed=0, inf_row=True):
    """-> rows f32 [n, dim] (on the binary16 grid if f16): the three special rows, then n - 3 rows as the module docstring says.
    inf_row=False leaves row INF_ROW a row of the construction: the corpora of the batched path, which a row of infinite
    norm keeps every query away from ("Row widths": an f32 index with an element beyond binary16 range stays on
    the f32 paths, and the guard band, which scales with the largest row norm, hands every query of a binary16 one back)."""
    assert n > N_SPECIAL
    rng = np.random.default_rng([8220 + seed, n, dim, int(f16)])
    raw = _raw(rng, _pattern(dim, seed), n, dim)
    rows = np.empty((n, dim), np.float32)
    for i in range(n):
        rows[i] = O.normalize(raw[i])
    if f16:
        rows = O.round_f16(rows)
    rows[ZERO_ROW] = 0.0
    rows[NAN_ROW, -1] = np.nan
    if inf_row:
        rows[INF_ROW, -1] = np.inf
    return rows


def queries(O, nq, dim, seed=0):
    """-> f32 [nq, dim], normalised, of the corpus' kind (the same pattern u)"""
    rng = np.random.default_rng([8300 + seed, nq, dim])
    raw = _raw(rng, _pattern(dim, seed), nq, dim)
    return np.stack([O.normalize(r) for r in raw])


@functools.lru_cache(maxsize=3)
def _case_cached(n, dim, f16, nq, inf_row):
    from oracle import oracle as O
    rows, qs = corpus(O, n, dim, f16, inf_row=inf_row), queries(O, nq, dim)
    scores = np.stack([O.scan(rows, q) for q in qs])
    for a in (rows, qs, scores):
        a.setflags(write=False)
    return rows, qs, scores


def case(n, dim, f16, nq=4, inf_row=True):
    """(rows, queries, oracle scores [nq, n]) of one corpus: computed once, shared by every path that runs it, read-only"""
    return _case_cached(int(n), int(dim), bool(f16), int(nq), bool(inf_row))


def topk(scores, k):
    """test_gpu_parity.oracle_topk on scores already scanned: NaN last, ties by row -> (rows u64, scores)"""
    key = np.where(np.isnan(scores), -np.inf, scores)
    order = np.lexsort((np.arange(len(scores)), -key.astype(np.float64)))[:k]
    return order.astype(np.uint64), scores[order]


def pattern_bits(a):
    """f32 -> u32 patterns, every NaN as the one quiet NaN the result unpacking writes (csrc/index.hip: unpack_results)"""
    a = np.ascontiguousarray(a, dtype=np.float32)
    b = a.view(np.uint32).copy()
    b[np.isnan(a)] = 0x7FC00000
    return b


# ---------------------------------------------------------------- fault models
MODELS = ("fma", "four_sums", "drop_last", "drop_unit", "skip_first_group", "repeat_first_group", "skip_last_group",
          "repeat_last_group", "next_row")
# the smallest width at which a model computes another real number than the reference chain.  next_row from 3: the rows
# of a 1-d corpus are all the vector (u), and at two columns whole sets of (row, query) pairs score the same bits
FROM_DIM = {"fma": 2, "four_sums": 4, "drop_last": 1, "drop_unit": 1, "skip_first_group": 32, "repeat_first_group": 32,
            "skip_last_group": 32, "repeat_last_group": 32, "next_row": 3}
# the share of the checked pairs whose bits must change
MIN_SHARE = {m: 1.0 for m in MODELS}
MIN_SHARE["fma"] = MIN_SHARE["four_sums"] = 1.0 / 8.0
GROUP = 16        # four units of four products: what chain_sum_lds adds per register set


def _chain(xt, yt, cols, fused=False, taps=()):
    """s = s + fl(x * y) over `cols` in that order, in f32 (fused: fl(s + x * y), the product exact in binary64);
    -> (s, {c: s before column c was added, for c in taps})"""
    s = np.zeros(xt.shape[1], np.float32)
    seen = {}
    for k in cols:
        if k in taps:
            seen[k] = s.copy()
        if fused:
            s = (s.astype(np.float64) + xt[k].astype(np.float64) * yt[k].astype(np.float64)).astype(np.float32)
        else:
            s = s + xt[k] * yt[k]
    return s, seen


def variant_scores(rows, qs, unit, models=MODELS):
    """{model: scores f32 [len(qs), len(rows)]} of rows . qs as a re-score with that fault would compute them, plus
    "reference": the strict left-to-right chain of rounded products.  unit = elements per aligned 16-byte unit of the
    stored rows (4: f32, 8: binary16).  A model that does not apply at this width (FROM_DIM) is left out."""
    n, dim = rows.shape
    nq = qs.shape[0]
    xt = np.ascontiguousarray(np.tile(rows, (nq, 1)).T)            # [dim, nq * n], query-major
    yt = np.ascontiguousarray(np.repeat(qs, n, axis=0).T)
    last_unit = (dim - 1) // unit * unit
    n_groups = dim // GROUP
    out = {}
    ref, seen = _chain(xt, yt, range(dim), taps={dim - 1, last_unit})
    out["reference"] = ref
    for m in models:
        if dim < FROM_DIM[m]:
            continue
        if m == "fma":                                             # (a) the compiler contracts s + x * q
            out[m] = _chain(xt, yt, range(dim), fused=True)[0]
        elif m == "four_sums":                                     # (b) four interleaved partial sums, combined at the end
            p = [_chain(xt, yt, range(j, dim, 4))[0] for j in range(4)]
            out[m] = (p[0] + p[1]) + (p[2] + p[3])
        elif m == "drop_last":                                     # (c)
            out[m] = seen[dim - 1]
        elif m == "drop_unit":                                     # (d) the last aligned 16-byte unit of the row
            out[m] = seen[last_unit]
        elif m == "next_row":                                      # (f) candidate i read with candidate i + 1's products
            out[m] = np.roll(ref.reshape(nq, n), -1, axis=1).reshape(-1)
        else:                                                      # (e) a register set of the pipeline skipped or added twice
            g = 0 if "first" in m else n_groups - 1
            cols = list(range(dim))
            grp = cols[g * GROUP:(g + 1) * GROUP]
            cols = cols[:g * GROUP] + (grp + grp if m.startswith("repeat") else []) + cols[(g + 1) * GROUP:]
            out[m] = _chain(xt, yt, cols)[0]
    return {m: v.reshape(nq, n) for m, v in out.items()}
