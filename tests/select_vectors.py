"""Score arrays designed for the rank searches of the top-k select (test_select_vectors_cpu.py proves what they reach,
test_gpu_select.py runs them): find_rank_bin / band_floor_key (select_dev.h), the fused batch select's find_bin
(select.hip), lds_find_rank_bin_1024 and the exact-key selectors behind sort_emit_rows (lds_select.h, sort_emit.h).

The lever: rows uploaded as given (normalize = 0) and a one-hot query e_g.  The oracle's left-to-right dot of row r is
then rows[r, g] bit for bit (every other product is an exact zero; only -0.0 comes back as +0.0), and so is every f32
scan's.  The nominated score array of query e_g IS column g: a column is written key by key,
    key = (bin1 << 21) | (bin2 << 10) | low      bin1: first radix digit (a quarter binade; bin 1536 is 2.0, bins below
                                                  1024 are the negative half, mirrored), bin2: second digit, low: 10 bits
and several queries read several columns of one corpus.

The model restates score_key, key_score and band_floor_key on integer keys with one f32 subtraction and returns what
the select must leave: mode, bin1, bin2, key_lo and the number of candidates (scores with key >= key_lo).
    fused tail (tail.hip)   DIRECT iff the scores in or above the k-th's digit-1 bin number <= direct_max: floor (bin1, 0)
    otherwise, and always in the split pipeline (select.hip): floor (bin1, bin2)
The band is 2 * rlr_default_guard_eps(dim) * scale, scale = |q| * |row|_max * 1.000002 where that exceeds 1.0001
(plan_bands / make_plan); |row|_max comes from the corpus as built.

Classes (the case names start with the letter):
  A  digit-1 rank at a bin edge b | b+1: a scores in b+1, m in b, c in b-1, mid-bin, the rest far below; k = a, a+1,
     a+m, a+m+1.  Edges at the wave and thread edges of the 256-thread finder (512 bins per wave, 8 per thread) and of
     the 1024-thread finders (128 per wave, 2 per thread), inside one thread, in the production range, and all of them
     mirrored into the negative half (there two positive scores lead, so the k-th is negative and the totals of the
     positive waves count)
  B  the same on the second digit inside one digit-1 bin, a positive and a negative one
  C  exactly 64 / 65 scores in or above the k-th's digit-1 bin (RLR_TAIL_DIRECT_MAX = 64), a handful of them between the
     DIRECT and the REFINE floor
  D  the zero crossing: the k-th score a subnormal or +0.0 (bin 1024) or a negative subnormal (bin 1023) under best scores
     near 1; every score under 2^-20 (the band swallows the bins); negatives only
  E  exactly C scores at or above the lowest floor, C = 1024 .. 4097: `low` keeps them in one digit-2 bin (1024 distinct
     low words, each used ceil(C / 1024) times: ties by row only among equal keys), `wide` spreads distinct keys over
     both sides of bit 10 and bit 21
  F  special values, results only: -0.0, NaN rows with k beyond the numbers, +-inf with the k-th score on them
  G  the best and the k-th score on rows n-1, n-2, n-3: the n % 4 tail of every float4 loop
"""
import functools

import numpy as np

F32 = np.float32
DIRECT, REFINE = 1, 2
CAP = 4096                     # kLdsSortCap: candidates of one query before the large-candidate path
LOCAL_CAP = 1024               # tail.hip: candidates one workgroup keeps for its own re-score
DEFAULT_DIRECT_MAX = 3584      # rlr_index::tail_direct_max
N_SINGLE, N_BATCH = 4099, 4100
DIM_SINGLE = 64
DIM_BATCH = 256                # the narrowest rows the shared scan takes (and a multiple of 128: the matrix-core batch)
MARGIN_ULPS = 32


# ---------------------------------------------------------------- the key map and the floor, restated
def score_key(x):
    b = np.atleast_1d(np.ascontiguousarray(x, dtype=np.float32)).view(np.uint32)
    k = np.where((b & 0x80000000) != 0, ~b, b | np.uint32(0x80000000)).astype(np.uint32)
    return np.where((b & 0x7FFFFFFF) > 0x7F800000, np.uint32(0), k).astype(np.uint32)


def key_score(k):
    k = np.atleast_1d(np.asarray(k, dtype=np.uint32))
    b = np.where((k & 0x80000000) != 0, k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32)
    return np.where(k == 0, np.uint32(0x7FC00000), b).astype(np.uint32).view(np.float32)


def band_floor_key(bin1, bin2, two_eps):
    key_floor = (int(bin1) << 21) | (int(bin2) << 10)
    if key_floor == 0:
        return 0
    with np.errstate(all="ignore"):
        lo = key_score(key_floor)[0] - F32(two_eps)          # one f32 subtraction; NaN -> key 0, -inf stays -inf
    key_lo = int(score_key(lo)[0])
    return min(key_lo, key_floor)


def default_guard_eps(dim):
    return (F32(dim) + F32(64.0)) * F32(5.9604645e-8) * F32(1.0625)


def two_eps_of(rows, dim=None, query_norm=1.0):
    """the band of a call over `rows` (stored as given) with queries of norm `query_norm`, by plan_bands / make_plan"""
    rows = np.asarray(rows)
    dim = rows.shape[1] if dim is None else dim
    with np.errstate(all="ignore"):
        ss = (rows.astype(np.float64) ** 2).sum(axis=1).astype(np.float32)
    ss = ss[~np.isnan(ss)]                                   # (a NaN row does not widen the band)
    sumsq = max(F32(1.0), ss.max()) if len(ss) else F32(1.0)
    f = float(query_norm) * float(np.sqrt(np.float64(sumsq))) * 1.000002
    scale = F32(1.0) if not f > 1.0001 else F32(f) if np.isfinite(f) else F32(3.0e38)
    with np.errstate(all="ignore"):
        return F32(2.0) * (default_guard_eps(dim) * scale)


def nomination_two_eps_of(rows, f16_rows=False, query_norm=1.0):
    """the band of the matrix-core batch over `rows`: 2 * nomination_eps(dim, dtype, scale, norm_sum) (gemm.hip)"""
    rows = np.asarray(rows)
    dim = rows.shape[1]
    rn = float(np.sqrt(max(1.0, float((rows.astype(np.float64) ** 2).sum(axis=1).max()))))
    f, nsum = query_norm * rn * 1.000002, query_norm + rn
    prod = 1.0 if not f > 1.0001 else f
    nsum = 2.0 if not nsum > 2.0001 else nsum * 1.000002
    op = 2.0 ** -11 if f16_rows else 2.0 ** -10
    return 2.0 * ((op * 1.001 + 2.0 * (dim + 64.0) * 2.0 ** -24) * prod + 2.0 ** -25 * np.sqrt(dim) * nsum) * 1.0625


BAND_CAP = 2048                # gemm.hip kBandCap: rows one query of a batch may re-score before it is handed back


def model(scores, k, two_eps, pipeline="fused", direct_max=DEFAULT_DIRECT_MAX):
    """what the select leaves for rank k of `scores`: pipeline "fused" (tail.hip) or "split" (select.hip)"""
    keys = score_key(scores)
    k = min(int(k), len(keys))
    kth = int(np.sort(keys)[::-1][k - 1])
    bin1 = kth >> 21
    n_ge = int(((keys >> 21) >= bin1).sum())
    direct = pipeline == "fused" and n_ge <= direct_max
    bin2 = 0 if direct else (kth >> 10) & 2047
    key_lo = band_floor_key(bin1, bin2, two_eps)
    return dict(mode=DIRECT if direct else REFINE, bin1=bin1, bin2=bin2, key_lo=key_lo, n_ge=n_ge, kth=kth,
                count=int((keys >= key_lo).sum()))


def tail_report(m, scores, k, pipeline="fused", direct_max=DEFAULT_DIRECT_MAX):
    """-> (n_candidates, n_retries) as rlr_profile counts them for model result `m`.  One rule beyond the count: a
    workgroup of the fused tail keeps at most LOCAL_CAP candidates of its slice; with more it flags an overflow, the finish
    reports max(count, CAP + 1) and the large-candidate path answers (tail.hip: collect_rescore / tail_finish).  Stage 1's
    slices never hold that many rows here; stage 2 (REFINE) runs few workgroups for a small k (launch_tail_stage2)."""
    count = m["count"]
    n = len(scores)
    if pipeline == "fused" and m["mode"] == REFINE:
        units = n // 4 + 1
        blocks = (units + 1023) // 1024
        if k > 256 or k > direct_max:
            blocks = max(blocks, (units + 63) // 64)
        blocks = max(2, blocks)
        assert blocks <= 64                                  # (below every device's CU count: the grid is not clipped)
        n4 = n // 4
        chunk = (n4 + blocks - 1) // blocks
        rows = np.flatnonzero(score_key(scores) >= m["key_lo"])
        owner = np.where(rows < n4 * 4, (rows // 4) // chunk, 0)       # the n % 4 tail belongs to workgroup 0
        if len(rows) and np.bincount(owner).max() > LOCAL_CAP:
            count = max(count, CAP + 1)
    return count, int(count > CAP)


def finder(hist, rank, threads, defect=None, drop_wave=None):
    """find_rank_bin (threads = 256, 8 bins per thread) / lds_find_rank_bin_1024 and the fused batch select's find_bin
    (threads = 1024, 2 per thread) as a model of their structure: per-thread sums, suffix sums inside a wave of 64, the
    totals of the waves above, then the thread's bins from its top bin down.  -> (bin, rank inside it, its count);
    (0, 1, 0) when no thread claims the rank, as the kernels' preset.  Defects for the mutation proof:
      drop_wave = w   the total of wave w is left out of the waves above
      "skip_top"      a thread starts one under its top bin         "skip_bottom"   ... stops one above its bottom bin
      "lt"            rank < with instead of rank <= with           "le"            above <= rank instead of above < rank"""
    hist = np.asarray(hist, np.int64)
    per = len(hist) // threads
    loc = hist.reshape(threads, per)
    sums = loc.sum(axis=1)
    waves = sums.reshape(-1, 64)
    suf = np.cumsum(waves[:, ::-1], axis=1)[:, ::-1]          # inclusive suffix sum inside the wave
    tot = waves.sum(axis=1)
    if drop_wave is not None:
        tot = tot.copy()
        tot[drop_wave] = 0
    above_waves = np.r_[np.cumsum(tot[::-1])[::-1][1:], 0]
    above_t = (above_waves[:, None] + suf - waves).reshape(threads)
    inner = np.cumsum(loc[:, ::-1], axis=1)[:, ::-1] - loc     # the thread's own bins above bin i
    top = per - 1
    if defect == "skip_top":
        inner = inner - loc[:, top:top + 1]
    above = above_t[:, None] + inner
    with_ = above + loc
    lo_ok = above <= rank if defect == "le" else above < rank
    hi_ok = rank < with_ if defect == "lt" else rank <= with_
    hit = lo_ok & hi_ok
    if defect == "skip_top":
        hit[:, top] = False
    if defect == "skip_bottom":
        hit[:, 0] = False
    where = np.flatnonzero(hit.reshape(-1))
    if not len(where):
        return 0, 1, 0
    b = int(where[0])                                         # several claims: the lowest bin (the later store of a thread)
    return b, int(rank - above.reshape(-1)[b]), int(hist[b])


def select_with(scores, k, two_eps, pipeline="fused", direct_max=DEFAULT_DIRECT_MAX, defect=None, drop_wave=None,
                threads=(256, 256), key_of=score_key, mode_le=True):
    """the select as the kernels run it -- histograms, `finder` per digit, band floor, collect -- with an optional
    defect.  threads: finder width of digit 1 and digit 2.  -> (count, candidate rows)"""
    keys = key_of(scores)
    k = min(int(k), len(keys))
    h1 = np.bincount(keys >> 21, minlength=2048)
    bin1, k2, in_bin = finder(h1, k, threads[0], defect, drop_wave)
    n_ge = k - k2 + in_bin
    direct = pipeline == "fused" and (n_ge <= direct_max if mode_le else n_ge < direct_max)
    if direct:
        bin2 = 0
    else:
        h2 = np.bincount((keys[(keys >> 21) == bin1] >> 10) & 2047, minlength=2048)
        bin2 = finder(h2, k2, threads[1], defect, drop_wave)[0]
    key_lo = band_floor_key(bin1, bin2, two_eps)
    rows = np.flatnonzero(keys >= key_lo)
    return len(rows), rows


def topk_rows(scores, k, among=None):
    """the oracle's order (score descending, NaN last, ties by row) over `among` (default: every row)"""
    idx = np.arange(len(scores)) if among is None else np.asarray(among)
    s = np.asarray(scores)[idx]
    key = np.where(np.isnan(s), 0.0, s).astype(np.float64)    # (-inf is a number: it orders in front of every NaN)
    return idx[np.lexsort((idx, -key, np.isnan(s)))[:k]]


# ---------------------------------------------------------------- pieces of a column
def mk(bin1, bin2, low):
    return (np.asarray(bin1, np.int64) << 21) | (np.asarray(bin2, np.int64) << 10) | np.asarray(low, np.int64)


def mk16(bin1, b2):
    """the key of digit-1 bin `bin1` whose value lies on the binary16 grid: 13 low value bits zero (b2: a multiple of 8; in
    the negative half the value's bits are the key's complement)"""
    bin1, b2 = np.asarray(bin1, np.int64), np.asarray(b2, np.int64)
    return np.where(bin1 < 1024, mk(bin1, b2 | 7, 1023), mk(bin1, b2, 0))


def vals(keys):
    return key_score(np.asarray(keys, np.int64).astype(np.uint32))


def spread(rng, bin1, count, f16=False, bin2_range=(600, 1400)):
    """`count` distinct keys of digit-1 bin `bin1`, away from its floors (f16: on the binary16 grid)"""
    lo, hi = bin2_range
    if f16:
        b2 = rng.choice(np.arange((lo + 7) // 8 * 8, hi, 8), size=count, replace=False)
        return mk16(bin1, b2)
    b2 = rng.choice(np.arange(lo, hi), size=count, replace=False)
    return mk(bin1, b2, rng.integers(256, 768, size=count))


def filler(rng, count, bins, f16=False):
    """keys of the rows that play no part: digit-1 bins [bins[0], bins[1]), anywhere inside them (ties allowed)"""
    b1 = rng.integers(bins[0], bins[1], size=count)
    if f16:
        return mk16(b1, rng.integers(0, 256, size=count) * 8)
    return mk(b1, rng.integers(0, 2048, size=count), rng.integers(0, 1024, size=count))


def pos_below(b):
    """filler bins of a positive column whose designed scores start in bin b: 2^-6 and less of them (and normal binary16)"""
    return (b - 48, b - 24)


def edge_keys(rng, hi_bin, a, m, c, f16=False, lead=()):
    """a keys in hi_bin, m in hi_bin - 1, c in hi_bin - 2; lead: (bin, count) pairs above them"""
    parts = [spread(rng, b, cnt, f16) for b, cnt in lead]
    parts += [spread(rng, hi_bin, a, f16), spread(rng, hi_bin - 1, m, f16), spread(rng, hi_bin - 2, c, f16)]
    return np.concatenate(parts)


A_EDGES = {1535: "wave and thread edge of all three finders (2.0)", 1663: "wave edge of the 1024-thread finders (2^33)",
           1543: "thread edge of the 256-thread finder", 1537: "thread edge of the 1024-thread finders",
           1536: "inside one thread", 1539: "inside one thread", 1531: "the production range", 1527: "the production range"}
A_POP = (5, 6, 4)              # a, m, c
A_LEAD = 2                     # positive scores in front of a negative column's a (they count among the a)
B_EDGES = (7, 127, 511, 1023, 1535, 2047)     # bin2 edge e | e+1; 2047: the top bin against bin 0 of the next digit-1 bin
B_BINS = {"pos": 1533, "neg": 514}
E_SIZES = (1024, 1025, 2048, 4095, 4096, 4097)


class Corpus:
    """columns of one corpus: designed keys on disjoint rows (unless a column names its rows), filler elsewhere"""

    def __init__(self, name, n, dim, seed, f16=False):
        self.name, self.n, self.dim, self.f16 = name, n, dim, f16
        self.rng = np.random.default_rng(seed)
        self.free = list(self.rng.permutation(n))
        self.cols, self.cases = [], []

    def reserve(self, rows):
        """named rows leave the pool the columns draw from"""
        named = set(int(r) for r in rows)
        self.free = [r for r in self.free if r not in named]

    def take(self, count):
        out, self.free = self.free[:count], self.free[count:]
        assert len(out) == count, "the corpus has no rows left for a disjoint column"
        return np.array(out, np.int64)

    def add(self, name, cls, designed, below, ks, rows=None, promise=None, shuffle=True):
        designed = np.asarray(designed, np.int64)
        col = vals(filler(self.rng, self.n, below, self.f16)).copy()
        if rows is None:
            rows = self.take(len(designed))
        else:
            self.reserve(rows)
        rows = np.asarray(rows, np.int64)
        order = self.rng.permutation(len(designed)) if shuffle else np.arange(len(designed))
        col[rows] = vals(designed[order])
        self.cols.append(col)
        self.cases.append(dict(name=name, cls=cls, corpus=self.name, col=len(self.cols) - 1, ks=[int(k) for k in ks],
                               counted=True, rows=rows, promise=promise or {}))

    def add_raw(self, name, cls, col, ks, counted, promise=None, rows=None):
        self.cols.append(np.asarray(col, np.float32))
        self.cases.append(dict(name=name, cls=cls, corpus=self.name, col=len(self.cols) - 1, ks=[int(k) for k in ks],
                               counted=counted, rows=np.asarray(rows if rows is not None else [], np.int64),
                               promise=promise or {}))

    def build(self, anchor=None):
        assert len(self.cols) <= self.dim
        rows = np.zeros((self.n, self.dim), np.float32)
        for g, col in enumerate(self.cols):
            rows[:, g] = col
        if anchor is not None:                               # one filler row pins |row|_max (and so the band) of the corpus
            rows[anchor[0], self.dim - 1] = anchor[1]
        rows.setflags(write=False)
        return rows


def add_edge(cp, name, cls, b, negative, rng, note=""):
    """class A column for edge b | b+1 (negative: its mirror 2046-b | 2047-b, two positive scores leading)"""
    a, m, c = A_POP
    if not negative:
        keys = edge_keys(rng, b + 1, a, m, c, cp.f16)
        hi, below = b + 1, pos_below(b)
    else:
        hi = 2047 - b
        keys = edge_keys(rng, hi, a - A_LEAD, m, c, cp.f16, lead=[(b, A_LEAD)])
        below = (hi - 8, hi - 4)
    ks = [a, a + 1, a + m, a + m + 1]
    cp.add(name, cls, keys, below, ks, promise=dict(bin1={a: hi, a + 1: hi - 1, a + m: hi - 1, a + m + 1: hi - 2},
                                                    pop=(hi, a - (A_LEAD if negative else 0), m, c), note=note))


def add_tail_rows(cp, name, negative, rng, order):
    """class G: the three best scores on rows n-1, n-2, n-3 in `order` (best first), six more in the same digit-1 bin, five
    in the bin below; k = 1 .. 4"""
    n = cp.n
    hi = 516 if negative else 1530
    top = np.sort(spread(rng, hi, 9, cp.f16, (900, 1400)))[::-1]
    low = spread(rng, hi - 1, 5, cp.f16)
    cp.reserve(list(order) + [0])
    rows = np.r_[np.array(order, np.int64), 0, cp.take(5 + 5)]
    below = (hi - 8, hi - 4) if negative else pos_below(hi)
    cp.add(name, "G", np.r_[top, low], below, [1, 2, 3, 4], rows=rows, shuffle=False,
           promise=dict(top=list(order) + [0], bin1={k: hi for k in (1, 2, 3, 4)}))


# ---------------------------------------------------------------- the corpora
def _single(name, seed, f16=False):
    return Corpus(name, N_SINGLE, DIM_SINGLE, seed, f16)


def build_A(sign, f16=False, with_G=False):
    cp = _single(f"A_{sign}" + ("_f16" if f16 else ""), 101 + (sign == "neg") + 10 * f16, f16)
    n = cp.n
    if with_G:
        add_tail_rows(cp, f"G_{sign}", sign == "neg", cp.rng, (n - 1, n - 3, n - 2) if sign == "pos" else (n - 2, n - 1, n - 3))
    for b, note in A_EDGES.items():
        if b == 1663:
            continue
        add_edge(cp, f"A_{sign}_{b}", "A", b, sign == "neg", cp.rng, note)
    return cp


def build_A_big():
    cp = _single("A_big", 103)
    add_edge(cp, "A_pos_1663", "A", 1663, False, cp.rng, A_EDGES[1663])
    add_edge(cp, "A_neg_1663", "A", 1663, True, cp.rng, A_EDGES[1663])
    return cp


def b_keys(rng, bin1, e):
    """class B: a = 3 keys in digit-2 bin e+1 (bin 0 of the next digit-1 bin for e = 2047), m = 4 in e, c = 3 in e-1.  The
    lowest three keep 700 ulps and more between them and the floor above them: clear of the band, which is 200 to 300"""
    a_keys = mk(bin1 + 1, 0, 512 + np.arange(3) * 7) if e == 2047 else mk(bin1, e + 1, 512 + np.arange(3) * 7)
    return np.r_[a_keys, mk(bin1, e, 300 + np.arange(4) * 11), mk(bin1, e - 1, 100 + np.arange(3) * 13)]


def add_B(cp, sign, e):
    b1 = B_BINS[sign]
    up = (b1 + 1, 0) if e == 2047 else (b1, e + 1)
    cp.add(f"B_{sign}_{e}", "B", b_keys(cp.rng, b1, e), pos_below(b1) if sign == "pos" else (b1 - 2, b1), [3, 4, 7, 8],
           promise=dict(floor={3: up, 4: (b1, e), 7: (b1, e), 8: (b1, e - 1)}))


def build_B_pos():
    cp = _single("B_pos", 111)
    for e in B_EDGES:
        add_B(cp, "pos", e)
    return cp


def build_B_neg(e):
    """(one corpus per column: a negative column's filler is larger than its designed scores, and six of them in one
    corpus would carry the band past half a digit-2 bin)"""
    cp = _single(f"B_neg_{e}", 120 + B_EDGES.index(e))
    add_B(cp, "neg", e)
    return cp


def build_C():
    cp = _single("C", 131)
    b = 1530
    for total in (64, 65):
        top = mk(b, cp.rng.choice(np.arange(1200, 1600), size=50, replace=False), cp.rng.integers(256, 768, size=50))
        between = mk(b, cp.rng.choice(np.arange(100, 500), size=total - 50, replace=False), cp.rng.integers(256, 768, size=total - 50))
        cp.add(f"C_{total}", "C", np.r_[top, between], pos_below(b), [50],
               promise=dict(n_ge=total, mode64=DIRECT if total <= 64 else REFINE, between=total - 50))
    return cp


def build_D():
    cp = _single("D", 141)
    rng = cp.rng
    neg_far = (509, 513)                                     # -1.5 .. -3.4
    near1 = spread(rng, 1531, 5)
    sub_pos = mk(1024, 0, 0) + rng.choice(np.arange(1000, 1 << 20), size=10, replace=False)
    zeros = np.full(20, mk(1024, 0, 0))
    cp.add("D_zero", "D", np.r_[near1, sub_pos, zeros], neg_far, [5, 6, 15, 16, 35],
           promise=dict(bin1={5: 1531, 6: 1024, 15: 1024, 16: 1024, 35: 1024}, count={6: 35, 15: 35, 16: 35, 35: 35}))
    sub_neg = mk(1023, 2047, 1023) - rng.choice(np.arange(1000, 1 << 20), size=10, replace=False)
    cp.add("D_neg_subnormal", "D", np.r_[spread(rng, 1531, 5), sub_neg], neg_far, [6, 15],
           promise=dict(bin1={6: 1023, 15: 1023}, count={6: 15, 15: 15}))
    tiny = mk(rng.integers(1292, 1448, size=600), rng.integers(0, 2048, size=600), rng.integers(0, 1024, size=600))
    assert len(np.unique(tiny)) == 600
    cp.add("D_tiny", "D", tiny, neg_far, [1, 300, 600], promise=dict(count={1: 600, 300: 600, 600: 600}, below=2.0 ** -20))
    cp.add("D_negatives", "D", np.r_[spread(rng, 515, 10), spread(rng, 514, 10)], (508, 511), [1, 10, 11, 20],
           promise=dict(bin1={1: 515, 10: 515, 11: 514, 20: 514}, all_negative=True))
    return cp


E_ANCHOR = (7, 8.0)            # row 7 is filler in every E column and carries 8.0 in the last dimension: |row|_max = 8


def e_keys(rng, C, variant):
    if variant == "low":
        return mk(1533, 700, np.arange(C) % 1024)
    k = np.unique(mk(rng.integers(1532, 1534, size=2 * C), rng.integers(0, 2048, size=2 * C), rng.integers(0, 1024, size=2 * C)))
    return rng.permutation(k)[:C]


def build_E():
    """every E column is designed on rows drawn anew (they overlap); rows 7 and 8 stay filler.  The `wide` columns are drawn
    again, seed by seed, until no key of theirs lies within the margin of a floor their cases ask for"""
    cp = _single("E", 151)
    pool = np.setdiff1d(np.arange(cp.n), [7, 8])
    two_eps = two_eps_of(np.array([[E_ANCHOR[1]] + [0.0] * (DIM_SINGLE - 1)], np.float32))     # (the anchor row's band)
    for variant in ("low", "wide"):
        for C in E_SIZES:
            ks = [1, 1024, 1025, min(C, CAP)]
            for seed in range(64):
                rng = np.random.default_rng(1510 + 64 * E_SIZES.index(C) + seed)
                keys = e_keys(rng, C, variant)
                rows = rng.choice(pool, size=C, replace=False)
                col = vals(filler(rng, cp.n, pos_below(1533))).copy()
                col[rows] = vals(keys)
                if all(margin(col, k, two_eps, pl, dm) >= 4 * MARGIN_ULPS for k in ks for pl, dm in PIPELINES.values()):
                    break
            else:
                raise AssertionError("no seed keeps the wide column clear of its floors")
            cp.add_raw(f"E_{variant}_{C}", "E", col, ks, True, promise=dict(C=C, variant=variant), rows=rows)
    return cp


def build_G():
    cp = _single("G", 161)
    n = cp.n
    add_tail_rows(cp, "G_pos", False, cp.rng, (n - 1, n - 3, n - 2))
    add_tail_rows(cp, "G_neg", True, cp.rng, (n - 2, n - 1, n - 3))
    return cp


def build_F(which):
    cp = _single(f"F_{which}", 171 + ["negzero", "nan", "inf"].index(which))
    rng, n = cp.rng, cp.n
    if which == "negzero":                                   # 6 positives, then -0.0 / +0.0 / subnormals of both signs in turn
        col = vals(filler(rng, n, (509, 513))).copy()
        rows = rng.choice(n, size=46, replace=False)
        col[rows[:6]] = vals(spread(rng, 1531, 6))
        col[rows[6:26:2]] = F32(-0.0)
        col[rows[7:26:2]] = F32(0.0)
        col[rows[26:36]] = vals(mk(1024, 0, 0) + rng.integers(1, 1 << 20, size=10))
        col[rows[36:46]] = vals(mk(1023, 2047, 1023) - rng.integers(1, 1 << 20, size=10))
        cp.add_raw("F_negzero", "F", col, [6, 7, 16, 17, 26, 36, 46], False, rows=rows)
    elif which == "nan":                                     # 99 numbers, 4000 NaN rows: k runs past the numbers
        col = np.full(n, np.nan, np.float32)
        rows = rng.choice(n, size=99, replace=False)
        col[rows] = vals(np.r_[spread(rng, 1531, 40), spread(rng, 1530, 40), spread(rng, 515, 19)])
        cp.add_raw("F_nan", "F", col, [99, 100, 120], False, rows=rows)
    else:                                                    # +inf x 2, 50 numbers, -inf x 5, NaN elsewhere
        col = np.full(n, np.nan, np.float32)
        rows = rng.choice(n, size=57, replace=False)
        col[rows[:2]] = np.inf
        col[rows[2:52]] = vals(np.r_[spread(rng, 1663, 25), spread(rng, 383, 25)])
        col[rows[52:]] = -np.inf
        cp.add_raw("F_inf", "F", col, [1, 2, 3, 52, 53, 55, 57, 60], False, rows=rows)
    return cp


# name -> (RLR_TAIL pipeline, direct_max) of the four modes of test_gpu_tail.MODES, plus class C's switch
PIPELINES = {"direct": ("fused", 4096), "refine": ("fused", 0), "default": ("fused", DEFAULT_DIRECT_MAX), "split": ("split", 0)}
MODE64 = ("fused", 64)

SINGLE = {"A_pos": lambda: build_A("pos"), "A_neg": lambda: build_A("neg"), "A_big": build_A_big, "B_pos": build_B_pos,
          **{f"B_neg_{e}": functools.partial(build_B_neg, e) for e in B_EDGES},
          "C": build_C, "D": build_D, "E": build_E, "G": build_G,
          **{f"F_{w}": functools.partial(build_F, w) for w in ("negzero", "nan", "inf")},
          "A_pos_f16": lambda: build_A("pos", f16=True, with_G=True), "A_neg_f16": lambda: build_A("neg", f16=True, with_G=True)}


def margin(col, k, two_eps, pipeline, direct_max):
    """ulps between the model's key_lo and the nearest score key"""
    m = model(col, k, two_eps, pipeline, direct_max)
    return int(np.abs(score_key(col).astype(np.int64) - m["key_lo"]).min())


@functools.lru_cache(maxsize=None)
def corpus(name):
    """-> (rows f32 [n, dim] read-only, cases, two_eps) of a corpus of SINGLE or BATCH"""
    if name == "batch":
        cp = Corpus("batch", N_BATCH, DIM_BATCH, 181, f16=True)
        n = cp.n
        add_tail_rows(cp, "G_pos", False, cp.rng, (n - 1, n - 3, n - 2))
        add_tail_rows(cp, "G_neg", True, cp.rng, (n - 2, n - 1, n - 3))
        for sign in ("pos", "neg"):
            for b in A_EDGES:
                if b != 1663:
                    add_edge(cp, f"A_{sign}_{b}", "A", b, sign == "neg", cp.rng, A_EDGES[b])
        rows = cp.build()
    else:
        cp = SINGLE[name]()
        rows = cp.build(anchor=E_ANCHOR if name == "E" else None)
    for c in cp.cases:
        c["rows"].setflags(write=False)
    return rows, cp.cases, two_eps_of(rows)


def one_hot(dim, g):
    q = np.zeros(dim, np.float32)
    q[g] = 1.0
    return q


def all_cases(names=None):
    """every (corpus name, case) of the single-query corpora"""
    for name in (names or SINGLE):
        for c in corpus(name)[1]:
            yield name, c


# ---------------------------------------------------------------- the sampled batch
N_SAMPLED, DIM_SAMPLED, SAMPLE, K_SAMPLED = 135037, 128, 65536, 12


@functools.lru_cache(maxsize=1)
def sampled_corpus():
    """One corpus above 131 072 rows (the batch then selects over a sample of its first 65 536 rows and filters the rest by
    the sample's floor): the designed top-12 of a column inside the sample rows or behind them (then the sample holds 14
    decoys three bins further down, which set its floor), positive or negative (tau below zero in the GEMM epilogue's
    compare).  Everything on the binary16 grid.  -> (rows, cases)"""
    rng = np.random.default_rng(191)
    n = N_SAMPLED
    rows = np.zeros((n, DIM_SAMPLED), np.float32)
    cases = []
    g = 0
    for sign in ("pos", "neg"):
        for where, (lo, hi) in (("inside", (0, SAMPLE)), ("behind", (SAMPLE, n))):
            top_bin = 1530 if sign == "pos" else 516
            below = pos_below(top_bin) if sign == "pos" else (top_bin - 8, top_bin - 4)
            col = vals(filler(rng, n, below, f16=True)).copy()
            at = rng.choice(np.arange(lo, hi), size=K_SAMPLED + 4, replace=False)
            if where == "behind":
                at[:3] = (n - 1, SAMPLE, SAMPLE + 255)
            col[at] = vals(np.r_[spread(rng, top_bin, K_SAMPLED, True), spread(rng, top_bin - 1, 4, True)])
            if where == "behind":                            # the sample's own k-th: decoys three bins down, far above the filler
                decoys = rng.choice(SAMPLE, size=K_SAMPLED + 2, replace=False)
                col[decoys] = vals(spread(rng, top_bin - 3, K_SAMPLED + 2, True))
            rows[:, g] = col
            cases.append(dict(name=f"sampled_{sign}_{where}", col=g, rows=at, sign=sign, where=where))
            g += 1
    rows.setflags(write=False)
    return rows, cases
