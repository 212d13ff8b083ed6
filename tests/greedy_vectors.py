"""Pools that put the greedy MMR chain (mmr_greedy_lazy_kernel<J>, J = 1, 2, 5, 8, 16, and mmr_greedy_kernel, csrc/exact.hip)
into each of its states on purpose (test_greedy_vectors_cpu.py proves that they reach them, test_gpu_greedy.py runs them).

Rows.  Every corpus row has at most two non-zero elements, both signed powers of two (or small dyadic numbers) on the
binary16 grid: element 0 is shared by all rows (`a`), element 1 + group holds the row's own `b`.  So
G[i][j] = a_i a_j + [group_i == group_j] b_i b_j: two exact products and one exact sum at most, whatever the order of the
additions and whether the rows are stored as f32 or binary16.  The Gram kernels (which have their own test) cannot colour the
result: what a pool shows is the chain.  Two more rows hold NaN / Inf elements (their whole Gram row is non-finite).

The traced restatement is mmr_restatement.mmr_from_gram with a record per pick: how many candidates held the maximum, the
winner's position in `remaining` and its candidate index, the sign of a logged zero, whether a candidate of finite relevance
had a non-finite MMR value, how many removals the kernel's tie replay starts from; and whether the loop broke early.

Plans: a plan is a list of pools of one stride P (rows, relevance, size, k, lambda per pool), built for one state of the
chain.  P = 64, 128, 320, 512, 1024 reach J = 1, 2, 5, 8, 16; 1030 is one pool through mmr_greedy_kernel.

numpy only; the oracle is passed in, as in mmr_restatement.py."""
import collections
import functools

import numpy as np

import mmr_restatement as R

DIM = 24
STRIDES = (64, 128, 320, 512, 1024)                              # the largest pool of each J: every register slot is in use
SINGLE = 1030                                                    # above 1024: one pool, mmr_greedy_kernel (LDS `rem`)
GREEDY_J = ((64, 1), (128, 2), (320, 5), (512, 8), (1024, 16))   # launch_mmr_greedy: J by the pool stride
BATCH_PLANS = ("slot_sweep", "tie_sweep", "tie_forms", "zeros", "maxsim", "overflow", "ends", "ragged")
SINGLE_PLANS = ("tie_forms", "zeros", "maxsim", "overflow", "ends")
NAN = float("nan")
FLT_MAX = float(np.finfo(np.float32).max)
BIG_LAM = float(2.0 ** 100)                                      # 1 - (-2^100) rounds to 2^100 in f32
REL_MAX = FLT_MAX / BIG_LAM                                      # the largest relevance whose 2^100-fold is finite


def greedy_j(P):
    """the register slots per lane of the kernel a pool stride of P runs (0: mmr_greedy_kernel)"""
    for limit, j in GREEDY_J:
        if P <= limit:
            return j
    return 0


# ---------------------------------------------------------------- rows
class Corpus:
    """rows by (a, group, b), deduplicated; `g` is the exact Gram entry of two finite rows"""

    def __init__(self):
        self.spec, self.at = [], {}

    def row(self, a, group=0, b=0.0):
        key = (float(a), int(group) if b else 0, float(b))
        if key not in self.at:
            assert 0 <= key[1] < DIM - 1
            self.at[key] = len(self.spec)
            self.spec.append(key)
        return self.at[key]

    def special(self, kind):
        if kind not in self.at:
            self.at[kind] = len(self.spec)
            self.spec.append(kind)
        return self.at[kind]

    def g(self, i, j):
        (a, gi, b), (c, gj, d) = self.spec[i], self.spec[j]
        return a * c + (b * d if gi == gj else 0.0)

    def rows(self):
        out = np.zeros((len(self.spec), DIM), np.float32)
        for i, s in enumerate(self.spec):
            if s == "nan":                                       # NaN in the shared element: NaN against every row
                out[i, 0], out[i, 3], out[i, 5] = np.nan, np.inf, 1.0
            elif s == "inf":                                     # +-Inf against a row with a != 0, NaN against a == 0
                out[i, 0] = np.inf
            else:
                out[i, 0], out[i, 1 + s[1]] = s[0], s[2]
        return out

    def finite(self):
        return np.array([not isinstance(s, str) for s in self.spec])

    def exact_gram(self):
        """the Gram matrix of the finite rows in exact arithmetic (binary64 holds every term), NaN where a row is not finite"""
        n = len(self.spec)
        out = np.full((n, n), np.nan)
        for i in range(n):
            for j in range(n):
                if not isinstance(self.spec[i], str) and not isinstance(self.spec[j], str):
                    out[i, j] = self.g(i, j)
        return out


# ---------------------------------------------------------------- plans
class Plan:
    """Q pools of stride P.  pool_rows u64 [Q, P] (corpus rows by slot), rel f32 [Q, P], sizes u32 [Q], k [Q], lam f32 [Q],
    state [Q] (what the pool was built for), aim [Q] = (pick, slot) the state is about (slot None: whichever wins), or None.
    The tail of every pool beyond its size holds valid row numbers and NaN relevance."""

    def __init__(self, name, P, fill):
        self.name, self.P, self._fill = name, P, np.asarray(fill, np.uint64)
        self._rows, self._rel, self.sizes, self.k, self.lam, self.state, self.aim = [], [], [], [], [], [], []

    def add(self, state, size, k, lam, slots, aim=None):
        q = len(self.sizes)
        rows = self._fill[(np.arange(self.P) * 7 + q * 3) % self._fill.size].copy()
        rel = np.full(self.P, np.nan, np.float32)
        for s, (r, v) in slots.items():
            assert 0 <= s < size <= self.P, (self.name, state, s, size)
            rows[s], rel[s] = r, v
        self._rows.append(rows); self._rel.append(rel)
        self.sizes.append(size); self.k.append(k); self.lam.append(np.float32(lam)); self.state.append(state); self.aim.append(aim)

    def freeze(self):
        self.pool_rows = np.ascontiguousarray(np.stack(self._rows), dtype=np.uint64)
        self.rel = np.ascontiguousarray(np.stack(self._rel), dtype=np.float32)
        self.sizes = np.asarray(self.sizes, np.uint32)
        self.k = np.asarray(self.k, np.uint32)
        self.lam = np.asarray(self.lam, np.float32)
        self.Q = self.sizes.size
        for a in (self.pool_rows, self.rel, self.sizes, self.k, self.lam):
            a.setflags(write=False)
        del self._rows, self._rel
        return self

    def calls(self):
        """the pools grouped by (k, lambda): one batch call each -> [(pool indices, k, lambda)]"""
        out = collections.OrderedDict()
        for q in range(self.Q):
            out.setdefault((int(self.k[q]), float(self.lam[q])), []).append(q)
        return [(np.array(qs), k, lam) for (k, lam), qs in out.items()]


def _same_mmr(cp, picked, r1, rel1, r2):
    """the relevance of row r2 at which it ties with (r1, rel1) under lambda = 0.5 once `picked` rows were selected"""
    ms = lambda r: max([0.0] + [cp.g(p, r) for p in picked])
    return rel1 + (ms(r2) - ms(r1))


def _slot_sweep(cp, P, fill):
    """pool c: slot c wins pick 2 alone (1.75 against 0); its lane holds no other number, slots c - 64 and c + 64 are NaN"""
    pl = Plan("slot_sweep", P, fill)
    one, half = cp.row(1.0), cp.row(0.5)
    for c in range(1, P):
        d = c + 1 if c + 1 < P else c - 1
        pl.add("fast_winner", P, 3, 0.5, {0: (one, NAN if c % 2 else 0.25), c: (half, 4.0), d: (one, 1.0)}, aim=(1, c))
    return pl


def _tie_sweep(cp, P, fill):
    """pool (c, way): slot c and one other candidate tie exactly at pick 3 and c wins by position.
    first   size c + 1: pick 1's swap_remove has put c (the last candidate) at position 0; the loser is slot 2
    second  size c + 2: pick 2 (slot 1) has moved c (then last) to position 1; the loser is slot 2
    own     size P: c stands at its own position, the loser c + 2 behind it (pick 2 is c + 1)
    In `first` and `second` the winner has the HIGHER index: a kernel that takes the lowest index picks slot 2."""
    pl = Plan("tie_sweep", P, fill)
    one, x = cp.row(1.0), cp.row(0.5, 1, 1.0)
    w, l = cp.row(0.5, 1, 0.5), cp.row(0.25, 1, 0.5)
    for c in range(1, P):
        for way in ("first", "second", "own"):
            if way == "first":
                if c < 3:
                    continue
                size, px, e = c + 1, 1, 2
            elif way == "second":
                if c < 3 or c + 2 > P:
                    continue
                size, px, e = c + 2, 1, 2
            else:
                if c + 2 > P - 2:
                    continue
                size, px, e = P, c + 1, c + 2
            rw, rl = (w, l) if (c + (way == "second")) % 2 else (l, w)
            rel_l = _same_mmr(cp, [one, x], rw, 2.0, rl)
            slots = {0: (one, NAN if c % 3 == 0 else 1.0), px: (x, 8.0), c: (rw, 2.0), e: (rl, rel_l)}
            pl.add("tie_" + way, size, 3, 0.5, slots, aim=(2, c))
    return pl


def _tie_forms(cp, P, fill):
    """all rows zero (max_sim stays 0, the MMR value is relevance / 2): the ties are those of the relevance"""
    pl = Plan("tie_forms", P, fill)
    z = cp.row(0.0)
    J = greedy_j(P)

    def zp(rels, rel0=1.0):
        out = {s: (z, v) for s, v in rels.items()}
        out[0] = (z, rel0)
        return out

    singles = {11: 8.0, 12: 7.0, 13: 6.0, 14: 5.0, 15: 4.0}
    pl.add("two_holders", P, 6, 0.5, zp({3: 10.0, P - 1: 10.0, **singles}), aim=(1, P - 1))
    pl.add("three_holders", P, 6, 0.5, zp({3: 10.0, 40: 10.0, P - 2: 10.0, **singles}, NAN), aim=(1, 3))
    pl.add("many_holders", P, 8, 0.5, zp({c: 1.0 for c in range(1, P)}), aim=(1, P - 1))
    if P > 64:
        pl.add("same_lane", P, 6, 0.5, zp({5: 10.0, 69: 10.0, **singles}), aim=(1, 5))
    if P > 128:
        far = 5 + 64 * ((P - 6) // 64)
        pl.add("same_lane", P, 6, 0.5, zp({far: 10.0, 5: 10.0, **singles}, NAN), aim=(1, None))
    first_lane = 64 * ((P - 1) // 64) if P > 64 else 1           # lane 0 holds no candidate when J = 1 (slot 0 goes first)
    pl.add("first_last_lane", P, 6, 0.5, zp({first_lane: 10.0, 63: 10.0, **singles}), aim=(1, min(first_lane, 63)))
    pl.add("picks_2_4_5", P, 7, 0.5, zp({5: 10.0, P - 1: 10.0, 7: 8.0, P - 2: 8.0, 40: 8.0, 9: 6.0, 10: 5.0}), aim=(3, P - 2))
    pl.add("last_pick", P, 6, 0.5, zp({3: 20.0, 4: 18.0, 5: 16.0, 6: 14.0, 7: 10.0, P - 1: 10.0, 9: 2.0}), aim=(5, P - 1))
    drain = {c: 3000.0 - c for c in range(1, P - 2)}
    drain[P - 2] = drain[P - 1] = 1.0
    pl.add("two_left", P, P + 7, 0.5, zp(drain), aim=(P - 2, None))
    return pl


def _zeros(cp, P, fill):
    pl = Plan("zeros", P, fill)
    z, one = cp.row(0.0), cp.row(1.0)

    def zp(rels, rel0=1.0):
        out = {s: (z, v) for s, v in rels.items()}
        out[0] = (z, rel0)
        return out

    pl.add("plus_single", P, 3, 0.5, zp({3: 0.0, 5: -1.0}), aim=(1, 3))
    pl.add("minus_single", P, 3, 0.5, zp({3: -0.0, 5: -1.0}), aim=(1, 3))
    pl.add("plus_single", P, 3, 0.5, zp({P - 1: 0.0, 5: -1.0}, NAN), aim=(1, P - 1))
    pl.add("minus_single", P, 3, 0.5, zp({P - 1: -0.0, 5: -1.0}, NAN), aim=(1, P - 1))
    pl.add("mixed_minus_wins", P, 3, 0.5, zp({3: -0.0, 9: 0.0, 5: -1.0}), aim=(1, 3))
    pl.add("mixed_plus_wins", P, 3, 0.5, zp({3: 0.0, 9: -0.0, 5: -1.0}), aim=(1, 3))
    pl.add("mixed_minus_wins", P, 3, 0.5, zp({P - 1: -0.0, 3: 0.0, 5: -1.0}), aim=(1, P - 1))
    pl.add("mixed_plus_wins", P, 3, 0.5, zp({P - 1: 0.0, 3: -0.0, 5: -1.0}), aim=(1, P - 1))
    # 0.5 * 1 - 0.5 * 1: a zero that is a difference, not a product
    pl.add("cancel", P, 3, 0.5, {0: (one, 2.0), 3: (one, 1.0), 5: (z, -1.0)}, aim=(1, 3))
    pl.add("lambda_0", P, 4, 0.0, zp({3: -0.0, 9: 0.0, 5: -1.0, 6: 0.0}), aim=(1, 3))
    pl.add("lambda_0", P, 4, 0.0, zp({3: 0.0, P - 1: -0.0, 5: -1.0}), aim=(1, P - 1))
    pl.add("lambda_1", P, 5, 1.0, zp({3: 5.0, 4: -2.0, 9: 7.0, P - 1: -1.0}), aim=(1, P - 1))
    pl.add("lambda_1", P, 5, 1.0, zp({3: 0.0, 4: -0.0, 9: -0.0, 10: 0.0}), aim=(1, 3))
    return pl


def _maxsim(cp, P, fill):
    pl = Plan("maxsim", P, fill)
    one, z = cp.row(1.0), cp.row(0.0)
    # every similarity read is negative: the floor of fold(0.0, max) holds and the logged values are relevance / 2
    c1, c2, c3 = cp.row(-0.5, 1, -1.0), cp.row(-0.25, 1, 1.0), cp.row(-0.125, 1, 0.5)
    pl.add("all_negative", P, 3, 0.5, {0: (one, 1.0), 2: (c1, 4.0), P - 1: (c2, 3.0), 7: (c3, 2.0)}, aim=(2, P - 1))
    # a pick whose row holds NaN / Inf: its Gram row is non-finite throughout and moves no running maximum
    half, quarter = cp.row(0.5), cp.row(0.25)
    for kind in ("nan", "inf"):
        bad = cp.special(kind)
        pl.add(kind + "_row_pick", P, 5, 0.5, {0: (one, 1.0), 6: (bad, 8.0), 9: (half, 4.0), P - 2: (quarter, 2.0), 3: (z, -1.0),
                                             20: (cp.row(-0.5), -2.0)}, aim=(2, 9))
        pl.add(kind + "_row_first", P, 4, 0.5, {0: (bad, 1.0), 9: (half, 4.0), P - 2: (quarter, 2.0), 3: (z, -1.0)}, aim=(1, 9))
    # 1/4 from slot 0, 1/2 from pick 2, 3/2 from pick 3: the logged value of pick 4 shows the last
    s0, p1, p2, t = cp.row(0.25), cp.row(0.5), cp.row(0.5, 3, 1.0), cp.row(1.0, 3, 1.0)
    pl.add("rising", P, 4, 0.5, {0: (s0, 1.0), 4: (p1, 16.0), P - 1: (p2, 12.0), 8: (t, 8.0)}, aim=(3, 8))
    # 3/2, then 1/2, then 1/4: the maximum keeps the first
    pl.add("falling", P, 4, 0.5, {0: (p2, 1.0), 4: (p1, 16.0), P - 1: (s0, 12.0), 8: (t, 8.0)}, aim=(3, 8))
    return pl


def _overflow(cp, P, fill):
    """lambda = -2^100: (1 - lambda) = 2^100 in f32, t0 = 2^100 * rel, and -lambda * max_sim = 2^100 * max_sim is ADDED.
    rel = 2^27 and max_sim = 2^27 give 2^127 + 2^127 = +inf from two finite terms."""
    pl = Plan("overflow", P, fill)
    z = cp.row(0.0)
    p, a, a2 = cp.row(0.0, 5, 2.0 ** 14), cp.row(0.0, 5, 2.0 ** 13), cp.row(0.0, 5, 2.0 ** 14)
    b, c = cp.row(0.0, 6, 1.0), cp.row(0.0, 7, 1.0)
    top, r27, r26, r25 = REL_MAX, 2.0 ** 27, 2.0 ** 26, 2.0 ** 25
    lo = -BIG_LAM
    pl.add("recount_pick", P, 3, lo, {0: (z, 1.0), 4: (p, top), 2: (a, r27), 9: (b, r26)}, aim=(2, 9))
    pl.add("recount_pick", P, 3, lo, {0: (z, NAN), 4: (p, top), P - 1: (a, r27), 9: (b, r26)}, aim=(2, 9))
    pl.add("recount_tie", P, 4, lo, {0: (z, 1.0), 4: (p, top), P - 1: (a, r27), 9: (b, r26), 3: (c, r26)}, aim=(2, 3))
    pl.add("recount_then_break", P, 6, lo, {0: (z, 1.0), 4: (p, top), 2: (a, r27), 9: (b, r26), P - 2: (c, r25)}, aim=(3, P - 2))
    pl.add("all_inf_break", P, 5, lo, {0: (z, 1.0), 4: (p, top), 2: (a, r27), P - 1: (a2, r26)}, aim=None)
    # the mirror: lambda = 2^100, (1 - lambda) = -2^100, negative relevance is attractive; lambda * max_sim is subtracted,
    # so a value can reach -inf (max_sim = 2^28) but never +inf
    hi = BIG_LAM
    pl.add("mirror_minus_inf", P, 4, hi, {0: (z, 1.0), 4: (p, -top), 2: (a2, -r27), 9: (b, -r26), 3: (c, -r25)}, aim=(2, 9))
    pl.add("mirror_break", P, 4, hi, {0: (z, 1.0), 4: (p, -top), 2: (a2, -r27), P - 1: (a2, -r26)}, aim=None)
    pl.add("mirror_t0_overflow", P, 4, hi, {0: (z, 1.0), 4: (p, -FLT_MAX), 2: (b, -r27), 9: (c, -r26)}, aim=(1, 2))
    return pl


def _ends(cp, P, fill):
    pl = Plan("ends", P, fill)
    z, one, half = cp.row(0.0), cp.row(1.0), cp.row(0.5)
    pl.add("size_1", 1, 5, 0.5, {0: (one, 1.0)})
    pl.add("size_1", 1, 5, 0.5, {0: (one, NAN)})
    pl.add("size_2", 2, 5, 0.5, {0: (one, 1.0), 1: (half, 2.0)})
    pl.add("size_2_nan", 2, 5, 0.5, {0: (one, np.inf), 1: (half, NAN)})
    full = {c: (int(fill[c % len(fill)]), 4000.0 - 3.0 * c) for c in range(P)}
    pl.add("k_0", P, 0, 0.5, full)
    pl.add("k_1", P, 1, 0.5, full)
    pl.add("k_P", P, P, 0.5, full)
    pl.add("k_P_plus_7", P, P + 7, 0.5, full)
    bad = {c: (z, (NAN, np.inf, -np.inf)[c % 3]) for c in range(1, P)}
    bad[0] = (one, 1.0)
    pl.add("all_non_finite", P, 5, 0.5, bad)
    pl.add("run_out", P, 10, 0.5, {0: (one, -np.inf), 7: (half, 1.0), P - 1: (one, 2.0), 3: (z, np.inf), 5: (z, -np.inf)})
    pl.add("run_out_sooner", P, 10, 0.5, {0: (one, 1.0), 7: (half, 1.0), 3: (z, np.inf), P - 1: (z, NAN)})
    # (1 - lambda) * rel = 2 * FLT_MAX: a finite relevance that is never selectable
    pl.add("t0_overflow", P, 5, -1.0, {0: (one, 1.0), 3: (z, FLT_MAX), 5: (z, 1.0), P - 1: (z, -FLT_MAX)})
    pl.add("t0_overflow_only", P, 5, -1.0, {0: (one, 1.0), 3: (z, FLT_MAX), P - 1: (z, -FLT_MAX)})
    return pl


def ragged_sizes(P):
    return [s for s in dict.fromkeys((P, P - 1, 65, 64, 1, 0, 33)) if s <= P]


def _ragged(cp, P, fill):
    """one batch call (k = 6, lambda = 0.5): every size three times.  In every form position 0 -- the pool's LAST candidate
    after pick 1 -- decides a tie: a kernel that takes the stride for the size finds a NaN slot there."""
    pl = Plan("ragged", P, fill)
    z, one = cp.row(0.0), cp.row(1.0)
    w, l = cp.row(0.5, 1, 0.5), cp.row(0.25, 1, 0.5)
    for form in range(3):
        for size in ragged_sizes(P)[form:] + ragged_sizes(P)[:form]:
            if size == 0:
                pl.add("size_0", 0, 6, 0.5, {})
            elif form == 0 or size < 4:                          # every candidate ties at every pick
                pl.add("all_tie", size, 6, 0.5, {c: (z, 1.0) for c in range(size)})
            elif form == 1:                                      # the last candidate ties with slot 1 and wins
                slots = {0: (one, 1.0), size - 1: (w, 2.0), 1: (l, _same_mmr(cp, [one], w, 2.0, l)), 2: (z, -1.0)}
                pl.add("last_ties", size, 6, 0.5, slots, aim=(1, size - 1))
            else:                                                # pairs of equal relevance from the end of the pool down
                slots = {c: (z, float(1000 - (size - 1 - c) // 2)) for c in range(1, size)}
                slots[0] = (z, NAN)
                pl.add("pairs", size, 6, 0.5, slots)
    return pl


_BUILDERS = dict(slot_sweep=_slot_sweep, tie_sweep=_tie_sweep, tie_forms=_tie_forms, zeros=_zeros, maxsim=_maxsim,
                 overflow=_overflow, ends=_ends, ragged=_ragged)


@functools.lru_cache(maxsize=None)
def _build():
    cp = Corpus()
    fill = [cp.row(2.0 ** -i, 8 + i, 2.0 ** -(i % 3)) for i in range(8)]
    plans = {}
    for P in STRIDES + (SINGLE,):
        for name in (BATCH_PLANS if P <= 1024 else SINGLE_PLANS):
            plans[name, P] = _BUILDERS[name](cp, P, fill).freeze()
    rows = cp.rows()
    rows.setflags(write=False)
    return cp, rows, plans


def corpus():
    """the rows every plan indexes (f32 [n, DIM], read-only): upload them as they are"""
    return _build()[1]


def corpus_spec():
    return _build()[0]


def plan(name, P):
    return _build()[2][name, P]


def plans(P=None):
    return [p for (_, s), p in _build()[2].items() if P is None or s == P]


@functools.lru_cache(maxsize=None)
def _gram_cached():
    from oracle import oracle as O
    g = R.gram(O, corpus())
    g.setflags(write=False)
    return g


def corpus_gram():
    """mmr_restatement.gram(oracle, corpus()), computed once per process and read-only"""
    return _gram_cached()


# ---------------------------------------------------------------- the traced restatement
Pick = collections.namedtuple("Pick", "holders pos idx moved lowest_idx holder_idx zero zero_signs nonfinite plus_inf minus_inf "
                                      "n_rem lane_mates nan_neighbours replayed")
End = collections.namedtuple("End", "n_rem finite_rel plus_inf minus_inf")


class PoolGram:
    """a pool's Gram matrix as a view of the corpus' (g[rows][:, rows], indexed per read and never copied): what
    mmr_from_gram and traced read is g[last pick, candidates]"""

    def __init__(self, g, rows):
        self.g, self.rows = g, np.asarray(rows, np.int64)

    def __getitem__(self, key):
        i, c = key
        return self.g[self.rows[i], self.rows[c]]


def traced(g, rel, k, lam, rows=None):
    """mmr_from_gram with a record per pick -> (order u32 [n], logged f32 [n], picks [n - 1], broke).
    rows != None: g is the corpus' matrix and the pool's is g[rows][:, rows] (indexed, never copied).
    Pick: holders of the maximum; the winner's position in `remaining` and its candidate index; moved = they differ;
    lowest_idx = the smallest index among the holders, holder_idx = the first eight of them in visiting order;
    zero = +1 / -1 / 0: the sign of a logged zero; zero_signs = the signs among the holders of a zero maximum; nonfinite / plus_inf / minus_inf = candidates of finite relevance whose MMR value is
    not finite / +inf / -inf; n_rem = entries of `remaining`; lane_mates = other selectable candidates in the winner's lane
    (index % 64); nan_neighbours = neither index - 64 nor index + 64 is selectable; replayed = for a tie, the number of picks
    made at the tie before (what the kernel's incremental replay starts from), -1 for a single holder.
    broke = None, or where the loop ended at `best == NEG_INFINITY`: End(entries of `remaining`, how many of them have a finite
    relevance, how many of those an MMR value of +inf / -inf)."""
    rel = np.ascontiguousarray(rel, dtype=np.float32)
    P = rel.size
    if P == 0:
        return np.zeros(0, np.uint32), np.zeros(0, np.float32), [], None
    if rows is not None:
        g = PoolGram(g, rows)
    lam = np.float32(lam)
    one_minus = np.float32(1.0) - lam
    rem = np.arange(P)
    order, logged, picks = [0], [np.float32(np.nan)], []
    n_rem = P - 1
    rem[0] = rem[n_rem]
    max_sim = np.zeros(P, dtype=np.float32)
    rel_finite = np.isfinite(rel)
    broke, replayed = None, 0
    with np.errstate(all="ignore"):
        while len(order) < k and n_rem > 0:
            c = rem[:n_rem].copy()
            sim = g[order[-1], c]
            max_sim[c] = np.where(np.isfinite(sim), np.maximum(max_sim[c], sim), max_sim[c])
            m = one_minus * rel[c] - lam * max_sim[c]
            ok = rel_finite[c] & np.isfinite(m)
            if not ok.any():
                fr = rel_finite[c]
                broke = End(n_rem, int(fr.sum()), int((fr & (m == np.inf)).sum()), int((fr & (m == -np.inf)).sum()))
                break
            masked = np.where(ok, m, -np.inf)
            at = int(np.argmax(masked))
            hold = np.flatnonzero(masked == masked[at])
            win = int(c[at])
            sel = set(c[ok].tolist())
            zero = 0 if m[at] != 0 else (-1 if np.signbit(m[at]) else 1)
            picks.append(Pick(
                holders=hold.size, pos=at, idx=win, moved=at != win, lowest_idx=int(c[hold].min()),
                holder_idx=tuple(c[hold[:8]].tolist()), zero=zero,
                zero_signs=frozenset((-1 if s else 1) for s in np.signbit(m[hold]).tolist()) if zero else frozenset(),
                nonfinite=int((rel_finite[c] & ~np.isfinite(m)).sum()), plus_inf=int((rel_finite[c] & (m == np.inf)).sum()),
                minus_inf=int((rel_finite[c] & (m == -np.inf)).sum()), n_rem=n_rem,
                lane_mates=sum(1 for o in sel if o % 64 == win % 64) - 1,
                nan_neighbours=(win - 64) not in sel and (win + 64) not in sel,
                replayed=replayed if hold.size > 1 else -1))
            if hold.size > 1:
                replayed = len(order)
            order.append(win)
            logged.append(m[at])
            n_rem -= 1
            rem[at] = rem[n_rem]
    return np.array(order, dtype=np.uint32), np.array(logged, dtype=np.float32), picks, broke


DEFECTS = ("tie_lowest_index", "tie_stale_positions", "zero_logged_plus", "zeros_ordered_by_bits", "max_sim_from_minus_inf",
           "max_sim_takes_non_finite", "infinite_selectable", "continues_past_no_finite", "odd_j_last_slot_dropped",
           "slot_0_needs_finite_score", "sizes_ignored")


def with_defect(defect, g, rows, rel, size, k, lam, stride):
    """a copy of the restatement with one planted defect (None: none) over a pool of `stride` slots of which `size` are
    valid -> (order, logged); test_greedy_vectors_cpu.py lists which plan has to notice which"""
    assert defect is None or defect in DEFECTS
    P = stride if defect == "sizes_ignored" else size
    rows = np.asarray(rows, np.int64)[:P]
    rel = np.ascontiguousarray(rel, dtype=np.float32)[:P]
    if P == 0 or (defect == "slot_0_needs_finite_score" and not np.isfinite(rel[0])):
        return np.zeros(0, np.uint32), np.zeros(0, np.float32)
    J = greedy_j(stride)
    lam = np.float32(lam)
    one_minus = np.float32(1.0) - lam
    rem = np.arange(P)
    order, logged = [0], [np.float32(np.nan)]
    n_rem = P - 1
    rem[0] = rem[n_rem]
    stale = np.arange(P)                                         # candidate -> position as of the tie before (none: never replayed)
    max_sim = np.full(P, -np.inf if defect == "max_sim_from_minus_inf" else 0.0, dtype=np.float32)
    rel_finite = np.isfinite(rel)
    with np.errstate(all="ignore"):
        while len(order) < k and n_rem > 0:
            c = rem[:n_rem].copy()
            sim = g[rows[order[-1]], rows[c]]
            if defect == "max_sim_takes_non_finite":
                max_sim[c] = np.fmax(max_sim[c], sim)
            else:
                max_sim[c] = np.where(np.isfinite(sim), np.maximum(max_sim[c], sim), max_sim[c])
            m = one_minus * rel[c] - lam * max_sim[c]
            ok = rel_finite[c] & np.isfinite(m)
            if defect == "infinite_selectable":
                ok = rel_finite[c] & ~np.isnan(m) & (m != -np.inf)
            if defect == "odd_j_last_slot_dropped" and J % 2:
                ok &= c // 64 != J - 1
            if not ok.any():
                if defect != "continues_past_no_finite":
                    break
                at = 0
            else:
                masked = np.where(ok, m, -np.inf)
                at = int(np.argmax(masked))
                hold = np.flatnonzero(masked == masked[at])
                if defect == "zeros_ordered_by_bits" and masked[at] == 0:
                    plus = hold[~np.signbit(m[hold])]
                    hold = plus if plus.size else hold
                    at = int(hold[0])
                if hold.size > 1 and defect == "tie_lowest_index":
                    at = int(hold[np.argmin(c[hold])])
                if hold.size > 1 and defect == "tie_stale_positions":
                    at = int(hold[np.argmin(stale[c[hold]])])
                    stale = np.full(P, P, np.int64)
                    stale[c] = np.arange(n_rem)
            order.append(int(c[at]))
            logged.append(np.float32(0.0) if defect == "zero_logged_plus" and m[at] == 0 else m[at])
            n_rem -= 1
            rem[at] = rem[n_rem]
    return np.array(order, dtype=np.uint32), np.array(logged, dtype=np.float32)


# ---------------------------------------------------------------- expectations and the summary
def trace_plan(pl, g):
    """[(order, logged, picks, broke)] per pool of the plan, g the corpus' Gram matrix"""
    out = []
    for q in range(pl.Q):
        s = int(pl.sizes[q])
        out.append(traced(g, pl.rel[q, :s], int(pl.k[q]), pl.lam[q], pl.pool_rows[q, :s]))
    return out


def width(pl):
    """columns that hold every pool's picks"""
    return max(1, int(np.minimum(np.maximum(pl.k, 1), np.maximum(pl.sizes, 1)).max()))


def expected(pl, g, traces=None):
    """(order u32 [Q, width], logged f32 [Q, width], n u32 [Q]); order / logged are valid up to n"""
    traces = trace_plan(pl, g) if traces is None else traces
    W = width(pl)
    order = np.zeros((pl.Q, W), np.uint32)
    logged = np.full((pl.Q, W), np.nan, np.float32)
    n = np.zeros(pl.Q, np.uint32)
    for q, (o, m, _, _) in enumerate(traces):
        order[q, : o.size], logged[q, : m.size], n[q] = o, m, o.size
    return order, logged, n


def states(pl, g, traces=None):
    """what the plan's pools reach: pools = state -> count; fast / tie = the (lane, j) = (index % 64, index // 64) of every
    winner with one holder / of every winner of a tie (J = greedy_j(P); for mmr_greedy_kernel the same split of the index);
    aimed_fast / aimed_tie = the same over the aimed picks only; traces = trace_plan's"""
    traces = trace_plan(pl, g) if traces is None else traces
    out = dict(J=greedy_j(pl.P), pools=collections.Counter(pl.state), fast=set(), tie=set(), aimed_fast=set(), aimed_tie=set(),
               traces=traces)
    for q, (_, _, picks, _) in enumerate(traces):
        for i, p in enumerate(picks):
            where = (p.idx % 64, p.idx // 64)
            out["tie" if p.holders > 1 else "fast"].add(where)
            if pl.aim[q] is not None and pl.aim[q][0] == i + 1 and pl.aim[q][1] in (None, p.idx):
                out["aimed_tie" if p.holders > 1 else "aimed_fast"].add(where)
    return out


def describe(pl, q, picks):
    """the state pool q was built for, with the winner's (lane, j) at the aimed pick"""
    aim = pl.aim[q]
    if aim is None or aim[0] - 1 >= len(picks):
        return f"{pl.name}[{q}] {pl.state[q]} (size {pl.sizes[q]}, k {pl.k[q]}, lambda {float(pl.lam[q])!r})"
    p = picks[aim[0] - 1]
    return (f"{pl.name}[{q}] {pl.state[q]} (size {pl.sizes[q]}, k {pl.k[q]}, lambda {float(pl.lam[q])!r}): pick {aim[0] + 1} is slot "
            f"{p.idx} = (lane {p.idx % 64}, j {p.idx // 64}) at position {p.pos}, {p.holders} holder(s)")
