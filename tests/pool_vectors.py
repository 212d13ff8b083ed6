"""Rows and lexical pairs that put the fused pool and blend stage into each of its states on purpose: hybrid_pool_body
(csrc/index_fused.hip; hybrid_pool_kernel and hybrid_pool_batch_kernel) and pool_prepare_body<FROM_CANDIDATES, COHERENT>
(csrc/pool_prepare.h; pool_prepare_kernel<true>, pool_prepare_kernel<false> and the fused tail's finish).
test_pool_vectors_cpu.py proves that the cases reach those states, test_gpu_pool.py runs them.

Rows.  The query is e_0 and row r is cos[r] * e_0 plus, in the corpora that diversified cases use, one signed power of two
in a column >= 1.  The cosine of row r is then cos[r] exactly, in any summation order and in every scoring kernel: a
difference a case shows is the blend's, never the scan's.  A Gram entry is cos_i cos_j + [same column] b_i b_j: with one
non-zero term it is ONE rounded product whatever the order of the additions, with two terms the products and the sum are
exact for the rows a diversified pool can hold (the CPU test proves both, for f32 and for the rows rounded to binary16).

The restatement (`expected`) is the host's arithmetic written out step by step over EVERY row of the corpus
(include/rlr_gpu.h and csrc/engine_host.h quote the reference lines: rag_engine.rs:515-519, :524-544):
    l = f32(lex / max_lex) for a lexical row, else 0;  combined = f32(f32(w_e * cos) + f32(w_l * l))
    order (combined desc, NaN last, row asc) with -0 == +0, cut to `need`
and the status the fused kernels must report for the `fetch` best rows by (cos desc, row asc):
    c_tail = combine(smallest fetched cos, 0)
    0 iff the fetch covers the index, or n_cand >= need and (c_tail is NaN or combined[need - 1] > c_tail); else 2
    1 when more rows tie with the fetch-th cosine than the candidate list holds (4096; 1024 for pool_prepare_kernel<true>),
      or when the sizes are outside the blend's slots (nothing runs then)
`expected(case, mode, defect)` is the same with one planted defect; the CPU test lists which plan has to notice which.

numpy only; the oracle is passed in where a function needs it."""
import collections
import functools

import numpy as np

import mmr_restatement as R

DIM = 16
F32 = np.float32
EPS = F32(1.1920929e-07)                                       # f32::EPSILON: the floor of max_lex
HASH_SLOTS = 4096                                               # kHybridHash
SLOTS = 4096                                                    # kHybridSlots
POOL_MAX = 1024                                                 # kPoolMax
SORT_CAP = 4096                                                 # kLdsSortCap
FROM_CANDIDATES_MAX = 512                                       # rlr_search_diverse: fetch <= 512 orders the candidate list itself
FETCH_MARGIN = 32                                               # kHybridFetchMargin
KTH_SLACK = 32
CHAIN_W = 0.7 * 2.0 ** -140                                     # 358 * 2^-149 in f32: times 1 - j 2^-24 it rounds to itself
CHAIN_W16 = 2.0 ** -148                                         # times 1 - j 2^-11 (j < 64): 2 * 2^-149; times 0.375: 2^-149
HYBRID_PLANS = ("hash", "reach", "arith", "zeros", "classes", "boundary", "sizes", "overflow", "emit")
DIVERSE_PLANS = ("zeros", "boundary", "chains", "ends", "overflow")
STATUS_0_PLANS = ("hash", "reach", "arith", "zeros", "classes", "sizes")   # no case of these may be excused by a fallback
HYBRID_MODES = ("default", "full")                              # RLR_HYBRID_FETCH unset / =full
DIVERSE_MODES = ("tail0", "tail1")                              # RLR_TAIL=0 / =1 (a fetch above 512 takes sort_emit in both)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def bucket(rows):
    """the home slot of a row in the blend's open-addressing table: (row * 2654435761u) >> 20"""
    return ((np.asarray(rows, np.uint64) * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)) >> np.uint64(20)


def f16_grid_desc(count, first=0x3C00):
    """the `count` largest binary16 values from `first` (1.0) down, as f32"""
    return np.arange(first, first - count, -1, dtype=np.int64).astype(np.uint16).view(np.float16).astype(np.float32)


# ---------------------------------------------------------------- corpora
class Corpus:
    """cos f32 [n]; col / val: the extra element of a row (col 0: none); head = the rows by (cos desc, row asc)"""

    def __init__(self, name, cos, col=None, val=None, f16=True):
        self.name, self.f16 = name, f16
        self.cos = np.ascontiguousarray(cos, dtype=np.float32)
        self.n = self.cos.size
        self.col = np.zeros(self.n, np.int64) if col is None else np.asarray(col, np.int64)
        self.val = np.zeros(self.n, np.float32) if val is None else np.asarray(val, np.float32)
        self.head = np.lexsort((np.arange(self.n), -self.cos.astype(np.float64)))
        for a in (self.cos, self.col, self.val, self.head):
            a.setflags(write=False)

    def rows(self):
        out = np.zeros((self.n, DIM), np.float32)
        out[:, 0] = self.cos
        extra = np.flatnonzero(self.col)
        out[extra, self.col[extra]] = self.val[extra]
        return out

    def gram(self, rows):
        """f32 Gram matrix of `rows`: the products in binary64 (exact), their sum, one rounding"""
        rows = np.asarray(rows, np.int64)
        a = self.cos[rows].astype(np.float64)
        g = np.outer(a, a)
        same = (self.col[rows][:, None] == self.col[rows][None, :]) & (self.col[rows][:, None] != 0)
        b = self.val[rows].astype(np.float64)
        return (g + np.where(same, np.outer(b, b), 0.0)).astype(np.float32)


N_BIG = 65536
ONE_BUCKET = 2003                                               # a bucket of 16 rows (buckets hold 14..18)


def _filler(n):
    """-(0.25 + (r % 1024) / 2048): far below every head row, exact in binary16"""
    return -(F32(0.25) + (np.arange(n) % 1024).astype(np.float32) / F32(2048.0))


def _head_corpus(name, n, head_rows, head_cos, extras=False, f16=True):
    cos = _filler(n)
    cos[head_rows] = head_cos
    col = val = None
    if extras:
        r = np.arange(n)
        col, val = 1 + r % (DIM - 1), np.where((r // (DIM - 1)) % 2 == 0, 0.5, -0.5).astype(np.float32)
    return Corpus(name, cos, col, val, f16)


def _spread(n, count, taken=()):
    """`count` distinct rows of [0, n) in a fixed scattered order, none of `taken`"""
    taken, out, j = set(int(t) for t in taken), [], 0
    while len(out) < count:
        r = (j * 40503 + 12345) % n
        j += 1
        if r not in taken:
            taken.add(r)
            out.append(r)
    return np.array(out, np.int64)


@functools.lru_cache(maxsize=None)
def big_special():
    """rows of the big corpus the hash plan is about: wrap = every row of buckets 4088..4095, low = three rows each of
    buckets 0..127 (they walk a wrapped chain), one = the 16 rows of bucket 2003, after = two rows each of the
    16 buckets behind it"""
    b = bucket(np.arange(N_BIG)).astype(np.int64)
    wrap = np.flatnonzero(b >= 4088)
    low = np.concatenate([np.flatnonzero(b == x)[:3] for x in range(128)])
    one = np.flatnonzero(b == ONE_BUCKET)
    after = np.concatenate([np.flatnonzero(b == x)[:2] for x in range(ONE_BUCKET + 1, ONE_BUCKET + 17)])
    return dict(wrap=wrap, low=low, one=one, after=after)


@functools.lru_cache(maxsize=None)
def corpus(name):
    if name == "big":
        # head: 8 scattered rows, then the special rows in a fixed shuffle, then scattered rows; cosines down the binary16
        # grid from 1.0 (4608 values reach 2^-4.5: at most 32 rows within 2^-10 of any of them)
        sp = big_special()
        special = np.concatenate([sp["wrap"], sp["low"], sp["one"], sp["after"]])
        special = special[np.random.default_rng(7).permutation(special.size)]
        rest = _spread(N_BIG, 4608 - special.size, special)
        head = np.concatenate([rest[:8], special, rest[8:]])
        return _head_corpus("big", N_BIG, head, f16_grid_desc(head.size), extras=True)
    if name in ("n9", "n17"):
        n = int(name[1:])
        return _head_corpus(name, n, (np.arange(n) * 5) % n, f16_grid_desc(n), extras=True)
    if name == "arith":
        # 512 arbitrary f32 cosines in [0.5, 1): the products with an arbitrary weight have 48 significant bits
        rng = np.random.default_rng(11)
        n = 2048
        head = _spread(n, 512)
        vals = np.sort(np.unique((0.5 + rng.random(1024) / 2).astype(np.float32)))[::-1][:512]
        return _head_corpus("arith", n, head, vals, f16=False)
    if name == "arith16":
        n = 2048
        return _head_corpus("arith16", n, _spread(n, 512), f16_grid_desc(512))
    if name in ("zeros4", "zeros600"):
        # `top` rows above, then 12 rows of cosine +-2^-12 interleaved by row (even +, odd -), then filler
        top, n = int(name[5:]), 4096
        cls = 100 + np.arange(12)
        head = _spread(n, top, cls)
        cos = _filler(n)
        cos[head] = f16_grid_desc(top)
        cos[cls] = np.where(cls % 2 == 0, 2.0 ** -12, -(2.0 ** -12))
        return Corpus(name, cos)
    if name in ("chain0", "chain560"):
        # `above` rows in (1.4, 2], then 64 cosines 1 - j 2^-24 on scattered rows, then 0.75 - i 2^-12, then filler
        above, n = int(name[5:]), 4096
        head = _spread(n, above + 64 + 700)
        vals = np.concatenate([F32(2.0) - np.arange(above, dtype=np.float32) * F32(2.0 ** -10),
                               F32(1.0) - np.arange(64, dtype=np.float32) * F32(2.0 ** -24),
                               F32(0.75) - np.arange(700, dtype=np.float32) * F32(2.0 ** -12)])
        return _head_corpus(name, n, head, vals, f16=False)
    if name == "chain16":
        # the binary16 form: 64 neighbours of the grid below 1.0 (1 - j 2^-11), then 0.375 - i 2^-12
        n = 4096
        head = _spread(n, 64 + 700)
        vals = np.concatenate([f16_grid_desc(64, 0x3BFF), F32(0.375) - np.arange(700, dtype=np.float32) * F32(2.0 ** -12)])
        return _head_corpus(name, n, head, vals)
    if name in ("ulp", "ulp600"):
        # 20 (600) rows above, one row at v + ulp, 40 rows AT v (a class of equal cosines that the fetch cuts), then
        # 0.5 - i 2^-12; the 600 rows above lie in (1.4, 2] so that need + 8 exceeds 512 fetched rows
        n = 4096
        above = 20 if name == "ulp" else 600
        head = _spread(n, above + 1 + 40 + 600)
        v = F32(0.75)
        top = (F32(1.0) - np.arange(20, dtype=np.float32) * F32(2.0 ** -8) if name == "ulp" else
               F32(2.0) - np.arange(600, dtype=np.float32) * F32(2.0 ** -10))
        vals = np.concatenate([top, [np.nextafter(v, F32(1.0))],
                               np.full(40, v, np.float32), F32(0.5) - np.arange(600, dtype=np.float32) * F32(2.0 ** -12)])
        return _head_corpus(name, n, head, vals, f16=False)
    if name == "ties5000":
        n = 8192
        return _head_corpus(name, n, _spread(n, 5000), np.ones(5000, np.float32))
    if name in ("band104", "band604"):
        # `above` distinct rows, then 1500 rows of one cosine: the class holds the fetch-th row of need = above - 4
        above, n = int(name[4:]), 8192
        head = _spread(n, above + 1500)
        return _head_corpus(name, n, head, np.concatenate([f16_grid_desc(above), np.full(1500, 0.125, np.float32)]))
    if name in ("text", "text_e1"):
        # the batched blend's corpus: 700 head rows seen from e_0; 100 of the other rows carry 1.0 in element 1, so that from
        # e_1 ("text_e1": the same rows, cos = element 1) a hundred rows tie for the best cosine
        n = TEXT_N
        head = _spread(n, 700)
        tied = np.setdiff1d(np.arange(n), head)[40:3000:29][:100]
        if name == "text_e1":
            cos = np.zeros(n, np.float32)
            cos[tied] = 1.0
            return Corpus(name, cos)
        cos = _filler(n)
        cos[head] = f16_grid_desc(700)
        col, val = np.zeros(n, np.int64), np.zeros(n, np.float32)
        col[tied], val[tied] = 1, 1.0
        return Corpus(name, cos, col, val)
    raise KeyError(name)


# ---------------------------------------------------------------- the batched blend (rlr_engine_search_text_batch)
TEXT_N = 4096
TEXT_TOP_K = 10                                                 # stage 1: need = initial_k = 30, BM25 limit = 5 * top_k = 50
TEXT_GHOSTS = tuple(range(TEXT_N + 1, TEXT_N + 6))               # chunks of a lexical index that ran ahead of the embeddings


def text_rows():
    """the one-token text of every row: `many` in 200 rows (21 of them among the 62 best cosines), `solo` in one row far
    from the fetch, `pad` everywhere else"""
    cp = corpus("text")
    texts = ["pad"] * TEXT_N
    for r in cp.head[0:600:3]:
        texts[int(r)] = "many"
    texts[int(cp.head[300 + 1])] = "solo"
    return texts


# (state, query text, query axis): side by side in one batch
TEXT_QUERIES = (("unknown_token", "nothing", 0), ("one_row", "solo", 0), ("more_rows_than_the_limit", "many", 0),
                ("all_rows_outside_the_index", "ghost", 0), ("boundary_rule_fails", "solo", 1), ("one_row", "solo", 0))


def text_oracle():
    """oracle/lexical.py's index over the texts and the chunks without an embedding"""
    from oracle import lexical as OL
    o = OL.LexicalIndex()
    for r, t in enumerate(text_rows()):
        o.add_chunk(r, t, rank=r)
    for g in TEXT_GHOSTS:
        o.add_chunk(g, "ghost", rank=g)
    return o


def text_pairs(o, text):
    return [(c, float(s)) for c, s in o.score(text, 5 * TEXT_TOP_K, keep_zero=False)]


def text_case(state, axis, pairs):
    """the case of one query of the batch: `pairs` = the BM25 pairs of its text; rows outside the index never become
    candidates (they would still count for max_lex: no query of this batch mixes the two)"""
    inside = [(r, s) for r, s in pairs if r < TEXT_N]
    assert not inside or len(inside) == len(pairs)
    return Case("hybrid", "text_batch", state, "text" if axis == 0 else "text_e1", 3 * TEXT_TOP_K, lex=inside)


# ---------------------------------------------------------------- cases
class Case:
    def __init__(self, entry, plan, state, corpus, need, w_e=0.7, w_l=0.3, lex=(), k=0, diversify=0, lam=0.5,
                 dtypes=("f32",), expect=None, note=""):
        self.entry, self.plan, self.state, self.corpus, self.need = entry, plan, state, corpus, int(need)
        self.w_e, self.w_l = F32(w_e), F32(w_l)
        pairs = sorted((int(r), s) for r, s in lex)
        self.lex_rows = np.array([r for r, _ in pairs], np.uint64)
        self.lex_scores = np.array([s for _, s in pairs], np.float32)
        assert np.unique(self.lex_rows).size == self.lex_rows.size
        self.k, self.diversify, self.lam = int(k), int(bool(diversify) or entry == "diverse"), F32(lam)
        self.dtypes, self.expect, self.note = tuple(dtypes), expect, note

    @property
    def n_lex(self):
        return self.lex_rows.size

    @property
    def max_lex(self):
        """fold(0.0, f32::max) over the scores (NaN ignored), then .max(f32::EPSILON)"""
        m = F32(0.0)
        for s in self.lex_scores:
            if s > m:
                m = s
        return m if m >= EPS else EPS

    @property
    def modes(self):
        return HYBRID_MODES if self.entry == "hybrid" else DIVERSE_MODES

    def describe(self):
        return (f"{self.entry}/{self.plan} {self.state} (corpus {self.corpus}, need {self.need}, n_lex {self.n_lex}, w_e "
                f"{float(self.w_e)!r}, w_l {float(self.w_l)!r}, k {self.k}, diversify {self.diversify}{', ' + self.note if self.note else ''})")


def fetch_of(case, mode, n):
    """(fetch, status of the size gate): rlr_search_diverse / hybrid_begin_impl"""
    need = min(case.need, n)
    if case.entry == "diverse":
        return min(n, need + 8), int(need > POOL_MAX)
    full = min(n, need + case.n_lex + 8)
    gate = int(need > POOL_MAX or case.n_lex > 2048 or full + case.n_lex > SLOTS)
    if mode == "batch":                                          # search_hybrid_batch: need + 32 whatever the pairs
        return min(n, need + FETCH_MARGIN), int(need > POOL_MAX)
    return (full if mode == "full" else min(full, need + FETCH_MARGIN)), gate


def candidate_cap(case, fetch):
    return 1024 if case.entry == "diverse" and fetch <= FROM_CANDIDATES_MAX else SORT_CAP


Expected = collections.namedtuple("Expected", "status n rows cos comb lex info")


def _order(comb, rows, defect=None):
    """(combined desc, NaN last, row asc), -0 == +0"""
    nan = np.isnan(comb)
    key = np.where(nan, 0.0, comb.astype(np.float64)) + 0.0
    if defect == "neg_zero_below":
        key = np.where((comb == 0) & np.signbit(comb), -1e-300, key)
    tie = -rows.astype(np.int64) if defect == "ties_desc" else rows.astype(np.int64)
    return np.lexsort((tie, -key, ~nan if defect == "nan_first" else nan))


def _table(lex_rows):
    """the open-addressing table after every lexical row was inserted one by one in list order -> slot of each row
    (WHICH rows share a cluster does not depend on the order of insertion, only who sits where inside it)"""
    used, slot = np.zeros(HASH_SLOTS, bool), np.zeros(len(lex_rows), np.int64)
    for j, h in enumerate(bucket(lex_rows).astype(np.int64)):
        while used[h]:
            h = (h + 1) % HASH_SLOTS
        used[h], slot[j] = True, h
    return used, slot


def expected(case, mode, defect=None):
    """the restatement (defect None) or a copy with one planted defect -> Expected; rows / cos / comb / lex in the order
    the call reports them (pool order, or pick order under MMR)"""
    cp = corpus(case.corpus)
    cos, n = cp.cos, cp.n
    none = lambda status, info=None: Expected(status, 0, None, None, None, None, info or {})
    need = min(case.need, n)
    fetch, gate = fetch_of(case, mode, n)
    if gate:
        return none(1, dict(gate=True))
    rows = np.arange(n, dtype=np.int64)
    with np.errstate(all="ignore"):
        max_lex = case.max_lex
        l = np.zeros(n, np.float32)
        lr = case.lex_rows.astype(np.int64)
        if defect == "recip_division":
            l[lr] = case.lex_scores * (F32(1.0) / max_lex)
        else:
            l[lr] = case.lex_scores / max_lex
        is_lex = np.zeros(n, bool)
        is_lex[lr] = True

        def combine(c, ll):
            t1 = case.w_l * ll
            if defect == "fma":
                return (case.w_e.astype(np.float64) * np.asarray(c, np.float64) + np.asarray(t1, np.float64)).astype(np.float32)
            return (case.w_e * c + t1).astype(np.float32) if isinstance(c, np.ndarray) else F32(F32(case.w_e * c) + t1)

        comb = combine(cos, l)
        fetched = cp.head[:fetch]
        cos_tail = cos[fetched[-1]]
        # exact ties with the fetch-th cosine are inside any band: more of them than the candidate list holds is status 1
        n_band = int((cos >= cos_tail).sum())
        info = dict(fetch=fetch, n_band_min=n_band, near=int(((cos < cos_tail) & (cos >= cos_tail - F32(2.0 ** -10))).sum()),
                    tied_beyond=n_band - fetch)
        if n_band > candidate_cap(case, fetch):
            return none(1, info)
        in_fetch = np.zeros(n, bool)
        in_fetch[fetched] = True
        cand_rows, cand_comb, cand_cos, cand_l = rows, comb, cos, l
        if defect == "drop_unfetched":
            keep = in_fetch | ~is_lex
            cand_rows, cand_comb, cand_cos, cand_l = rows[keep], comb[keep], cos[keep], l[keep]
        if defect in ("flag_ignored", "probe_no_wrap"):
            dup = lr[in_fetch[lr]]
            if defect == "probe_no_wrap":                        # a fetched row whose pair sits in a wrapped slot is not found
                _, slot = _table(case.lex_rows)
                lost = slot < bucket(case.lex_rows).astype(np.int64)
                dup = lr[in_fetch[lr] & lost]
                l0 = l.copy()
                l0[dup] = 0.0
                cand_comb, cand_l = combine(cos, l0), l0
            cand_rows = np.concatenate([rows, dup])
            cand_comb = np.concatenate([cand_comb, comb[dup]])
            cand_cos = np.concatenate([cos, cos[dup]])
            cand_l = np.concatenate([cand_l, l[dup]])
        order = _order(cand_comb, cand_rows, defect)
        cut = need + 1 if defect == "cut_need_plus_1" else need
        pool = order[: min(cut, order.size)]
        n_cand = fetch + int((~in_fetch[lr]).sum())
        c_tail = combine(cos[fetched[0]] if defect == "tail_from_largest" else cos_tail, F32(0.0))
        c_need = cand_comb[order[need - 1]]
        info.update(n_cand=n_cand, c_tail=c_tail, c_need=c_need, covers=fetch >= n)
        if fetch < n:
            beats = c_need >= c_tail if defect == "boundary_ge" else c_need > c_tail
            if not (n_cand >= need and (np.isnan(c_tail) or beats)):
                return none(2, info)
    p_rows, p_cos, p_comb, p_l = cand_rows[pool], cand_cos[pool], cand_comb[pool], cand_l[pool]
    if case.diversify:
        picks, _ = R.mmr_from_gram(cp.gram(p_rows), p_comb, case.k, case.lam)
        picks = picks.astype(np.int64)
        info["picks"] = picks
        p_l_out = p_l[: picks.size] if defect == "lex_pool_order" else p_l[picks]
        p_rows, p_cos, p_comb, p_l = p_rows[picks], p_cos[picks], p_comb[picks], p_l_out
    return Expected(0, p_rows.size, p_rows.astype(np.uint64), p_cos, p_comb, p_l, info)


DEFECTS = ("fma", "recip_division", "neg_zero_below", "boundary_ge", "tail_from_largest", "flag_ignored", "probe_no_wrap",
           "drop_unfetched", "ties_desc", "nan_first", "cut_need_plus_1", "lex_pool_order")


def same(a, b):
    """two Expected agree in everything a call reports"""
    if a.status != b.status or a.n != b.n:
        return False
    if a.status:
        return True
    return (np.array_equal(a.rows, b.rows) and np.array_equal(bits(a.cos), bits(b.cos)) and
            np.array_equal(bits(a.comb), bits(b.comb)) and np.array_equal(bits(a.lex), bits(b.lex)))


# ---------------------------------------------------------------- the blend's own states
def hash_state(case, mode):
    """what the open-addressing table of the case looks like: the longest run of occupied slots, whether a run passes
    slot 4095 into slot 0, fetched rows without a pair that must walk over occupied slots to an empty one (and the longest
    such walk), fetched rows with a pair, and of those the ones whose pair sits in a wrapped slot"""
    cp = corpus(case.corpus)
    fetch, _ = fetch_of(case, mode, cp.n)
    used, slot = _table(case.lex_rows)
    home = bucket(case.lex_rows).astype(np.int64)
    runs, run = [], 0
    for u in np.concatenate([used, used]):
        run = run + 1 if u else 0
        runs.append(run)
    fetched = cp.head[:fetch]
    is_lex = np.zeros(cp.n, bool)
    is_lex[case.lex_rows.astype(np.int64)] = True
    walks = []
    for r in fetched[~is_lex[fetched]]:
        h, w = int(bucket(r)), 0
        while used[h]:
            h, w = (h + 1) % HASH_SLOTS, w + 1
        walks.append(w)
    in_fetch = np.zeros(cp.n, bool)
    in_fetch[fetched] = True
    lf = in_fetch[case.lex_rows.astype(np.int64)]
    return dict(longest_run=min(max(runs, default=0), HASH_SLOTS), wraps=bool(used[HASH_SLOTS - 1] and used[0]),
                walkers=int(sum(w > 0 for w in walks)), longest_walk=max(walks, default=0), fetched_lex=int(lf.sum()),
                unfetched_lex=int((~lf).sum()), fetched_lex_wrapped=int((lf & (slot < home)).sum()),
                longest_probe=int(((slot - home) % HASH_SLOTS).max()) if slot.size else 0)


def score_key(c):
    """csrc/common.h: the order-preserving map f32 -> u32, NaN -> 0"""
    b = int(bits(c).ravel()[0])
    if (b & 0x7FFFFFFF) > 0x7F800000:
        return 0
    return (~b & 0xFFFFFFFF) if b & 0x80000000 else (b | 0x80000000)


def slot_key(c, row):
    """hybrid_pool_body's key of a candidate: -0 is keyed as +0"""
    return (score_key(F32(0.0) if c == 0 else c) << 32) | (0xFFFFFFFF - int(row))


def slot_keys(case, mode):
    """the 64-bit keys hybrid_pool_body holds in its fetch + n_lex slots ((ordered combined score, ~row); 0 = empty: a
    lexical pair the fetch reached) -> (keys u64 [fetch + n_lex], n_cand)"""
    cp = corpus(case.corpus)
    fetch, _ = fetch_of(case, mode, cp.n)
    with np.errstate(all="ignore"):
        l = np.zeros(cp.n, np.float32)
        l[case.lex_rows.astype(np.int64)] = case.lex_scores / case.max_lex
        comb = (case.w_e * cp.cos + case.w_l * l).astype(np.float32)
    fetched = cp.head[:fetch]
    in_fetch = np.zeros(cp.n, bool)
    in_fetch[fetched] = True
    keys = [slot_key(comb[r], r) for r in fetched]
    n_cand = fetch
    for r in case.lex_rows.astype(np.int64):
        if in_fetch[r]:
            keys.append(0)
        else:
            keys.append(slot_key(comb[r], r))
            n_cand += 1
    return keys, n_cand


def kth_trace(keys, k, slack=KTH_SLACK):
    """the digit walk of lds_kth_key64 (csrc/lds_select.h) restated over Python integers -> (key_lo, passes, how it
    ended: 'done' above the last digit / 'shift0' at it / 'no_open_bits', keys >= key_lo)"""
    all_and, all_or = (1 << 64) - 1, 0
    for v in keys:
        all_and &= v
        all_or |= v
    diff = all_and ^ all_or
    full = (1 << 64) - 1
    prefix, mask, rank, next_hi, passes, end = all_and & ~diff & full, ~diff & full, k, 64, 0, "no_open_bits"
    for _ in range(8):
        open_ = diff if next_hi >= 64 else diff & ((1 << next_hi) - 1)
        if open_ == 0:
            end = "no_open_bits"
            break
        top = open_.bit_length()
        nbits = min(top, 11)
        shift, nb = top - nbits, 1 << nbits
        hist = collections.Counter((v >> shift) & (nb - 1) for v in keys if (v & mask) == prefix)
        above, passes = 0, passes + 1
        for b in range(nb - 1, -1, -1):
            if above < rank <= above + hist[b]:
                break
            above += hist[b]
        prefix |= b << shift
        mask |= (nb - 1) << shift
        done = hist[b] - (rank - above) <= slack
        rank -= above
        next_hi = shift
        if done or shift == 0:
            end = "shift0" if shift == 0 else "done"
            break
    return prefix, passes, end, sum(1 for v in keys if v >= prefix and v != 0)


# ---------------------------------------------------------------- plans
def _lex_scores(count, seed, lo=0.5, hi=9.0):
    return (lo + (hi - lo) * np.random.default_rng(seed).random(count)).astype(np.float32)


def _hybrid_hash():
    H, big, sp, out = "hybrid", corpus("big"), big_special(), []
    both = ("f32", "f16")
    one, wrap = sp["one"], sp["wrap"]
    out.append(Case(H, "hash", "one_bucket", "big", 1024, lex=zip(one, _lex_scores(one.size, 1)), dtypes=both))
    out.append(Case(H, "hash", "wrap_all_fetched", "big", 1024, lex=zip(wrap, _lex_scores(wrap.size, 2)), dtypes=both))
    # need 40: the fetch (72 rows) holds only some of the special rows -- chains of fetched and unfetched pairs
    out.append(Case(H, "hash", "wrap_partly_fetched", "big", 40, lex=zip(wrap, _lex_scores(wrap.size, 3))))
    # the largest n_lex the gate admits: every lexical row far down the corpus, then with the wrapped chain among them
    tail = np.setdiff1d(np.arange(N_BIG), big.head[:4608])
    out.append(Case(H, "hash", "gate_max_need_1", "big", 1, lex=zip(tail[:2043], _lex_scores(2043, 4))))
    rows = np.concatenate([wrap, one, np.setdiff1d(tail, np.concatenate([wrap, one]))[: 1532 - wrap.size - one.size]])
    out.append(Case(H, "hash", "gate_max_need_1024", "big", 1024, lex=zip(rows, _lex_scores(1532, 5)), dtypes=both))
    out.append(Case(H, "hash", "gate_refused", "big", 1, lex=zip(tail[:2044], _lex_scores(2044, 6)), expect=dict(default=1, full=1)))
    out.append(Case(H, "hash", "gate_refused", "big", 1024, lex=zip(tail[:1533], _lex_scores(1533, 7)), expect=dict(default=1, full=1)))
    # a dense table: 2043 pairs, all fetched special rows walk
    rows = np.concatenate([wrap, sp["low"][::3], np.setdiff1d(tail, wrap)[: 2043 - wrap.size - sp["low"][::3].size]])
    out.append(Case(H, "hash", "dense_table", "big", 2, lex=zip(rows, _lex_scores(2043, 8))))
    return out


def _hybrid_reach():
    H, big, out = "hybrid", corpus("big"), []
    both = ("f32", "f16")
    need, fetch = 100, 132                                       # 25 pairs and more: the fetch is need + 32
    inside, outside = big.head[10:fetch:5], big.head[fetch + 5: fetch + 200: 9]
    out.append(Case(H, "reach", "all_inside", "big", need, lex=zip(inside, _lex_scores(inside.size, 11)), dtypes=both))
    out.append(Case(H, "reach", "none_inside", "big", need, lex=zip(outside, _lex_scores(outside.size, 12)), dtypes=both))
    half = np.concatenate([inside[:10], outside[:10]])
    out.append(Case(H, "reach", "half_inside", "big", need, lex=zip(half, _lex_scores(20, 13)), dtypes=both))
    out.append(Case(H, "reach", "n_lex_0", "big", need, dtypes=both))
    last = np.concatenate([[big.head[need + 6 + 8 - 1]], outside[:5]])   # six pairs: the fetch is need + 6 + 8 in both modes
    out.append(Case(H, "reach", "lex_is_last_fetched", "big", need, lex=zip(last, _lex_scores(6, 14)), dtypes=both))
    return out


def _hybrid_arith():
    H, out = "hybrid", []
    for name, dt in (("arith", ("f32",)), ("arith16", ("f32", "f16"))):
        cp = corpus(name)
        lex = np.concatenate([cp.head[3:96:2], cp.head[140:200:5]])
        sc = _lex_scores(lex.size, 21, 0.01, 7.3)
        out.append(Case(H, "arith", "fma_and_division", name, 96, w_e=0.7, w_l=0.3, lex=zip(lex, sc), dtypes=dt))
        out.append(Case(H, "arith", "fma_and_division", name, 96, w_e=0.61803, w_l=1.7, lex=zip(lex, sc * F32(1e-3)), dtypes=dt))
        out.append(Case(H, "arith", "negative_w_l", name, 96, w_e=0.7, w_l=-0.3, lex=zip(cp.head[5:40:6], _lex_scores(6, 22)), dtypes=dt))
        sc = _lex_scores(lex.size, 23)
        sc[::5] *= F32(-0.02)                                    # small enough to stay in the pool: negative scores are reported
        out.append(Case(H, "arith", "negative_lexical", name, 96, lex=zip(lex, sc), dtypes=dt))
        tiny = (_lex_scores(lex.size, 24, 0.05, 1.0) * EPS).astype(np.float32)
        out.append(Case(H, "arith", "max_lex_epsilon", name, 96, lex=zip(lex, tiny), dtypes=dt))
    # NaN lexical scores: ordered last by row, reported as NaN -- only a pool that holds the whole index shows them
    out.append(Case(H, "arith", "nan_lexical", "n17", 17, lex=[(2, 1.5), (5, np.nan), (6, 0.25), (11, np.nan), (3, np.nan)],
                    dtypes=("f32", "f16")))
    return out


def _zero_lex(cp):
    """lexical pairs of the zeros corpora: the class rows 104 and 105 get a negative lexical term that underflows (-0 from a
    product, whatever the cosine's sign), one top row cancels exactly (+0 from a difference)"""
    return [(104, -1.0), (105, -1.0), (int(cp.head[1]), 4096.0)]


def _hybrid_zeros():
    H, out = "hybrid", []
    for name, top in (("zeros4", 4), ("zeros600", 600)):
        need = top + 6                                           # the cut falls inside the class of 12 zeros
        out.append(Case(H, "zeros", "minus_w_l", name, need, w_e=2.0 ** -140, w_l=-0.0))
        out.append(Case(H, "zeros", "minus_w_l", name, need + 3, w_e=2.0 ** -140, w_l=-0.0))
        out.append(Case(H, "zeros", "plus_w_l", name, need, w_e=2.0 ** -140, w_l=0.0))
        # l = -2^-12: w_l l = -2^-152 -> -0.  Row 105: -0 + -0 = -0; row 104: +0 + -0 = +0; the rest of the class + (+0) = +0
        out.append(Case(H, "zeros", "negative_lexical_term", name, need, w_e=2.0 ** -140, w_l=2.0 ** -140, lex=_zero_lex(corpus(name))))
    # exact cancellation: w_e cos = 2^-12 against w_l l = -2^-12 -> +0, in the middle of rows whose score is -0 or +0
    cp = corpus("zeros4")
    lex = [(r, 2.0 ** -12) for r in (100, 102, 106)] + [(int(cp.head[0]), 1.0)]
    out.append(Case(H, "zeros", "cancellation", "zeros4", 8, w_e=1.0, w_l=-1.0, lex=lex,
                    note="rows 100, 102, 106 and the best row cancel to +0: ranks 7..10, ordered by row"))
    return out


def _hybrid_classes():
    H, big, out = "hybrid", corpus("big"), []
    tail = np.setdiff1d(np.arange(N_BIG), big.head[:4608])
    cls = tail[5:30000:20][:1500]
    # w_l l = 1 and |w_e cos| < 2^-30: every lexical row scores exactly 1.0, the row word of the key decides the cut
    for need, dt in ((700, ("f32", "f16")), (1, ("f32",)), (1024, ("f32",))):
        out.append(Case(H, "classes", "one_score_1500", "big", need, w_e=2.0 ** -30, w_l=1.0, lex=zip(cls, np.full(1500, 3.0)), dtypes=dt))
    out.append(Case(H, "classes", "one_score_2043", "big", 1, w_e=2.0 ** -30, w_l=1.0, lex=zip(tail[:2043], np.full(2043, 3.0))))
    # rows 0..63 of the tail: keys that differ only in the low row bits
    low = tail[tail < 4096][:48]
    out.append(Case(H, "classes", "low_row_bits", "big", 8, w_e=2.0 ** -30, w_l=1.0, lex=zip(low, np.full(low.size, 3.0))))
    # 400 consecutive rows and one fetched lexical row (an empty slot: key 0, so bit 63 varies and the digits end at bits
    # 8..0): the bin of 512 rows above the last digit holds too many, the walk runs to shift == 0
    dense = np.concatenate([tail[tail >= 1000][:400], [big.head[3]]])
    out.append(Case(H, "classes", "dense_rows_last_digit", "big", 100, w_e=2.0 ** -30, w_l=1.0, lex=zip(dense, np.full(401, 3.0))))
    # two classes one high score bit apart (1.0 and 0.5), 40 + 900 rows
    sc = np.concatenate([np.full(40, 4.0), np.full(900, 2.0)])
    out.append(Case(H, "classes", "one_high_score_bit", "big", 30, w_e=2.0 ** -30, w_l=1.0, lex=zip(cls[:940], sc)))
    out.append(Case(H, "classes", "one_high_score_bit", "big", 500, w_e=2.0 ** -30, w_l=1.0, lex=zip(cls[:940], sc)))
    # no lexical pair: distinct scores, the fetch is need + 8, within the slack
    out.append(Case(H, "classes", "distinct_scores", "big", 200, dtypes=("f32", "f16")))
    out.append(Case(H, "classes", "distinct_scores_many", "big", 64, lex=zip(cls[:1200], _lex_scores(1200, 31))))
    return out


def _hybrid_boundary():
    H, out = "hybrid", []
    ulp, e = corpus("ulp"), dict
    # w_e = 1: combined = cos.  need 21 is the row at v + ulp, the fetch (need + 8 without pairs) ends inside the class of cosine v
    out.append(Case(H, "boundary", "one_ulp_above", "ulp", 21, w_e=1.0, w_l=0.0, expect=e(default=0, full=0)))
    out.append(Case(H, "boundary", "equal", "ulp", 22, w_e=1.0, w_l=0.0, expect=e(default=2, full=2)))
    out.append(Case(H, "boundary", "one_ulp_above", "ulp600", 601, w_e=1.0, w_l=0.0, expect=e(default=0, full=0)))
    out.append(Case(H, "boundary", "equal", "ulp600", 602, w_e=1.0, w_l=0.0, expect=e(default=2, full=2)))
    # one lexical row on top and ranks 20..51 of the cosine order pushed down by a lexical term of -1: the 22nd best row is a
    # row of the class, equal to c_tail (default fetch: 54 rows, the last of them in the class)
    v = F32(0.75)
    down = [(int(r), -1.0) for r in ulp.head[20:52]]
    out.append(Case(H, "boundary", "equal_from_outside", "ulp", 22, w_e=1.0, w_l=1.0, lex=down + [(int(ulp.head[300]), 1.0)],
                    expect=e(default=2, full=0), note="the full fetch (62 rows) passes the class: its tail is below v"))
    # the same with the whole class pushed down: the 22nd row is a lexical row at v - ulp(v) exactly, one ulp BELOW c_tail
    below = np.nextafter(v, F32(0.0))
    lexrow = int(ulp.head[400])
    term = F32(below - ulp.cos[lexrow])                           # exact: both on the 2^-24 grid of [0.25, 1)
    assert F32(ulp.cos[lexrow] + term) == below
    out.append(Case(H, "boundary", "one_ulp_below", "ulp", 22, w_e=1.0, w_l=1.0,
                    lex=[(int(r), -1.0) for r in ulp.head[20:61]] + [(lexrow, term), (int(ulp.head[300]), 1.0)],
                    expect=e(default=2, full=0), note="full: 71 rows fetched, c_tail is far below"))
    term = F32(np.nextafter(v, F32(1.0)) - ulp.cos[lexrow])
    out.append(Case(H, "boundary", "one_ulp_above_lexical", "ulp", 22, w_e=1.0, w_l=1.0,
                    lex=[(int(r), -1.0) for r in ulp.head[20:52]] + [(lexrow, term), (int(ulp.head[300]), 1.0)],
                    expect=e(default=0, full=0)))
    for name, base, dt in (("chain0", 0, ("f32",)), ("chain560", 560, ("f32",)), ("chain16", 0, ("f32", "f16"))):
        # 64 distinct cosines, one product (358 * 2^-149; binary16 grid: 2 * 2^-149): without pairs the fetch is need + 8 and
        # the chain reaches the last fetched row (fetch = base + 64) / stops one row before it
        w = CHAIN_W if name != "chain16" else CHAIN_W16
        out.append(Case(H, "boundary", "chain_reaches_last", name, base + 56, w_e=w, w_l=0.0, expect=e(default=2, full=2), dtypes=dt))
        out.append(Case(H, "boundary", "chain_stops_before", name, base + 57, w_e=w, w_l=0.0, expect=e(default=0, full=0), dtypes=dt))
        out.append(Case(H, "boundary", "chains_of_two", name, base + 20, w_e=0.7, w_l=0.0, expect=e(default=0, full=0), dtypes=dt))
    # 40 lexical rows outside: the default fetch is need + 32, the full one need + 48
    cp = corpus("chain0")
    lex = list(zip(cp.head[200:240], np.full(40, 0.0)))
    out.append(Case(H, "boundary", "chain_and_fetch_mode", "chain0", 16, w_e=CHAIN_W, w_l=0.0, lex=lex, expect=e(default=2, full=2),
                    note="both fetches end on the chain"))
    out.append(Case(H, "boundary", "chain_and_fetch_mode", "chain0", 32, w_e=CHAIN_W, w_l=0.0, lex=lex, expect=e(default=2, full=0),
                    note="default: 64 rows, the last on the chain; full: 80 rows"))
    out.append(Case(H, "boundary", "chain_and_fetch_mode", "chain0", 33, w_e=CHAIN_W, w_l=0.0, lex=lex, expect=e(default=0, full=0)))
    return out


def _hybrid_sizes():
    H, big, out = "hybrid", corpus("big"), []
    tail = np.setdiff1d(np.arange(N_BIG), big.head[:4608])
    out.append(Case(H, "sizes", "need_clamped", "n9", 100, lex=[(1, 2.0), (7, 0.5)], dtypes=("f32", "f16")))
    out.append(Case(H, "sizes", "need_clamped", "n9", 100))
    out.append(Case(H, "sizes", "need_1", "big", 1, lex=[(int(big.head[40]), 2.0)]))
    out.append(Case(H, "sizes", "need_1024", "big", 1024, lex=zip(big.head[1100:1200:7], _lex_scores(15, 41))))
    out.append(Case(H, "sizes", "slots_full", "big", 2, lex=zip(tail[100:2143], _lex_scores(2043, 42)),
                    note="need + 2 n_lex + 8 = 4096"))
    out.append(Case(H, "sizes", "slots_full", "big", 1024, lex=zip(tail[100:1632], _lex_scores(1532, 43)), note="need + 2 n_lex + 8 = 4096"))
    lex = list(zip(big.head[70:90:3], _lex_scores(7, 44)))
    out.append(Case(H, "sizes", "k_0", "big", 60, lex=lex, k=0, diversify=1))
    out.append(Case(H, "sizes", "k_above_need", "big", 60, lex=lex, k=75, diversify=1))
    out.append(Case(H, "sizes", "k_above_need", "n9", 100, lex=[(1, 2.0)], k=30, diversify=1))
    return out


def _hybrid_overflow():
    return [Case("hybrid", "overflow", "ties_5000", "ties5000", 10, expect=dict(default=1, full=1), dtypes=("f32", "f16")),
            Case("hybrid", "overflow", "ties_5000", "ties5000", 10, lex=[(3, 1.0), (9, 2.0)], expect=dict(default=1, full=1))]


def _hybrid_emit():
    H, big, out = "hybrid", corpus("big"), []
    for need, k in ((60, 20), (120, 40), (300, 100)):             # pool strides of the greedy kernels with J = 1, 2, 5
        fetch = need + 32
        lex = np.concatenate([big.head[5:need:7], big.head[fetch + 3: fetch + 60: 4]])
        out.append(Case(H, "emit", f"mmr_pool_{need}", "big", need, lex=zip(lex, _lex_scores(lex.size, 50 + need, 3.0, 9.0)), k=k,
                        diversify=1, lam=0.5, dtypes=("f32", "f16")))
        out.append(Case(H, "emit", f"mmr_pool_{need}", "big", need, k=k, diversify=1, lam=0.3))
    out.append(Case(H, "emit", "mmr_zeros", "zeros4", 10, w_e=2.0 ** -140, w_l=-0.0, k=10, diversify=1, lam=0.5))
    return out


def _diverse():
    D, out = "diverse", []
    e = dict
    for name, top in (("zeros4", 4), ("zeros600", 600)):
        for need in (top + 6, top + 5, top + 9):
            out.append(Case(D, "zeros", "minus_w_l", name, need, w_e=2.0 ** -140, w_l=-0.0, k=need, lam=0.5))
        out.append(Case(D, "zeros", "plus_w_l", name, top + 6, w_e=2.0 ** -140, w_l=0.0, k=top + 6, lam=0.5))
    out.append(Case(D, "boundary", "one_ulp_above", "ulp", 21, w_e=1.0, w_l=0.0, k=7, expect=e(tail0=0, tail1=0)))
    out.append(Case(D, "boundary", "equal", "ulp", 22, w_e=1.0, w_l=0.0, k=7, expect=e(tail0=2, tail1=2)))
    # the same two sides behind 600 rows: 609 / 610 fetched rows, sort_emit + pool_prepare_kernel<false>, which takes c_tail
    # from the last fetched cosine and c_need from its own rank loop
    out.append(Case(D, "boundary", "one_ulp_above", "ulp600", 601, w_e=1.0, w_l=0.0, k=7, expect=e(tail0=0, tail1=0)))
    out.append(Case(D, "boundary", "equal", "ulp600", 602, w_e=1.0, w_l=0.0, k=7, expect=e(tail0=2, tail1=2)))
    for name, base, dt in (("chain0", 0, ("f32",)), ("chain560", 560, ("f32",)), ("chain16", 0, ("f32", "f16"))):
        w = CHAIN_W if name != "chain16" else CHAIN_W16
        out.append(Case(D, "chains", "chain_reaches_last", name, base + 56, w_e=w, k=10, expect=e(tail0=2, tail1=2), dtypes=dt))
        out.append(Case(D, "chains", "chain_stops_before", name, base + 57, w_e=w, k=10, expect=e(tail0=0, tail1=0), dtypes=dt))
        out.append(Case(D, "chains", "chains_of_two", name, base + 30, w_e=0.7, k=12, expect=e(tail0=0, tail1=0), dtypes=dt))
    out.append(Case(D, "ends", "pool_above_n", "n9", 100, k=5, dtypes=("f32", "f16")))
    out.append(Case(D, "ends", "n_just_above_need", "n9", 8, k=5))
    out.append(Case(D, "ends", "fetch_covers", "n17", 12, k=6, lam=0.3))
    out.append(Case(D, "ends", "pool_60", "big", 60, k=20, dtypes=("f32", "f16")))
    out.append(Case(D, "ends", "pool_600", "big", 600, k=25, dtypes=("f32", "f16")))
    out.append(Case(D, "ends", "pool_1024", "big", 1024, k=5))
    # 1500 rows tie with the fetch-th cosine; the need-th row stands above the class
    out.append(Case(D, "overflow", "candidates_above_1024", "band104", 100, k=10, expect=e(tail0=1, tail1=1), dtypes=("f32", "f16")))
    out.append(Case(D, "overflow", "same_rows_large_fetch", "band604", 600, k=10, expect=e(tail0=0, tail1=0), dtypes=("f32", "f16")))
    out.append(Case(D, "overflow", "ties_5000", "ties5000", 10, k=5, expect=e(tail0=1, tail1=1)))
    return out


_HYBRID = dict(hash=_hybrid_hash, reach=_hybrid_reach, arith=_hybrid_arith, zeros=_hybrid_zeros, classes=_hybrid_classes,
               boundary=_hybrid_boundary, sizes=_hybrid_sizes, overflow=_hybrid_overflow, emit=_hybrid_emit)


@functools.lru_cache(maxsize=None)
def plan(entry, name):
    """the cases of one plan (a tuple; the cases are shared, do not change them)"""
    if entry == "hybrid":
        return tuple(_HYBRID[name]())
    return tuple(c for c in _diverse() if c.plan == name)


def cases(entry=None):
    out = []
    for e, names in (("hybrid", HYBRID_PLANS), ("diverse", DIVERSE_PLANS)):
        if entry in (None, e):
            for nm in names:
                out.extend(plan(e, nm))
    return out


@functools.lru_cache(maxsize=None)
def want(entry, name, index, mode):
    """expected(plan(entry, name)[index], mode), computed once per process"""
    return expected(plan(entry, name)[index], mode)
