"""Capped hybrid search (rlr_search_capped; the capped finish of rust-local-rag_amd/csrc/group.hip), pure numpy: the
definition every layer is held to, a restatement of the device path with plantable defects, and small designed cases that
each defect must break.  tests/test_capped_vectors_cpu.py holds these to each other and pins the definition to the oracle;
tests/test_gpu_capped.py holds the device to `define`.

The definition: every allowed row has cos (the reference-order dot product), lexn = bm25 / max_lex (0 without a lexical
pair; pairs outside the allowed rows are no candidates) and combined = w_e * cos + w_l * lexn in f32 -- two rounded
products, one add.  Walk the rows in the engine's candidate order (combined descending, NaN last, row ascending, -0 and +0
tying), accept a row unless per_doc rows of its document are accepted, stop at `need`.  A row tagged DOC_NONE -- and every
row of an index without a column -- is a group of its own and is never capped."""
import numpy as np

import grouped_vectors as G

DOC_NONE = G.DOC_NONE
F32_EPSILON = np.float32(1.1920929e-07)
GROUP_CAP, LEX_CAP, NEED_MAX = 2048, 2048, 1024           # what the one-workgroup finish holds (kernels.h)
W_EMBEDDING, W_LEXICAL = 0.7, 0.3                         # the engine's default blend (oracle.search)


def f32(x):
    return np.asarray(x, dtype=np.float32)


def max_lex_of(lex_scores):
    """max(lexical scores, f32::EPSILON) over EVERY pair, as the engine computes it"""
    s = f32(lex_scores)
    m = np.float32(0.0)
    for v in s:                                            # fold(0.0, f32::max): NaN scores are ignored
        if v > m:
            m = v
    return m if m >= F32_EPSILON else F32_EPSILON


def lexn_of(n, lex_rows, lex_scores, max_lex):
    """normalised lexical score per row (0 without a pair; a repeated row keeps its LAST score, rows >= n are dropped)"""
    l = np.zeros(n, np.float32)
    has = np.zeros(n, bool)
    for r, s in zip(np.asarray(lex_rows, np.int64), f32(lex_scores)):
        if 0 <= r < n:
            l[r] = np.float32(s) / np.float32(max_lex)
            has[r] = True
    return l, has


def combine(w_e, w_l, cos, lexn):
    """two rounded f32 products and one rounded add, elementwise"""
    with np.errstate(all="ignore"):
        t0 = np.float32(w_e) * f32(cos)
        t1 = np.float32(w_l) * f32(lexn)
        return (t0 + t1).astype(np.float32)


def need_of(n_allowed, top_k, stage=0, diversify=False):
    """what the uncapped entry keeps: min(top_k, N) | initial_k | min(N, max(3 top_k, top_k + 10))"""
    k = max(top_k, 1)
    if diversify:
        return min(n_allowed, max(3 * top_k, top_k + 10))
    return min(n_allowed, 3 * k) if stage else min(n_allowed, k)


def allowed_rows(n, allowed):
    if allowed is None:
        return np.arange(n, dtype=np.int64)
    a = np.asarray(allowed)
    return np.flatnonzero(a) if a.dtype == bool else np.unique(a.astype(np.int64))


def define(exact, docs, lex_rows, lex_scores, w_e, w_l, need, per_doc, allowed=None, max_lex=None):
    """THE DEFINITION -> dict(rows u64, comb f32, cos f32, lexn f32, docs u32): the first `need` accepted rows in order.
    exact: oracle.scan(rows, q); docs: u32 per row or None; lex_*: the BM25 pairs; allowed: rows or a mask"""
    e = f32(exact)
    n = e.size
    docs = np.full(n, DOC_NONE, np.uint32) if docs is None else np.asarray(docs, np.uint32)
    rows = allowed_rows(n, allowed)
    ml = max_lex_of(lex_scores) if max_lex is None else np.float32(max_lex)
    inside = np.zeros(n, bool)
    inside[rows] = True
    keep = [i for i, r in enumerate(np.asarray(lex_rows, np.int64)) if 0 <= r < n and inside[r]]
    lexn, _ = lexn_of(n, np.asarray(lex_rows, np.int64)[keep], f32(lex_scores)[keep], ml)
    comb = combine(w_e, w_l, e, lexn)
    order = rows[G.result_order(comb[rows], rows)]
    got = G.walk(order, docs, min(need, rows.size), per_doc).astype(np.int64) if need > 0 and rows.size else np.zeros(0, np.int64)
    return dict(rows=got.astype(np.uint64), comb=comb[got], cos=e[got], lexn=lexn[got], docs=docs[got])


def define_search(O, rows, q, docs, lex_rows, lex_scores, w_e, w_l, top_k, per_doc, diversity=0.0, stage=0, allowed=None):
    """the engine entry over the definition: oracle.scan, the f32 blend, the walk, and -- diversified -- oracle.mmr over
    the accepted pool.  q: the NORMALISED query.  -> the same dict, in pick order"""
    lam = min(max(float(diversity), 0.0), 1.0)
    diversify = lam != 0.0
    n_allowed = allowed_rows(rows.shape[0], allowed).size
    need = need_of(n_allowed, top_k, stage, diversify)
    pool = define(O.scan(rows, q), docs, lex_rows, lex_scores, w_e, w_l, need, per_doc, allowed)
    if not diversify or pool["rows"].size == 0:
        return pool
    order, _ = O.mmr(rows[pool["rows"].astype(np.int64)], pool["comb"], top_k, lam)
    return {k: v[order] for k, v in pool.items()}


# ---- the device path, restated ---------------------------------------------------------------------------------------
def score_key(x):
    """the order-preserving map f32 -> u32 of common.h (NaN -> 0)"""
    b = int(np.float32(x).view(np.uint32))
    if (b & 0x7FFFFFFF) > 0x7F800000:
        return 0
    return (~b & 0xFFFFFFFF) if b & 0x80000000 else (b | 0x80000000)


def key_score(k):
    b = (k & 0x7FFFFFFF) if k & 0x80000000 else (~k & 0xFFFFFFFF)
    return np.uint32(b).view(np.float32)


def comb_key(c):
    return score_key(np.float32(0.0) if c == 0 else c)


def bin_floor(a):
    """the floor of the 22-bit bin of a nominated score: U of the collect"""
    u = key_score(score_key(a) & ~0x3FF)
    return np.float32(-np.inf) if np.isnan(u) else u


def bound_key(t, u, eps, w_e, w_l):
    """capped_bound_key of group.hip: 0 = nothing left behind, 0xFFFFFFFF = no number"""
    with np.errstate(all="ignore"):
        thr = np.float32(max(np.float32(t), np.float32(u))) - np.float32(2.0 * eps)
        if thr == -np.inf:
            return 0
        eb = np.float32(thr + np.float32(eps))
        if np.isnan(eb):
            return 0xFFFFFFFF
        if eb != np.inf:
            eb = np.nextafter(np.float32(0.0) if eb == 0 else eb, np.float32(np.inf), dtype=np.float32)
        cb = combine(w_e, w_l, eb, np.float32(0.0))
    return 0xFFFFFFFF if np.isnan(cb) else comb_key(cb)


DEFECTS = ("cap_in_cosine_order", "lexical_counted_twice", "lexical_exempt", "rank_by_nominated", "boundary_ignored",
           "untagged_capped", "ties_higher_row")


def device_path(nominated, exact, docs, lex_rows, lex_scores, w_e, w_l, need, per_doc, eps, allowed=None, max_lex=None,
                defect=None):
    """-> (status, result dict).  status 0: decided here; 1: capacity; 2: undecidable here (boundary tie, NaN rows
    needed); 3: by rule.  The grouped collect over the cosine nominations with k = need (grouped_vectors.fast_path's
    heads, t_g and U -- U the floor of the need-th head's bin), united with the lexical rows, blended, ranked inside the
    document by (combined, row), accepted below per_doc, ordered, cut -- then the boundary rule."""
    a = f32(nominated).astype(np.float64)
    e = f32(exact)
    n = e.size
    docs = np.full(n, DOC_NONE, np.uint32) if docs is None else np.asarray(docs, np.uint32)
    rows = allowed_rows(n, allowed)
    inside = np.zeros(n, bool)
    inside[rows] = True
    ml = max_lex_of(lex_scores) if max_lex is None else np.float32(max_lex)
    lr = np.asarray(lex_rows, np.int64)
    keep = [i for i, r in enumerate(lr) if 0 <= r < n and inside[r]]
    lexn, is_lex = lexn_of(n, lr[keep], f32(lex_scores)[keep], ml)
    need = min(need, rows.size)
    empty = dict(rows=np.zeros(0, np.uint64), comb=f32([]), cos=f32([]), lexn=f32([]), docs=np.zeros(0, np.uint32))
    if need > NEED_MAX or is_lex.sum() > LEX_CAP or not w_e > 0 or not np.isfinite(w_e) or not w_l >= 0 or not np.isfinite(w_l) \
            or (f32(lex_scores)[keep] < 0).any():
        return 3, empty
    a = np.where(inside, a, np.nan)                          # a masked row has no nomination
    tagged = docs != DOC_NONE
    valid = ~np.isnan(a)
    tg = np.full(n, -np.inf)
    head = np.zeros(n, bool)
    seen = {}
    for r in [r for r in G.result_order(a) if valid[r]]:     # descending nominated key
        if not tagged[r]:
            head[r] = True
            continue
        c = seen.get(int(docs[r]), 0)
        seen[int(docs[r])] = c + 1
        head[r] = c < per_doc
        if c == per_doc - 1:
            tg[docs == docs[r]] = a[r]
    tg[~tagged] = -np.inf
    hv = np.sort(a[head])[::-1]
    U = bin_floor(hv[need - 1]) if hv.size >= need else np.float32(-np.inf)
    with np.errstate(all="ignore"):
        thr = (np.maximum(f32(tg), U) - np.float32(2.0 * eps)).astype(np.float32)
    cand = np.flatnonzero(valid & ~(f32(a) < thr))
    if cand.size > GROUP_CAP:
        return 1, empty
    comb = combine(w_e, w_l, e, lexn)
    extra = np.flatnonzero(is_lex & ~np.isin(np.arange(n), cand))
    union = np.concatenate([cand, extra, np.flatnonzero(is_lex & np.isin(np.arange(n), cand))
                            if defect == "lexical_counted_twice" else np.zeros(0, np.int64)]).astype(np.int64)
    saw_nan = bool(np.isnan(comb[union]).any())
    union = union[~np.isnan(comb[union])]
    capped = tagged.copy()
    if defect == "untagged_capped":
        capped[:] = True
    if defect == "lexical_exempt":
        capped &= ~is_lex
    rank_key = e if defect == "cap_in_cosine_order" else f32(a) if defect == "rank_by_nominated" else comb
    by_rank = union[G.result_order(rank_key[union], union, higher_row_first=defect == "ties_higher_row")]
    accepted = []
    taken = {}
    for r in by_rank:
        d = int(docs[r])
        if capped[r]:
            if taken.get(d, 0) >= per_doc:
                continue
            taken[d] = taken.get(d, 0) + 1
        accepted.append(int(r))
    accepted = np.asarray(accepted, np.int64)
    out = accepted[G.result_order(comb[accepted], accepted, higher_row_first=defect == "ties_higher_row")][:need]
    res = dict(rows=out.astype(np.uint64), comb=comb[out], cos=e[out], lexn=lexn[out], docs=docs[out])
    status = 0
    all_collected = cand.size == int(valid.sum())
    if not all_collected and defect != "boundary_ignored":
        req = bound_key(-np.inf, U, eps, w_e, w_l) if U != -np.inf else 0
        for d in {int(docs[r]) for r in union if tagged[r]}:
            kb = bound_key(tg[np.flatnonzero(docs == d)[0]], U, eps, w_e, w_l)
            above = sum(1 for r in union if docs[r] == d and comb_key(comb[r]) > kb)
            if kb != 0 and above < per_doc:
                req = max(req, kb)
        if req != 0 and not (accepted.size >= need and comb_key(comb[out[need - 1]]) > req):
            status = 2
    if accepted.size < need and (int(valid.sum()) < rows.size or saw_nan):
        status = 2
    return status, res


# ---- designed cases ----------------------------------------------------------------------------------------------------
# Each: exact scores (the nominated scores are the same unless `a` is given), documents, lexical pairs, weights, need,
# per_doc, eps, the status the device path must report.  On the device they are rows (e_i, 0, .., 0) against the query
# (1, 0, .., 0): every dot product is exact in any order, so a = e there too and a tiny band is honest.
EPS = 1.0e-6
TIE_EPS = 5.0e-9


def _case(e, docs, lex, w_e, w_l, need, per_doc, eps=EPS, status=0, allowed=None, a=None):
    lex = sorted(lex)
    return dict(e=f32(e), a=f32(e if a is None else a), docs=None if docs is None else np.asarray(docs, np.uint32),
                lex_rows=np.asarray([r for r, _ in lex], np.uint64), lex_scores=f32([s for _, s in lex]), w_e=w_e, w_l=w_l,
                need=need, per_doc=per_doc, eps=eps, status=status, allowed=allowed)


def case_lexical_displaces_best_cosine():
    """document 1: row 0 is its best by cosine, row 2 -- far down -- its best by combined: per_doc = 1 must answer row 2"""
    e = [0.90, 0.80, 0.20, 0.70, 0.60, 0.50, 0.10]
    docs = [1, 2, 1, 3, 3, 4, 5]
    return _case(e, docs, [(2, 4.0)], 0.3, 0.7, 3, 1)


def case_lexical_row_of_a_full_document():
    """document 7 is full by cosine (rows 0..2 lead, per_doc = 2); its lexical row 5 ranks third inside it by combined
    score and must NOT come back, although the lexical row of document 10 does; row 1 is lexical AND a cosine candidate"""
    e = [0.95, 0.94, 0.93, 0.50, 0.40, 0.30, 0.20, 0.10]
    docs = [7, 7, 7, 8, 9, 7, 10, 11]
    return _case(e, docs, [(1, 2.0), (5, 1.0), (6, 4.0)], 0.7, 0.3, 5, 2)


def case_mth_place_by_a_far_lexical_row():
    """document 3 (every fifth row): its second place (per_doc = 2) goes to lexical row 40, ninth of its ten rows by
    cosine, which lands between the document's best and second best cosine rows in combined order"""
    e = np.linspace(0.9, 0.1, 50)
    docs = np.where(np.arange(50) % 5 == 0, 3, 100 + np.arange(50))
    return _case(e, docs, [(40, 2.4), (41, 9.0)], 0.3, 0.7, 6, 2)


def tie_cosine():
    """a bin floor c in [0.84, 1) whose predecessor rounds to the same product under w_e = 0.3"""
    w = np.float32(0.3)
    key = score_key(np.float32(0.9)) & ~0x3FF
    while True:
        c = key_score(key)
        below = np.nextafter(c, np.float32(0.0), dtype=np.float32)
        if w * c == w * below:
            return c, below
        key += 0x400


def case_rounding_tie_outside_the_band():
    """rows 1..4 lead; row 9 (cosine c, a bin floor) is the fifth head; row 0 scores one ulp below c -- under the band of
    TIE_EPS it is left behind -- and 0.3 * its cosine rounds to 0.3 * c: it ties, has the smaller row and belongs ahead"""
    c, below = tie_cosine()
    e = f32([below, 0.99, 0.98, 0.97, 0.96, 0.5, 0.4, 0.3, 0.2, c])
    return _case(e, np.arange(10) + 50, [], 0.3, 0.0, 5, 1, eps=TIE_EPS, status=2)


def case_signed_zero_combined():
    """w_l = -0: a cosine that underflows under w_e gives combined -0, a zero cosine +0; they tie and the row decides"""
    tiny = np.float32(-1.0e-45)
    e = f32([tiny, 0.0, tiny, 0.0, tiny, 0.0, -0.5])
    return _case(e, [1, 1, 2, 2, 3, 3, 4], [], 0.3, -0.0, 4, 1)


def case_fewer_documents_than_need():
    """three documents, per_doc = 2, need = 10: six rows come back and that is no error"""
    e = np.linspace(0.9, 0.2, 30)
    return _case(e, np.arange(30) % 3, [(29, 2.0)], 0.7, 0.3, 10, 2)


def case_nan_row_needed():
    """five rows, one of them NaN, need = 5 with every row its own document: the NaN row is wanted to fill the list"""
    e = f32([0.5, np.nan, 0.4, 0.3, 0.2])
    return _case(e, np.arange(5) + 1, [(3, 1.0)], 0.7, 0.3, 5, 1, status=2)


def case_lexical_rows_outside_the_filter():
    """the allowed rows are the even ones; lexical rows 1 and 3 lie outside (they still count for max_lex), 4 inside"""
    e = np.linspace(0.9, 0.1, 12)
    return _case(e, np.arange(12) // 2, [(1, 8.0), (3, 6.0), (4, 2.0)], 0.7, 0.3, 4, 1, allowed=np.arange(0, 12, 2))


def case_untagged_rows():
    """the three best rows are untagged: all come back whatever per_doc"""
    e = [0.9, 0.8, 0.7, 0.6, 0.5]
    return _case(e, [DOC_NONE, DOC_NONE, DOC_NONE, 1, 1], [(4, 1.0)], 0.7, 0.3, 4, 1)


def case_equal_scores():
    """equal combined scores inside a document (rows 1, 2) and across documents (rows 4, 5): the lower row wins"""
    e = [0.1, 0.6, 0.6, 0.2, 0.5, 0.5, 0.05]
    return _case(e, [1, 2, 2, 3, 4, 5, 6], [], 0.7, 0.3, 2, 1)


def case_nominated_order_disagrees():
    """document 5: row 3 is the best by exact score, rows 4..6 by nomination (all within the band)"""
    e = f32([0.30, 0.31, 0.32, 0.80000, 0.79999, 0.79998, 0.79997, 0.50, 0.49])
    a = e.astype(np.float64)
    a[3] -= 0.9e-4
    a[4:7] += 0.9e-4
    return _case(e, [1, 2, 3, 5, 5, 5, 5, 6, 6], [], 0.7, 0.3, 3, 1, eps=1.0e-4, a=a)


CASES = {"lexical_displaces_best_cosine": case_lexical_displaces_best_cosine,
         "lexical_row_of_a_full_document": case_lexical_row_of_a_full_document,
         "mth_place_by_a_far_lexical_row": case_mth_place_by_a_far_lexical_row,
         "rounding_tie_outside_the_band": case_rounding_tie_outside_the_band,
         "signed_zero_combined": case_signed_zero_combined,
         "fewer_documents_than_need": case_fewer_documents_than_need,
         "nan_row_needed": case_nan_row_needed,
         "lexical_rows_outside_the_filter": case_lexical_rows_outside_the_filter,
         "untagged_rows": case_untagged_rows,
         "equal_scores": case_equal_scores,
         "nominated_order_disagrees": case_nominated_order_disagrees}
# the cases the device realises with exact dot products (a = e); the last one needs nominations that differ
DEVICE_CASES = tuple(k for k in CASES if k != "nominated_order_disagrees")
# the designed case each defect must break
BROKEN_BY = {"cap_in_cosine_order": ("lexical_displaces_best_cosine", "mth_place_by_a_far_lexical_row"),
             "lexical_counted_twice": ("lexical_row_of_a_full_document",),
             "lexical_exempt": ("lexical_row_of_a_full_document",),
             "rank_by_nominated": ("nominated_order_disagrees",),
             "boundary_ignored": ("rounding_tie_outside_the_band",),
             "untagged_capped": ("untagged_rows",),
             "ties_higher_row": ("equal_scores", "signed_zero_combined")}


def run_define(c):
    return define(c["e"], c["docs"], c["lex_rows"], c["lex_scores"], c["w_e"], c["w_l"], c["need"], c["per_doc"], c["allowed"])


def run_device(c, defect=None):
    return device_path(c["a"], c["e"], c["docs"], c["lex_rows"], c["lex_scores"], c["w_e"], c["w_l"], c["need"], c["per_doc"],
                       c["eps"], c["allowed"], defect=defect)


def same(a, b):
    """two result dicts, compared as bit patterns (a NaN equals a NaN)"""
    def eq(x, y):
        x, y = f32(x), f32(y)
        return x.shape == y.shape and bool(np.all((x.view(np.uint32) == y.view(np.uint32)) | (np.isnan(x) & np.isnan(y))))
    return (np.array_equal(a["rows"], b["rows"]) and np.array_equal(a["docs"], b["docs"]) and eq(a["comb"], b["comb"]) and
            eq(a["cos"], b["cos"]) and eq(a["lexn"], b["lexn"]))
