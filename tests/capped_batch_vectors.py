"""Batched capped search (rlr_search_capped_batch; capped_finish_multi_kernel of rust-local-rag_amd/csrc/group.hip and
capped_batch_chunk of index_grouped.hip), pure numpy: one chunk of queries restated on top of tests/capped_vectors.py (the
definition and the single device path) and tests/grouped_batch_vectors.py (the workspace rule and the split), with the
defects batching can introduce planted one at a time, and designed chunks that each defect must break.  The definition is
capped_vectors.define query by query (then the oracle's greedy MMR over the pool, when diversified).
tests/test_capped_batch_vectors_cpu.py holds the restatement to it; tests/test_gpu_capped_batch.py holds the device to it.

The chunk, as the library runs it:
  host     query q's pairs are lex_rows / lex_scores [lex_offsets[q], lex_offsets[q + 1]); pairs outside the allowed rows
           are dropped; a query with more than LEX_CAP pairs left, a negative or NaN score or a max_lex that is not a
           positive number goes BY RULE (form 3), alone; the others' pairs are laid out `stride` apart with a count each.
  collect  per query, on its own nominated scores: heads, t_g, U, the candidates (capped_vectors.device_path's first half).
  finish   per query, one workgroup: its candidates united with ITS lexical slice under ITS max_lex, flags of its own,
           blended, capped in combined order, the boundary rule against ITS t_g and U; the pool into ITS slice of the
           output planes, info = {pool size, status}, pool size 0 with a non-zero status.
  MMR      one batched launch; query q's pool size is the finish's sizes[q].
  host     status 0: read out (form 0); status 1 -> form 1, status 2 -> form 2: that query alone goes to the single path
           (here: the definition); its neighbours stay decided."""
import numpy as np

import capped_vectors as CV
import grouped_batch_vectors as GB
import grouped_vectors as G
import mmr_restatement as M

f32 = CV.f32
DOC_NONE = CV.DOC_NONE
LEX_CAP = CV.LEX_CAP

DEFECTS = ("slice_of_query_0", "offset_as_count", "max_lex_of_neighbour", "flags_shared", "no_query_stride",
           "pool_size_of_neighbour", "boundary_of_neighbour", "status_takes_chunk", "status_keeps_pool", "lex_limit_on_total")

# the workspace rule and the split are the grouped batch's, with k = need
chunk_width = GB.chunk_width
split = GB.split


# ---- the definition ----------------------------------------------------------------------------------------------------
def define_query(c, q):
    """THE DEFINITION for query q of a chunk -> result dict in answer order (pick order when diversified)"""
    lo, hi = int(c["lex_offsets"][q]), int(c["lex_offsets"][q + 1])
    pool = CV.define(c["e"][q], c["docs"], c["lex_rows"][lo:hi], c["lex_scores"][lo:hi], c["w_e"], c["w_l"], c["need"],
                     c["per_doc"], c.get("allowed"), max_lex=c["max_lex"][q])
    if not c.get("diversify") or pool["rows"].size == 0:
        return pool
    r = pool["rows"].astype(np.int64)
    order, _ = M.mmr_from_gram(c["sim"][np.ix_(r, r)], pool["comb"], c["k"], c["lam"])
    return {k: v[order] for k, v in pool.items()}


def define_chunk(c):
    return [define_query(c, q) for q in range(len(c["e"]))]


# ---- one query's collect and finish, restated (capped_vectors.device_path in two halves) -------------------------------
def collect(a, docs, need, per_doc, eps, inside):
    """heads, t_g, U and the candidates of one query over its nominated scores"""
    a = np.where(inside, f32(a).astype(np.float64), np.nan)
    n = a.size
    tagged = docs != DOC_NONE
    valid = ~np.isnan(a)
    tg = np.full(n, -np.inf)
    head = np.zeros(n, bool)
    seen = {}
    for r in [r for r in G.result_order(a) if valid[r]]:
        if not tagged[r]:
            head[r] = True
            continue
        cnt = seen.get(int(docs[r]), 0)
        seen[int(docs[r])] = cnt + 1
        head[r] = cnt < per_doc
        if cnt == per_doc - 1:
            tg[docs == docs[r]] = a[r]
    tg[~tagged] = -np.inf
    hv = np.sort(a[head])[::-1]
    U = CV.bin_floor(hv[need - 1]) if hv.size >= need else np.float32(-np.inf)
    with np.errstate(all="ignore"):
        thr = (np.maximum(f32(tg), U) - np.float32(2.0 * eps)).astype(np.float32)
    cand = np.flatnonzero(valid & ~(f32(a) < thr))
    return dict(cand=cand, tg=tg, U=U, n_valid=int(valid.sum()))


def finish(st, bound, e, docs, lrow, lscore, max_lex, flags, w_e, w_l, need, per_doc, eps, n_allowed):
    """one workgroup of the multi finish -> (status, pool dict).  st: the query's collect; bound: the collect whose t_g
    and U the boundary rule reads (the query's own); lrow / lscore: the slice the workgroup reads; flags: its
    lexical-pair flags (pair j is one of the candidates), zero on entry"""
    n = e.size
    cand = st["cand"]
    empty = dict(rows=np.zeros(0, np.uint64), comb=f32([]), cos=f32([]), lexn=f32([]), docs=np.zeros(0, np.uint32))
    if cand.size > CV.GROUP_CAP or lrow.size > LEX_CAP:
        return 1, empty
    tagged = docs != DOC_NONE
    lexn = np.zeros(n, np.float32)
    with np.errstate(all="ignore"):
        for j, r in enumerate(lrow):
            lexn[r] = np.float32(lscore[j]) / np.float32(max_lex)
            if r in cand:
                flags[j] = 1
    extra = np.asarray([r for j, r in enumerate(lrow) if not flags[j]], np.int64)
    comb = CV.combine(w_e, w_l, e, lexn)
    union = np.concatenate([cand, extra]).astype(np.int64)
    saw_nan = bool(np.isnan(comb[union]).any())
    union = union[~np.isnan(comb[union])]
    accepted, taken = [], {}
    for r in union[G.result_order(comb[union], union)]:
        d = int(docs[r])
        if tagged[r]:
            if taken.get(d, 0) >= per_doc:
                continue
            taken[d] = taken.get(d, 0) + 1
        accepted.append(int(r))
    accepted = np.asarray(accepted, np.int64)
    out = accepted[:need]
    res = dict(rows=out.astype(np.uint64), comb=comb[out], cos=f32(e)[out], lexn=lexn[out], docs=docs[out])
    status = 0
    if cand.size != st["n_valid"]:
        U, tg = bound["U"], bound["tg"]
        req = CV.bound_key(-np.inf, U, eps, w_e, w_l) if U != -np.inf else 0
        for d in {int(docs[r]) for r in union if tagged[r]}:
            kb = CV.bound_key(tg[np.flatnonzero(docs == d)[0]], U, eps, w_e, w_l)
            above = sum(1 for r in union if docs[r] == d and CV.comb_key(comb[r]) > kb)
            if kb != 0 and above < per_doc:
                req = max(req, kb)
        if req != 0 and not (accepted.size >= need and CV.comb_key(comb[out[need - 1]]) > req):
            status = 2
    if accepted.size < need and (st["n_valid"] < n_allowed or saw_nan):
        status = 2
    return status, res


def single_device_path(a, e, docs, lex_rows, lex_scores, w_e, w_l, need, per_doc, eps, allowed=None, max_lex=None):
    """collect + finish for ONE query: must equal capped_vectors.device_path (held to it by the CPU test)"""
    e = f32(e)
    n = e.size
    docs = G._docs(docs, n)
    rows = CV.allowed_rows(n, allowed)
    inside = np.zeros(n, bool)
    inside[rows] = True
    ml = CV.max_lex_of(lex_scores) if max_lex is None else np.float32(max_lex)
    lr, ls = _inside_pairs(lex_rows, lex_scores, inside)
    need = min(need, rows.size)
    if _by_rule(lr, ls, ml, w_e, w_l, need, LEX_CAP):
        return 3, None
    st = collect(a, docs, need, per_doc, eps, inside)
    return finish(st, st, e, docs, lr, ls, ml, np.zeros(lr.size, np.uint32), w_e, w_l, need, per_doc, eps, rows.size)


def _inside_pairs(lex_rows, lex_scores, inside):
    lr, ls = np.asarray(lex_rows, np.int64), f32(lex_scores)
    keep = [i for i, r in enumerate(lr) if 0 <= r < inside.size and inside[r]]
    return lr[keep], ls[keep]


def _by_rule(lr, ls, max_lex, w_e, w_l, need, lex_cap):
    with np.errstate(all="ignore"):
        return bool(need > CV.NEED_MAX or lr.size > lex_cap or not w_e > 0 or not np.isfinite(w_e) or not w_l >= 0 or
                    not np.isfinite(w_l) or not (ls >= 0).all() or not (np.isfinite(max_lex) and max_lex > 0))


# ---- the chunk -------------------------------------------------------------------------------------------------------
def chunk_path(c, defect=None):
    """-> per query dict(res=result dict in answer order, form=0..3, size=the pool size the MMR launch was given)"""
    E, A = f32(c["e"]), f32(c["a"])
    nq, n = E.shape
    docs = G._docs(c["docs"], n)
    rows = CV.allowed_rows(n, c.get("allowed"))
    inside = np.zeros(n, bool)
    inside[rows] = True
    need = min(c["need"], rows.size)
    per_doc, eps, w_e, w_l = c["per_doc"], c["eps"], c["w_e"], c["w_l"]
    lex_cap = c.get("lex_cap", LEX_CAP)
    off = [int(o) for o in c["lex_offsets"]]
    # host: the slices, the per-query rules, the strided layout
    slices, rule = [], []
    for q in range(nq):
        lo = 0 if defect == "slice_of_query_0" else off[q]
        cnt = off[q + 1] if defect == "offset_as_count" else off[q + 1] - off[q]
        slices.append(_inside_pairs(c["lex_rows"][lo:lo + cnt], c["lex_scores"][lo:lo + cnt], inside))
    total = sum(lr.size for lr, _ in slices)
    for q in range(nq):
        lr, ls = slices[q]
        size = total if defect == "lex_limit_on_total" else lr.size
        rule.append(_by_rule(lr, ls, np.float32(c["max_lex"][q]), w_e, w_l, need, lex_cap) or size > lex_cap)
    stride = max([1] + [slices[q][0].size for q in range(nq) if not rule[q]])
    lrow = np.zeros(nq * stride, np.int64)
    lscore = np.zeros(nq * stride, np.float32)
    lcnt = np.zeros(nq, np.int64)
    for q in range(nq):
        if not rule[q]:
            lr, ls = slices[q]
            lrow[q * stride:q * stride + lr.size], lscore[q * stride:q * stride + lr.size], lcnt[q] = lr, ls, lr.size
    # device: collect per query, then the finish per query into the output planes
    states = [collect(A[q], docs, need, per_doc, eps, inside) for q in range(nq)]
    planes = dict(rows=np.zeros(nq * need, np.uint64), comb=np.zeros(nq * need, np.float32), cos=np.zeros(nq * need, np.float32),
                  lexn=np.zeros(nq * need, np.float32), docs=np.zeros(nq * need, np.uint32))
    info = np.zeros(2 * nq, np.int64)
    sizes = np.zeros(nq, np.int64)
    shared_flags = np.zeros(stride, np.uint32)
    for q in range(nq):
        flags = shared_flags if defect == "flags_shared" else np.zeros(stride, np.uint32)
        ml = c["max_lex"][(q + 1) % nq] if defect == "max_lex_of_neighbour" else c["max_lex"][q]
        bound = states[(q + 1) % nq] if defect == "boundary_of_neighbour" else states[q]
        status, res = finish(states[q], bound, E[q], docs, lrow[q * stride:q * stride + lcnt[q]],
                             lscore[q * stride:q * stride + lcnt[q]], np.float32(ml), flags, w_e, w_l, need, per_doc, eps,
                             rows.size)
        base, ib = (0, 0) if defect == "no_query_stride" else (q * need, 2 * q)
        n_pool = res["rows"].size
        for k, v in res.items():
            planes[k][base:base + n_pool] = v
            planes[k][base + n_pool:base + need] = DOC_NONE if k == "docs" else 0
        info[ib] = n_pool if (status == 0 or defect == "status_keeps_pool") else 0
        info[ib + 1] = status
        sizes[ib // 2] = info[ib]
    # the batched MMR: one launch, pool sizes from the finish
    orders = []
    for q in range(nq):
        size = int(sizes[(q + 1) % nq] if defect == "pool_size_of_neighbour" else sizes[q])
        if c.get("diversify") and size:
            r = planes["rows"][q * need:q * need + size].astype(np.int64)
            order, _ = M.mmr_from_gram(c["sim"][np.ix_(r, r)], planes["comb"][q * need:q * need + size], c["k"], c["lam"])
            orders.append(order.astype(np.int64))
        else:
            orders.append(np.arange(size))
    # host: read out, hand back
    statuses = [int(info[2 * q + 1]) for q in range(nq)]
    if defect == "status_takes_chunk" and any(statuses):
        statuses = [max(statuses)] * nq
    out = []
    for q in range(nq):
        form = 3 if rule[q] else (0, 1, 2)[statuses[q]]
        if form == 0:
            o = orders[q] + q * need
            res = {k: v[o] for k, v in planes.items()}
        else:
            res = define_query(c, q)                         # the single path answers: the definition
        out.append(dict(res=res, form=form, size=int(sizes[q])))
    return out


# ---- designed chunks -----------------------------------------------------------------------------------------------------
EPS = CV.EPS


def _chunk(e, docs, lex, max_lex, w_e, w_l, need, per_doc, eps=EPS, a=None, allowed=None, **more):
    """lex: one sorted list of (row, score) per query"""
    e = f32(e)
    lex = [sorted(l) for l in lex]
    off = np.concatenate([[0], np.cumsum([len(l) for l in lex])]).astype(np.uint64)
    c = dict(e=e, a=e.copy() if a is None else f32(a), docs=None if docs is None else np.asarray(docs, np.uint32),
             lex_rows=np.asarray([r for l in lex for r, _ in l], np.uint64), lex_scores=f32([s for l in lex for _, s in l]),
             lex_offsets=off, max_lex=f32(max_lex), w_e=w_e, w_l=w_l, need=need, per_doc=per_doc, eps=eps, allowed=allowed)
    c.update(more)
    return c


def case_each_query_its_own_pairs():
    """three queries over the same cosines; each one's lexical row lifts a different document's far row to the top"""
    e = np.tile(np.linspace(0.9, 0.1, 9, dtype=np.float32), (3, 1))
    docs = [1, 1, 1, 2, 2, 2, 3, 3, 3]
    return _chunk(e, docs, [[(2, 4.0)], [(5, 4.0), (8, 1.0)], [(8, 4.0)]], [4.0, 4.0, 4.0], 0.3, 0.7, 3, 1)


def case_each_query_its_own_normaliser():
    """the same pair for both queries, max_lex 2 for the first and 8 for the second: row 5 leads only under the first"""
    e = np.tile(np.linspace(0.9, 0.4, 6, dtype=np.float32), (2, 1))
    return _chunk(e, [1, 2, 3, 4, 5, 6], [[(5, 2.0)], [(5, 2.0)]], [2.0, 8.0], 0.5, 0.5, 2, 1)


def case_a_flag_of_the_neighbour():
    """query 0's only pair (row 0) is one of its candidates; query 1's only pair (row 7) is far below ITS band and no
    candidate: pair 0 flagged for both drops row 7 from query 1's union.  Every row its own document, need 2 of 8"""
    e = np.array([np.linspace(0.9, 0.2, 8), np.linspace(0.9, 0.2, 8)], np.float32)
    return _chunk(e, np.arange(8) + 10, [[(0, 1.0)], [(7, 9.0)]], [1.0, 9.0], 0.3, 0.7, 2, 1)


def _sim(n, pairs):
    """a similarity matrix: 1 on the diagonal, 0.1 elsewhere, the given (i, j, value) entries on both sides"""
    sim = np.full((n, n), 0.1, np.float32)
    np.fill_diagonal(sim, 1.0)
    for i, j, v in pairs:
        sim[i, j] = sim[j, i] = v
    return sim


def case_short_pools_under_mmr():
    """three documents, per_doc 1, need 5: the documents run out and every pool holds 3 of its 5 slots (the column is the
    call's, so the pools of a chunk run short together); rows 0 and 1 are near duplicates, so the greedy order differs
    from the pool order for query 0 and not for query 1"""
    e = np.array([[0.9, 0.8, 0.7, 0.6, 0.5, 0.4], [0.1, 0.9, 0.2, 0.3, 0.8, 0.7]], np.float32)
    return _chunk(e, [1, 2, 3, 1, 2, 3], [[], []], [1.0, 1.0], 1.0, 0.0, 5, 1, diversify=True, k=3, lam=0.5,
                  sim=_sim(6, [(0, 1, 0.99), (1, 4, 0.2)]))


def case_boundary_tie_beside_a_decided_query():
    """query 0 is capped_vectors' rounding tie under the 5e-9 band (status 2).  A band below one ulp closes no group, so
    query 1 is decided the other way: its scores share one 22-bit bin (0.5 is a bin floor, the bin is 6.1e-5 wide), the
    collect leaves no row behind and there is nothing to bound.  Diversified with k = need: every pool row is picked, so a wrong pool is a wrong answer, and query 1's pool size matters"""
    t = CV.case_rounding_tie_outside_the_band()
    n = t["e"].size
    e1 = (np.float32(0.5) + np.arange(n, dtype=np.float32)[::-1] * np.float32(3.0e-6)).astype(np.float32)
    return _chunk(np.stack([t["e"], e1]), t["docs"], [[], []], [1.0, 1.0], t["w_e"], t["w_l"], t["need"], t["per_doc"],
                  eps=t["eps"], diversify=True, k=t["need"], lam=0.5, sim=_sim(n, [(0, 1, 0.95)]))


def case_lexical_limit_per_query():
    """a limit of 3 pairs per query (lex_cap): 2 + 3 + 4 pairs -- only the third query goes by rule, not the chunk"""
    e = np.tile(np.linspace(0.9, 0.1, 10, dtype=np.float32), (3, 1))
    lex = [[(8, 1.0), (9, 2.0)], [(5, 1.0), (6, 2.0), (7, 3.0)], [(1, 1.0), (2, 2.0), (3, 3.0), (4, 4.0)]]
    return _chunk(e, np.arange(10) // 2, lex, [2.0, 3.0, 4.0], 0.6, 0.4, 3, 1, lex_cap=3)


def case_negative_score_goes_alone():
    """query 1 carries a negative lexical score: by rule, alone; queries 0 and 2 are decided"""
    e = np.tile(np.linspace(0.9, 0.1, 6, dtype=np.float32), (3, 1))
    return _chunk(e, [1, 1, 2, 2, 3, 3], [[(5, 1.0)], [(4, -1.0)], [(3, 2.0)]], [1.0, 1.0, 2.0], 0.7, 0.3, 2, 1)


CASES = {f.__name__[5:]: f for f in (case_each_query_its_own_pairs, case_each_query_its_own_normaliser,
                                     case_a_flag_of_the_neighbour, case_short_pools_under_mmr,
                                     case_boundary_tie_beside_a_decided_query, case_lexical_limit_per_query,
                                     case_negative_score_goes_alone)}
# the forms every chunk must report
FORMS = {"each_query_its_own_pairs": [0, 0, 0], "each_query_its_own_normaliser": [0, 0], "a_flag_of_the_neighbour": [0, 0],
         "short_pools_under_mmr": [0, 0], "boundary_tie_beside_a_decided_query": [2, 0], "lexical_limit_per_query": [0, 0, 3],
         "negative_score_goes_alone": [0, 3, 0]}
# the designed chunk each defect must break, and what of it goes wrong: the answer, the forms, or the pool size handed to
# the Gram / greedy launches (a handed-back query is answered by the single path, so a defect in WHO is handed back
# shows in the forms only, and a pool size that is not zeroed costs launches, not answers)
BROKEN_BY = {"slice_of_query_0": ("each_query_its_own_pairs", "answer"),
             "offset_as_count": ("each_query_its_own_pairs", "answer"),
             "max_lex_of_neighbour": ("each_query_its_own_normaliser", "answer"),
             "flags_shared": ("a_flag_of_the_neighbour", "answer"),
             "no_query_stride": ("each_query_its_own_pairs", "answer"),
             "pool_size_of_neighbour": ("boundary_tie_beside_a_decided_query", "answer"),
             "boundary_of_neighbour": ("boundary_tie_beside_a_decided_query", "answer"),
             "status_takes_chunk": ("boundary_tie_beside_a_decided_query", "forms"),
             "status_keeps_pool": ("boundary_tie_beside_a_decided_query", "size"),
             "lex_limit_on_total": ("lexical_limit_per_query", "forms")}


def same(a, b):
    return CV.same(a, b)
