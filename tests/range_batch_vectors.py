"""Batched range search (rlr_search_range_batch; the batched tail of rust-local-rag_amd/csrc/range.hip), pure numpy: a
restatement of the device path behind either shared pass with plantable defects, and small designed cases that each
defect must break.  The definition is range_vectors.expect, query by query; tests/test_range_batch_vectors_cpu.py holds
the restatement to it, tests/test_gpu_range_batch.py holds the device to it.

The device path, per query q of a batch (tau[q] a number; a NaN anywhere in tau refuses the whole call):
  lo[q], hi[q] = range_vectors.bounds(tau[q], 2 eps)            one pair per query, computed once
  shared scan   the pass leaves query q's nominated scores at q * stride (stride = the rows rounded up to 4), NaN for a
                masked row.  Collect as the single path: NaN skipped (not counted in n_valid); count-only and a >= hi: a
                sure hit; else !(a < lo): re-scored, a hit iff e >= tau.  n_valid below the allowed rows: handed back.
  GEMM          the pass appends every (a, row) with a >= lo[q] to query q's list (a NaN lo takes every row) -- masked
                rows too: it reads every row -- and counts them in a word whose bit 31 a kernel sets when a workgroup's
                own list overflowed.  Finish: bit 31 set, or the count above CAND_CAP: handed back.  Else per candidate:
                mask bit clear: dropped; count-only and a >= hi: a sure hit; else re-scored, a hit iff e >= tau.
  both          n_hits counts every hit.  Rows wanted and n_hits > FINISH_MAX: handed back.  Else the keys (exact score,
                row) in result order, the first min(n_hits, cap) returned.
A query handed back is answered by the single-query path, i.e. the definition.  status: 0 decided, 1 candidates, 2 hits,
3 NaN nominations."""
import numpy as np

import range_vectors as R

F32 = np.float32
CAND_CAP = 8192               # batch_finish_capacity(): the candidates the GEMM keeps per query
FINISH_MAX = R.FINISH_MAX     # kRangeFinishMax: the keys a query keeps when rows are wanted
MARK = 1 << 31

DEFECTS = ("band_of_query_0", "overflow_ignored", "bit31_in_count", "masked_counted", "sure_hit_on_nomination",
           "n_total_clipped", "wrong_stride", "nan_tau_is_minus_inf")


def stride_of(n):
    return (n + 3) // 4 * 4


def per_query_bounds(taus, eps, defect=None):
    """[(lo, hi)] per query; the defect: the band of query 0 for everyone"""
    b = [R.bounds(t, F32(2.0) * F32(eps)) for t in taus]
    return [b[0]] * len(b) if defect == "band_of_query_0" else b


def gemm_lists(nominated, taus, eps, cand_cap=CAND_CAP, marked=(), defect=None):
    """what the nomination GEMM leaves in filter mode: per query the candidate rows in arrival order (here: ascending;
    only the first cand_cap are stored) and the count word (bit 31 for the queries in `marked`, whose list lost
    entries: the stored list is then cut to half)"""
    out = []
    for q, (lo, _) in enumerate(per_query_bounds(taus, eps, defect)):
        a = np.asarray(nominated[q], np.float32)
        with np.errstate(invalid="ignore"):
            cand = np.flatnonzero(a >= (F32(-np.inf) if np.isnan(lo) else lo))
        word = int(cand.size)
        stored = cand[:cand_cap]
        if q in marked:
            word |= MARK
            stored = stored[:stored.size // 2]
        out.append((stored, word))
    return out


def device_path(nominated, exact, eps, taus, cap, allowed=None, path="gemm", cand_cap=CAND_CAP, finish_max=FINISH_MAX, marked=(),
                defect=None):
    """nominated / exact: [Q, n] with |a - e| <= eps -> per query (rows u64, scores f32, n_total, status)"""
    nominated, exact = np.asarray(nominated, np.float32), np.asarray(exact, np.float32)
    taus = np.asarray(taus, np.float32).copy()
    if np.isnan(taus).any():
        if defect != "nan_tau_is_minus_inf":
            raise ValueError("a NaN in tau")
        taus[np.isnan(taus)] = -np.inf
    nq, n = exact.shape
    mask = R._allowed_mask(n, allowed)
    n_allowed = int(mask.sum())
    bnd = per_query_bounds(taus, eps, defect)
    lists = gemm_lists(nominated, taus, eps, cand_cap, marked, defect) if path == "gemm" else None
    # the shared scan's score arrays, flat: query q at q * stride (the floats between two arrays are nobody's: zeros here)
    stride = stride_of(n)
    flat = np.zeros(nq * stride, np.float32)
    for q in range(nq):
        flat[q * stride:q * stride + n] = np.where(mask, nominated[q], np.nan)
    out = []
    for q in range(nq):
        tau, (lo, hi), e = taus[q], bnd[q], exact[q]
        status = 0
        with np.errstate(invalid="ignore"):
            if path == "gemm":
                cand, word = lists[q]
                if defect == "bit31_in_count":
                    over = int(np.array([word], np.uint32).view(np.int32)[0]) > cand_cap   # a signed reading: the mark makes it negative
                elif defect == "overflow_ignored":
                    over = False
                else:
                    over = bool(word & MARK) or word > cand_cap
                if over:
                    status = 1
                a = nominated[q][cand]
                keep = np.ones(cand.size, bool) if defect == "masked_counted" else mask[cand]
            else:
                base = q * (n if defect == "wrong_stride" else stride)
                a_all = flat[base:base + n]
                valid = R.score_key(a_all) != 0
                if int(valid.sum()) < n_allowed:
                    status = 3
                cand = np.flatnonzero(valid & ~(a_all < lo))
                a = a_all[cand]
                keep = np.ones(cand.size, bool)
            sure = keep & (a >= hi) if (cap == 0 or defect == "sure_hit_on_nomination") else np.zeros(cand.size, bool)
            hit = keep & (sure | (e[cand] >= tau))
        key = np.where(sure & (cap != 0), a, e[cand])                    # (a key from a nomination only under the defect)
        n_hits = int(hit.sum())
        if status == 0 and cap and n_hits > finish_max:
            status = 2
        if status != 0:
            rows, n_total = R.expect(e, tau, cap, mask)
            out.append((rows, e[rows.astype(np.int64)], n_total, status))
            continue
        rows, key = cand[hit], key[hit]
        order = R.result_order(key, rows)[:cap]
        out.append((rows[order].astype(np.uint64), key[order].astype(np.float32), min(n_hits, finish_max) if defect == "n_total_clipped" else n_hits, 0))
    return out


def definition(exact, taus, cap, allowed=None):
    out = []
    for e, t in zip(np.asarray(exact, np.float32), np.asarray(taus, np.float32)):
        rows, n_total = R.expect(e, t, cap, allowed)
        out.append((rows, e[rows.astype(np.int64)], n_total))
    return out


# ---- designed cases: dict(nominated, exact, eps, taus, cap, allowed, path, + capacities / marks) ---------------------------
EPS = 1.0e-4


def _near(tau, offsets_in_eps):
    return (np.float64(tau) + np.asarray(offsets_in_eps, np.float64) * EPS).astype(np.float32)


def case_two_bands():
    """query 0 asks 0.9, query 1 asks 0.2: query 1's hits around 0.2 lie far below query 0's band"""
    e = np.array([[0.95, 0.5, 0.21, 0.1, 0.3], [0.1, 0.25, 0.95, 0.19, 0.2]], np.float32)
    return dict(nominated=e.copy(), exact=e, eps=EPS, taus=[0.9, 0.2], cap=10, path="gemm")


def case_more_candidates_than_the_list_holds():
    """six candidates against a list of four: the two hits that arrive last are beyond it -- handed back, not ignored"""
    e = np.array([[0.6, 0.7, 0.8, 0.9, 0.95, 0.99, 0.1], [0.1, 0.2, 0.3, 0.9, 0.1, 0.2, 0.3]], np.float32)
    return dict(nominated=e.copy(), exact=e, eps=EPS, taus=[0.5, 0.5], cap=10, path="gemm", cand_cap=4)


def case_marked_list():
    """query 1's count word carries the bit-31 mark and its stored list lost entries: handed back"""
    e = np.array([[0.9, 0.1, 0.2, 0.3], [0.9, 0.8, 0.7, 0.6]], np.float32)
    return dict(nominated=e.copy(), exact=e, eps=EPS, taus=[0.5, 0.5], cap=10, path="gemm", marked=(1,))


def case_hit_outside_the_mask():
    """the GEMM nominates row 0, the best hit of all, although the filter masks it: the finish drops it"""
    e = np.array([[0.95, 0.7, 0.3, 0.6, 0.9], [0.2, 0.6, 0.7, 0.1, 0.99]], np.float32)
    return dict(nominated=e.copy(), exact=e, eps=EPS, taus=[0.5, 0.5], cap=10, path="gemm", allowed=np.array([1, 2, 3]))


def case_sure_hits_with_rows_wanted():
    """rows 0 and 1 nominate far above hi in the order opposite to their exact scores: with rows wanted every candidate
    is re-scored and the exact scores order them; count-only they are sure hits and the count is the same"""
    e = np.array([[0.80001, 0.80002, 0.1], [0.3, 0.2, 0.1]], np.float32)
    a = e.copy()
    a[0, 0], a[0, 1] = 0.80005, 0.79995
    return dict(nominated=a, exact=e, eps=EPS, taus=[0.5, 0.25], cap=10, path="gemm")


def case_more_hits_than_the_finish_counts():
    """five hits against a finish of three, count-only: n_total is five"""
    e = np.array([[0.6, 0.9, 0.7, 0.1, 0.8, 0.55], [0.1, 0.2, 0.3, 0.4, 0.6, 0.1]], np.float32)
    return dict(nominated=e.copy(), exact=e, eps=EPS, taus=[0.5, 0.5], cap=0, path="gemm", finish_max=3)


def case_more_hits_than_the_finish_holds():
    """the same with rows wanted: handed back (status 2), all five returned"""
    c = case_more_hits_than_the_finish_counts()
    c["cap"] = 10
    return c


def case_five_rows_three_queries():
    """five rows: the score arrays of the shared scan are 8 floats apart, not 5"""
    e = np.array([[0.9, 0.1, 0.1, 0.1, 0.1], [0.1, 0.9, 0.1, 0.1, 0.1], [0.1, 0.1, 0.1, 0.1, 0.9]], np.float32)
    return dict(nominated=e.copy(), exact=e, eps=EPS, taus=[0.5, 0.5, 0.5], cap=10, path="scan")


def case_band_decisions_behind_the_scan():
    """a hit nominated 0.85 eps below tau (query 0) and, count-only, a miss nominated 0.5 eps above it (query 1)"""
    e = np.array([[0.9, _near(0.5, [0.05])[0], 0.1], [0.9, _near(0.7, [-0.4])[0], 0.1]], np.float32)
    a = e.copy()
    a[0, 1], a[1, 1] = _near(0.5, [-0.85])[0], _near(0.7, [0.5])[0]
    return dict(nominated=a, exact=e, eps=EPS, taus=[0.5, 0.7], cap=0, path="scan")


def case_nan_nomination_behind_the_scan():
    """query 1 nominates NaN for row 2 while its exact score is a hit: handed back (status 3), query 0 is decided"""
    e = np.array([[0.9, 0.3, 0.8, 0.6], [0.9, 0.3, 0.8, 0.6]], np.float32)
    a = e.copy()
    a[1, 2] = np.nan
    return dict(nominated=a, exact=e, eps=EPS, taus=[0.5, 0.5], cap=10, path="scan")


def case_nan_tau():
    """a NaN threshold in slot 1: the call is refused, nobody's rows are returned"""
    e = np.array([[0.9, 0.1], [0.2, 0.3]], np.float32)
    return dict(nominated=e.copy(), exact=e, eps=EPS, taus=[0.5, np.nan], cap=10, path="gemm")


CASES = {f.__name__[5:]: f for f in (case_two_bands, case_more_candidates_than_the_list_holds, case_marked_list,
                                     case_hit_outside_the_mask, case_sure_hits_with_rows_wanted,
                                     case_more_hits_than_the_finish_counts, case_more_hits_than_the_finish_holds,
                                     case_five_rows_three_queries, case_band_decisions_behind_the_scan,
                                     case_nan_nomination_behind_the_scan, case_nan_tau)}
# the designed case each defect must break
BROKEN_BY = {"band_of_query_0": "two_bands", "overflow_ignored": "more_candidates_than_the_list_holds",
             "bit31_in_count": "marked_list", "masked_counted": "hit_outside_the_mask",
             "sure_hit_on_nomination": "sure_hits_with_rows_wanted", "n_total_clipped": "more_hits_than_the_finish_counts",
             "wrong_stride": "five_rows_three_queries", "nan_tau_is_minus_inf": "nan_tau"}
# the status per query every case must report
STATUS = {"two_bands": [0, 0], "more_candidates_than_the_list_holds": [1, 0], "marked_list": [0, 1],
          "hit_outside_the_mask": [0, 0], "sure_hits_with_rows_wanted": [0, 0], "more_hits_than_the_finish_counts": [0, 0],
          "more_hits_than_the_finish_holds": [2, 0], "five_rows_three_queries": [0, 0, 0],
          "band_decisions_behind_the_scan": [0, 0], "nan_nomination_behind_the_scan": [0, 3]}


def run(case, defect=None):
    c = dict(case)
    return device_path(c.pop("nominated"), c.pop("exact"), c.pop("eps"), c.pop("taus"), c.pop("cap"), defect=defect, **c)
