"""Range search (rlr_search_range; rust-local-rag_amd/csrc/range.hip), pure numpy: the definition every layer is held
to, a restatement of the device path with plantable defects, and small designed cases that each defect must break.
tests/test_range_vectors_cpu.py holds these to each other; tests/test_gpu_range.py holds the device to `expect`.

The contract: over the allowed rows, row r is a hit iff e(r) >= tau in IEEE f32 comparison (e = the reference-order dot
product, oracle.scan): a NaN is never a hit, +Inf is one, -0 >= +0 holds.  n_total = the number of hits whatever cap
is; the hits in the library's result order (score descending by rlr_pack_result's key, row ascending); the first
min(n_total, cap) are returned; cap = 0 only counts."""
import numpy as np

F32 = np.float32
DEVICE_MAX = 65536            # RLR_RANGE_DEVICE_MAX
FINISH_MAX = 2048             # kRangeFinishMax: what the one-workgroup finish orders


def score_key(s):
    """common.h score_key: order-preserving f32 -> u32, NaN -> 0"""
    b = np.ascontiguousarray(s, dtype=np.float32).view(np.uint32).astype(np.uint64)
    nan = (b & 0x7FFFFFFF) > 0x7F800000
    k = np.where(b & 0x80000000, ~b & 0xFFFFFFFF, b | 0x80000000)
    return np.where(nan, 0, k).astype(np.uint64)


def result_order(scores, rows, higher_row_first=False):
    """indices into `scores` in the library's result order (packed key descending = score key desc, row asc)"""
    rows = np.asarray(rows, dtype=np.int64)
    return np.lexsort((-rows if higher_row_first else rows, -score_key(scores).astype(np.int64)))


def _allowed_mask(n, allowed):
    if allowed is None:
        return np.ones(n, bool)
    a = np.asarray(allowed)
    if a.dtype == bool:
        return a.copy()
    m = np.zeros(n, bool)
    m[a.astype(np.int64)] = True
    return m


def expect(exact_scores, tau, cap, allowed=None):
    """THE DEFINITION: threshold and order over oracle.scan -> (rows u64 [min(n_total, cap)], n_total)"""
    e = np.asarray(exact_scores, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        hit = _allowed_mask(e.size, allowed) & (e >= F32(tau))      # IEEE: NaN false, -0 >= +0 true
    rows = np.flatnonzero(hit)
    rows = rows[result_order(e[rows], rows)]
    return rows[:cap].astype(np.uint64), int(hit.sum())


# ---- the device path, restated ------------------------------------------------------------------------------------------
def step(x, up):
    """one ulp outward (kernels.h range_step): NaN and the infinity on that side stay"""
    x = F32(x)
    if np.isnan(x) or x == (np.inf if up else -np.inf):
        return x
    return np.nextafter(x, F32(np.inf if up else -np.inf), dtype=np.float32)


def bounds(tau, two_eps):
    """kernels.h range_bounds in the same f32 arithmetic: lo <= tau - 2 eps, hi >= tau + 2 eps in real arithmetic"""
    with np.errstate(invalid="ignore", over="ignore"):
        return step(F32(tau) - F32(two_eps), False), step(F32(tau) + F32(two_eps), True)


DEFECTS = ("band_zero", "strict_greater", "hi_without_margin", "count_from_nominations", "n_total_clipped",
           "ties_higher_row", "nan_rows_dropped", "masked_rows_counted", "negative_zero_below")


def device_path(nominated, exact, eps, tau, cap, allowed=None, defect=None):
    """nominated (a) and exact (e) scores with |a - e| <= eps over the allowed rows -> (rows, n_total, form).
    The scan leaves NaN for masked rows; collect: skip score_key(a) == 0 (not counted in n_valid); count-only and
    a >= hi: a sure hit; else !(a < lo): re-scored, a hit iff e >= tau; n_hits counts every hit.  Host: n_valid below
    the allowed rows -> form 2 (the definition answers); rows wanted and n_hits > min(cap, DEVICE_MAX) -> form 1 (n_total
    from the device, the rows the top-k answer at k = cap); else form 0."""
    a = np.asarray(nominated, dtype=np.float32).copy()
    e = np.asarray(exact, dtype=np.float32)
    tau = F32(tau)
    mask = _allowed_mask(e.size, allowed)
    if defect != "masked_rows_counted":
        a[~mask] = np.nan
    valid = score_key(a) != 0
    n_valid, n_allowed = int(valid.sum()), int(mask.sum())
    lo, hi = bounds(tau, F32(2.0) * F32(eps))
    if defect == "band_zero":
        lo = tau
    if defect == "hi_without_margin":
        hi = tau
    with np.errstate(invalid="ignore"):
        if defect == "strict_greater":
            is_hit = e > tau
        elif defect == "negative_zero_below":
            is_hit = ~np.isnan(e) & (score_key(e) >= score_key(tau))
        else:
            is_hit = e >= tau
        sure = valid & (a >= hi) if cap == 0 else np.zeros(e.size, bool)
        cand = valid & ~sure & ~(a < lo)
        hits = cand & is_hit
        n_hits = int(sure.sum() + hits.sum())
        if defect == "count_from_nominations":
            n_hits = int((valid & (a >= tau)).sum())
    if n_valid < n_allowed and defect != "nan_rows_dropped":
        rows, n_total = expect(e, tau, cap, mask)
        return rows, n_total, 2
    if cap and n_hits > min(cap, DEVICE_MAX):
        rows, _ = expect(e, tau, cap, mask)                    # the top-k answer at k = cap
        return rows, (min(n_hits, cap) if defect == "n_total_clipped" else n_hits), 1
    rows = np.flatnonzero(hits)
    rows = rows[result_order(e[rows], rows, higher_row_first=defect == "ties_higher_row")][:cap]
    return rows.astype(np.uint64), n_hits, 0


# ---- designed cases: (nominated, exact, eps, tau, cap, allowed) ------------------------------------------------------
EPS = 1.0e-4
TAU = F32(0.5)


def _near(offsets_in_eps):
    return (np.float64(TAU) + np.asarray(offsets_in_eps, np.float64) * EPS).astype(np.float32)


def case_hit_nominated_below():
    """row 1 is a hit (e just above tau) whose nomination lies 0.9 eps BELOW tau: only the band finds it; and a count
    taken from nominations misses it"""
    e = np.array([0.9, _near([0.05])[0], 0.1, -0.3], np.float32)
    a = e.copy()
    a[1] = _near([-0.85])[0]
    return a, e, EPS, TAU, 10, None


def case_miss_nominated_above_count_only():
    """count-only: row 2 is a miss (e 0.4 eps below tau) whose nomination lies 0.5 eps ABOVE tau: a sure-hit bound
    without its margin counts it unseen"""
    e = np.array([0.9, 0.7, _near([-0.4])[0], 0.1], np.float32)
    a = e.copy()
    a[2] = _near([0.5])[0]
    return a, e, EPS, TAU, 0, None


def case_score_equal_to_tau():
    """row 1 scores tau exactly: e >= tau holds, e > tau does not"""
    e = np.array([0.8, TAU, np.nextafter(TAU, F32(0)), 0.2], np.float32)
    return e.copy(), e, EPS, TAU, 10, None


def case_more_hits_than_cap():
    """five hits, cap 3: the first three in order, n_total 5 (form 1)"""
    e = np.array([0.6, 0.9, 0.7, 0.1, 0.8, 0.55], np.float32)
    return e.copy(), e, EPS, TAU, 3, None


def case_duplicates():
    """rows 1, 3 and 4 score the same: ascending row order among them"""
    e = np.array([0.6, 0.7, 0.9, 0.7, 0.7, 0.2], np.float32)
    return e.copy(), e, EPS, TAU, 10, None


def case_nan_nomination():
    """row 2's nomination is NaN while its exact score is a hit (a sum that overflowed in one order only): the device
    cannot know -- form 2, the exact form answers"""
    e = np.array([0.9, 0.3, 0.8, 0.6], np.float32)
    a = e.copy()
    a[2] = np.nan
    return a, e, EPS, TAU, 10, None


def case_hit_outside_the_mask():
    """row 0, the best hit of all, is outside the filter"""
    e = np.array([0.95, 0.7, 0.3, 0.6, 0.9], np.float32)
    return e.copy(), e, EPS, TAU, 10, np.array([1, 2, 3])


def case_negative_zero():
    """tau = +0 and a row scoring -0: -0 >= +0 holds (the score key of -0 lies below that of +0)"""
    e = np.array([0.5, -0.0, -1e-3, 0.0], np.float32)
    return e.copy(), e, EPS, F32(0.0), 10, None


CASES = {"hit_nominated_below": case_hit_nominated_below,
         "miss_nominated_above_count_only": case_miss_nominated_above_count_only,
         "score_equal_to_tau": case_score_equal_to_tau, "more_hits_than_cap": case_more_hits_than_cap,
         "duplicates": case_duplicates, "nan_nomination": case_nan_nomination,
         "hit_outside_the_mask": case_hit_outside_the_mask, "negative_zero": case_negative_zero}
# the designed case(s) each defect must break
BROKEN_BY = {"band_zero": ("hit_nominated_below",), "strict_greater": ("score_equal_to_tau",),
             "hi_without_margin": ("miss_nominated_above_count_only",),
             "count_from_nominations": ("hit_nominated_below", "miss_nominated_above_count_only"),
             "n_total_clipped": ("more_hits_than_cap",), "ties_higher_row": ("duplicates",),
             "nan_rows_dropped": ("nan_nomination",), "masked_rows_counted": ("hit_outside_the_mask",),
             "negative_zero_below": ("negative_zero",)}
