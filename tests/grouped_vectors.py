"""Grouped top-k (rlr_search_topk_grouped; rust-local-rag_amd/csrc/group.hip), pure numpy: the model every layer is held
to, a restatement of the device's fast path with plantable defects, and small designed cases that each defect must break.
tests/test_grouped_vectors_cpu.py holds these to each other; tests/test_gpu_grouped.py holds the device to `expect`.

The contract: take the allowed rows in the library's result order (reference-order score descending, row ascending, NaN
last, +0 = -0), walk it, accept a row unless per_doc rows of its document are already accepted, stop at k.  A row tagged
DOC_NONE -- and every row of an index without a column -- is a group of its own and is never capped."""
import numpy as np

DOC_NONE = 0xFFFFFFFF


def result_order(scores, rows=None, higher_row_first=False):
    """indices into `scores` in the library's result order; rows[i] = the row number of entry i (default: i)"""
    s = np.asarray(scores, dtype=np.float32).astype(np.float64)
    rows = np.arange(s.size, dtype=np.int64) if rows is None else np.asarray(rows, dtype=np.int64)
    nan = np.isnan(s)
    # (-s: +0 and -0 compare equal; NaN is ordered by the flag, its -s replaced by a number)
    return np.lexsort((-rows if higher_row_first else rows, np.where(nan, 0.0, -s), nan))


def _docs(docs, n):
    return np.full(n, DOC_NONE, np.uint32) if docs is None else np.asarray(docs, dtype=np.uint32)


def walk(order, docs, k, per_doc, cap_untagged=False):
    """the walk over `order` (row numbers): accept unless per_doc rows of the document are already accepted, stop at k"""
    taken, out = {}, []
    for r in order:
        d = int(docs[r])
        if d != DOC_NONE or cap_untagged:
            if taken.get(d, 0) >= per_doc:
                continue
            taken[d] = taken.get(d, 0) + 1
        out.append(int(r))
        if len(out) == k:
            break
    return np.asarray(out, dtype=np.uint64)


def expect(exact_scores, docs, k, per_doc, allowed=None):
    """THE MODEL: the result rows.  exact_scores: oracle.scan(rows, q); docs: u32 per row or None (no column); allowed:
    row numbers or a boolean mask, None = every row"""
    e = np.asarray(exact_scores, dtype=np.float32)
    docs = _docs(docs, e.size)
    rows = np.arange(e.size) if allowed is None else np.flatnonzero(allowed) if np.asarray(allowed).dtype == bool \
        else np.unique(np.asarray(allowed, dtype=np.int64))
    return walk(rows[result_order(e[rows], rows)], docs, k, per_doc)


def expect_union(exact_scores, docs, k, per_doc, allowed=None):
    """the second statement: the top k of the union of every group's top per_doc rows"""
    e = np.asarray(exact_scores, dtype=np.float32)
    docs = _docs(docs, e.size)
    rows = np.arange(e.size) if allowed is None else np.unique(np.asarray(allowed, dtype=np.int64))
    union = [rows[docs[rows] == DOC_NONE]]
    for d in np.unique(docs[rows]):
        if d != DOC_NONE:
            g = rows[docs[rows] == d]
            union.append(g[result_order(e[g], g)][:per_doc])
    u = np.concatenate(union)
    return u[result_order(e[u], u)][:k].astype(np.uint64)


# ---- the device's fast path, restated -------------------------------------------------------------------------------
# Defects that can change an answer.  Dropping t_g or U from max(t_g, U) is not among them: either only LOWERS the
# threshold, so the candidates are a superset and the finish returns the same rows (HARMLESS; held to that).  The unsafe
# way to ignore t_g is in the heads -- every row counted as a head puts U above documents that must answer.
DEFECTS = ("band_eps", "heads_ignore_tg", "ties_higher_row", "untagged_capped", "rank_by_nominated")
HARMLESS = ("threshold_ignores_tg", "threshold_ignores_u")


def fast_path(nominated, exact, docs, k, per_doc, eps, defect=None):
    """nominated (a) and exact (e) scores with |a - e| <= eps -> the rows the device path returns.
    per-group ranks by nominated key, t_g = the group's per_doc-th; heads = every group's top per_doc + the untagged rows;
    U = the k-th head (-inf with fewer); candidates a >= max(t_g, U) - 2 eps; exact order, rank inside the group among the
    candidates, accept below per_doc, first k."""
    a = np.asarray(nominated, dtype=np.float32).astype(np.float64)
    e = np.asarray(exact, dtype=np.float32)
    n = a.size
    docs = _docs(docs, n)
    tagged = docs != DOC_NONE if defect != "untagged_capped" else np.ones(n, bool)
    valid = ~np.isnan(a)
    nom_order = [r for r in result_order(a) if valid[r]]
    tg = np.full(n, -np.inf)
    head = np.zeros(n, bool)
    seen = {}
    for r in nom_order:                                   # descending nominated key
        if not tagged[r]:
            head[r] = True
            continue
        c = seen.get(int(docs[r]), 0)
        seen[int(docs[r])] = c + 1
        if c < per_doc:
            head[r] = True
        if c == per_doc - 1:
            tg[docs == docs[r]] = a[r]
    if defect != "untagged_capped":
        tg[~tagged] = -np.inf
    if defect == "heads_ignore_tg":
        head = valid.copy()
    hv = np.sort(a[head])[::-1]
    U = hv[k - 1] if hv.size >= k else -np.inf
    band = eps if defect == "band_eps" else 2.0 * eps
    t = np.maximum(tg, U)
    if defect == "threshold_ignores_tg":
        t = np.full(n, U)
    if defect == "threshold_ignores_u":
        t = tg
    cand = np.flatnonzero(valid & (a >= t - band))
    key = a if defect == "rank_by_nominated" else e
    order = cand[result_order(key[cand], cand, higher_row_first=defect == "ties_higher_row")]
    if defect == "rank_by_nominated":                     # group ranks from the nominated order, emitted in exact order
        keep = set(walk(order, docs, n, per_doc).tolist())
        kept = np.asarray([r for r in cand if r in keep], dtype=np.int64)
        return kept[result_order(e[kept], kept)][:k].astype(np.uint64)
    return walk(order, docs, k, per_doc, cap_untagged=defect == "untagged_capped")


# ---- designed cases: (nominated, exact, docs, k, per_doc, eps) --------------------------------------------------------
EPS = 1.0e-4


def case_decoy_document():
    """document 5 holds X (row 3) and decoys: X is the document's best by exact score, a decoy by nomination -- nominated
    order and exact order disagree INSIDE the group -- and X's nominated score lies between t_g - 2 eps and t_g - eps"""
    e = np.array([0.30, 0.31, 0.32, 0.80000, 0.79999, 0.79998, 0.79997, 0.50, 0.49], np.float32)
    a = e.astype(np.float64).copy()
    a[3] -= 0.9 * EPS
    a[4:7] += 0.9 * EPS
    docs = np.array([1, 2, 3, 5, 5, 5, 5, 6, 6], np.uint32)
    return a.astype(np.float32), e, docs, 3, 1, EPS


def case_kth_across_documents():
    """every row its own document, k = 3: X (row 0) is the third by exact score; decoys just below it nominate above it,
    so U comes from decoys and X's nominated score lies between U - 2 eps and U - eps"""
    e = np.array([0.70000, 0.90, 0.85, 0.69999, 0.69998, 0.69997, 0.2, 0.1], np.float32)
    a = e.astype(np.float64).copy()
    a[0] -= 0.9 * EPS
    a[3:6] += 0.9 * EPS
    return a.astype(np.float32), e, np.arange(10, 18, dtype=np.uint32), 3, 1, EPS


def case_long_document():
    """one document of 50 rows close to the query, five others far below: with every row counted as a head, U sits
    inside the long document and the other documents' rows are never collected"""
    e = np.concatenate([np.linspace(0.95, 0.90, 50), [0.5, 0.4, 0.3, 0.2, 0.1]]).astype(np.float32)
    docs = np.concatenate([np.full(50, 9), np.arange(20, 25)]).astype(np.uint32)
    return e.copy(), e, docs, 5, 1, EPS


def case_duplicates():
    """equal scores inside one document (rows 1, 2) and across documents (rows 4, 5): the lower row wins"""
    e = np.array([0.1, 0.6, 0.6, 0.2, 0.5, 0.5, 0.05], np.float32)
    docs = np.array([1, 2, 2, 3, 4, 5, 6], np.uint32)
    return e.copy(), e, docs, 2, 1, EPS


def case_untagged_rows():
    """untagged rows are groups of their own: the three best rows are all DOC_NONE and all come back"""
    e = np.array([0.9, 0.8, 0.7, 0.6, 0.5], np.float32)
    docs = np.array([DOC_NONE, DOC_NONE, DOC_NONE, 1, 1], np.uint32)
    return e.copy(), e, docs, 4, 1, EPS


CASES = {"decoy_document": case_decoy_document, "kth_across_documents": case_kth_across_documents,
         "long_document": case_long_document, "duplicates": case_duplicates, "untagged_rows": case_untagged_rows}
# the designed case each defect must break
BROKEN_BY = {"band_eps": ("decoy_document", "kth_across_documents"), "heads_ignore_tg": ("long_document",),
             "ties_higher_row": ("duplicates",), "untagged_capped": ("untagged_rows",),
             "rank_by_nominated": ("decoy_document",)}
