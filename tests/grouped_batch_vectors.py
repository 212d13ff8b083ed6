"""Batched grouped top-k (rlr_search_topk_grouped_batch; the batched tail of rust-local-rag_amd/csrc/group.hip), pure
numpy: the workspace rule and the chunk split as pure functions, a restatement of the shared-table device path with
plantable defects, and small designed cases that each defect must break.  The definition is grouped_vectors.expect, query
by query; tests/test_grouped_batch_vectors_cpu.py holds the restatement to it, tests/test_gpu_grouped_batch.py holds the
device to it.

The device path, for a chunk of queries behind one shared scan (query q's nominated scores at q * stride, NaN for a masked
row and for a NaN nomination):
  table    ONE key table for the chunk (open addressing, the document id of every row that is active for any query), a
           value plane per query: vals[(q * slots + slot) * per_doc + j] = the j-th largest packed nominated key
           (score key << 32 | ~row) of the slot's document BY QUERY q.  A row whose score is NaN for q has key 0 and is
           skipped for q only.
  heads    per query: t_g = the per_doc-th value of the row's document in q's plane (0: a smaller group, an untagged
           row); a row is a head when its packed key >= t_g; U = the floor of the 22-bit bin of the k-th head's key
           (-inf with fewer than k heads), from q's own histogram.
  collect  per query: rows with a >= max(t_g, U) - 2 eps in f32 arithmetic, by q's own t_g; more than CAND_CAP: status 1.
  finish   per query: exact packed order, rank inside the document among the candidates, accept below per_doc, first k;
           a short answer while allowed rows have NaN nominations: status 2.
A query whose status is not 0 is handed to the single-query path, i.e. the definition; its neighbours stay decided."""
import numpy as np

import grouped_vectors as G
import range_vectors as R

F32 = np.float32
DOC_NONE = G.DOC_NONE
CAND_CAP = 2048               # kGroupCap: the candidates a query's finish holds
MAX_WIDTH = 8

DEFECTS = ("plane_of_query_0", "plane_stride", "nan_skips_all", "hist_added", "tg_of_neighbour", "overflow_unflagged",
           "overflow_takes_chunk", "width_ignores_per_doc")


# ---- the workspace rule and the split -----------------------------------------------------------------------------------
def table_bits(n_allowed):
    """index_grouped.hip group_table_bits: twice the documents the table can meet, at least 1024 slots"""
    bits = 10
    while bits < 32 and (1 << bits) < 2 * n_allowed:
        bits += 1
    return bits


def stride_of(n):
    return (n + 3) // 4 * 4


def workspace_bytes(w, n_rows, n_allowed, per_doc):
    """key table + w value planes + w t_g arrays + w score arrays"""
    slots = 1 << table_bits(n_allowed)
    return 4 * slots + w * (8 * per_doc * slots + 8 * n_rows + 4 * stride_of(n_rows))


def chunk_width(n_rows, row_bytes, n_allowed, per_doc, defect=None):
    """the largest w in 2..8 whose workspace stays at or below the bytes of the rows; 0: none (by rule, one by one)"""
    if defect == "width_ignores_per_doc":
        per_doc = 1
    for w in range(MAX_WIDTH, 1, -1):
        if workspace_bytes(w, n_rows, n_allowed, per_doc) <= n_rows * row_bytes:
            return w
    return 0


def split(n_queries, w):
    """the chunk sizes of a batch: ceil(n / w) consecutive chunks, the remainder spread evenly (9 -> 5 + 4); a chunk of
    one query goes one by one.  w < 2: every query one by one."""
    w = min(w, n_queries)
    if w < 2:
        return [1] * n_queries
    n_chunks = -(-n_queries // w)
    return [n_queries // n_chunks + (1 if i < n_queries % n_chunks else 0) for i in range(n_chunks)]


def forms_by_rule(n_queries, w):
    """(queries the shared chunks take, queries that go by rule) for a batch at chunk width w"""
    sizes = split(n_queries, w)
    return sum(s for s in sizes if s >= 2), sum(s for s in sizes if s < 2)


# ---- the device path of one chunk, restated ------------------------------------------------------------------------------
def _hash(doc, bits):
    return ((int(doc) * 0x9E3779B1) & 0xFFFFFFFF) >> (32 - bits)


class _Table:
    def __init__(self, bits):
        self.bits, self.keys = bits, {}

    def find(self, doc, insert=False):
        mask = (1 << self.bits) - 1
        h = _hash(doc, self.bits)
        for _ in range(mask + 1):
            if self.keys.get(h, DOC_NONE) == doc:
                return h
            if h not in self.keys:
                if not insert:
                    return None
                self.keys[h] = int(doc)
                return h
            h = (h + 1) & mask
        return None


def _key_score(key):
    key = int(key)
    b = (key & 0x7FFFFFFF) if key & 0x80000000 else (~key & 0xFFFFFFFF)
    return np.array([b], np.uint32).view(np.float32)[0]


def device_path(nominated, exact, docs, k, per_doc, eps, allowed=None, cand_cap=CAND_CAP, defect=None):
    """nominated / exact: [Q, n] with |a - e| <= eps -> per query (rows u64, status)"""
    nominated, exact = np.asarray(nominated, np.float32), np.asarray(exact, np.float32)
    nq, n = exact.shape
    docs = G._docs(docs, n)
    mask = R._allowed_mask(n, allowed)
    n_allowed = int(mask.sum())
    stride = stride_of(n)
    flat = np.zeros(nq * stride, np.float32)
    for q in range(nq):
        flat[q * stride:q * stride + n] = np.where(mask, nominated[q], np.nan)
    keys = np.stack([R.score_key(flat[q * stride:q * stride + n]) for q in range(nq)]).astype(np.uint64)
    packed = (keys << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - np.arange(n, dtype=np.uint64))
    bits = table_bits(n_allowed)
    slots = 1 << bits
    table = _Table(bits)
    vals = {}

    def at(q, slot, j):
        return (slot * per_doc + j) if defect == "plane_stride" else ((q * slots + slot) * per_doc + j)

    # the rounds: round j over every row, then round j + 1 (bounds come from the launch before)
    for j in range(per_doc):
        new = dict(vals)
        for row in range(n):
            if docs[row] == DOC_NONE:
                continue
            if defect == "nan_skips_all" and (keys[:, row] == 0).any():
                continue
            for q in range(nq):
                if keys[q, row] == 0:
                    continue
                slot = table.find(docs[row], insert=j == 0) if j == 0 else table.find(docs[row])
                if slot is None:
                    continue
                v = int(packed[q, row])
                if j > 0 and not v < vals.get(at(q, slot, j - 1), 0):
                    continue
                new[at(q, slot, j)] = max(new.get(at(q, slot, j), 0), v)
        vals = new
    # heads: t_g per row and query, the head keys per query
    tg = np.zeros((nq, n), np.uint64)
    head_keys = []
    for q in range(nq):
        plane = 0 if defect == "plane_of_query_0" else q
        hk = []
        for row in range(n):
            if keys[q, row] == 0:
                continue
            if docs[row] != DOC_NONE:
                slot = table.find(docs[row])
                tg[q, row] = vals.get(at(plane, slot, per_doc - 1), 0) if slot is not None else 0
            if int(packed[q, row]) >= int(tg[q, row]):
                hk.append(int(keys[q, row]))
        head_keys.append(hk)
    two_eps = F32(2.0) * F32(eps)
    out = []
    for q in range(nq):
        hk = list(head_keys[q])
        if defect == "hist_added" and q > 0:
            hk += head_keys[q - 1]
        hk.sort(reverse=True)
        u = F32(-np.inf)
        if len(hk) >= k:
            u = _key_score(hk[k - 1] & ~0x3FF)
            if np.isnan(u):
                u = F32(-np.inf)
        tq = tg[(q + 1) % nq] if defect == "tg_of_neighbour" else tg[q]
        a = flat[q * stride:q * stride + n]
        cand = []
        with np.errstate(invalid="ignore", over="ignore"):
            for row in range(n):
                if keys[q, row] == 0:
                    continue
                tkey = int(tq[row]) >> 32
                t = _key_score(tkey) if tkey else F32(-np.inf)
                thr = F32(max(t, u)) - two_eps
                if not a[row] < thr:
                    cand.append(row)
        status = 0
        if len(cand) > cand_cap:
            if defect == "overflow_unflagged":
                cand = cand[:cand_cap]                        # (the slots are handed out in arrival order: here ascending)
            else:
                status = 1
        cand = np.asarray(cand, np.int64)
        rows = G.walk(cand[R.result_order(exact[q][cand], cand)], docs, k, per_doc)
        n_valid = int((keys[q] != 0).sum())
        if status == 0 and rows.size < min(k, n_allowed) and n_valid < n_allowed:
            status = 2
        out.append((rows, status))
    if defect == "overflow_takes_chunk" and any(s for _, s in out):
        worst = max(s for _, s in out)
        out = [(r, worst) for r, _ in out]
    # a handed-back query is answered by the single-query path: the definition
    return [(r if s == 0 else definition(exact[q:q + 1], docs, k, per_doc, allowed)[0], s) for q, (r, s) in enumerate(out)]


def definition(exact, docs, k, per_doc, allowed=None):
    """THE DEFINITION per query.  (The packed order of the library, in which +0 sorts above -0, is grouped_vectors' order
    on every score the designed cases use.)"""
    return [G.expect(e, docs, k, per_doc, allowed) for e in np.asarray(exact, np.float32)]


# ---- designed cases: dict(nominated, exact, docs, k, per_doc, eps, + allowed / cand_cap) -------------------------------
EPS = 1.0e-4


def case_two_queries_two_planes():
    """query 0 scores every row far above query 1: read through query 0's plane, query 1's rows are all below `their`
    document's best and none is a head, none a candidate"""
    e = np.array([[0.9, 0.8, 0.7, 0.6], [0.1, 0.2, 0.3, 0.4]], np.float32)
    return dict(nominated=e.copy(), exact=e, docs=np.array([1, 1, 2, 2], np.uint32), k=2, per_doc=1, eps=EPS)


def case_three_planes_two_deep():
    """three queries, per_doc = 2: with one plane for all, the second-best of a document is the second-best over ALL
    queries and the low-scoring queries lose their rows"""
    e = np.array([[0.95, 0.90, 0.85, 0.5, 0.4], [0.30, 0.35, 0.25, 0.6, 0.1], [0.10, 0.15, 0.20, 0.05, 0.02]], np.float32)
    return dict(nominated=e.copy(), exact=e, docs=np.array([7, 7, 7, 8, 8], np.uint32), k=3, per_doc=2, eps=EPS)


def case_nan_for_one_query():
    """row 0 nominates NaN for query 0 and is query 1's best row, in a document of two: skipped for query 1 too, the
    document's t_g falls to row 1, both of its rows count as heads, U rises above document B and row 2 is never collected"""
    e = np.array([[0.05, 0.2, 0.7, 0.6], [0.9, 0.8, 0.5, 0.1]], np.float32)
    a = e.copy()
    a[0, 0] = np.nan
    return dict(nominated=a, exact=e, docs=np.array([1, 1, 2, 3], np.uint32), k=2, per_doc=1, eps=EPS)


def case_high_and_low_heads():
    """every row its own document; query 0's heads are all far above query 1's: counted into query 1's histogram they
    put its U above every row it has"""
    e = np.array([[0.9, 0.8, 0.7], [0.3, 0.2, 0.1]], np.float32)
    return dict(nominated=e.copy(), exact=e, docs=np.array([4, 5, 6], np.uint32), k=2, per_doc=1, eps=EPS)


def case_neighbours_thresholds():
    """query 0 scores low, query 1 high, k above the number of documents (U = -inf): with query 1's t_g as its
    threshold, query 0 collects nothing"""
    e = np.array([[0.1, 0.2, 0.3, 0.4], [0.9, 0.8, 0.7, 0.6]], np.float32)
    return dict(nominated=e.copy(), exact=e, docs=np.array([1, 1, 2, 2], np.uint32), k=3, per_doc=1, eps=EPS)


def case_more_candidates_than_the_finish_holds():
    """six untagged rows of query 0 inside one band, the best ones last, against a finish of four: query 0 is handed
    back (status 1); query 1 has two candidates and stays decided"""
    e = np.array([[0.50000, 0.50001, 0.50002, 0.50003, 0.50004, 0.50005, 0.1], [0.9, 0.1, 0.1, 0.1, 0.1, 0.1, 0.8]], np.float32)
    return dict(nominated=e.copy(), exact=e, docs=None, k=2, per_doc=1, eps=EPS, cand_cap=4)


def case_short_answer_with_a_nan():
    """query 1 nominates NaN for row 2 and k asks for more rows than its numbers fill: handed back (status 2), the NaN
    row's exact score decides; query 0 is decided"""
    e = np.array([[0.9, 0.3, 0.8, 0.6], [0.9, 0.3, 0.8, 0.6]], np.float32)
    a = e.copy()
    a[1, 2] = np.nan
    return dict(nominated=a, exact=e, docs=None, k=4, per_doc=1, eps=EPS)


def case_band_decisions():
    """decoys nominated above X inside one document (query 0) and across documents (query 1): the 2 eps band collects X"""
    a0, e0, d0, _, _, _ = G.case_decoy_document()
    e1 = np.array([0.70000, 0.90, 0.85, 0.69999, 0.69998, 0.69997, 0.2, 0.1, 0.05], np.float32)
    a1 = e1.astype(np.float64)
    a1[0] -= 0.9 * EPS
    a1[3:6] += 0.9 * EPS
    return dict(nominated=np.stack([a0, a1.astype(np.float32)]), exact=np.stack([e0, e1]), docs=d0, k=3, per_doc=1, eps=EPS)


def case_five_rows_three_queries():
    """five rows: the score arrays are 8 floats apart; a filter leaves rows 0, 2 and 4"""
    e = np.array([[0.9, 0.1, 0.2, 0.1, 0.3], [0.1, 0.9, 0.4, 0.1, 0.2], [0.1, 0.1, 0.1, 0.95, 0.9]], np.float32)
    return dict(nominated=e.copy(), exact=e, docs=np.array([1, 1, 2, 2, DOC_NONE], np.uint32), k=2, per_doc=1, eps=EPS,
                allowed=np.array([0, 2, 4]))


CASES = {f.__name__[5:]: f for f in (case_two_queries_two_planes, case_three_planes_two_deep, case_nan_for_one_query,
                                     case_high_and_low_heads, case_neighbours_thresholds,
                                     case_more_candidates_than_the_finish_holds, case_short_answer_with_a_nan,
                                     case_band_decisions, case_five_rows_three_queries)}
# the designed case each defect of the device path must break (width_ignores_per_doc: the workspace rule, held separately)
BROKEN_BY = {"plane_of_query_0": "two_queries_two_planes", "plane_stride": "three_planes_two_deep",
             "nan_skips_all": "nan_for_one_query", "hist_added": "high_and_low_heads",
             "tg_of_neighbour": "neighbours_thresholds", "overflow_unflagged": "more_candidates_than_the_finish_holds",
             "overflow_takes_chunk": "more_candidates_than_the_finish_holds"}
# the status per query every case must report
STATUS = {"two_queries_two_planes": [0, 0], "three_planes_two_deep": [0, 0, 0], "nan_for_one_query": [0, 0],
          "high_and_low_heads": [0, 0], "neighbours_thresholds": [0, 0], "more_candidates_than_the_finish_holds": [1, 0],
          "short_answer_with_a_nan": [0, 2], "band_decisions": [0, 0], "five_rows_three_queries": [0, 0, 0]}


def run(case, defect=None):
    c = dict(case)
    return device_path(c.pop("nominated"), c.pop("exact"), c.pop("docs"), c.pop("k"), c.pop("per_doc"), c.pop("eps"),
                       defect=defect, **c)
