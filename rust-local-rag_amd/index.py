"""GpuIndex: numpy-facing wrapper of the rlr_index C handle (include/rlr_gpu.h)."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _native as N


def _f32(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float32)


def _u64(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.uint64)


DOC_NONE = 0xFFFFFFFF  # RLR_DOC_NONE: a row that belongs to no document


def _u32(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.uint32)


def _u32ptr(a: np.ndarray):
    return a.ctypes.data_as(N.u32p)


def _fp(a: np.ndarray):
    return a.ctypes.data_as(N.f32p)


def _up(a: np.ndarray):
    return a.ctypes.data_as(N.u64p)


@dataclass
class Profile:
    n_searches: int
    n_scan_launches: int
    scan_ms: float
    select_ms: float
    rescore_ms: float
    total_ms: float
    scan_bytes: int
    n_candidates: int
    n_retries: int
    n_batches: int = 0
    n_batch_queries: int = 0
    batch_gemm_ms: float = 0.0
    batch_other_ms: float = 0.0
    batch_gemm_bytes: int = 0
    batch_gemm_flops: float = 0.0
    n_batch_fallbacks: int = 0
    batch_main_ms: float = 0.0
    batch_main_bytes: int = 0
    batch_main_flops: float = 0.0
    n_mmr: int = 0
    mmr_ms: float = 0.0
    n_batches_without_image: int = 0
    n_f16_range_fallbacks: int = 0


class RowFilter:
    """A fixed set of rows of one GpuIndex (rlr_filter): made by GpuIndex.filter_rows / filter_ranges, passed as `filter=`
    to the search calls.  Immutable; stale (every filtered call raises RLR_E_INVALID) once the index is mutated.  A
    context manager; close() releases the device memory."""

    def __init__(self, index: "GpuIndex", handle: C.c_void_p):
        self._L = index._L
        self._index = index  # (keeps the index alive as long as the filter)
        self._h = handle

    @property
    def handle(self) -> C.c_void_p:
        return self._h

    def info(self) -> dict:
        """index_rows, n_allowed, path ("list" / "scan": how searches with this filter run), stale"""
        rows, allowed, path, stale = C.c_uint64(), C.c_uint64(), C.c_int32(), C.c_int32()
        N.check(self._L.rlr_filter_info(self._h, C.byref(rows), C.byref(allowed), C.byref(path), C.byref(stale)))
        return {"index_rows": int(rows.value), "n_allowed": int(allowed.value), "path": ("list", "scan")[path.value],
                "stale": bool(stale.value)}

    def read(self):
        """the filter's DEVICE copies, copied back: (mask u64 [ceil(index_rows / 64)], list u32 [n_allowed])"""
        info = self.info()
        mask = np.zeros((info["index_rows"] + 63) // 64, dtype=np.uint64)
        rows = np.zeros(info["n_allowed"], dtype=np.uint32)
        N.check(self._L.rlr_filter_read(self._h, _up(mask) if mask.size else None,
                                        rows.ctypes.data_as(N.u32p) if rows.size else None))
        return mask, rows

    def set_path(self, path: str) -> None:
        """measurement hook (tools/bench_filtered.py): "list" or "scan" from now on; results do not depend on it"""
        N.check(self._L.rlr_filter_set_path(self._h, {"list": 0, "scan": 1}[path]))

    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h:
            self._L.rlr_filter_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class GpuIndex:
    """Dense chunk-embedding matrix resident in HBM + the search entry points."""

    def __init__(self, dim: int, dtype: str = "f32", device: int = 0):
        self._L = N.lib()
        self._h = C.c_void_p()
        code = {"f32": N.RLR_F32, "f16": N.RLR_F16}[dtype]
        N.check(self._L.rlr_index_create(dim, code, device, C.byref(self._h)))
        self.dim = dim
        self.dtype = dtype
        self.device = device

    # -- lifetime ---------------------------------------------------------
    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h:
            self._L.rlr_index_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @property
    def handle(self) -> C.c_void_p:
        return self._h

    def __len__(self) -> int:
        n = C.c_uint64()
        N.check(self._L.rlr_index_info(self._h, C.byref(n), None, None, None))
        return int(n.value)

    # -- mutation -----------------------------------------------------------
    def upload(self, rows, normalize: bool = False) -> None:
        rows = _f32(rows).reshape(-1, self.dim) if np.size(rows) else np.zeros((0, self.dim), np.float32)
        N.check(self._L.rlr_index_upload(self._h, _fp(rows), rows.shape[0], int(normalize)))

    def append(self, rows, normalize: bool = False) -> int:
        rows = _f32(rows).reshape(-1, self.dim)
        first = C.c_uint64()
        N.check(self._L.rlr_index_append(self._h, _fp(rows), rows.shape[0], int(normalize), C.byref(first)))
        return int(first.value)

    def delete_rows(self, rows) -> None:
        rows = _u64(rows).ravel()
        if rows.size:
            N.check(self._L.rlr_index_delete_rows(self._h, _up(rows), rows.size))

    def reserve(self, n_rows: int) -> None:
        N.check(self._L.rlr_index_reserve(self._h, n_rows))

    def fill_synthetic(self, n_rows: int, seed: int, row0: int = 0, n_clusters: int = 0) -> None:
        N.check(self._L.rlr_index_fill_synthetic(self._h, n_rows, row0, seed, n_clusters))

    def enable_batch_image(self, on: bool = True, single_query: bool = False, q8: bool = False) -> None:
        """Optional nomination copies of the rows (results never change, only the bytes the scan streams):
        on            binary16 image for the batched matrix-core path (dim * 2 bytes per row)
        single_query  single queries over f32 rows nominate from that image too (half the scan bytes)
        q8            8-bit copy + per-row scale for single queries (a quarter of the scan bytes; dim * 1 + 4 B/row)"""
        flags = (1 if (on or single_query) else 0) | (2 if single_query else 0) | (4 if q8 else 0)
        N.check(self._L.rlr_index_enable_batch_image(self._h, flags))

    # -- row filters -----------------------------------------------------------
    def filter_rows(self, rows) -> RowFilter:
        """the given rows (any order, duplicates ignored) as a RowFilter"""
        rows = _u64(rows).ravel()
        h = C.c_void_p()
        N.check(self._L.rlr_filter_create_rows(self._h, _up(rows) if rows.size else None, rows.size, C.byref(h)))
        return RowFilter(self, h)

    def filter_ranges(self, ranges) -> RowFilter:
        """the union of the (first, count) ranges as a RowFilter (a document is a contiguous run of rows)"""
        r = _u64(list(ranges)).reshape(-1, 2) if len(ranges) else np.zeros((0, 2), np.uint64)
        first, count = np.ascontiguousarray(r[:, 0]), np.ascontiguousarray(r[:, 1])
        h = C.c_void_p()
        N.check(self._L.rlr_filter_create_ranges(self._h, _up(first) if r.shape[0] else None,
                                                 _up(count) if r.shape[0] else None, r.shape[0], C.byref(h)))
        return RowFilter(self, h)

    # -- document column ---------------------------------------------------------
    def set_documents(self, doc_of_row) -> None:
        """the whole column at once: one uint32 document id per row (DOC_NONE: no document)"""
        d = _u32(doc_of_row).ravel()
        N.check(self._L.rlr_index_set_documents(self._h, _u32ptr(d) if d.size else None, d.size))

    def tag_rows(self, first: int, count: int, doc: int) -> None:
        """rows [first, first + count) belong to document `doc` from now on"""
        N.check(self._L.rlr_index_tag_rows(self._h, first, count, doc))

    def get_documents(self, first: int = 0, count: "int | None" = None) -> np.ndarray:
        """the document ids of rows [first, first + count) (to the end by default); DOC_NONE everywhere before any tag"""
        if count is None:
            count = len(self) - first
        out = np.zeros(max(count, 0), dtype=np.uint32)
        N.check(self._L.rlr_index_get_documents(self._h, first, count, _u32ptr(out) if out.size else None))
        return out

    def filter_documents(self, docs) -> RowFilter:
        """every row tagged with one of these document ids as a RowFilter, built on the device from the column"""
        d = _u32(docs).ravel()
        h = C.c_void_p()
        N.check(self._L.rlr_filter_create_documents(self._h, _u32ptr(d) if d.size else None, d.size, C.byref(h)))
        return RowFilter(self, h)

    def delete_documents(self, docs) -> np.ndarray:
        """delete every row tagged with one of these document ids (stable compaction, as delete_rows) -> the deleted
        OLD row numbers, ascending"""
        d = _u32(docs).ravel()
        dp = _u32ptr(d) if d.size else None
        cap, n = 4096, C.c_uint64()
        rows = np.zeros(cap, dtype=np.uint64)
        st = self._L.rlr_index_delete_documents(self._h, dp, d.size, _up(rows), cap, C.byref(n))
        if st == N.RLR_E_RANGE and n.value > cap:  # (nothing was changed: again with room for every row number)
            cap = int(n.value)
            rows = np.zeros(cap, dtype=np.uint64)
            st = self._L.rlr_index_delete_documents(self._h, dp, d.size, _up(rows), cap, C.byref(n))
        N.check(st)
        return rows[:int(n.value)].copy()

    # -- hot path ------------------------------------------------------------
    def search_topk(self, queries, k: int, guard_eps: float = -1.0, filter: "RowFilter | None" = None):
        """queries: [Q, dim] (or [dim]) already normalised -> (rows u64 [Q,k'], cos f32 [Q,k']); filter: only these rows"""
        q = _f32(queries).reshape(-1, self.dim)
        nq = q.shape[0]
        rows = np.zeros((nq, max(k, 1)), dtype=np.uint64)
        cos = np.zeros((nq, max(k, 1)), dtype=np.float32)
        n_out = np.zeros(max(nq, 1), dtype=np.uint32)
        if filter is not None:
            N.check(self._L.rlr_search_topk_filtered(self._h, filter.handle, _fp(q), nq, k, guard_eps, _up(rows), _fp(cos),
                                                     n_out.ctypes.data_as(N.u32p)))
        else:
            N.check(self._L.rlr_search_topk(self._h, _fp(q), nq, k, guard_eps, _up(rows), _fp(cos),
                                            n_out.ctypes.data_as(N.u32p)))
        kk = int(n_out[0]) if nq else 0
        return rows[:, :kk], cos[:, :kk]

    def search_topk_scoped(self, queries, k: int, filters, guard_eps: float = -1.0):
        """queries: [Q, dim] already normalised, filters: one RowFilter per query (entries may repeat) -> a list of
        (rows u64 [k_q], cos f32 [k_q]) per query with k_q = min(k, rows of that query's filter): query q is
        search_topk(queries[q], k, filter=filters[q]).  Chunks of up to 8 queries share one masked pass over the union of
        their filters (rlr_search_topk_scoped)."""
        q = _f32(queries).reshape(-1, self.dim)
        nq = q.shape[0]
        filters = list(filters)
        if len(filters) != nq:
            raise ValueError(f"{nq} queries but {len(filters)} filters")
        handles = (C.c_void_p * max(nq, 1))(*[None if f is None else f.handle for f in filters])
        rows = np.zeros((nq, max(k, 1)), dtype=np.uint64)
        cos = np.zeros((nq, max(k, 1)), dtype=np.float32)
        n_out = np.zeros(max(nq, 1), dtype=np.uint32)
        N.check(self._L.rlr_search_topk_scoped(self._h, handles, _fp(q), nq, k, guard_eps, _up(rows), _fp(cos),
                                               n_out.ctypes.data_as(N.u32p)))
        return [(rows[i, :int(n_out[i])], cos[i, :int(n_out[i])]) for i in range(nq)]

    def search_topk_grouped(self, queries, k: int, per_document: int = 1, filter: "RowFilter | None" = None,
                            guard_eps: float = -1.0):
        """the best k rows per query with at most `per_document` (1..8) from any one document (rlr_search_topk_grouped);
        untagged rows are never capped.  queries: [Q, dim] (or [dim]) already normalised -> a list of
        (rows u64 [k_q], cos f32 [k_q], docs u32 [k_q]) per query; k_q < k when the documents run out"""
        q = _f32(queries).reshape(-1, self.dim)
        nq = q.shape[0]
        rows = np.zeros((nq, max(k, 1)), dtype=np.uint64)
        cos = np.zeros((nq, max(k, 1)), dtype=np.float32)
        docs = np.zeros((nq, max(k, 1)), dtype=np.uint32)
        n_out = np.zeros(max(nq, 1), dtype=np.uint32)
        N.check(self._L.rlr_search_topk_grouped(self._h, None if filter is None else filter.handle, _fp(q), nq, k, per_document,
                                                guard_eps, _up(rows), _fp(cos), _u32ptr(docs), _u32ptr(n_out)))
        return [(rows[i, :int(n_out[i])], cos[i, :int(n_out[i])], docs[i, :int(n_out[i])]) for i in range(nq)]

    def grouped_forms(self, reset: bool = False) -> list:
        """queries search_topk_grouped served by each form: [device-selected, exact on candidate overflow, exact because
        NaN nominations were needed or a masked row came back, exact by rule] (rlr_index_grouped_forms)"""
        counts = np.zeros(4, dtype=np.uint64)
        N.check(self._L.rlr_index_grouped_forms(self._h, _up(counts), int(reset)))
        return [int(c) for c in counts]

    def search_topk_grouped_batch(self, queries, k: int, per_document: int = 1, filter: "RowFilter | None" = None,
                                  guard_eps: float = -1.0):
        """search_topk_grouped with the queries of the call sharing passes over the rows (rlr_search_topk_grouped_batch):
        the same arguments, the same list of (rows u64, cos f32, docs u32) per query, bit for bit -- chunks of up to 8
        queries share one scan and one document table (set_grouped_sharing, grouped_batch_forms)"""
        q = _f32(queries).reshape(-1, self.dim)
        nq = q.shape[0]
        rows = np.zeros((nq, max(k, 1)), dtype=np.uint64)
        cos = np.zeros((nq, max(k, 1)), dtype=np.float32)
        docs = np.zeros((nq, max(k, 1)), dtype=np.uint32)
        n_out = np.zeros(max(nq, 1), dtype=np.uint32)
        N.check(self._L.rlr_search_topk_grouped_batch(self._h, None if filter is None else filter.handle, _fp(q), nq, k,
                                                      per_document, guard_eps, _up(rows), _fp(cos), _u32ptr(docs), _u32ptr(n_out)))
        return [(rows[i, :int(n_out[i])], cos[i, :int(n_out[i])], docs[i, :int(n_out[i])]) for i in range(nq)]

    def set_grouped_sharing(self, mode: int) -> None:
        """when search_topk_grouped_batch shares a pass: 0 where the cost model expects it to win (the default), 1 never,
        2 wherever the shape allows (rlr_index_set_grouped_sharing); the answers do not depend on it"""
        N.check(self._L.rlr_index_set_grouped_sharing(self._h, int(mode)))

    def grouped_batch_forms(self, reset: bool = False) -> list:
        """queries search_topk_grouped_batch served by each form: [selected on the device behind a shared scan, handed to
        the single-query path on a capacity, handed to it because NaN nominations were needed / a masked row came back /
        the workspace could not be reserved, handed to it by rule] (rlr_index_grouped_batch_forms)"""
        counts = np.zeros(4, dtype=np.uint64)
        N.check(self._L.rlr_index_grouped_batch_forms(self._h, _up(counts), int(reset)))
        return [int(c) for c in counts]

    def search_range(self, queries, tau, cap: int, filter: "RowFilter | None" = None, guard_eps: float = -1.0):
        """every row whose reference-order score is at least tau (rlr_search_range).  queries: [Q, dim] (or [dim]) already
        normalised, tau: one threshold or one per query -> a list of (rows u64, cos f32, n_total) per query: the first
        min(n_total, cap) hits in (score desc, row asc) order and the exact number of hits, whatever cap is.  cap = 0
        only counts."""
        q = _f32(queries).reshape(-1, self.dim)
        nq = q.shape[0]
        t = _f32(tau).ravel()
        if t.size == 1:
            t = np.full(nq, t[0], dtype=np.float32)
        if t.size != nq:
            raise ValueError(f"{nq} queries but {t.size} thresholds")
        cap = int(cap)
        rows = np.zeros((nq, max(cap, 1)), dtype=np.uint64)
        cos = np.zeros((nq, max(cap, 1)), dtype=np.float32)
        n_out = np.zeros(max(nq, 1), dtype=np.uint32)
        n_total = np.zeros(max(nq, 1), dtype=np.uint64)
        N.check(self._L.rlr_search_range(self._h, None if filter is None else filter.handle, _fp(q), nq, _fp(t), cap, guard_eps,
                                         _up(rows), _fp(cos), _u32ptr(n_out), _up(n_total)))
        if cap == 0:
            return [(rows[i, :0], cos[i, :0], int(n_total[i])) for i in range(nq)]
        return [(rows[i, :int(n_out[i])], cos[i, :int(n_out[i])], int(n_total[i])) for i in range(nq)]

    def count_range(self, queries, tau, filter: "RowFilter | None" = None) -> list:
        """how many rows score at least tau, per query (rlr_search_range with cap = 0: nothing is fetched)"""
        return [n for _, _, n in self.search_range(queries, tau, 0, filter=filter)]

    def range_forms(self, reset: bool = False) -> list:
        """queries search_range served by each form: [decided on the device, capacity (more hits than cap or than the
        device holds: the count from the device, the rows from the top-k path or the exact form), exact because allowed
        rows with NaN nominations exist or a masked row came back, exact by rule] (rlr_index_range_forms)"""
        counts = np.zeros(4, dtype=np.uint64)
        N.check(self._L.rlr_index_range_forms(self._h, _up(counts), int(reset)))
        return [int(c) for c in counts]

    def search_range_batch(self, queries, tau, cap: int, filter: "RowFilter | None" = None, guard_eps: float = -1.0):
        """search_range with the queries of the call sharing passes over the rows (rlr_search_range_batch): the same
        arguments, the same list of (rows u64, cos f32, n_total) per query, bit for bit -- 2..8 queries share one scan,
        more share one matrix-core pass per 1024 where the rows allow it (set_range_sharing, range_batch_forms)"""
        q = _f32(queries).reshape(-1, self.dim)
        nq = q.shape[0]
        t = _f32(tau).ravel()
        if t.size == 1:
            t = np.full(nq, t[0], dtype=np.float32)
        if t.size != nq:
            raise ValueError(f"{nq} queries but {t.size} thresholds")
        cap = int(cap)
        rows = np.zeros((nq, max(cap, 1)), dtype=np.uint64)
        cos = np.zeros((nq, max(cap, 1)), dtype=np.float32)
        n_out = np.zeros(max(nq, 1), dtype=np.uint32)
        n_total = np.zeros(max(nq, 1), dtype=np.uint64)
        N.check(self._L.rlr_search_range_batch(self._h, None if filter is None else filter.handle, _fp(q), nq, _fp(t), cap, guard_eps,
                                               _up(rows), _fp(cos), _u32ptr(n_out), _up(n_total)))
        if cap == 0:
            return [(rows[i, :0], cos[i, :0], int(n_total[i])) for i in range(nq)]
        return [(rows[i, :int(n_out[i])], cos[i, :int(n_out[i])], int(n_total[i])) for i in range(nq)]

    def count_range_batch(self, queries, tau, filter: "RowFilter | None" = None) -> list:
        """how many rows score at least tau, per query, over shared passes (rlr_search_range_batch with cap = 0)"""
        return [n for _, _, n in self.search_range_batch(queries, tau, 0, filter=filter)]

    def set_range_sharing(self, mode: int) -> None:
        """when search_range_batch shares a pass: 0 where the cost model expects it to win (the default), 1 never, 2
        wherever the shape allows (rlr_index_set_range_sharing); the answers do not depend on it"""
        N.check(self._L.rlr_index_set_range_sharing(self._h, int(mode)))

    def range_batch_forms(self, reset: bool = False) -> list:
        """queries search_range_batch served by each form: [decided on the device behind a shared scan, behind the
        matrix-core pass, handed to the single-query path because a device capacity was exceeded, handed to it by rule]
        (rlr_index_range_batch_forms)"""
        counts = np.zeros(4, dtype=np.uint64)
        N.check(self._L.rlr_index_range_batch_forms(self._h, _up(counts), int(reset)))
        return [int(c) for c in counts]

    def search_capped(self, query, need: int, per_document: int, k: int = 0, lam: float = 0.0, diversify: bool = False,
                      w_embedding: float = 1.0, w_lexical: float = 0.0, lex_rows=None, lex_scores=None, max_lex: float = 1.0,
                      filter: "RowFilter | None" = None, guard_eps: float = -1.0):
        """rlr_search_hybrid with at most `per_document` (1..8) candidates from any one document (rlr_search_capped): the
        allowed rows in combined order (w_embedding * cos + w_lexical * lex / max_lex), a row accepted unless
        per_document rows of its document are, `need` accepted rows -- the answer, or with `diversify` the MMR pool k
        rows are picked from with `lam`.  query: [dim], already normalised; lex_rows ascending and unique.
        -> (rows u64, cos f32, combined f32, lexn f32, docs u32), as many as came together"""
        q = _f32(query).reshape(self.dim)
        lr = _u64(lex_rows if lex_rows is not None else [])
        ls = _f32(lex_scores if lex_scores is not None else [])
        if lr.size != ls.size:
            raise ValueError("lex_rows and lex_scores differ in length")
        cap = max(int(need), 1)
        rows = np.zeros(cap, dtype=np.uint64)
        cos, comb, lexn = (np.zeros(cap, dtype=np.float32) for _ in range(3))
        docs = np.zeros(cap, dtype=np.uint32)
        n_out = np.zeros(1, dtype=np.uint32)
        N.check(self._L.rlr_search_capped(self._h, None if filter is None else filter.handle, _fp(q), need, k, lam, int(diversify),
                                          w_embedding, w_lexical, _up(lr) if lr.size else None, _fp(ls) if ls.size else None,
                                          lr.size, max_lex, per_document, guard_eps, _up(rows), _fp(cos), _fp(comb), _fp(lexn),
                                          _u32ptr(docs), _u32ptr(n_out)))
        n = int(n_out[0])
        return rows[:n], cos[:n], comb[:n], lexn[:n], docs[:n]

    def capped_forms(self, reset: bool = False) -> list:
        """queries search_capped served by each form: [decided on the device, exact on capacity, exact because it was
        undecidable there (NaN rows needed, a masked row came back, a boundary tie), exact by rule] (rlr_index_capped_forms)"""
        counts = np.zeros(4, dtype=np.uint64)
        N.check(self._L.rlr_index_capped_forms(self._h, _up(counts), int(reset)))
        return [int(c) for c in counts]

    def search_capped_batch(self, queries, need: int, per_document: int, k: int = 0, lam: float = 0.0, diversify: bool = False,
                            w_embedding: float = 1.0, w_lexical: float = 0.0, lex_rows=None, lex_scores=None, max_lex=None,
                            filter: "RowFilter | None" = None, guard_eps: float = -1.0):
        """search_capped with the queries of the call sharing passes over the rows (rlr_search_capped_batch).  queries:
        [Q, dim], already normalised; lex_rows / lex_scores: one sequence per query (None: no pairs at all), each query's
        rows ascending and unique; max_lex: one value per query (None: 1.0); everything else holds for the whole call.
        -> a list of (rows u64, cos f32, combined f32, lexn f32, docs u32) per query, bit for bit what search_capped
        returns for that query alone (set_capped_sharing, capped_batch_forms)"""
        q = _f32(queries).reshape(-1, self.dim)
        nq = q.shape[0]
        lrs = [_u64(r) for r in lex_rows] if lex_rows is not None else [_u64([]) for _ in range(nq)]
        lss = [_f32(s) for s in lex_scores] if lex_scores is not None else [_f32([]) for _ in range(nq)]
        if len(lrs) != nq or len(lss) != nq or any(r.size != s.size for r, s in zip(lrs, lss)):
            raise ValueError("lex_rows / lex_scores: one sequence per query, of equal lengths")
        off = np.zeros(nq + 1, dtype=np.uint64)
        off[1:] = np.cumsum([r.size for r in lrs], dtype=np.uint64)
        lr = np.ascontiguousarray(np.concatenate(lrs)) if nq else _u64([])
        ls = np.ascontiguousarray(np.concatenate(lss)) if nq else _f32([])
        ml = np.ones(max(nq, 1), dtype=np.float32) if max_lex is None else _f32(max_lex).ravel()
        if max_lex is not None and ml.size != nq:
            raise ValueError(f"{nq} queries but {ml.size} max_lex values")
        cap = max(int(need), 1)
        rows = np.zeros((max(nq, 1), cap), dtype=np.uint64)
        cos, comb, lexn = (np.zeros((max(nq, 1), cap), dtype=np.float32) for _ in range(3))
        docs = np.zeros((max(nq, 1), cap), dtype=np.uint32)
        n_out = np.zeros(max(nq, 1), dtype=np.uint32)
        N.check(self._L.rlr_search_capped_batch(self._h, None if filter is None else filter.handle, _fp(q), nq, need, k, lam,
                                                int(diversify), w_embedding, w_lexical, _up(lr) if lr.size else None,
                                                _fp(ls) if ls.size else None, _up(off), _fp(ml), per_document, guard_eps, _up(rows),
                                                _fp(cos), _fp(comb), _fp(lexn), _u32ptr(docs), _u32ptr(n_out)))
        out = []
        for i in range(nq):
            n = int(n_out[i])
            out.append((rows[i, :n], cos[i, :n], comb[i, :n], lexn[i, :n], docs[i, :n]))
        return out

    def set_capped_sharing(self, mode: int) -> None:
        """when search_capped_batch shares a pass: 0 where the cost model expects it to win (the default), 1 never, 2
        wherever the shape allows (rlr_index_set_capped_sharing); the answers do not depend on it"""
        N.check(self._L.rlr_index_set_capped_sharing(self._h, int(mode)))

    def capped_batch_forms(self, reset: bool = False) -> list:
        """queries search_capped_batch served by each form: [decided on the device behind a shared scan, handed to the
        single path on a capacity, handed to it as undecidable there (the boundary rule, NaN rows wanted, a masked row came
        back, no workspace), handed to it by rule] (rlr_index_capped_batch_forms)"""
        counts = np.zeros(4, dtype=np.uint64)
        N.check(self._L.rlr_index_capped_batch_forms(self._h, _up(counts), int(reset)))
        return [int(c) for c in counts]

    def search_topk_device(self, queries, k: int, d_out_ptr: int, stream: int = 0, guard_eps: float = -1.0) -> None:
        q = _f32(queries).reshape(-1, self.dim)
        N.check(self._L.rlr_search_topk_device(self._h, _fp(q), q.shape[0], k, guard_eps,
                                               C.c_void_p(d_out_ptr), C.c_void_p(stream)))

    def search_topk_device_begin(self, queries, k: int, d_out_ptr: int, stream: int = 0, guard_eps: float = -1.0):
        """enqueue the search, make `stream` wait for it, return a ticket for search_topk_device_end"""
        q = _f32(queries).reshape(-1, self.dim)
        t = C.c_void_p()
        N.check(self._L.rlr_search_topk_device_begin(self._h, _fp(q), q.shape[0], k, guard_eps, C.c_void_p(d_out_ptr),
                                                     C.c_void_p(stream), C.byref(t)))
        return t

    def search_topk_device_end(self, ticket) -> int:
        """join; -> number of queries whose results are invalid (guard band overflow: redo synchronously)"""
        n = C.c_uint32()
        N.check(self._L.rlr_search_topk_device_end(self._h, ticket, C.byref(n)))
        return n.value

    def score_rows(self, query, rows) -> np.ndarray:
        q = _f32(query).ravel()
        rows = _u64(rows).ravel()
        out = np.zeros(rows.size, dtype=np.float32)
        if rows.size:
            N.check(self._L.rlr_score_rows(self._h, _fp(q), _up(rows), rows.size, _fp(out)))
        return out

    def fetch_rows(self, rows) -> np.ndarray:
        rows = _u64(rows).ravel()
        out = np.zeros((rows.size, self.dim), dtype=np.float32)
        if rows.size:
            N.check(self._L.rlr_fetch_rows(self._h, _up(rows), rows.size, _fp(out)))
        return out

    def mmr_select(self, pool_rows, pool_scores, k: int, lam: float):
        pool_rows = _u64(pool_rows).ravel()
        pool_scores = _f32(pool_scores).ravel()
        P = pool_rows.size
        order = np.zeros(max(P, 1), dtype=np.uint32)
        mmr = np.zeros(max(P, 1), dtype=np.float32)
        n = C.c_uint32()
        N.check(self._L.rlr_mmr_select(self._h, _up(pool_rows), _fp(pool_scores), P, k, lam,
                                       order.ctypes.data_as(N.u32p), _fp(mmr), C.byref(n)))
        return order[: n.value], mmr[: n.value]

    def mmr_select_batch(self, pool_rows, pool_scores, pool_sizes, k: int, lam: float):
        """pool_rows/pool_scores: [Q, P]; pool_sizes: [Q] -> (order u32 [Q, P], mmr f32 [Q, P], n u32 [Q])"""
        pool_rows = _u64(pool_rows)
        pool_scores = _f32(pool_scores)
        nq, P = pool_rows.shape
        sizes = np.ascontiguousarray(pool_sizes, dtype=np.uint32)
        order = np.zeros((nq, max(P, 1)), dtype=np.uint32)
        mmr = np.zeros((nq, max(P, 1)), dtype=np.float32)
        n = np.zeros(max(nq, 1), dtype=np.uint32)
        N.check(self._L.rlr_mmr_select_batch(self._h, _up(pool_rows), _fp(pool_scores), sizes.ctypes.data_as(N.u32p), nq, P,
                                             k, lam, order.ctypes.data_as(N.u32p), _fp(mmr), n.ctypes.data_as(N.u32p)))
        return order, mmr, n[:nq]

    def fetch_rows_device(self, rows, d_out_ptr: int) -> None:
        """rows of this index as dense f32 values into device memory at `d_out_ptr` (len(rows) x dim floats)"""
        rows = _u64(rows).ravel()
        if rows.size:
            N.check(self._L.rlr_fetch_rows_device(self._h, _up(rows), rows.size, C.c_void_p(d_out_ptr)))

    def row_bytes(self) -> int:
        """bytes of one stored row: dim elements of the index' dtype, padded to 16 bytes (rlr_index_row_bytes)"""
        b = C.c_uint32()
        N.check(self._L.rlr_index_row_bytes(self._h, C.byref(b)))
        return int(b.value)

    def gather_rows_device(self, rows, d_out_ptr: int) -> None:
        """rows of this index as stored (row_bytes() bytes each, dense) into device memory at `d_out_ptr`"""
        rows = _u64(rows).ravel()
        if rows.size:
            N.check(self._L.rlr_gather_rows_device(self._h, _up(rows), rows.size, C.c_void_p(d_out_ptr)))

    def mmr_select_staged(self, d_staged_ptr: int, n_staged: int, pool_slots, pool_scores, pool_sizes, k: int, lam: float):
        """mmr_select_batch for pools whose rows sit in a staged matrix in device memory: `n_staged` raw rows of this index'
        dtype at row_bytes() pitch (what gather_rows_device writes); pool_slots [Q, P] index that matrix"""
        pool_slots = _u64(pool_slots)
        pool_scores = _f32(pool_scores)
        nq, P = pool_slots.shape
        sizes = np.ascontiguousarray(pool_sizes, dtype=np.uint32)
        order = np.zeros((nq, max(P, 1)), dtype=np.uint32)
        mmr = np.zeros((nq, max(P, 1)), dtype=np.float32)
        n = np.zeros(max(nq, 1), dtype=np.uint32)
        N.check(self._L.rlr_mmr_select_staged(self._h, C.c_void_p(d_staged_ptr), n_staged, _up(pool_slots), _fp(pool_scores),
                                              sizes.ctypes.data_as(N.u32p), nq, P, k, lam, order.ctypes.data_as(N.u32p),
                                              _fp(mmr), n.ctypes.data_as(N.u32p)))
        return order, mmr, n[:nq]

    def mmr_select_values(self, d_values_ptr: int, pool_scores, pool_sizes, k: int, lam: float):
        """mmr_select_batch for pools whose row values are in device memory: [Q, P, dim] f32 at `d_values_ptr`"""
        pool_scores = _f32(pool_scores)
        nq, P = pool_scores.shape
        sizes = np.ascontiguousarray(pool_sizes, dtype=np.uint32)
        order = np.zeros((nq, max(P, 1)), dtype=np.uint32)
        mmr = np.zeros((nq, max(P, 1)), dtype=np.float32)
        n = np.zeros(max(nq, 1), dtype=np.uint32)
        N.check(self._L.rlr_mmr_select_values(self._h, C.c_void_p(d_values_ptr), _fp(pool_scores),
                                              sizes.ctypes.data_as(N.u32p), nq, P, k, lam,
                                              order.ctypes.data_as(N.u32p), _fp(mmr), n.ctypes.data_as(N.u32p)))
        return order, mmr, n[:nq]

    # -- coalescing of concurrent single-query searches -----------------------
    def set_coalescing(self, max_group: int, linger_us: int = 0) -> None:
        """concurrent single-query searches share one pass over the rows, up to max_group (2..8) at a time; 0 or 1:
        off (the default).  linger_us: how long a caller that finds the index idle waits for others.  A mutator: no
        search may run on the index meanwhile."""
        N.check(self._L.rlr_index_set_coalescing(self._h, max_group, linger_us))

    def coalesce_stats(self, reset: bool = False) -> dict:
        """the coalescer's counters (rlr_coalesce_stats) as a dict; group_size is a list indexed by group size"""
        st = N.CoalesceStatsC()
        N.check(self._L.rlr_index_coalesce_stats(self._h, C.byref(st), int(reset)))
        out = {f: getattr(st, f) for f, _ in N.CoalesceStatsC._fields_}
        out["group_size"] = list(st.group_size)
        return out

    # -- measurement ---------------------------------------------------------
    def profile_enable(self, on: bool = True) -> None:
        N.check(self._L.rlr_profile_enable(self._h, int(on)))

    def profile_read(self, reset: bool = False) -> Profile:
        p = N.ProfileC()
        N.check(self._L.rlr_profile_read(self._h, C.byref(p), int(reset)))
        return Profile(*(getattr(p, f) for f, _ in N.ProfileC._fields_))

    def probe_bandwidth(self, mode: int, reps: int = 5):
        """measured-peak denominators over the index's own rows: mode 0 read-only stream, 1 device-to-device copy
        -> (GB/s, ms per launch)"""
        g, ms = C.c_double(), C.c_double()
        N.check(self._L.rlr_index_probe_bandwidth(self._h, mode, reps, C.byref(g), C.byref(ms)))
        return g.value, ms.value


class MultiGpuIndex:
    """One process, several GPUs (rlr_multi_*): contiguous row shards, host-side merge."""

    def __init__(self, dim: int, device_ids, dtype: str = "f32"):
        self._L = N.lib()
        self._h = C.c_void_p()
        ids = np.ascontiguousarray(device_ids, dtype=np.int32)
        code = {"f32": N.RLR_F32, "f16": N.RLR_F16}[dtype]
        N.check(self._L.rlr_multi_create(dim, code, ids.size, ids.ctypes.data_as(N.i32p), C.byref(self._h)))
        self.dim = dim

    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h:
            self._L.rlr_multi_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __len__(self) -> int:
        n = C.c_uint64()
        N.check(self._L.rlr_multi_info(self._h, C.byref(n), None))
        return int(n.value)

    def upload(self, rows, normalize: bool = False) -> None:
        rows = _f32(rows).reshape(-1, self.dim)
        N.check(self._L.rlr_multi_upload(self._h, _fp(rows), rows.shape[0], int(normalize)))

    def fill_synthetic(self, n_rows: int, seed: int, n_clusters: int = 0) -> None:
        N.check(self._L.rlr_multi_fill_synthetic(self._h, n_rows, seed, n_clusters))

    def enable_batch_image(self, flags: int = 1) -> None:
        """rlr_index_enable_batch_image on every shard (1: binary16 image for batches, 3: + single queries, 4: 8-bit copy)"""
        N.check(self._L.rlr_multi_enable_batch_image(self._h, flags))

    def set_exchange(self, mode: str) -> None:
        """"host": per-shard lists merged on the host (default); "rccl": ncclAllGather of the packed partial top-k
        lists + merge kernel on the first device (one shard per device; librccl loaded on first use)"""
        N.check(self._L.rlr_multi_set_exchange(self._h, {"host": 0, "rccl": 1}[mode]))

    def search_topk(self, queries, k: int, guard_eps: float = -1.0):
        q = _f32(queries).reshape(-1, self.dim)
        nq = q.shape[0]
        rows = np.zeros((nq, max(k, 1)), dtype=np.uint64)
        cos = np.zeros((nq, max(k, 1)), dtype=np.float32)
        n_out = np.zeros(max(nq, 1), dtype=np.uint32)
        N.check(self._L.rlr_multi_search_topk(self._h, _fp(q), nq, k, guard_eps, _up(rows), _fp(cos),
                                              n_out.ctypes.data_as(N.u32p)))
        kk = int(n_out[0]) if nq else 0
        return rows[:, :kk], cos[:, :kk]

    def score_rows(self, query, rows) -> np.ndarray:
        q = _f32(query).ravel()
        rows = _u64(rows).ravel()
        out = np.zeros(rows.size, dtype=np.float32)
        if rows.size:
            N.check(self._L.rlr_multi_score_rows(self._h, _fp(q), _up(rows), rows.size, _fp(out)))
        return out

    def fetch_rows(self, rows) -> np.ndarray:
        rows = _u64(rows).ravel()
        out = np.zeros((rows.size, self.dim), dtype=np.float32)
        if rows.size:
            N.check(self._L.rlr_multi_fetch_rows(self._h, _up(rows), rows.size, _fp(out)))
        return out

    def mmr_select(self, pool_rows, pool_scores, k: int, lam: float):
        pool_rows = _u64(pool_rows).ravel()
        pool_scores = _f32(pool_scores).ravel()
        P = pool_rows.size
        order = np.zeros(max(P, 1), dtype=np.uint32)
        mmr = np.zeros(max(P, 1), dtype=np.float32)
        n = C.c_uint32()
        N.check(self._L.rlr_multi_mmr_select(self._h, _up(pool_rows), _fp(pool_scores), P, k, lam,
                                             order.ctypes.data_as(N.u32p), _fp(mmr), C.byref(n)))
        return order[: n.value], mmr[: n.value]

    def mmr_select_batch(self, pool_rows, pool_scores, pool_sizes, k: int, lam: float):
        """pools strided by P = pool_rows.shape[1]; -> (order [nq, P], mmr [nq, P], n_selected [nq])"""
        pool_rows = _u64(pool_rows)
        nq, P = pool_rows.shape
        pool_scores = _f32(pool_scores).reshape(nq, P)
        sizes = np.ascontiguousarray(pool_sizes, dtype=np.uint32)
        order = np.zeros((max(nq, 1), max(P, 1)), dtype=np.uint32)
        mmr = np.zeros((max(nq, 1), max(P, 1)), dtype=np.float32)
        n = np.zeros(max(nq, 1), dtype=np.uint32)
        N.check(self._L.rlr_multi_mmr_select_batch(self._h, _up(pool_rows), _fp(pool_scores), sizes.ctypes.data_as(N.u32p), nq, P, k,
                                                   lam, order.ctypes.data_as(N.u32p), _fp(mmr), n.ctypes.data_as(N.u32p)))
        return order[:nq], mmr[:nq], n[:nq]

    def stats(self, reset: bool = False) -> dict:
        st = N.MultiStatsC()
        N.check(self._L.rlr_multi_stats(self._h, C.byref(st), int(reset)))
        return {name: getattr(st, name) for name, _ in N.MultiStatsC._fields_}

    # ---- RagEngine::search / search_with_diversity over the sharded corpus (rlr_multi_engine_*) ----
    # results: numpy records (row, score, embedding_score, lexical_score, initial_score), global rows
    _HIT = np.dtype([("row", "<u8"), ("score", "<f4"), ("embedding_score", "<f4"), ("lexical_score", "<f4"),
                     ("initial_score", "<f4")])

    @staticmethod
    def _lex_args(lex_rows, lex_scores):
        if lex_rows is None or len(lex_rows) == 0:
            return np.zeros(1, np.uint64), np.zeros(1, np.float32), 0
        lr, ls = _u64(lex_rows).ravel(), _f32(lex_scores).ravel()
        return lr, ls, int(lr.size)

    def engine_search(self, query, top_k: int, weights=None, lex_rows=None, lex_scores=None, stage: int = 0):
        q = _f32(query).ravel()
        cap = max(3 * max(top_k, 1), 1)
        hits = (N.SearchHitC * cap)()
        n = C.c_uint32()
        lr, ls, nl = self._lex_args(lex_rows, lex_scores)
        wc = weights.to_c() if weights is not None else None
        N.check(self._L.rlr_multi_engine_search(self._h, _fp(q), q.size, top_k, C.byref(wc) if wc is not None else None, _up(lr),
                                                _fp(ls), nl, stage, hits, cap, C.byref(n)))
        return np.frombuffer(hits, dtype=self._HIT, count=n.value).copy()

    def engine_search_with_diversity(self, query, top_k: int, diversity_factor: float, weights=None, lex_rows=None,
                                     lex_scores=None):
        q = _f32(query).ravel()
        cap = max(3 * max(top_k, 1), top_k + 10)
        hits = (N.SearchHitC * cap)()
        n = C.c_uint32()
        lr, ls, nl = self._lex_args(lex_rows, lex_scores)
        wc = weights.to_c() if weights is not None else None
        N.check(self._L.rlr_multi_engine_search_with_diversity(self._h, _fp(q), q.size, top_k, float(diversity_factor),
                                                               C.byref(wc) if wc is not None else None, _up(lr), _fp(ls), nl,
                                                               hits, cap, C.byref(n)))
        return np.frombuffer(hits, dtype=self._HIT, count=n.value).copy()

    def engine_search_text(self, lexical, query, tokens: str, top_k: int, diversity_factor: float, weights=None, stage: int = 0):
        """lexical: a LexicalIndex over the global rows; tokens: the host's tokenize(query), space separated"""
        q = _f32(query).ravel()
        cap = max(3 * max(top_k, 1), top_k + 10)
        hits = (N.SearchHitC * cap)()
        n = C.c_uint32()
        tok = tokens.encode("utf-8")
        wc = weights.to_c() if weights is not None else None
        N.check(self._L.rlr_multi_engine_search_text(self._h, lexical._h, _fp(q), q.size, tok, len(tok), top_k,
                                                     float(diversity_factor), stage, C.byref(wc) if wc is not None else None,
                                                     hits, cap, C.byref(n)))
        return np.frombuffer(hits, dtype=self._HIT, count=n.value).copy()

    def engine_search_with_diversity_batch(self, queries, top_k: int, diversity_factor: float, weights=None):
        q = _f32(queries)
        if q.ndim == 1:
            q = q.reshape(1, -1)
        nq, dq = q.shape
        cap = max(3 * max(top_k, 1), top_k + 10)
        hits = (N.SearchHitC * (cap * max(nq, 1)))()
        n_out = np.zeros(max(nq, 1), dtype=np.uint32)
        wc = weights.to_c() if weights is not None else None
        N.check(self._L.rlr_multi_engine_search_with_diversity_batch(self._h, _fp(q), dq, nq, top_k, float(diversity_factor),
                                                                     C.byref(wc) if wc is not None else None, hits, cap,
                                                                     n_out.ctypes.data_as(N.u32p)))
        allh = np.frombuffer(hits, dtype=self._HIT, count=cap * max(nq, 1)).reshape(max(nq, 1), cap)
        return [allh[i, : int(n_out[i])].copy() for i in range(nq)]

    def engine_embedding_candidates(self, query, count: int):
        q = _f32(query).ravel()
        rows = np.zeros(max(count, 1), dtype=np.uint64)
        sc = np.zeros(max(count, 1), dtype=np.float32)
        n = C.c_uint32()
        N.check(self._L.rlr_multi_engine_embedding_candidates(self._h, _fp(q), q.size, count, _up(rows), _fp(sc), C.byref(n)))
        return rows[: n.value], sc[: n.value]


def default_guard_eps(dim: int) -> float:
    return float(N.lib().rlr_default_guard_eps(dim))


def device_count() -> int:
    return int(N.lib().rlr_device_count())
