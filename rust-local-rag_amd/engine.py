"""RagEngine: the reference's search-side operator interface over the GPU index.

Mirrors rust-local-rag `RagEngine::{search, search_with_diversity,
get_embedding_candidates}` (src/rag_engine.rs:470-701, :717-759, :415-461) and the API
layer `search_documents` / `http_search` / `format_search_results`
(src/mcp_server.rs:81-110, :371-389, :599-637) -- same names, argument meaning and
edge-case behaviour.  The numerics run in librlr_gpu.so (csrc/engine.cpp + HIP kernels);
this file only carries chunk metadata and marshals arguments.

Outside this path and therefore passed IN by the caller: the query *embedding* (the
reference obtains it from Ollama, embeddings.rs:91-102), BM25 candidates
(`LexicalIndex::score`) as (chunk_id, score) pairs, and the LLM reranker.
"""
from __future__ import annotations

import ctypes as C
import itertools
import uuid
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _native as N
from .index import GpuIndex, RowFilter, _f32
from .lexical import LexicalIndex, tokenize


@dataclass
class QueryWeights:  # rag_engine.rs:1846-1865
    embedding: Optional[float] = None
    lexical: Optional[float] = None
    reranker: Optional[float] = None
    initial: Optional[float] = None

    def to_c(self) -> N.QueryWeightsC:
        c = N.QueryWeightsC()
        for name in ("embedding", "lexical", "reranker", "initial"):
            v = getattr(self, name)
            setattr(c, "has_" + name, int(v is not None))
            setattr(c, name, float(v) if v is not None else 0.0)
        return c


@dataclass
class ResolvedWeights:  # rag_engine.rs:1877-1896
    embedding: float
    lexical: float
    reranker: float
    initial: float

    @staticmethod
    def from_query_weights(weights: Optional[QueryWeights]) -> "ResolvedWeights":
        out = N.ResolvedWeightsC()
        if weights is None:
            N.lib().rlr_resolve_weights(None, C.byref(out))
        else:
            c = weights.to_c()
            N.lib().rlr_resolve_weights(C.byref(c), C.byref(out))
        return ResolvedWeights(out.embedding, out.lexical, out.reranker, out.initial)


def resolve_weight(override: Optional[float], default: float) -> float:
    """rag_engine.rs:1869-1873"""
    has = override is not None
    return float(N.lib().rlr_resolve_weight(int(has), float(override) if has else 0.0, float(default)))


def normalize(v) -> np.ndarray:
    """rag_engine.rs:1763-1771 (host side, reference order)"""
    a = _f32(v).copy()
    N.lib().rlr_normalize(a.ctypes.data_as(N.f32p), a.size)
    return a


@dataclass
class DocumentChunk:  # rag_engine.rs:46-59 (embedding lives in HBM, not here)
    id: str
    document_name: str
    text: str
    chunk_index: int
    page_number: int = 0
    section: Optional[str] = None
    metadata: Optional[dict] = None  # ChunkMetadata (:61-70) as loaded; written back unchanged by save_to_disk


@dataclass
class SearchResult:  # rag_engine.rs:72-100
    text: str
    score: float
    document: str
    chunk_id: str
    chunk_index: int
    page_number: int
    section: Optional[str] = None
    embedding_score: Optional[float] = None
    lexical_score: Optional[float] = None
    initial_score: Optional[float] = None
    reranker_score: Optional[float] = None
    yes_logprob: Optional[float] = None
    no_logprob: Optional[float] = None
    row: int = -1  # position in the GPU matrix (not part of the reference struct)

    def to_json(self) -> dict:
        """serde shape incl. skip_serializing_if = Option::is_none (rag_engine.rs:83-99)"""
        d = {"text": self.text, "score": self.score, "document": self.document, "chunk_id": self.chunk_id,
             "chunk_index": self.chunk_index, "page_number": self.page_number, "section": self.section}
        for k in ("embedding_score", "lexical_score", "initial_score", "reranker_score", "yes_logprob", "no_logprob"):
            v = getattr(self, k)
            if v is not None:
                d[k] = v
        return d


@dataclass
class SearchRequest:  # mcp_server.rs:17-31
    query_embedding: Sequence[float]
    top_k: Optional[int] = None
    diversity_factor: Optional[float] = None
    weights: Optional[QueryWeights] = None
    lexical: Sequence[Tuple[str, float]] = field(default_factory=list)
    query: Optional[str] = None   # the query text (mcp_server.rs:19); scored by the GPU LexicalIndex when given
    documents: Optional[Sequence[str]] = None  # search only inside these documents (None: the whole corpus; []: nothing)
    per_document: Optional[int] = None  # at most this many (1..8) results from any one document (None: no cap)


def document_ranges(chunks: Sequence[DocumentChunk], documents) -> List[Tuple[int, int]]:
    """The rows of `documents` in a row -> chunk table as (first, count) runs, ascending.  A document is one run as a
    rule (add_document appends, removal compacts stably); unknown names contribute no rows."""
    want = set(documents)
    runs: List[Tuple[int, int]] = []
    start = None
    for r, ch in enumerate(chunks):
        if ch.document_name in want:
            if start is None:
                start = r
        elif start is not None:
            runs.append((start, r - start))
            start = None
    if start is not None:
        runs.append((start, len(chunks) - start))
    return runs


class RagEngine:
    """Search half of the reference's RagEngine with the embeddings resident on one GPU."""

    def __init__(self, dim: int, dtype: str = "f32", device: int = 0, accelerate: Optional[str] = None):
        """accelerate: None | "image" | "q8" -- keep an optional nomination copy of the rows so the scan streams
        a half / a quarter of the bytes (GpuIndex.enable_batch_image); results are unchanged"""
        self.index = GpuIndex(dim, dtype, device)
        if accelerate == "image":
            self.index.enable_batch_image(True, single_query=True)
        elif accelerate == "q8":
            self.index.enable_batch_image(False, q8=True)
        elif accelerate is not None:
            raise ValueError("accelerate must be None, 'image' or 'q8'")
        self.lexical = LexicalIndex(device)          # BM25 postings in HBM (rag_engine.rs:112)
        self.dim = dim
        self._chunks: List[DocumentChunk] = []       # row -> chunk
        self._row_of: Dict[str, int] = {}            # chunk_id -> row
        self._filters: Dict[frozenset, RowFilter] = {}  # documents -> their rows as a filter; dropped by every mutation
        self._doc_ids: Dict[str, int] = {}           # document name -> its id in the index's document column
        self._tagged: Optional[list] = None          # the chunk table the column was last made to agree with ...
        self._tagged_len = 0                         # ... and its length then (see _sync_documents)

    _next_doc_id = itertools.count()                 # shared by every engine: an id is never reused within a process

    def close(self) -> None:
        self._drop_filters()
        self.index.close()
        self.lexical.close()

    # -- document scopes -----------------------------------------------------------------------
    def _drop_filters(self) -> None:
        for f in self._filters.values():
            f.close()
        self._filters = {}

    def _filter_for(self, documents: Sequence[str]) -> RowFilter:
        """the rows of these documents as a RowFilter (cached until the next add_document / remove_document)"""
        key = frozenset(documents)
        f = self._filters.get(key)
        if f is not None and f.info()["stale"]:  # (the index was replaced behind the engine: load_from_disk)
            self._drop_filters()
            f = None
        if f is None:
            self._sync_documents()
            f = self.index.filter_documents([self._doc_ids[d] for d in key if d in self._doc_ids])  # built on the device
            self._filters[key] = f
        return f

    def _doc_id(self, document_name: str) -> int:
        doc = self._doc_ids.get(document_name)
        if doc is None:
            doc = self._doc_ids[document_name] = next(RagEngine._next_doc_id)
        return doc

    def _sync_documents(self) -> None:
        """The index's document column names the document of every row.  add_document / remove_document keep it so; a
        chunk table that was replaced as a whole (load_from_disk, a synthetic corpus) is tagged here, in one call."""
        if self._tagged is self._chunks and self._tagged_len == len(self._chunks):
            return
        ids = np.fromiter((self._doc_id(ch.document_name) for ch in self._chunks), dtype=np.uint32, count=len(self._chunks))
        self.index.set_documents(ids)
        self._tagged, self._tagged_len = self._chunks, len(self._chunks)

    # -- index mutation (sites rag_engine.rs:347-348, :358-384) --------------------------
    def add_document(self, document_name: str, texts: Sequence[str], embeddings, pages: Optional[Sequence[int]] = None,
                     sections: Optional[Sequence[Optional[str]]] = None, report_duplicates_above: Optional[float] = None):
        """Replace `document_name`'s chunks: drop its old rows, normalise and append the new ones -> the new chunk ids.
        `report_duplicates_above`: a cosine; the call then returns (ids, duplicates) with, per new chunk, the ids of the
        chunks ALREADY in the corpus (the document's own old chunks are gone by then) at or above it -- found before
        the append, by search_range."""
        self.remove_document(document_name)
        emb = _f32(embeddings).reshape(len(texts), self.dim)
        duplicates = None if report_duplicates_above is None else self._duplicates_of(emb, float(report_duplicates_above))
        first = self.index.append(emb, normalize=True)  # normalize(&mut embedding) :358-359, on the GPU
        ids = []
        for i, text in enumerate(texts):
            cid = str(uuid.uuid4())
            ch = DocumentChunk(cid, document_name, text, i, pages[i] if pages else 0, sections[i] if sections else None)
            self._chunks.append(ch)
            self._row_of[cid] = first + i
            self.lexical.add_chunk(first + i, text)   # lexical_index.add_chunk(&chunk.id, &chunk.text) :382
            ids.append(cid)
        self.index.tag_rows(first, len(texts), self._doc_id(document_name))  # (append left them in no document)
        self._tagged_len = len(self._chunks)
        self._drop_filters()
        return ids if duplicates is None else (ids, duplicates)

    def remove_document(self, document_name: str) -> int:
        self._sync_documents()
        doc = self._doc_ids.get(document_name)
        if doc is None:
            return 0
        # chunks.retain(|_, c| c.document_name != filename): which rows go is decided on the device from the column
        dead = self.index.delete_documents([doc])
        if dead.size:
            self._drop_filters()
            self.lexical.remove_rows(dead)
            self._cut_rows(dead.astype(np.int64))
            self._tagged, self._tagged_len = self._chunks, len(self._chunks)
        return int(dead.size)

    def _cut_rows(self, dead: np.ndarray) -> None:
        """Cut the (ascending) rows `dead` out of the row -> chunk table and renumber chunk_id -> row, as the index's
        stable compaction renumbered the rows: whole runs of surviving chunks are copied as slices, and only the rows
        from the first dead one on get a new number."""
        old, first = self._chunks, int(dead[0])
        complete = len(self._row_of) == len(old)        # (a planted table may come without its ids: rebuild them all)
        edges = np.flatnonzero(np.diff(dead) != 1)
        starts, ends = dead[np.r_[0, edges + 1]], dead[np.r_[edges, dead.size - 1]] + 1   # the dead runs [start, end)
        if complete:
            for a, b in zip(starts, ends):
                for ch in old[a:b]:
                    self._row_of.pop(ch.id, None)
        new = old[:first]
        for end, nxt in zip(ends, np.r_[starts[1:], len(old)]):
            new += old[end:nxt]
        self._chunks = new
        if complete:
            for r in range(first, len(new)):
                self._row_of[new[r].id] = r
        else:
            self._row_of = {ch.id: r for r, ch in enumerate(new)}

    def __len__(self) -> int:
        return len(self._chunks)

    # -- helpers ---------------------------------------------------------------------------
    def _lex(self, lexical: Sequence[Tuple[str, float]], query_text: Optional[str] = None, limit: int = 0):
        if query_text is not None:
            # `self.lexical_index.score(query, top_k.saturating_mul(5))` :505, on the GPU
            lr, ls = self.lexical.score(query_text, limit)
            if lr.size == 0:
                return np.zeros(1, np.uint64), np.zeros(1, np.float32), 0
            return np.ascontiguousarray(lr), np.ascontiguousarray(ls), int(lr.size)
        rows = [self._row_of[cid] for cid, _ in lexical if cid in self._row_of]
        scores = [s for cid, s in lexical if cid in self._row_of]
        lr = np.ascontiguousarray(rows if rows else [0], dtype=np.uint64)
        ls = np.ascontiguousarray(scores if scores else [0], dtype=np.float32)
        return lr, ls, len(rows)

    _HIT_DTYPE = np.dtype([("row", "<u8"), ("score", "<f4"), ("embedding_score", "<f4"), ("lexical_score", "<f4"),
                           ("initial_score", "<f4")])   # = _native.SearchHitC

    def _results(self, hits, n: int) -> List[SearchResult]:
        if n == 0:
            return []
        # one view over the ctypes array and one tolist() instead of 5 n attribute reads (a third of a 0.3 ms search)
        rows = np.frombuffer(hits, dtype=self._HIT_DTYPE, count=n).tolist()
        chunks = self._chunks
        out = []
        for row, score, emb, lex, init in rows:
            ch = chunks[row]
            out.append(SearchResult(ch.text, score, ch.document_name, ch.id, ch.chunk_index, ch.page_number, ch.section,
                                    emb, lex, init, None, None, None, row))
        return out

    # -- RagEngine::search (rag_engine.rs:470-701) -----------------------------------------
    def search(self, query_embedding, top_k: int, weights: Optional[QueryWeights] = None,
               lexical: Sequence[Tuple[str, float]] = (), stage: int = 0,
               query_text: Optional[str] = None, documents: Optional[Sequence[str]] = None,
               per_document: Optional[int] = None) -> List[SearchResult]:
        """`lexical`: BM25 pairs computed by the caller, or `query_text`: scored by the GPU LexicalIndex.
        `documents`: search only inside these documents -- the reference's search over the corpus that holds only their
        chunks (None: the whole corpus; an empty list or unknown names: no rows, no results).
        `per_document`: at most this many (1..8) results from any one document, capped in combined-score order on the
        device (rlr_engine_search_capped); None: no cap, the paths below untouched."""
        q = _f32(query_embedding).ravel()
        cap = max(3 * max(top_k, 1), 1)
        hits = (N.SearchHitC * cap)()
        n = C.c_uint32()
        wc = weights.to_c() if weights is not None else None
        if per_document is not None:
            return self._search_capped(q, top_k, 0.0, stage, wc, lexical, query_text, documents, per_document, hits, cap,
                                       5 * max(top_k, 1))
        if documents is not None:
            f = self._filter_for(documents)
            if query_text is not None:
                tok = " ".join(tokenize(query_text)).encode("utf-8")
                N.check(N.lib().rlr_engine_search_text_filtered(
                    self.index.handle, self.lexical._h, f.handle, q.ctypes.data_as(N.f32p), q.size, tok, len(tok), top_k, 0.0,
                    stage, C.byref(wc) if wc is not None else None, hits, cap, C.byref(n)))
            else:
                lr, ls, nl = self._lex(lexical, None, 5 * max(top_k, 1))
                N.check(N.lib().rlr_engine_search_filtered(
                    self.index.handle, f.handle, q.ctypes.data_as(N.f32p), q.size, top_k,
                    C.byref(wc) if wc is not None else None, lr.ctypes.data_as(N.u64p), ls.ctypes.data_as(N.f32p), nl, stage,
                    hits, cap, C.byref(n)))
            return self._results(hits, n.value)
        if query_text is not None:
            # BM25 of the text beside the scan, blended on the device: one enqueue, one synchronisation
            tok = " ".join(tokenize(query_text)).encode("utf-8")
            N.check(N.lib().rlr_engine_search_text(self.index.handle, self.lexical._h, q.ctypes.data_as(N.f32p), q.size, tok,
                                                   len(tok), top_k, 0.0, stage, C.byref(wc) if wc is not None else None, hits,
                                                   cap, C.byref(n)))
            return self._results(hits, n.value)
        lr, ls, nl = self._lex(lexical, None, 5 * max(top_k, 1))   # top_k.max(1) then saturating_mul(5) :490, :505
        N.check(N.lib().rlr_engine_search(self.index.handle, q.ctypes.data_as(N.f32p), q.size, top_k,
                                          C.byref(wc) if wc is not None else None, lr.ctypes.data_as(N.u64p),
                                          ls.ctypes.data_as(N.f32p), nl, stage, hits, cap, C.byref(n)))
        return self._results(hits, n.value)

    # -- RagEngine::search_with_diversity (rag_engine.rs:717-759) --------------------------
    def search_with_diversity(self, query_embedding, top_k: int, diversity_factor: float,
                              weights: Optional[QueryWeights] = None,
                              lexical: Sequence[Tuple[str, float]] = (),
                              query_text: Optional[str] = None,
                              documents: Optional[Sequence[str]] = None,
                              per_document: Optional[int] = None) -> List[SearchResult]:
        """`documents`: as for search -- the MMR pool is then min(rows of the documents, max(3 top_k, top_k + 10)).
        `per_document`: as for search -- the cap is applied to the MMR pool, so it holds for the picks."""
        q = _f32(query_embedding).ravel()
        cap = max(3 * max(top_k, 1), top_k + 10)
        hits = (N.SearchHitC * cap)()
        n = C.c_uint32()
        lam = min(max(float(diversity_factor), 0.0), 1.0)
        k_eff = top_k if lam == 0.0 else max(3 * top_k, top_k + 10)  # the top_k `search` sees (:728-735)
        wc = weights.to_c() if weights is not None else None
        if per_document is not None:
            return self._search_capped(q, top_k, float(diversity_factor), 0, wc, lexical, query_text, documents, per_document,
                                       hits, cap, 5 * max(k_eff, 1))
        if documents is not None:
            f = self._filter_for(documents)
            if query_text is not None:
                tok = " ".join(tokenize(query_text)).encode("utf-8")
                N.check(N.lib().rlr_engine_search_text_filtered(
                    self.index.handle, self.lexical._h, f.handle, q.ctypes.data_as(N.f32p), q.size, tok, len(tok), top_k,
                    float(diversity_factor), 0, C.byref(wc) if wc is not None else None, hits, cap, C.byref(n)))
            else:
                lr, ls, nl = self._lex(lexical, None, 5 * max(k_eff, 1))
                N.check(N.lib().rlr_engine_search_with_diversity_filtered(
                    self.index.handle, f.handle, q.ctypes.data_as(N.f32p), q.size, top_k, float(diversity_factor),
                    C.byref(wc) if wc is not None else None, lr.ctypes.data_as(N.u64p), ls.ctypes.data_as(N.f32p), nl,
                    hits, cap, C.byref(n)))
            return self._results(hits, n.value)
        if query_text is not None:
            tok = " ".join(tokenize(query_text)).encode("utf-8")
            N.check(N.lib().rlr_engine_search_text(self.index.handle, self.lexical._h, q.ctypes.data_as(N.f32p), q.size, tok,
                                                   len(tok), top_k, float(diversity_factor), 0,
                                                   C.byref(wc) if wc is not None else None, hits, cap, C.byref(n)))
            return self._results(hits, n.value)
        lr, ls, nl = self._lex(lexical, None, 5 * max(k_eff, 1))    # search() treats 0 as 1 (:490) before * 5 (:505)
        N.check(N.lib().rlr_engine_search_with_diversity(
            self.index.handle, q.ctypes.data_as(N.f32p), q.size, top_k, float(diversity_factor),
            C.byref(wc) if wc is not None else None, lr.ctypes.data_as(N.u64p), ls.ctypes.data_as(N.f32p), nl,
            hits, cap, C.byref(n)))
        return self._results(hits, n.value)

    def _search_capped(self, q, top_k: int, diversity_factor: float, stage: int, wc, lexical, query_text, documents,
                       per_document: int, hits, cap: int, lex_limit: int) -> List[SearchResult]:
        """search / search_with_diversity with `per_document` set: rlr_engine_search_text_capped with a query text,
        rlr_engine_search_capped with the caller's BM25 pairs"""
        if not isinstance(per_document, int) or isinstance(per_document, bool) or not 1 <= per_document <= N.MAX_PER_DOCUMENT:
            raise ValueError(f"per_document must be an integer in 1..{N.MAX_PER_DOCUMENT}")
        if len(self._chunks) == 0:
            return []
        self._sync_documents()
        f = self._filter_for(documents) if documents is not None else None
        fh = f.handle if f is not None else None
        n = C.c_uint32()
        if query_text is not None:
            tok = " ".join(tokenize(query_text)).encode("utf-8")
            N.check(N.lib().rlr_engine_search_text_capped(
                self.index.handle, self.lexical._h, fh, q.ctypes.data_as(N.f32p), q.size, tok, len(tok), top_k,
                diversity_factor, stage, C.byref(wc) if wc is not None else None, per_document, hits, cap, C.byref(n)))
        else:
            lr, ls, nl = self._lex(lexical, None, lex_limit)
            N.check(N.lib().rlr_engine_search_capped(
                self.index.handle, fh, q.ctypes.data_as(N.f32p), q.size, top_k, diversity_factor, stage,
                C.byref(wc) if wc is not None else None, lr.ctypes.data_as(N.u64p), ls.ctypes.data_as(N.f32p), nl, per_document,
                hits, cap, C.byref(n)))
        return self._results(hits, n.value)

    def _search_capped_batch(self, q: np.ndarray, texts: Optional[Sequence[str]], top_k: int, diversity_factor: float,
                             stage: int, weights: Optional[QueryWeights], documents, per_document: int) -> List[List[SearchResult]]:
        """the batched entries with `per_document` set: rlr_engine_search_text_capped_batch with query texts (one batched
        BM25, then the capped batch), rlr_engine_search_capped_batch without -- per query what _search_capped returns"""
        if not isinstance(per_document, int) or isinstance(per_document, bool) or not 1 <= per_document <= N.MAX_PER_DOCUMENT:
            raise ValueError(f"per_document must be an integer in 1..{N.MAX_PER_DOCUMENT}")
        nq, dq = q.shape
        if len(self._chunks) == 0 or nq == 0:
            return [[] for _ in range(nq)]
        self._sync_documents()
        f = self._filter_for(documents) if documents is not None else None
        fh = f.handle if f is not None else None
        cap = max(3 * max(top_k, 1), top_k + 10)
        hits = (N.SearchHitC * (cap * nq))()
        n_out = np.zeros(nq, dtype=np.uint32)
        wc = weights.to_c() if weights is not None else None
        wp = C.byref(wc) if wc is not None else None
        offsets = np.zeros(nq + 1, dtype=np.uint64)
        if texts is not None:
            toks = [" ".join(tokenize(t)).encode("utf-8") for t in texts]
            offsets[1:] = np.cumsum([len(t) for t in toks], dtype=np.uint64)
            N.check(N.lib().rlr_engine_search_text_capped_batch(
                self.index.handle, self.lexical._h, fh, q.ctypes.data_as(N.f32p), dq, nq, b"".join(toks),
                offsets.ctypes.data_as(N.u64p), top_k, float(diversity_factor), stage, wp, per_document, hits, cap,
                n_out.ctypes.data_as(N.u32p)))
        else:
            N.check(N.lib().rlr_engine_search_capped_batch(
                self.index.handle, fh, q.ctypes.data_as(N.f32p), dq, nq, top_k, float(diversity_factor), stage, wp, None, None,
                offsets.ctypes.data_as(N.u64p), per_document, hits, cap, n_out.ctypes.data_as(N.u32p)))
        out = []
        for i in range(nq):
            view = (N.SearchHitC * cap).from_buffer(hits, i * cap * C.sizeof(N.SearchHitC))
            out.append(self._results(view, int(n_out[i])))
        return out

    # -- tail of RagEngine::search when a reranker answered (rag_engine.rs:599-700) --------------
    def finish_with_reranker(self, candidates: Sequence[SearchResult], reranked: Sequence[Tuple[str, float]],
                             top_k: int, weights: Optional[QueryWeights] = None) -> List[SearchResult]:
        """candidates: `search(..., stage=1)`; reranked: the reranker's (chunk_id, relevance) list in its
        order (empty = reranker absent/failed -> fallback ordering by initial score)."""
        n = len(candidates)
        cand = (N.SearchHitC * max(n, 1))()
        for i, r in enumerate(candidates):
            cand[i].row, cand[i].score, cand[i].embedding_score = r.row, r.score, r.embedding_score or 0.0
            cand[i].lexical_score, cand[i].initial_score = r.lexical_score or 0.0, r.initial_score or 0.0
        known = [(self._row_of[c], s) for c, s in reranked if c in self._row_of]
        rr = np.ascontiguousarray([r for r, _ in known] or [0], dtype=np.uint64)
        rs = np.ascontiguousarray([s for _, s in known] or [0], dtype=np.float32)
        top_k = max(top_k, 1)
        out = (N.SearchHitC * max(n, 1))()
        rer = np.zeros(max(n, 1), np.float32)
        has = np.zeros(max(n, 1), np.int32)
        n_out = C.c_uint32()
        wc = weights.to_c() if weights is not None else None
        N.check(N.lib().rlr_engine_blend_reranked(cand, n, rr.ctypes.data_as(N.u64p), rs.ctypes.data_as(N.f32p), len(known),
                                                  top_k, C.byref(wc) if wc is not None else None, out,
                                                  rer.ctypes.data_as(N.f32p), has.ctypes.data_as(N.i32p), max(n, 1),
                                                  C.byref(n_out)))
        res = self._results(out, n_out.value)
        for i, r in enumerate(res):
            r.reranker_score = float(rer[i]) if has[i] else None
        return res

    # -- additive batched entry point (oracle: loop search_with_diversity over the batch) -------
    def search_with_diversity_batch(self, query_embeddings, top_k: int, diversity_factor: float,
                                    weights: Optional[QueryWeights] = None,
                                    documents: Optional[Sequence[str]] = None,
                                    scopes: Optional[Sequence[Sequence[str]]] = None,
                                    per_document: Optional[int] = None) -> List[List[SearchResult]]:
        """`documents`: as for search_with_diversity -- every query searches only inside these documents (None: the
        whole corpus; an empty list or unknown names: no rows, an empty list per query); chunks of up to 8 queries
        share one masked pass over the documents' rows.
        `scopes`: one document list PER QUERY instead (not together with `documents`): query i is
        search_with_diversity(q_i, ..., documents=scopes[i]); chunks of up to 8 queries share one masked pass over the
        union of their scopes (rlr_engine_search_with_diversity_batch_scoped).
        `per_document`: as for search_with_diversity, through the batched capped search (not together with `scopes`);
        None: no cap, the paths below untouched."""
        q = _f32(query_embeddings)
        if q.ndim == 1:
            q = q.reshape(1, -1)
        nq, dq = q.shape
        if per_document is not None:
            if scopes is not None:
                raise ValueError("search_with_diversity_batch: `per_document` cannot be combined with `scopes`")
            return self._search_capped_batch(np.ascontiguousarray(q), None, top_k, float(diversity_factor), 0, weights, documents,
                                             per_document)
        cap = max(3 * max(top_k, 1), top_k + 10)
        hits = (N.SearchHitC * (cap * max(nq, 1)))()
        n_out = np.zeros(max(nq, 1), dtype=np.uint32)
        wc = weights.to_c() if weights is not None else None
        if scopes is not None:
            if documents is not None:
                raise ValueError("search_with_diversity_batch: give `documents` or `scopes`, not both")
            scopes = list(scopes)
            if len(scopes) != nq:
                raise ValueError(f"{nq} query embeddings but {len(scopes)} scopes")
            for s in scopes:  # (a look-up that finds the index replaced drops every cached filter, those made just before too)
                self._filter_for(s)
            filters = [self._filter_for(s) for s in scopes]
            handles = (C.c_void_p * max(nq, 1))(*[f.handle for f in filters])
            N.check(N.lib().rlr_engine_search_with_diversity_batch_scoped(
                self.index.handle, handles, q.ctypes.data_as(N.f32p), dq, nq, top_k, float(diversity_factor),
                C.byref(wc) if wc is not None else None, hits, cap, n_out.ctypes.data_as(N.u32p)))
        elif documents is not None:
            if not document_ranges(self._chunks, documents):
                return [[] for _ in range(nq)]
            f = self._filter_for(documents)
            N.check(N.lib().rlr_engine_search_with_diversity_batch_filtered(
                self.index.handle, f.handle, q.ctypes.data_as(N.f32p), dq, nq, top_k, float(diversity_factor),
                C.byref(wc) if wc is not None else None, hits, cap, n_out.ctypes.data_as(N.u32p)))
        else:
            N.check(N.lib().rlr_engine_search_with_diversity_batch(
                self.index.handle, q.ctypes.data_as(N.f32p), dq, nq, top_k, float(diversity_factor),
                C.byref(wc) if wc is not None else None, hits, cap, n_out.ctypes.data_as(N.u32p)))
        out = []
        for i in range(nq):
            view = (N.SearchHitC * cap).from_buffer(hits, i * cap * C.sizeof(N.SearchHitC))
            out.append(self._results(view, int(n_out[i])))
        return out

    # -- many query texts at once (oracle: search / search_with_diversity with query_text, per query) -------------
    def search_text_batch(self, query_embeddings, query_texts: Sequence[str], top_k: int, diversity_factor: float = 0.0,
                          weights: Optional[QueryWeights] = None, stage: int = 0, return_info: bool = False,
                          documents: Optional[Sequence[str]] = None,
                          scopes: Optional[Sequence[Sequence[str]]] = None,
                          per_document: Optional[int] = None):
        """`search_with_diversity(q, top_k, diversity_factor, weights, query_text=t)` (diversity 0: `search(q, top_k,
        weights, stage=stage, query_text=t)`) for every (q, t) pair, bit for bit, through the batched kernels.  Returns
        one result list per query, and with return_info also a dict of how the queries were served.
        `documents`: every query searches only inside these documents, as with `documents=` on the single calls (None:
        the whole corpus; an empty list or unknown names: no rows, an empty list per query) -- one masked batched BM25,
        one filtered top-k call, one scoring of the lexical rows and one MMR per sub-batch
        (rlr_engine_search_text_batch_filtered).
        `scopes`: one document list PER QUERY instead (not together with `documents`): query i is the single call with
        query_text=t_i and documents=scopes[i] ([] or unknown names: an empty scope, no results for that query) -- one
        batched BM25 with a mask per query, one scoped top-k call over the union of the scopes, one scoring of the lexical
        rows and one MMR per sub-batch (rlr_engine_search_text_batch_scoped).
        `per_document`: as on the single calls, through one batched BM25 and the batched capped search
        (rlr_engine_search_text_capped_batch; not together with `scopes`; the info dict is then all zeros); None: no
        cap, the paths below untouched."""
        if scopes is not None and documents is not None:
            raise ValueError("search_text_batch: give `documents` or `scopes`, not both")
        if scopes is not None and per_document is not None:
            raise ValueError("search_text_batch: `per_document` cannot be combined with `scopes`")
        q = _f32(query_embeddings)
        if q.ndim == 1:
            q = q.reshape(1, -1)
        nq, dq = q.shape
        if len(query_texts) != nq:
            raise ValueError(f"{nq} query embeddings but {len(query_texts)} query texts")
        if per_document is not None:
            res = self._search_capped_batch(np.ascontiguousarray(q), list(query_texts), top_k, float(diversity_factor), stage,
                                            weights, documents, per_document)
            if return_info:
                return res, {name: 0 for name, _ in N.TextBatchInfoC._fields_}
            return res
        if scopes is not None:
            scopes = list(scopes)
            if len(scopes) != nq:
                raise ValueError(f"{nq} query embeddings but {len(scopes)} scopes")
        toks = [" ".join(tokenize(t)).encode("utf-8") for t in query_texts]
        offsets = np.zeros(nq + 1, dtype=np.uint64)
        offsets[1:] = np.cumsum([len(t) for t in toks], dtype=np.uint64) if nq else []
        blob = b"".join(toks)
        cap = max(3 * max(top_k, 1), top_k + 10)   # the most hits a query can have (stage 1 or the MMR pool's cut)
        hits = (N.SearchHitC * (cap * max(nq, 1)))()
        n_out = np.zeros(max(nq, 1), dtype=np.uint32)
        info = N.TextBatchInfoC()
        wc = weights.to_c() if weights is not None else None
        tail = (q.ctypes.data_as(N.f32p), dq, nq, blob, offsets.ctypes.data_as(N.u64p), top_k, float(diversity_factor), stage,
                C.byref(wc) if wc is not None else None, hits, cap, n_out.ctypes.data_as(N.u32p), C.byref(info))
        if scopes is not None:
            for s in scopes:  # (a look-up that finds the index replaced drops every cached filter, those made just before too)
                self._filter_for(s)
            filters = [self._filter_for(s) for s in scopes]
            handles = (C.c_void_p * max(nq, 1))(*[f.handle for f in filters])
            N.check(N.lib().rlr_engine_search_text_batch_scoped(self.index.handle, self.lexical._h, handles, *tail))
        elif documents is None:
            N.check(N.lib().rlr_engine_search_text_batch(self.index.handle, self.lexical._h, *tail))
        elif document_ranges(self._chunks, documents):
            f = self._filter_for(documents)
            N.check(N.lib().rlr_engine_search_text_batch_filtered(self.index.handle, self.lexical._h, f.handle, *tail))
        out = []
        for i in range(nq):
            view = (N.SearchHitC * cap).from_buffer(hits, i * cap * C.sizeof(N.SearchHitC))
            out.append(self._results(view, int(n_out[i])))
        if return_info:
            return out, {name: int(getattr(info, name)) for name, _ in N.TextBatchInfoC._fields_}
        return out

    def search_documents_batch(self, requests: Sequence[SearchRequest], share_scopes: bool = False,
                               share_text_scopes: bool = False, share_capped: bool = False) -> List[List[SearchResult]]:
        """search_documents for every request, grouped by (top_k, diversity, weights, documents) after its caps and
        clamps.  Unscoped groups run through search_text_batch (a request without text is scored with no query terms);
        scoped groups without query text through search_with_diversity_batch(documents=...); the scoped requests of a
        group WITH query text through one search_text_batch(documents=...) when there are two or more of them, a lone
        one through search_documents.
        share_scopes: the scoped requests WITHOUT query text of one (top_k, diversity, weights) key go through one
        search_with_diversity_batch(scopes=...) call, whatever their scopes; everything else routes as above.
        share_text_scopes (independent of share_scopes): the scoped requests WITH query text of one (top_k, diversity,
        weights) key go through one search_text_batch(scopes=...) call, whatever their scopes, when there are two or
        more of them; a lone one through search_documents.
        share_capped: the requests that set per_document, of one (top_k, diversity, weights, documents, per_document)
        key, go through one batched capped call when there are two or more of them (those with query text through
        search_text_batch(per_document=...), those without through search_with_diversity_batch(per_document=...)); a
        lone one through search_documents.  False (the default): one search_documents call for each."""
        groups: Dict[tuple, List[int]] = {}
        shared: Dict[tuple, List[int]] = {}
        shared_text: Dict[tuple, List[int]] = {}
        capped: List[int] = []
        for i, r in enumerate(requests):
            if r.lexical:
                raise ValueError("search_documents_batch: requests carry caller-computed lexical pairs; "
                                 "use search_documents")
            if r.per_document is not None:
                capped.append(i)
                continue
            top_k = min(r.top_k if r.top_k is not None else N.DEFAULT_TOP_K, N.MAX_TOP_K)
            div = r.diversity_factor if r.diversity_factor is not None else N.DEFAULT_DIVERSITY
            div = min(max(div, 0.0), 1.0)
            w = r.weights
            wkey = None if w is None else (w.embedding, w.lexical, w.reranker, w.initial)
            scope = None if r.documents is None else frozenset(r.documents)  # ([] is a scope: no rows)
            if share_scopes and scope is not None and not r.query:
                shared.setdefault((top_k, div, wkey), []).append(i)
                continue
            if share_text_scopes and scope is not None and r.query:
                shared_text.setdefault((top_k, div, wkey), []).append(i)
                continue
            groups.setdefault((top_k, div, wkey, scope), []).append(i)
        out: List[List[SearchResult]] = [[] for _ in requests]
        if share_capped:  # (the batched capped search: one call per key and kind of request)
            capped_groups: Dict[tuple, List[int]] = {}
            for i in capped:
                r = requests[i]
                top_k = min(r.top_k if r.top_k is not None else N.DEFAULT_TOP_K, N.MAX_TOP_K)
                div = r.diversity_factor if r.diversity_factor is not None else N.DEFAULT_DIVERSITY
                div = min(max(div, 0.0), 1.0)
                w = r.weights
                wkey = None if w is None else (w.embedding, w.lexical, w.reranker, w.initial)
                scope = None if r.documents is None else frozenset(r.documents)
                # (a request without a query goes through the entry without text, as search_documents sends it)
                capped_groups.setdefault((top_k, div, wkey, scope, r.per_document, r.query is not None), []).append(i)
            for (top_k, div, _, scope, m, has_text), members in capped_groups.items():
                if len(members) < 2:
                    out[members[0]] = self.search_documents(requests[members[0]])
                    continue
                w = requests[members[0]].weights
                docs = None if scope is None else sorted(scope)
                emb = np.stack([_f32(requests[i].query_embedding).ravel() for i in members])
                if has_text:
                    res = self.search_text_batch(emb, [requests[i].query for i in members], top_k, div, w, documents=docs,
                                                 per_document=m)
                else:
                    res = self.search_with_diversity_batch(emb, top_k, div, w, documents=docs, per_document=m)
                for i, r_i in zip(members, res):
                    out[i] = r_i
        else:
            for i in capped:  # (one capped call each: the present loop)
                out[i] = self.search_documents(requests[i])
        for (top_k, div, _), members in shared.items():
            emb = np.stack([_f32(requests[i].query_embedding).ravel() for i in members])
            scopes = [sorted(set(requests[i].documents)) for i in members]
            for i, res in zip(members, self.search_with_diversity_batch(emb, top_k, div, requests[members[0]].weights,
                                                                        scopes=scopes)):
                out[i] = res
        for (top_k, div, _), members in shared_text.items():
            if len(members) < 2:  # (a batch of one is outside the fused path)
                out[members[0]] = self.search_documents(requests[members[0]])
                continue
            emb = np.stack([_f32(requests[i].query_embedding).ravel() for i in members])
            texts = [requests[i].query for i in members]
            scopes = [sorted(set(requests[i].documents)) for i in members]
            for i, res in zip(members, self.search_text_batch(emb, texts, top_k, div, requests[members[0]].weights,
                                                              scopes=scopes)):
                out[i] = res
        for (top_k, div, _, scope), members in groups.items():
            w = requests[members[0]].weights
            if scope is None:
                emb = np.stack([_f32(requests[i].query_embedding).ravel() for i in members])
                texts = [requests[i].query or "" for i in members]
                for i, res in zip(members, self.search_text_batch(emb, texts, top_k, div, w)):
                    out[i] = res
                continue
            plain = [i for i in members if not requests[i].query]
            if plain:
                emb = np.stack([_f32(requests[i].query_embedding).ravel() for i in plain])
                for i, res in zip(plain, self.search_with_diversity_batch(emb, top_k, div, w, documents=sorted(scope))):
                    out[i] = res
            text = [i for i in members if requests[i].query]
            if len(text) >= 2:
                emb = np.stack([_f32(requests[i].query_embedding).ravel() for i in text])
                texts = [requests[i].query for i in text]
                for i, res in zip(text, self.search_text_batch(emb, texts, top_k, div, w, documents=sorted(scope))):
                    out[i] = res
            elif text:  # (a batch of one is outside the fused path)
                out[text[0]] = self.search_documents(requests[text[0]])
        return out

    # -- RagEngine::get_embedding_candidates (rag_engine.rs:415-461) -----------------------
    def get_embedding_candidates(self, query_embedding, count: int) -> List[Tuple[str, float]]:
        q = _f32(query_embedding).ravel()
        rows = np.zeros(max(count, 1), dtype=np.uint64)
        sc = np.zeros(max(count, 1), dtype=np.float32)
        n = C.c_uint32()
        N.check(N.lib().rlr_engine_embedding_candidates(self.index.handle, q.ctypes.data_as(N.f32p), q.size, count,
                                                        rows.ctypes.data_as(N.u64p), sc.ctypes.data_as(N.f32p),
                                                        C.byref(n)))
        return [(self._chunks[int(rows[i])].id, float(sc[i])) for i in range(n.value)]

    # -- at most `per_document` chunks from any one document (rlr_search_topk_grouped; no reference site) ----
    def search_per_document(self, query_embedding, top_k: int, per_document: int = 1,
                            documents: Optional[Sequence[str]] = None) -> List[SearchResult]:
        """The best `top_k` chunks by cosine with at most `per_document` (1..8) from any one document, selected on the
        device.  Embedding-only: score = embedding_score = initial_score = the cosine, the lexical score is 0; the query
        is normalised as `search` normalises it.  `documents`: only inside these (as `search`)."""
        if top_k <= 0 or len(self._chunks) == 0:
            return []
        self._sync_documents()
        f = self._filter_for(documents) if documents is not None else None
        q = normalize(_f32(query_embedding).ravel())
        rows, cos, _ = self.index.search_topk_grouped(q, top_k, per_document, filter=f)[0]
        out = []
        for row, c in zip(rows.tolist(), cos.tolist()):
            ch = self._chunks[row]
            out.append(SearchResult(ch.text, c, ch.document_name, ch.id, ch.chunk_index, ch.page_number, ch.section,
                                    c, 0.0, c, None, None, None, row))
        return out

    def rank_documents(self, query_embedding, top_k: int,
                       documents: Optional[Sequence[str]] = None) -> List[Tuple[str, SearchResult]]:
        """The `top_k` documents closest to the query, each with its best chunk: search_per_document with one chunk
        per document, keyed by document name."""
        return [(r.document, r) for r in self.search_per_document(query_embedding, top_k, 1, documents)]

    def search_per_document_batch(self, query_embeddings, top_k: int, per_document: int = 1,
                                  documents: Optional[Sequence[str]] = None) -> List[List[SearchResult]]:
        """search_per_document for every row of `query_embeddings` through one search_topk_grouped_batch call: the rows
        are read once per shared pass, not once per query.  Per query exactly what search_per_document returns."""
        emb = _f32(query_embeddings).reshape(-1, self.dim)
        if top_k <= 0 or len(self._chunks) == 0 or emb.shape[0] == 0:
            return [[] for _ in range(emb.shape[0])]
        self._sync_documents()
        f = self._filter_for(documents) if documents is not None else None
        q = np.stack([normalize(e) for e in emb])
        res = self.index.search_topk_grouped_batch(q, top_k, per_document, filter=f)
        return [self._embedding_results(rows, cos) for rows, cos, _ in res]

    def rank_documents_batch(self, query_embeddings, top_k: int,
                             documents: Optional[Sequence[str]] = None) -> List[List[Tuple[str, SearchResult]]]:
        """rank_documents for every row of `query_embeddings`, the queries sharing passes over the rows"""
        return [[(r.document, r) for r in res] for res in self.search_per_document_batch(query_embeddings, top_k, 1, documents)]

    # -- every chunk at or above a cosine, and how many (rlr_search_range; no reference site) ---------------
    def _embedding_results(self, rows, cos) -> List[SearchResult]:
        out = []
        for row, c in zip(rows.tolist(), cos.tolist()):
            ch = self._chunks[row]
            out.append(SearchResult(ch.text, c, ch.document_name, ch.id, ch.chunk_index, ch.page_number, ch.section,
                                    c, 0.0, c, None, None, None, row))
        return out

    def search_above(self, query_embedding, min_score: float, limit: int = 100,
                     documents: Optional[Sequence[str]] = None) -> Tuple[List[SearchResult], int]:
        """Every chunk whose cosine with the query is at least `min_score`: the best `limit` of them in (cosine desc, row
        asc) order and the exact number of such chunks, whatever `limit` is.  Embedding-only (score = embedding_score =
        initial_score = the cosine, lexical score 0); the query is normalised as `search` normalises it.  `documents`:
        only inside these (as `search`)."""
        if len(self._chunks) == 0:
            return [], 0
        f = self._filter_for(documents) if documents is not None else None
        q = _f32(query_embedding).ravel()
        cap = max(int(limit), 0)
        hits = (N.SearchHitC * max(cap, 1))()
        n, total = C.c_uint32(), C.c_uint64()
        N.check(N.lib().rlr_engine_search_range(self.index.handle, f.handle if f is not None else None, q.ctypes.data_as(N.f32p),
                                                q.size, float(min_score), cap, hits, C.byref(n), C.byref(total)))
        return self._results(hits, n.value), int(total.value)

    def count_above(self, query_embedding, min_score: float, documents: Optional[Sequence[str]] = None) -> int:
        """how many chunks score at least `min_score` (nothing is fetched)"""
        return self.search_above(query_embedding, min_score, 0, documents)[1]

    def similar_chunks(self, chunk_id: str, min_score: float, limit: int = 100,
                       documents: Optional[Sequence[str]] = None) -> Tuple[List[SearchResult], int]:
        """The chunks at or above `min_score` against a STORED chunk (its row as the query, as stored: the rows are the
        reference's normalised values), without the chunk itself; the total does not count it either."""
        row = self._row_of[chunk_id]
        f = self._filter_for(documents) if documents is not None else None
        q = self.index.fetch_rows([row])[0]
        rows, cos, total = self.index.search_range(q, min_score, max(int(limit), 0) + 1, filter=f)[0]
        in_scope = documents is None or self._chunks[row].document_name in set(documents)
        if in_scope and self.index.score_rows(q, [row])[0] >= np.float32(min_score):
            total -= 1                                       # the chunk itself is one of the hits
        keep = rows != np.uint64(row)
        rows, cos = rows[keep][:max(int(limit), 0)], cos[keep][:max(int(limit), 0)]
        return self._embedding_results(rows, cos), total

    def _duplicates_of(self, emb: np.ndarray, min_score: float, f: Optional[RowFilter] = None) -> List[List[str]]:
        """per row of `emb` (raw embeddings, normalised here as the append normalises them): the ids of the chunks in
        the index (inside `f`) at or above `min_score`, best first -- one search_range_batch call: the rows are read
        once per shared pass, not once per embedding"""
        if len(self._chunks) == 0 or emb.shape[0] == 0:
            return [[] for _ in range(emb.shape[0])]
        q = np.stack([normalize(e) for e in emb])
        res = self.index.search_range_batch(q, min_score, 256, filter=f)
        out = []
        for i, (rows, _, total) in enumerate(res):
            if total > rows.size:                            # (a boilerplate chunk: fetch them all)
                rows = self.index.search_range(q[i], min_score, total, filter=f)[0][0]
            out.append([self._chunks[int(r)].id for r in rows])
        return out

    def duplicates_of(self, embeddings, min_score: float, documents: Optional[Sequence[str]] = None) -> List[List[str]]:
        """Per embedding (raw; normalised as add_document normalises them): the ids of the stored chunks whose cosine
        with it is at least `min_score`, best first -- what add_document(report_duplicates_above=) reports, without
        adding anything.  `documents`: only inside these (as `search`).  The embeddings share passes over the rows."""
        emb = _f32(embeddings).reshape(-1, self.dim)
        if len(self._chunks) == 0:
            return [[] for _ in range(emb.shape[0])]
        f = self._filter_for(documents) if documents is not None else None
        return self._duplicates_of(emb, float(min_score), f)

    def duplicate_chunks(self, min_score: float, limit_per_chunk: int = 256) -> List[Tuple[str, str, float]]:
        """The corpus against itself: every pair of stored chunks whose cosine is at least `min_score`, as (id_a, id_b,
        cosine) with row_a < row_b, each pair once, a chunk never with itself; ordered by row_a, then best first.  Blocks
        of up to 256 stored rows are fetched and used as the queries of one search_range_batch call each, so the whole
        comparison costs ceil(N / 256) passes over the rows, not N.  `limit_per_chunk` bounds the hits looked at per
        chunk (its best ones, the chunk itself among them): a chunk with more partners than that reports its best."""
        n = len(self._chunks)
        cap = max(int(limit_per_chunk), 1)
        pairs: List[Tuple[str, str, float]] = []
        for first in range(0, n, 256):
            block = np.arange(first, min(first + 256, n))
            q = self.index.fetch_rows(block)
            for a, (rows, cos, _) in zip(block.tolist(), self.index.search_range_batch(q, min_score, cap)):
                for b, c in zip(rows.tolist(), cos.tolist()):
                    if b > a:
                        pairs.append((self._chunks[a].id, self._chunks[b].id, c))
        return pairs

    # -- API layer: search_documents / http_search (mcp_server.rs:81-110, :371-389) --------
    def search_documents(self, request: SearchRequest) -> List[SearchResult]:
        top_k = min(request.top_k if request.top_k is not None else N.DEFAULT_TOP_K, N.MAX_TOP_K)
        div = request.diversity_factor if request.diversity_factor is not None else N.DEFAULT_DIVERSITY
        div = min(max(div, 0.0), 1.0)
        return self.search_with_diversity(request.query_embedding, top_k, div, request.weights, request.lexical,
                                          request.query, request.documents, request.per_document)


def format_search_results(results: Sequence[SearchResult]) -> str:
    """mcp_server.rs:599-637"""
    if not results:
        return "No results found."
    parts = []
    for i, r in enumerate(results):
        provenance = f"{r.document} (page {r.page_number})" if r.page_number > 0 else r.document
        section = f"*Section: {r.section}*\n" if r.section is not None else ""
        x = float(np.float32(r.score) * np.float32(100.0))
        # f32::round: half away from zero
        percentage = int(np.floor(abs(x) + 0.5) * (1 if x >= 0 else -1))
        parts.append(f"**{i + 1}. [{percentage}%] {provenance}**\n{section}\n{r.text}\n")
    return "\n---\n\n".join(parts)
