// lexical_internal.h -- library-internal view of a BM25 scoring call that leaves its result on the device, so the hybrid
// search (csrc/engine.cpp: rlr_engine_search_text) can run it beside the cosine scan and blend without a host round trip.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

struct rlr_lexical;
struct rlr_index;

namespace rlr {

// An enqueued scoring call.  From lexical_enqueue to lexical_finish the caller holds one of the index' workspaces and
// its readers' lock: mutators wait, other scoring calls do not.
struct LexPending {
    rlr_lexical *lx = nullptr;
    void *ws = nullptr;                 // the leased workspace
    void *stream = nullptr;             // hipStream_t: its stream; `ready` is recorded there behind the last kernel
    void *ready = nullptr;              // hipEvent_t (opaque here: csrc/engine.cpp is built without the HIP headers)
    const uint64_t *d_packed = nullptr; // pack_result(score, row) keys, the best `*d_count` by (score desc, row asc)
    const uint32_t *d_count = nullptr;  // how many of them are valid (<= limit)
    uint32_t limit = 0;                 // 0: no document can match (empty index / unknown terms) -- nothing was enqueued
    bool locked = false;
    bool may_retry = false; // the sampled selection was used: the count may read kLexicalRetry
    bool unpacked = false;  // the scoring stream also wrote the rows / scores / header a LexSink asked for (in front of `ready`)
};

// Where a hybrid search wants a scoring call's result unpacked (index_fused.hip: lex_unpack_kernel): lexical_enqueue launches that
// on ITS stream in front of `ready`, so the search's own stream finds rows, scores and header (count, max score) in place
// when it has joined -- one dependent launch less behind the join.
struct LexSink {
    uint32_t *d_rows = nullptr; // `n_bound` slots
    float *d_scores = nullptr;  // `n_bound` slots
    void *d_header = nullptr;   // HybridLexHeader
    uint32_t n_bound = 0;       // most pairs the search takes
    uint32_t n_index_rows = 0;  // rows of the embedding index (pairs beyond it are marked, see lex_unpack_kernel)
};
// (index_fused.hip) no error check inside: the caller's hipGetLastError sees it
void launch_lex_unpack(const uint64_t *d_packed, const uint32_t *d_count, uint32_t limit, const LexSink &sink, void *stream);

// LexicalIndex::score (rag_engine.rs:2169-2225) up to the ordered result list in device memory.  No synchronisation.
// need_sorted = false: d_packed holds the same set in no particular order (saves the final LDS sort; lexical_fetch
// needs the sorted form)
// exact_passes = false lets large candidate sets go through the sampled 3-launch selection: *d_count (and lexical_fetch's
// *n_out) may then read kLexicalRetry -- repeat the call with exact_passes = true
int32_t lexical_enqueue(rlr_lexical *lx, const char *tokens, size_t len, uint32_t limit, LexPending *out, bool need_sorted,
                        bool exact_passes, const LexSink *sink = nullptr);
constexpr uint32_t kLexicalRetry = 0xFFFFFFFFu;
// copy the result to the host (synchronises the scoring stream); valid between enqueue and finish
int32_t lexical_fetch(LexPending *p, uint64_t *rows_out, float *scores_out, uint32_t *n_out);
// rlr_lexical_score without the sampled attempt, for a query whose fused search came back with kLexicalRetry (status 3):
// counts the retry (rlr_lexical_segments: select_retries) and goes straight to the exact radix passes
int32_t lexical_score_exact(rlr_lexical *lx, const char *tokens, size_t len, uint32_t limit, uint64_t *rows_out,
                            float *scores_out, uint32_t *n_out);
// hand the workspace back once every consumer of d_packed has finished (the caller synchronised them);
// ok = false: something failed after the enqueue -- the workspace is re-zeroed before its next use
void lexical_finish(LexPending *p, bool ok);

// index_fused.hip: rlr_search_hybrid (include/rlr_gpu.h) in two enqueues, so that the BM25 kernels can be launched in between:
// begin puts the scan .. sort of the need + n_lex_bound + 8 best rows by cosine on the index' stream (*fallback != 0: not
// covered by the fused kernels, no ticket); finish joins `lex` (null or limit 0: no lexical pair) by event, enqueues
// blend .. results, synchronises and consumes the ticket; abort drains and frees a ticket that will not be finished.
struct HybridTicket;
// behind_scan (may be null): called once the scan is queued and before the select .. sort launches are -- the place to launch
// work for another stream that should run beside the scan (a BM25 call hands the LexSink it gets on to lexical_enqueue);
// not called when *fallback != 0; its error is begin's error.
int32_t search_hybrid_begin(rlr_index *ix, const float *query, uint32_t need, uint32_t k, float lambda, int32_t diversify,
                            float w_embedding, float w_lexical, uint32_t n_lex_bound, float guard_eps, HybridTicket **ticket,
                            int32_t *fallback, int32_t (*behind_scan)(void *, const LexSink *) = nullptr,
                            void *behind_scan_arg = nullptr);
int32_t search_hybrid_finish(HybridTicket *ticket, const LexPending *lex, uint64_t *rows_out, float *cos_out, float *score_out,
                             float *lex_out, uint32_t *n_out, int32_t *fallback);
void search_hybrid_abort(HybridTicket *ticket);

// ---- many queries at once (csrc/engine.cpp: rlr_engine_search_text_batch) ------------------------------------------------
// Where a batched hybrid search wants the lexical pairs of query q: rows / scores at [q * bound, ...), header q (index_fused.hip's
// HybridLexHeader: count, max score), as lex_unpack_kernel writes them for one query.
struct LexBatchSink {
    uint32_t *d_rows = nullptr;
    float *d_scores = nullptr;
    void *d_headers = nullptr;
    uint32_t bound = 0;        // slots per query (>= limit)
    uint32_t n_index_rows = 0; // rows of the embedding index (pairs beyond it are marked)
};
struct LexBatchPending {
    rlr_lexical *lx = nullptr;
    void *ws = nullptr;    // the leased workspace
    void *ready = nullptr; // hipEvent_t recorded behind the unpack: the sink is complete there
    bool locked = false;   // the readers' lock, held from enqueue to finish
    std::vector<uint64_t> table; // the uploaded term table (kept until the copy has run)
};
// BM25 of nq queries (tokens[offsets[q] .. offsets[q + 1]) each) -> the best `limit` (<= sink.bound, <= RLR_LEXICAL_MAX_LIMIT)
// pairs of every query unpacked into `sink`, on the workspace's stream.  No synchronisation.  too_many_terms[q] = 1: the
// query has more unique known terms than the batched kernel takes; it was left without pairs (score it alone).
// filter (may be null: every row): the view of a current row filter on the device of `lx` (filter_internal.h; the caller
// checked both) -- only its rows are candidates, with the semantics of rlr_lexical_score_filtered per query; the caller
// keeps the filter alive until lexical_batch_finish.
// scopes (may be null; exclusive with filter): nq such views, one per query (entries may repeat) -- query q's candidates are
// the rows of scopes[q], with the semantics of rlr_lexical_score_filtered(scopes[q]) per query; a query with an empty scope
// gets no terms and costs nothing.  The views may belong to indexes of different sizes.
struct FilterView;
int32_t lexical_batch_enqueue(rlr_lexical *lx, uint32_t nq, const char *tokens, const uint64_t *offsets, uint32_t limit,
                              const LexBatchSink &sink, uint8_t *too_many_terms, LexBatchPending *out,
                              const FilterView *filter = nullptr, const FilterView *scopes = nullptr);
// drains the workspace's stream, hands it back and drops the readers' lock (also after a failed enqueue)
void lexical_batch_finish(LexBatchPending *p, bool ok);
// (index_fused.hip) query q's keys at d_sel[q * sel_stride], count at d_count[q * count_stride]; no error check inside
void launch_lex_unpack_batch(const uint64_t *d_sel, uint32_t sel_stride, const uint32_t *d_count, uint32_t count_stride,
                             uint32_t nq, uint32_t limit, const LexBatchSink &sink, void *stream);

// The most results a fused search returns -- MMR picks k (at least one) of the `need` pool rows, a search
// without diversification returns the pool.
inline uint32_t result_k_cap(uint32_t k, uint32_t need, bool diversify)
{
    return diversify ? std::max<uint32_t>(std::min<uint32_t>(std::max<uint32_t>(k, 1u), need), 1u) : need;
}

// index_fused.hip: the cosine side, blend and MMR of nq hybrid searches at once.  `queries`: nq prepared (normalised, dim-long)
// queries; `need`, `k`, `lambda`, `diversify`, weights, `n_lex_bound` as for search_hybrid_begin.  lex_launch (may be null:
// no lexical pairs) is called once the workspace exists, before the cosine batch: it enqueues the BM25 chain into the sink
// on its own stream and returns the event to join (*ready).  Results of query q at [q * k_cap, ...) with k_cap =
// result_k_cap(k, need, diversify); status[q] != 0: not decided here (1 overflow, 2 fetch boundary) --
// the caller re-runs that query alone.  Two host synchronisations: the cosine batch and the results.
int32_t search_hybrid_batch(rlr_index *ix, const float *queries, uint32_t nq, uint32_t need, uint32_t k, float lambda,
                            int32_t diversify, float w_embedding, float w_lexical, uint32_t n_lex_bound,
                            int32_t (*lex_launch)(void *, const LexBatchSink *, void **ready), void *lex_arg, uint64_t *rows_out,
                            float *cos_out, float *score_out, float *lex_out, uint32_t *n_out, uint32_t *status);

} // namespace rlr
