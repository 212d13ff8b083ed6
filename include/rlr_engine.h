/*
 * rlr_engine.h -- host-side mirror of the reference's operator interface for the hot
 * path, layered on the device ABI of rlr_gpu.h.  It is what RagEngine::search /
 * search_with_diversity / get_embedding_candidates (rust-local-rag
 * src/rag_engine.rs:470-701, :717-759, :415-461) do between "query embedding obtained"
 * (:493) and "results handed back" -- same names, argument meaning and edge-case
 * behaviour -- written in C++ because this image has no Rust toolchain.  A Rust host
 * binds rlr_gpu.h directly and keeps its own copy of this logic.
 *
 * Everything that is not the hot path stays with the caller: the query string ->
 * embedding step (embeddings.rs), BM25 (`LexicalIndex::score`, passed in as
 * (row, score) pairs), the LLM reranker and chunk metadata.
 */
#ifndef RLR_ENGINE_H
#define RLR_ENGINE_H

#include "rlr_gpu.h"
#include "rlr_lexical.h"

#ifdef __cplusplus
extern "C" {
#endif

/* QueryWeights (rag_engine.rs:1846-1865): optional per-query overrides. */
typedef struct rlr_query_weights {
    int32_t has_embedding;
    float embedding;
    int32_t has_lexical;
    float lexical;
    int32_t has_reranker;
    float reranker;
    int32_t has_initial;
    float initial;
} rlr_query_weights;

/* ResolvedWeights (rag_engine.rs:1877-1896) */
typedef struct rlr_resolved_weights {
    float embedding, lexical, reranker, initial;
} rlr_resolved_weights;

/* SearchResult's numeric fields (rag_engine.rs:72-100); `row` stands in for chunk_id. */
typedef struct rlr_search_hit {
    uint64_t row;
    float score;           /* = initial_score when no reranker ran (:682) */
    float embedding_score; /* raw cosine (:689) */
    float lexical_score;   /* bm25 / max_bm25, 0 if the row is not a lexical candidate (:527-530) */
    float initial_score;   /* w_e * embedding + w_l * lexical (:531-532) */
} rlr_search_hit;

/* API-layer constants (mcp_server.rs:85-86, :359-364) */
#define RLR_MAX_TOP_K 100
#define RLR_DEFAULT_TOP_K 5
#define RLR_DEFAULT_DIVERSITY 0.3f

/* resolve_weight (rag_engine.rs:1869-1873): override if finite and in [0,1], else default */
float rlr_resolve_weight(int32_t has_override, float w, float dflt);
/* ResolvedWeights::from_query_weights (:1888-1895); defaults 0.7/0.3/0.7/0.3 or the
 * RAG_{EMBEDDING,LEXICAL,RERANKER,INITIAL_SCORE}_WEIGHT environment (:1813-1841), cached
 * on first use like the reference's OnceLock. `w` may be NULL. */
void rlr_resolve_weights(const rlr_query_weights *w, rlr_resolved_weights *out);
/* normalize (rag_engine.rs:1763-1771), host side, reference order. */
void rlr_normalize(float *v, size_t n);

/* RagEngine::search, exact-scan branch, reranker absent.
 *   query_raw/dq  raw query embedding (normalised here, :494; zip-truncated or
 *                 zero-extended to the index dim like dot_product's zip, :1778)
 *   top_k         0 is treated as 1 (:490)
 *   lex_*         LexicalIndex::score output as (row, bm25) pairs, may be empty
 *   stage         0: final results, min(top_k, N) hits (:667-698)
 *                 1: the initial_k = min(N, max(3*top_k, top_k)) candidates a reranker
 *                    would receive (:544-561)
 * Ordering: (initial_score desc, row asc), NaN last -- the build's definition of the
 * reference's unspecified tie order. */
int32_t rlr_engine_search(rlr_index *idx, const float *query_raw, uint32_t dq, uint32_t top_k,
                          const rlr_query_weights *weights, const uint64_t *lex_rows,
                          const float *lex_scores, uint32_t n_lex, int32_t stage,
                          rlr_search_hit *out, uint32_t cap, uint32_t *n_out);

/* RagEngine::search_with_diversity (:717-759): clamp lambda, lambda == 0 -> search,
 * else pool = max(3k, k+10), search(pool), MMR on the GPU. */
int32_t rlr_engine_search_with_diversity(rlr_index *idx, const float *query_raw, uint32_t dq,
                                         uint32_t top_k, float diversity_factor,
                                         const rlr_query_weights *weights, const uint64_t *lex_rows,
                                         const float *lex_scores, uint32_t n_lex,
                                         rlr_search_hit *out, uint32_t cap, uint32_t *n_out);

/* search / search_with_diversity as the reference calls them from search_documents (mcp_server.rs:81-110): with the
 * query TEXT, whose BM25 scores it blends in (`self.lexical_index.score(query, top_k.saturating_mul(5))`, :505).
 * `query_tokens`: the host's tokenize(query), space separated (as for rlr_lexical_score); `lex`: the GPU LexicalIndex
 * whose rows are the rows of `idx`.  diversity_factor == 0 (after the clamp): search(top_k) with `stage` as in
 * rlr_engine_search; otherwise search_with_diversity (stage ignored).  Same results as rlr_lexical_score followed by
 * rlr_engine_search / rlr_engine_search_with_diversity with its pairs -- but the BM25 kernels run on their own stream
 * beside the cosine scan, their result never leaves the device, and blend, ordering, cut and MMR follow in the same
 * enqueue: one host synchronisation per query (0.85 -> 0.31 ms at 100 k chunks).  Falls back to exactly those
 * two calls when the fused kernels do not cover the request (w_embedding == 0, more than 1024 candidates kept or
 * 2048 lexical pairs, a rounding-tie chain at the fetch boundary). */
int32_t rlr_engine_search_text(rlr_index *idx, rlr_lexical *lex, const float *query_raw, uint32_t dq,
                               const char *query_tokens, size_t tokens_len, uint32_t top_k, float diversity_factor,
                               int32_t stage, const rlr_query_weights *weights, rlr_search_hit *out, uint32_t cap,
                               uint32_t *n_out);

/* rlr_engine_search_text for many queries at once: what a host with a batch of query texts at hand (an eval run, a
 * request queue) would otherwise get from n_queries single calls, bit for bit -- same rows, order and score bits per query,
 * whichever path a query takes inside.  Query q: raw embedding queries_raw + q * dq, tokens
 * tokens[token_offsets[q] .. token_offsets[q + 1]) (space separated, as for rlr_lexical_score); hits at out[q * cap],
 * n_out[q] of them.  top_k, diversity_factor, stage and weights apply to the whole batch with the meaning they have in
 * rlr_engine_search_text.  The BM25 of every query runs in one chain on the lexical index' stream (LDS accumulators per
 * (query, row slice), term-order sums, no dense per-query accumulator), beside one batched top-k of the cosine side;
 * exact cosines of the lexical rows, blend, order and cut follow for every query at once, then one batched MMR: two host
 * synchronisations per sub-batch of up to 256 queries.  Queries the fused kernels cannot decide are re-run alone through
 * rlr_engine_search_text (`info`, may be NULL, says how many and why).  Holds the lexical readers' lock per sub-batch;
 * other searches may run concurrently; never joins a coalesced group.  RLR_E_INVALID: a null index, lexical index or
 * output, decreasing token_offsets, or cap below the result count of a query (min(top_k, N) or initial_k). */
typedef struct rlr_text_batch_info {
    uint32_t n_batched;        /* queries served end to end by the batched kernels */
    uint32_t n_single;         /* queries re-run alone through rlr_engine_search_text; the three below sum to it */
    uint32_t n_single_lexical; /* ... because their BM25 selection handed back (the batched selection is exact: 0 today) */
    uint32_t n_single_blend;   /* ... because a rounding tie reached the cosine fetch boundary / pool undecidable */
    uint32_t n_single_shape;   /* ... because the request is outside the fused kernels (w_embedding == 0, pool > 1024,
                                *     > 2048 lexical pairs, > 128 unique known terms in the query, a batch of one) */
} rlr_text_batch_info;
int32_t rlr_engine_search_text_batch(rlr_index *idx, rlr_lexical *lex, const float *queries_raw, uint32_t dq,
                                     uint32_t n_queries, const char *tokens, const uint64_t *token_offsets,
                                     uint32_t top_k, float diversity_factor, int32_t stage,
                                     const rlr_query_weights *weights, rlr_search_hit *out, uint32_t cap,
                                     uint32_t *n_out, rlr_text_batch_info *info);

/* ---- the same searches inside a set of rows (rlr_filter, include/rlr_gpu.h: "search only in these documents") ----
 * search_F is the reference's search over the corpus that holds only the rows of the filter F, in ascending row order,
 * with the rows mapped back to index rows.  Two choices are made here and hold for all three entry points:
 *   - N is |F| everywhere the reference uses the corpus size: top_k is clamped to |F|, initial_k = min(|F|, 3 * top_k),
 *     the MMR pool is min(|F|, max(3 * top_k, top_k + 10)), and |F| = 0 returns no hits with RLR_OK (:476-478);
 *   - the lexical term keeps the statistics of the WHOLE lexical index (total_docs, average length, df, idf): the
 *     filter restricts candidates, not corpus statistics.  The lexical candidates of _search_text_filtered are the
 *     limit = 5 * k_eff best rows of F with bm25 > 0 by (bm25 desc, row asc) (rlr_lexical_score_filtered), and
 *     max_lexical (:515-519) is taken over that list.
 * (lex_rows given to the first two that lie outside F are not candidates, exactly as rows beyond the corpus are not in
 * rlr_engine_search; like those they still count towards max_lexical.)  Blend, pool sizing, tie widening and fall-backs
 * are the code of the unfiltered and sharded engines (csrc/engine_host.h) over rlr_search_topk_filtered,
 * rlr_score_rows and rlr_mmr_select; _search_text_filtered runs rlr_lexical_score_filtered and then one of the other
 * two (two host synchronisations: the fused one-enqueue hybrid path takes no filter).  A stale filter, or one of another
 * index: RLR_E_INVALID. */
int32_t rlr_engine_search_filtered(rlr_index *idx, const rlr_filter *f, const float *query_raw, uint32_t dq, uint32_t top_k,
                                   const rlr_query_weights *weights, const uint64_t *lex_rows, const float *lex_scores,
                                   uint32_t n_lex, int32_t stage, rlr_search_hit *out, uint32_t cap, uint32_t *n_out);
int32_t rlr_engine_search_with_diversity_filtered(rlr_index *idx, const rlr_filter *f, const float *query_raw, uint32_t dq,
                                                  uint32_t top_k, float diversity_factor, const rlr_query_weights *weights,
                                                  const uint64_t *lex_rows, const float *lex_scores, uint32_t n_lex,
                                                  rlr_search_hit *out, uint32_t cap, uint32_t *n_out);
int32_t rlr_engine_search_text_filtered(rlr_index *idx, rlr_lexical *lex, const rlr_filter *f, const float *query_raw,
                                        uint32_t dq, const char *query_tokens, size_t tokens_len, uint32_t top_k,
                                        float diversity_factor, int32_t stage, const rlr_query_weights *weights,
                                        rlr_search_hit *out, uint32_t cap, uint32_t *n_out);
/* RagEngine::search / search_with_diversity with at most per_doc results from any one document (the document column of
 * include/rlr_gpu.h; rows tagged RLR_DOC_NONE and an index without a column are never capped), over the whole index
 * (f null) or inside a filter.  The query is normalised and the weights are resolved as the other entries do; `need` is
 * what the uncapped entry computes over the allowed rows: min(top_k, N) at stage 0, initial_k at stage 1,
 * min(N, max(3*top_k, top_k + 10)) under diversification (diversity_factor clamped to 0..1, != 0).  The candidates are
 * walked in combined order and a row is accepted unless per_doc rows of its document are (rlr_search_capped); under
 * diversification the accepted list is the pool of mmr_diversify, so the cap holds for the picks.  Fewer than `need`
 * accepted rows is no error.  per_doc outside 1..RLR_MAX_PER_DOCUMENT: RLR_E_INVALID; a stale filter: RLR_E_INVALID; an
 * empty filter or index: RLR_OK with *n_out = 0.  One host synchronisation. */
int32_t rlr_engine_search_capped(rlr_index *idx, const rlr_filter *f, const float *query_raw, uint32_t dq, uint32_t top_k,
                                 float diversity_factor, int32_t stage, const rlr_query_weights *weights,
                                 const uint64_t *lex_rows, const float *lex_scores, uint32_t n_lex, uint32_t per_doc,
                                 rlr_search_hit *out, uint32_t cap, uint32_t *n_out);
/* The same from query text: rlr_lexical_score (rlr_lexical_score_filtered with a filter) with the limit
 * rlr_engine_search_text uses, then the capped chain.  Two host synchronisations (the BM25 call, the search). */
int32_t rlr_engine_search_text_capped(rlr_index *idx, rlr_lexical *lex, const rlr_filter *f, const float *query_raw,
                                      uint32_t dq, const char *query_tokens, size_t tokens_len, uint32_t top_k,
                                      float diversity_factor, int32_t stage, const rlr_query_weights *weights,
                                      uint32_t per_doc, rlr_search_hit *out, uint32_t cap, uint32_t *n_out);
/* rlr_engine_search_capped for n_queries requests that share top_k, diversity_factor, stage, the weights, per_doc and
 * the filter: every query is prepared as that entry prepares it and the selection is ONE rlr_search_capped_batch
 * (include/rlr_gpu.h), so per query the hits carry the bits of the single entry.  Query q is queries_raw + q * dq; its
 * caller-computed pairs are lex_rows / lex_scores [lex_offsets[q], lex_offsets[q + 1]) (n_queries + 1 non-decreasing
 * offsets).  Hits of query q start at out[q * cap], their count is n_out[q]; cap must hold a query's largest result.
 * Argument and error rules as for rlr_engine_search_capped. */
int32_t rlr_engine_search_capped_batch(rlr_index *idx, const rlr_filter *f, const float *queries_raw, uint32_t dq,
                                       uint32_t n_queries, uint32_t top_k, float diversity_factor, int32_t stage,
                                       const rlr_query_weights *weights, const uint64_t *lex_rows, const float *lex_scores,
                                       const uint64_t *lex_offsets, uint32_t per_doc, rlr_search_hit *out, uint32_t cap,
                                       uint32_t *n_out);
/* The same from query text, laid out as rlr_engine_search_text_batch takes it (a token blob and n_queries + 1 offsets):
 * ONE rlr_lexical_score_batch (rlr_lexical_score_batch_filtered with a filter) with the limit
 * rlr_engine_search_text_capped uses, then the capped batch -- two host synchronisations per set of chunks instead of two
 * per query.  Where that limit is outside what the batched BM25 takes, every query goes through
 * rlr_engine_search_text_capped. */
int32_t rlr_engine_search_text_capped_batch(rlr_index *idx, rlr_lexical *lex, const rlr_filter *f, const float *queries_raw,
                                            uint32_t dq, uint32_t n_queries, const char *tokens, const uint64_t *token_offsets,
                                            uint32_t top_k, float diversity_factor, int32_t stage,
                                            const rlr_query_weights *weights, uint32_t per_doc, rlr_search_hit *out,
                                            uint32_t cap, uint32_t *n_out);
/* Every chunk whose cosine with the query is at least min_cosine, and how many there are (rlr_search_range,
 * include/rlr_gpu.h), over the whole index (f null) or inside a filter.  No reference site: the reference only colours
 * results by fixed score thresholds.  The query is normalised as rlr_engine_search does (rlr_normalize, zip-truncated
 * or zero-extended to the index dim); hits are filled as get_embedding_candidates defines them (w_e = 1, no lexical
 * term): score = embedding_score = initial_score = the cosine, lexical_score = 0.  *n_total_out is the exact number of
 * hits whatever cap is; the first min(n_total, cap) in (cosine desc, row asc) order go to out, *n_out is their count.
 * cap == 0 only counts (out and n_out may be null).  A NaN min_cosine, a stale filter: RLR_E_INVALID; an empty filter
 * or index: RLR_OK with both counts 0. */
int32_t rlr_engine_search_range(rlr_index *idx, const rlr_filter *f, const float *query_raw, uint32_t dq, float min_cosine,
                                uint32_t cap, rlr_search_hit *out, uint32_t *n_out, uint64_t *n_total_out);
/* rlr_engine_search_range for n_queries raw query embeddings (dq floats each) with a threshold each, through ONE
 * rlr_search_range_batch call: the queries share passes over the rows (include/rlr_gpu.h).  Query q equals
 * rlr_engine_search_range(query q, min_cosine[q]) bit for bit; its hits start at out[q * cap], n_out[q] is their count,
 * n_total_out[q] the exact number of hits.  cap == 0 only counts (out and n_out may be null). */
int32_t rlr_engine_search_range_batch(rlr_index *idx, const rlr_filter *f, const float *queries_raw, uint32_t n_queries,
                                      uint32_t dq, const float *min_cosine, uint32_t cap, rlr_search_hit *out,
                                      uint32_t *n_out, uint64_t *n_total_out);
/* rlr_engine_search_with_diversity_batch inside a filter: n_queries raw query embeddings, no lexical pairs; query q
 * equals rlr_engine_search_with_diversity_filtered(query q, n_lex = 0), N = |F| everywhere.  Hits of query q start at
 * out[q * cap]; n_out[q] = their count (every one 0 when |F| = 0).  The candidates come from ONE
 * rlr_search_topk_filtered call -- chunks of up to 8 queries share one masked pass over f32 rows of 256 / 512 / 768 /
 * 1024 elements; binary16 rows, other widths and other pitches run query by query -- and the MMR from
 * rlr_mmr_select_batch.  Argument checks and error codes of rlr_engine_search_with_diversity_batch; a stale filter, or
 * one of another index: RLR_E_INVALID before any GPU work.  Queries WITH text inside a filter:
 * rlr_engine_search_text_batch_filtered (one filter) and rlr_engine_search_text_batch_scoped (a filter per query) below. */
int32_t rlr_engine_search_with_diversity_batch_filtered(rlr_index *idx, const rlr_filter *f, const float *queries_raw,
                                                        uint32_t dq, uint32_t n_queries, uint32_t top_k,
                                                        float diversity_factor, const rlr_query_weights *weights,
                                                        rlr_search_hit *out, uint32_t cap, uint32_t *n_out);
/* The same with a filter PER QUERY (requests scoped to different documents): query q equals
 * rlr_engine_search_with_diversity_filtered(idx, filters[q], query q, n_lex = 0), and N is |F_q| per query -- need_q =
 * min(|F_q|, k_eff) with k_eff = top_k (diversity 0) or max(3 * top_k, top_k + 10), fetch_q = min(|F_q|, need_q + 8).
 * ONE rlr_search_topk_scoped call with the largest fetch (chunks of up to 8 queries share one masked pass over the
 * union of their scopes), ONE rlr_mmr_select_batch with pool_sizes[q] = need_q.  An empty filter gives n_out[q] = 0.
 * The fall-backs of the other batched calls: w_embedding == 0 or a pool above 1024 loops the single call; a query whose
 * rounding-tie chain reaches its last fetched row is re-run alone.  A null array, a null, stale or foreign entry:
 * RLR_E_INVALID before any GPU work.  Queries WITH text and a filter each: rlr_engine_search_text_batch_scoped. */
int32_t rlr_engine_search_with_diversity_batch_scoped(rlr_index *idx, const rlr_filter *const *filters,
                                                      const float *queries_raw, uint32_t dq, uint32_t n_queries,
                                                      uint32_t top_k, float diversity_factor,
                                                      const rlr_query_weights *weights, rlr_search_hit *out, uint32_t cap,
                                                      uint32_t *n_out);
/* rlr_engine_search_text_batch inside a filter: query q equals rlr_engine_search_text_filtered(query q, tokens q), bit
 * for bit, N = |F| everywhere (|F| = 0: no hits, RLR_OK).  Per sub-batch of up to 256 queries: one masked batched BM25
 * (rlr_lexical_score_batch_filtered, limit = 5 * k_seen as the single call computes it), one rlr_search_topk_filtered
 * call for all queries with fetch = min(|F|, need + the longest lexical list + 8), one batched scoring of every query's
 * lexical rows, the single call's blend arithmetic per query on the host, one rlr_mmr_select_batch -- one host
 * synchronisation per stage.  A query whose rounding-tie chain reaches the last fetched row is re-run alone through
 * rlr_engine_search_text_filtered (info->n_single_blend); the whole call loops that entry point (n_single_shape) when
 * w_embedding == 0, a weight is not finite, more than 1024 candidates are kept, or the batch has one query.  A query with more than 128 unique
 * known terms has its BM25 scored alone inside the lexical call and stays in the batch.  Argument checks of
 * rlr_engine_search_text_batch; a null, stale or foreign filter: RLR_E_INVALID before any GPU work. */
int32_t rlr_engine_search_text_batch_filtered(rlr_index *idx, rlr_lexical *lex, const rlr_filter *f, const float *queries_raw,
                                              uint32_t dq, uint32_t n_queries, const char *tokens,
                                              const uint64_t *token_offsets, uint32_t top_k, float diversity_factor,
                                              int32_t stage, const rlr_query_weights *weights, rlr_search_hit *out,
                                              uint32_t cap, uint32_t *n_out, rlr_text_batch_info *info);
/* The same with a filter PER QUERY -- the request mcp_server.rs:89-93 serves carries a query text and a document list of
 * its own, so a request queue holds text queries scoped to different documents.  Query q equals
 * rlr_engine_search_text_filtered(idx, lex, filters[q], query q, tokens q, ...), bit for bit; N is |F_q| per query where
 * the reference uses the corpus size (:476-478, :490, :544, :734), so need_q, the pool size and the result count differ
 * inside one batch, while the BM25 limit = 5 * k_seen (:505) depends on top_k alone.  Per sub-batch of
 * text_sub_batch(largest need) queries: ONE rlr_lexical_score_batch_scoped (a grid row per query with its own mask), ONE
 * rlr_search_topk_scoped with k = the largest min(|F_q|, need_q + lexical count of q + 8) -- query q looks at its own
 * first min(|F_q|, need_q + its lexical count + 8) rows, the fetch of the single call's first round -- one batched scoring
 * of the lexical rows, the single call's blend per query (:515-532) with that query's N and need, and ONE
 * rlr_mmr_select_batch with P = the largest need and pool_sizes[q] = need_q.  A query with an empty filter gets
 * n_out[q] = 0 and counts neither in n_batched nor in n_single.  A query whose rounding-tie chain reaches its last
 * looked-at row is re-run alone (n_single_blend); the whole call loops the single entry point (n_single_shape counts every
 * query) when w_embedding == 0, a weight is not finite, the largest need is above 1024, or the batch has one query.
 * Entries of `filters` may repeat.  A null array, a null, stale or foreign entry, or a cap below the result count of some
 * query: RLR_E_INVALID before any GPU work; the other argument checks of rlr_engine_search_text_batch_filtered. */
int32_t rlr_engine_search_text_batch_scoped(rlr_index *idx, rlr_lexical *lex, const rlr_filter *const *filters,
                                            const float *queries_raw, uint32_t dq, uint32_t n_queries, const char *tokens,
                                            const uint64_t *token_offsets, uint32_t top_k, float diversity_factor,
                                            int32_t stage, const rlr_query_weights *weights, rlr_search_hit *out,
                                            uint32_t cap, uint32_t *n_out, rlr_text_batch_info *info);

/* Additive batched entry point (the reference has no batched API; its oracle is "loop
 * search_with_diversity over the batch"): n_queries raw query embeddings,
 * no lexical candidates.  Hits of query q start at out[q * cap]; n_out[q] = their count.
 * The scan runs through the batched (matrix-core) path of rlr_search_topk and the MMR through
 * rlr_mmr_select_batch; results are identical to n_queries single calls. */
int32_t rlr_engine_search_with_diversity_batch(rlr_index *idx, const float *queries_raw, uint32_t dq,
                                               uint32_t n_queries, uint32_t top_k, float diversity_factor,
                                               const rlr_query_weights *weights, rlr_search_hit *out,
                                               uint32_t cap, uint32_t *n_out);

/* The tail of RagEngine::search once a reranker has answered (:599-700), SURVEY 8(f) row f2:
 * blended = w_reranker * relevance/max_relevance + w_initial * initial/max_initial over the
 * stage-1 candidates the reranker scored (in the reranker's order, unknown/repeated rows
 * skipped), stable sort desc, truncate to top_k, then fill from the remaining candidates by
 * initial score.  Pure host arithmetic on <= 3*top_k items.
 *   candidates / n_candidates   output of rlr_engine_search(stage = 1)
 *   rer_rows / rer_relevance    the reranker's (row, relevance) list; n_reranked == 0 = reranker
 *                               absent or failed -> pure fallback ordering
 *   out / has_reranker_out / reranker_score_out   final results (score = blended or initial),
 *                               per-result flag and raw relevance (SearchResult.reranker_score) */
int32_t rlr_engine_blend_reranked(const rlr_search_hit *candidates, uint32_t n_candidates,
                                  const uint64_t *rer_rows, const float *rer_relevance, uint32_t n_reranked,
                                  uint32_t top_k, const rlr_query_weights *weights, rlr_search_hit *out,
                                  float *reranker_score_out, int32_t *has_reranker_out, uint32_t cap,
                                  uint32_t *n_out);

/* RagEngine::get_embedding_candidates (:415-461), `None` arm: top `count` by cosine. */
int32_t rlr_engine_embedding_candidates(rlr_index *idx, const float *query_raw, uint32_t dq,
                                        uint32_t count, uint64_t *rows_out, float *scores_out,
                                        uint32_t *n_out);

/* ---- the same entry points over a corpus sharded across several GPUs in ONE process (rlr_multi, include/rlr_gpu.h) ----
 * The reference is a single-process server whose surface is RagEngine::search / search_with_diversity
 * (rag_engine.rs:470-475, :717-723, called from mcp_server.rs:89-93); a corpus that does not fit one GPU (BASELINE
 * config 4: 100 M x 768 f32) is held by an rlr_multi and searched through these.  Same arguments, defaults, fall-backs
 * and results as the rlr_engine_* functions above over one index holding every row -- the host logic is the same code
 * (csrc/engine_host.h) on the sharded primitives: per-shard scan + exchange + merge for the candidates
 * (rlr_multi_search_topk: host merge or RCCL all-gather, rlr_multi_set_exchange), reference-order cosines of the
 * lexical rows from the shards that own them, and MMR with the on-fabric winner-row exchange
 * (rlr_multi_mmr_select(_batch)).  Row numbers are global.  `lex` of _search_text is ONE GPU LexicalIndex over the
 * global rows (BM25 postings are small next to the embeddings; they stay on one device). */
int32_t rlr_multi_engine_search(rlr_multi *m, const float *query_raw, uint32_t dq, uint32_t top_k,
                                const rlr_query_weights *weights, const uint64_t *lex_rows, const float *lex_scores,
                                uint32_t n_lex, int32_t stage, rlr_search_hit *out, uint32_t cap, uint32_t *n_out);
int32_t rlr_multi_engine_search_with_diversity(rlr_multi *m, const float *query_raw, uint32_t dq, uint32_t top_k,
                                               float diversity_factor, const rlr_query_weights *weights,
                                               const uint64_t *lex_rows, const float *lex_scores, uint32_t n_lex,
                                               rlr_search_hit *out, uint32_t cap, uint32_t *n_out);
int32_t rlr_multi_engine_search_text(rlr_multi *m, rlr_lexical *lex, const float *query_raw, uint32_t dq,
                                     const char *query_tokens, size_t tokens_len, uint32_t top_k, float diversity_factor,
                                     int32_t stage, const rlr_query_weights *weights, rlr_search_hit *out, uint32_t cap,
                                     uint32_t *n_out);
/* BASELINE config 5's shape (1024 queries, top-100, lambda 0.7 over a sharded corpus): one batched top-k per shard +
 * exchange, per-query pools, one batched cross-shard MMR. */
int32_t rlr_multi_engine_search_with_diversity_batch(rlr_multi *m, const float *queries_raw, uint32_t dq,
                                                     uint32_t n_queries, uint32_t top_k, float diversity_factor,
                                                     const rlr_query_weights *weights, rlr_search_hit *out,
                                                     uint32_t cap, uint32_t *n_out);
int32_t rlr_multi_engine_embedding_candidates(rlr_multi *m, const float *query_raw, uint32_t dq, uint32_t count,
                                              uint64_t *rows_out, float *scores_out, uint32_t *n_out);

/* ---- corpus file at scale ---------------------------------------------------------
 * `chunks_{model}.json` (PersistedState, rag_engine.rs:1478-1499; read whole with serde_json :1555-1557) read
 * in one streaming pass over the memory-mapped file: the embedding arrays go straight into a dense row-major f32
 * matrix (row r = the r-th chunk of the file; decimal -> binary64 correctly rounded -> binary32, serde_json's f32
 * path; null = a non-finite value; shorter / longer arrays are zero-extended / truncated to `dim` like
 * dot_product's zip :1778), everything else is copied verbatim into `meta_json`, the same document with every
 * embedding array replaced by [] -- id, text, metadata, document_hashes, version, model: small enough for the
 * host's own JSON library.  Buffers are malloc'ed; release them with rlr_json_free_corpus. */
typedef struct rlr_json_corpus {
    float *rows;       /* n_rows x dim */
    uint64_t n_rows;
    uint32_t dim;
    char *meta_json;   /* NUL-terminated */
    uint64_t meta_len;
} rlr_json_corpus;
int32_t rlr_json_load_corpus(const char *path, uint32_t dim, rlr_json_corpus *out);
void rlr_json_free_corpus(rlr_json_corpus *c);
/* The same, uploaded: replaces all rows of `idx` (rlr_index_upload; normalize_on_device = 1 reproduces the
 * reference's re-normalise-on-load :1678-1680 on the GPU).  `meta_out` (nullable) receives the metadata document
 * (rows == NULL there: they live in HBM). */
int32_t rlr_index_load_json(rlr_index *idx, const char *path, int32_t normalize_on_device, rlr_json_corpus *meta_out);
/* One embedding as save_to_disk writes it (:1477-1518, serde_json pretty printer): "[", one value per line at
 * indent + 2 spaces -- the shortest decimal that reads back as the same binary32, non-finite as null -- and "]" at
 * `indent`.  Returns the bytes needed; the text was written (no terminating NUL) only if that is <= cap. */
uint64_t rlr_json_format_embedding(const float *v, uint32_t dim, uint32_t indent, char *out, uint64_t cap);

#ifdef __cplusplus
}
#endif
#endif /* RLR_ENGINE_H */
