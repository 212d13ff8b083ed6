// engine_capped.cpp -- rlr_engine_search_capped / rlr_engine_search_text_capped (include/rlr_engine.h): RagEngine::search /
// search_with_diversity with at most per_doc candidates from any one document, over the whole index or inside a row
// filter.  The host half is what the other engine entries do -- normalise the query, resolve the weights, the lexical map
// with max_lexical, the sizes of engine_host.h -- and the selection is rlr_search_capped (include/rlr_gpu.h): one scan, the
// cap in combined order on the device, the MMR chain behind it.  A translation unit of its own, as engine_filtered.cpp is.
// Compiled with -ffp-contract=off like engine.cpp.
#include "../../include/rlr_engine.h"
#include "../../include/rlr_lexical.h"
#include "engine_host.h"
#include "filter_internal.h"
#include "lexical_internal.h"

#include <algorithm>
#include <vector>

using namespace rlr_host;

extern "C" {

int32_t rlr_engine_search_capped(rlr_index *idx, const rlr_filter *f, const float *query_raw, uint32_t dq, uint32_t top_k,
                                 float diversity_factor, int32_t stage, const rlr_query_weights *weights, const uint64_t *lex_rows,
                                 const float *lex_scores, uint32_t n_lex, uint32_t per_doc, rlr_search_hit *out, uint32_t cap,
                                 uint32_t *n_out)
{
    if (!idx || !n_out || (!query_raw && dq) || (n_lex && (!lex_rows || !lex_scores)))
        return RLR_E_INVALID;
    *n_out = 0;
    if (per_doc < 1 || per_doc > RLR_MAX_PER_DOCUMENT)
        return RLR_E_INVALID;
    uint64_t n_index = 0, N = 0;
    uint32_t dim = 0;
    int32_t st = rlr_index_info(idx, &n_index, &dim, nullptr, nullptr);
    if (st != RLR_OK)
        return st;
    N = n_index;
    rlr::FilterView v{};
    if (f) {
        if ((st = rlr::filter_check(idx, f)) != RLR_OK) // a stale filter, or one of another index: before any GPU work
            return st;
        if ((st = rlr::filter_view(f, &v)) != RLR_OK)
            return st;
        N = v.n_allowed;
    }
    if (N == 0) // :476-478
        return RLR_OK;
    const TextSizes ts = text_sizes(top_k, diversity_factor);
    const uint64_t need = need_of(N, ts.k_seen, ts.diversify ? 0 : stage);
    rlr_resolved_weights w;
    rlr_resolve_weights(weights, &w);
    const std::vector<float> q = prepare_query(query_raw, dq, dim);
    const LexPrep lex = prepare_lexical_in(
        [&](uint64_t row) { return f ? row < v.index_rows && ((v.h_mask[row >> 6] >> (row & 63)) & 1ull) : row < n_index; }, lex_rows,
        lex_scores, n_lex);
    const uint32_t nd = static_cast<uint32_t>(std::min<uint64_t>(need, 0xFFFFFFFFull));
    const uint32_t n_res_max = rlr::result_k_cap(top_k, nd, ts.diversify);
    if (!out || cap < n_res_max)
        return RLR_E_INVALID;
    std::vector<uint64_t> rows(n_res_max);
    std::vector<float> cosv(n_res_max), comb(n_res_max), lexv(n_res_max);
    uint32_t n = 0;
    st = rlr_search_capped(idx, f, q.data(), nd, top_k, ts.lambda, ts.diversify ? 1 : 0, w.embedding, w.lexical, lex.rows.data(),
                           lex.scores.data(), static_cast<uint32_t>(lex.rows.size()), lex.max_lex, per_doc, -1.0f, rows.data(),
                           cosv.data(), comb.data(), lexv.data(), nullptr, &n);
    if (st != RLR_OK)
        return st;
    for (uint32_t i = 0; i < n; ++i) {
        out[i].row = rows[i];
        out[i].score = comb[i];
        out[i].embedding_score = cosv[i];
        out[i].lexical_score = lexv[i];
        out[i].initial_score = comb[i];
    }
    *n_out = n;
    return RLR_OK;
}

int32_t rlr_engine_search_text_capped(rlr_index *idx, rlr_lexical *lex, const rlr_filter *f, const float *query_raw, uint32_t dq,
                                      const char *query_tokens, size_t tokens_len, uint32_t top_k, float diversity_factor,
                                      int32_t stage, const rlr_query_weights *weights, uint32_t per_doc, rlr_search_hit *out,
                                      uint32_t cap, uint32_t *n_out)
{
    if (!idx || !lex || !n_out || (!query_raw && dq) || (tokens_len && !query_tokens))
        return RLR_E_INVALID;
    *n_out = 0;
    const TextSizes ts = text_sizes(top_k, diversity_factor); // the sizes rlr_engine_search_text works with
    std::vector<uint64_t> lrows(ts.lcap);
    std::vector<float> lscores(ts.lcap);
    uint32_t n_lex = 0;
    const int32_t st = f ? rlr_lexical_score_filtered(lex, f, query_tokens, tokens_len, ts.limit, lrows.data(), lscores.data(), &n_lex)
                         : rlr_lexical_score(lex, query_tokens, tokens_len, ts.limit, lrows.data(), lscores.data(), &n_lex);
    if (st != RLR_OK)
        return st;
    return rlr_engine_search_capped(idx, f, query_raw, dq, top_k, diversity_factor, stage, weights, lrows.data(), lscores.data(), n_lex,
                                    per_doc, out, cap, n_out);
}

// rlr_engine_search_capped for n_queries queries: every query prepared as that entry prepares it, then ONE
// rlr_search_capped_batch.  Query q's pairs are lex_rows / lex_scores [lex_offsets[q], lex_offsets[q + 1]).
int32_t rlr_engine_search_capped_batch(rlr_index *idx, const rlr_filter *f, const float *queries_raw, uint32_t dq, uint32_t n_queries,
                                       uint32_t top_k, float diversity_factor, int32_t stage, const rlr_query_weights *weights,
                                       const uint64_t *lex_rows, const float *lex_scores, const uint64_t *lex_offsets, uint32_t per_doc,
                                       rlr_search_hit *out, uint32_t cap, uint32_t *n_out)
{
    if (!idx || (n_queries && (!n_out || !lex_offsets || (dq && !queries_raw))))
        return RLR_E_INVALID;
    for (uint32_t q = 0; q < n_queries; ++q)
        n_out[q] = 0;
    for (uint32_t q = 0; q < n_queries; ++q)
        if (lex_offsets[q + 1] < lex_offsets[q] || lex_offsets[q + 1] - lex_offsets[q] > 0xFFFFFFFFull)
            return RLR_E_INVALID;
    if (n_queries && lex_offsets[n_queries] > lex_offsets[0] && (!lex_rows || !lex_scores))
        return RLR_E_INVALID;
    if (per_doc < 1 || per_doc > RLR_MAX_PER_DOCUMENT)
        return RLR_E_INVALID;
    uint64_t n_index = 0, N = 0;
    uint32_t dim = 0;
    int32_t st = rlr_index_info(idx, &n_index, &dim, nullptr, nullptr);
    if (st != RLR_OK)
        return st;
    N = n_index;
    rlr::FilterView v{};
    if (f) {
        if ((st = rlr::filter_check(idx, f)) != RLR_OK) // a stale filter, or one of another index: before any GPU work
            return st;
        if ((st = rlr::filter_view(f, &v)) != RLR_OK)
            return st;
        N = v.n_allowed;
    }
    if (N == 0 || n_queries == 0) // :476-478
        return RLR_OK;
    const TextSizes ts = text_sizes(top_k, diversity_factor);
    const uint64_t need = need_of(N, ts.k_seen, ts.diversify ? 0 : stage);
    rlr_resolved_weights w;
    rlr_resolve_weights(weights, &w);
    const uint32_t nd = static_cast<uint32_t>(std::min<uint64_t>(need, 0xFFFFFFFFull));
    const uint32_t n_res_max = rlr::result_k_cap(top_k, nd, ts.diversify);
    if (!out || cap < n_res_max)
        return RLR_E_INVALID;
    std::vector<float> qs(static_cast<size_t>(n_queries) * dim);
    std::vector<uint64_t> lrows, loff(static_cast<size_t>(n_queries) + 1, 0);
    std::vector<float> lscores, max_lex(n_queries);
    for (uint32_t q = 0; q < n_queries; ++q) {
        const std::vector<float> pq = prepare_query(queries_raw ? queries_raw + static_cast<size_t>(q) * dq : nullptr, dq, dim);
        std::copy(pq.begin(), pq.end(), qs.begin() + static_cast<size_t>(q) * dim);
        const LexPrep lex = prepare_lexical_in(
            [&](uint64_t row) { return f ? row < v.index_rows && ((v.h_mask[row >> 6] >> (row & 63)) & 1ull) : row < n_index; },
            lex_rows + lex_offsets[q], lex_scores + lex_offsets[q], static_cast<uint32_t>(lex_offsets[q + 1] - lex_offsets[q]));
        lrows.insert(lrows.end(), lex.rows.begin(), lex.rows.end());
        lscores.insert(lscores.end(), lex.scores.begin(), lex.scores.end());
        loff[q + 1] = lrows.size();
        max_lex[q] = lex.max_lex;
    }
    const size_t n_slots = static_cast<size_t>(n_queries) * nd;
    std::vector<uint64_t> rows(n_slots);
    std::vector<float> cosv(n_slots), comb(n_slots), lexv(n_slots);
    std::vector<uint32_t> got(n_queries, 0);
    st = rlr_search_capped_batch(idx, f, qs.data(), n_queries, nd, top_k, ts.lambda, ts.diversify ? 1 : 0, w.embedding, w.lexical,
                                 lrows.data(), lscores.data(), loff.data(), max_lex.data(), per_doc, -1.0f, rows.data(), cosv.data(),
                                 comb.data(), lexv.data(), nullptr, got.data());
    if (st != RLR_OK)
        return st;
    for (uint32_t q = 0; q < n_queries; ++q) {
        rlr_search_hit *o = out + static_cast<size_t>(q) * cap;
        const size_t b = static_cast<size_t>(q) * nd;
        const uint32_t n = std::min(got[q], cap);
        for (uint32_t i = 0; i < n; ++i) {
            o[i].row = rows[b + i];
            o[i].score = comb[b + i];
            o[i].embedding_score = cosv[b + i];
            o[i].lexical_score = lexv[b + i];
            o[i].initial_score = comb[b + i];
        }
        n_out[q] = n;
    }
    return RLR_OK;
}

// rlr_engine_search_text_capped for n_queries queries: ONE batched BM25 call with the limit the single entry uses, then
// the capped batch -- two host synchronisations per chunk-set instead of two per query.  A limit the batched BM25 does not
// take (beyond RLR_LEXICAL_MAX_LIMIT) sends the call through the single entry, query by query.
int32_t rlr_engine_search_text_capped_batch(rlr_index *idx, rlr_lexical *lex, const rlr_filter *f, const float *queries_raw,
                                            uint32_t dq, uint32_t n_queries, const char *tokens, const uint64_t *token_offsets,
                                            uint32_t top_k, float diversity_factor, int32_t stage, const rlr_query_weights *weights,
                                            uint32_t per_doc, rlr_search_hit *out, uint32_t cap, uint32_t *n_out)
{
    if (!idx || !lex || !text_batch_args(queries_raw, dq, n_queries, tokens, token_offsets, n_out))
        return RLR_E_INVALID;
    if (n_queries == 0)
        return RLR_OK;
    const TextSizes ts = text_sizes(top_k, diversity_factor);
    if (ts.limit < 1 || ts.limit > RLR_LEXICAL_MAX_LIMIT) {
        if (!out)
            return RLR_E_INVALID;
        for (uint32_t q = 0; q < n_queries; ++q) {
            const int32_t st = rlr_engine_search_text_capped(
                idx, lex, f, queries_raw ? queries_raw + static_cast<size_t>(q) * dq : nullptr, dq, tokens ? tokens + token_offsets[q] : nullptr,
                static_cast<size_t>(token_offsets[q + 1] - token_offsets[q]), top_k, diversity_factor, stage, weights, per_doc,
                out + static_cast<size_t>(q) * cap, cap, &n_out[q]);
            if (st != RLR_OK)
                return st;
        }
        return RLR_OK;
    }
    std::vector<uint64_t> lrows(static_cast<size_t>(n_queries) * ts.limit), loff(static_cast<size_t>(n_queries) + 1, 0);
    std::vector<float> lscores(lrows.size());
    std::vector<uint32_t> n_lex(n_queries, 0);
    const int32_t st = f ? rlr_lexical_score_batch_filtered(lex, f, n_queries, tokens, token_offsets, ts.limit, lrows.data(), lscores.data(),
                                                            n_lex.data(), nullptr, nullptr)
                         : rlr_lexical_score_batch(lex, n_queries, tokens, token_offsets, ts.limit, lrows.data(), lscores.data(),
                                                   n_lex.data(), nullptr, nullptr);
    if (st != RLR_OK)
        return st;
    // (the pairs of query q start at q * limit: packed to offsets)
    for (uint32_t q = 0; q < n_queries; ++q) {
        const size_t from = static_cast<size_t>(q) * ts.limit, to = loff[q];
        if (from != to) {
            std::copy(lrows.begin() + from, lrows.begin() + from + n_lex[q], lrows.begin() + to);
            std::copy(lscores.begin() + from, lscores.begin() + from + n_lex[q], lscores.begin() + to);
        }
        loff[q + 1] = to + n_lex[q];
    }
    return rlr_engine_search_capped_batch(idx, f, queries_raw, dq, n_queries, top_k, diversity_factor, stage, weights, lrows.data(),
                                          lscores.data(), loff.data(), per_doc, out, cap, n_out);
}

} // extern "C"
