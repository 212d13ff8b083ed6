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

} // extern "C"
