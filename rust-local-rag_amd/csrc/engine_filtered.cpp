// engine_filtered.cpp -- rlr_engine_search_filtered / _search_with_diversity_filtered / _search_text_filtered /
// _search_with_diversity_batch_filtered / _search_with_diversity_batch_scoped / _search_text_batch_filtered /
// _search_text_batch_scoped (include/rlr_engine.h): RagEngine::search / search_with_diversity inside a row filter.  The corpus the reference's
// code sees is the filter's rows in ascending order: the host half is engine_host.h over a backend whose candidate
// universe is the filter -- its size where the reference uses the corpus size, its bit where a lexical pair is checked
// against the corpus, its first rows where w_embedding == 0 enumerates rows -- and whose top-k is
// rlr_search_topk_filtered.  score_rows and mmr are the unfiltered ones: the rows they are given are allowed rows already.
// A translation unit of its own, as text_batch.cpp is: engine.cpp stays free of the filtered device entry points.
// Compiled with -ffp-contract=off like engine.cpp.
#include "../../include/rlr_engine.h"
#include "../../include/rlr_lexical.h"
#include "engine_host.h"
#include "filter_internal.h"
#include "lexical_internal.h"

#include <algorithm>
#include <cmath>
#include <vector>

using namespace rlr_host;

namespace {

struct FilteredBackend {
    rlr_index *idx;
    const rlr_filter *f;
    rlr::FilterView v;
    uint64_t n_rows = 0; // |F|
    uint32_t dim = 0;
    bool holds(uint64_t row) const { return row < v.index_rows && ((v.h_mask[row >> 6] >> (row & 63)) & 1ull); }
    void first_rows(uint64_t take, uint64_t *rows) const
    {
        uint64_t at = 0;
        const uint64_t n_words = (v.index_rows + 63) / 64;
        for (uint64_t w = 0; w < n_words && at < take; ++w)
            for (uint64_t m = v.h_mask[w]; m && at < take; m &= m - 1)
                rows[at++] = w * 64 + static_cast<uint64_t>(__builtin_ctzll(m));
    }
    int32_t topk(const float *queries, uint32_t nq, uint32_t k, uint64_t *rows, float *cos, uint32_t *n) const
    {
        return rlr_search_topk_filtered(idx, f, queries, nq, k, -1.0f, rows, cos, n);
    }
    int32_t score_rows(const float *query, const uint64_t *rows, uint32_t n, float *cos) const
    {
        return rlr_score_rows(idx, query, rows, n, cos);
    }
    int32_t mmr(const uint64_t *pool_rows, const float *pool_scores, const uint32_t *pool_sizes, uint32_t nq, uint32_t P,
                uint32_t k, float lambda, uint32_t *order, uint32_t *n_sel) const
    {
        if (nq == 1)
            return rlr_mmr_select(idx, pool_rows, pool_scores, pool_sizes[0], k, lambda, order, nullptr, n_sel);
        return rlr_mmr_select_batch(idx, pool_rows, pool_scores, pool_sizes, nq, P, k, lambda, order, nullptr, n_sel);
    }
};

int32_t filtered_backend(rlr_index *idx, const rlr_filter *f, FilteredBackend *be)
{
    be->idx = idx;
    be->f = f;
    int32_t st = rlr::filter_view(f, &be->v); // (null, stale)
    if (st != RLR_OK)
        return st;
    uint64_t n = 0;
    st = rlr_index_info(idx, &n, &be->dim, nullptr, nullptr);
    be->n_rows = be->v.n_allowed;
    return st;
}

// The scopes of a batched text search: ONE filter for every query (f) or a filter per query (filters, f == nullptr).
// The one-filter form is the per-query form with filters[q] == f; what differs is named here and at `look` below.
struct TextScopes {
    rlr_index *idx;
    rlr_lexical *lex;
    const rlr_filter *f;
    const rlr_filter *const *filters;
    std::vector<FilteredBackend> one; // the backend of f, or of every filters[q]
    const rlr_filter *filter(uint32_t q) const { return f ? f : filters[q]; }
    const FilteredBackend &be(uint32_t q) const { return one[f ? 0 : q]; }
    // BM25 of queries q0 .. q0 + m - 1 inside their scopes: the MASKED or the SCOPED batched kernel
    int32_t bm25(uint32_t q0, uint32_t m, const char *tokens, const uint64_t *offsets, uint32_t lcap, uint64_t *rows, float *scores,
                 uint32_t *n) const
    {
        return f ? rlr_lexical_score_batch_filtered(lex, f, m, tokens, offsets + q0, lcap, rows, scores, n, nullptr, nullptr)
                 : rlr_lexical_score_batch_scoped(lex, filters + q0, m, tokens, offsets + q0, lcap, rows, scores, n, nullptr, nullptr);
    }
    // their top-k in ONE call: query q gets min(k, |F_q|) rows back
    int32_t topk(uint32_t q0, const float *queries, uint32_t m, uint32_t k, uint64_t *rows, float *cos, uint32_t *n) const
    {
        return f ? one[0].topk(queries, m, k, rows, cos, n)
                 : rlr_search_topk_scoped(idx, filters + q0, queries, m, k, -1.0f, rows, cos, n);
    }
};

// rlr_engine_search_text_filtered for many queries, query q inside sc.filter(q): per sub-batch ONE batched BM25, ONE top-k
// call, ONE scoring of every query's lexical rows, the arithmetic of blend_search's w_embedding != 0 branch per query
// (blend_fetched: the same union, combine, order and boundary rule) and ONE batched MMR over the decided, non-empty
// pools with P = the largest need.  N, need, the pool size and the result count are per query; the BM25 limit depends
// on top_k alone.  A query with an empty scope has no result, neither batched nor single (:476-478).
int32_t text_batch_chain(const TextScopes &sc, const float *queries_raw, uint32_t dq, uint32_t n_queries, const char *tokens,
                         const uint64_t *token_offsets, uint32_t top_k, float diversity_factor, int32_t stage,
                         const rlr_query_weights *weights, rlr_search_hit *out, uint32_t cap, uint32_t *n_out,
                         rlr_text_batch_info *info)
{
    if (n_queries == 0)
        return RLR_OK;
    // the sizes rlr_engine_search_text_filtered works with, per query where they depend on |F_q|
    const TextSizes ts = text_sizes(top_k, diversity_factor);
    const bool diversify = ts.diversify;
    const uint32_t lcap = ts.lcap, dim = sc.be(0).dim;
    rlr_resolved_weights w;
    rlr_resolve_weights(weights, &w);
    std::vector<uint64_t> need(n_queries, 0);
    uint64_t max_need = 0, n_res_max = 0;
    uint32_t n_live = 0; // queries with a non-empty scope (one filter: all or none)
    for (uint32_t q = 0; q < n_queries; ++q) {
        const uint64_t N = sc.be(q).n_rows;
        if (N == 0)
            continue;
        ++n_live;
        need[q] = need_of(N, ts.k_seen, diversify ? 0 : stage);
        max_need = std::max(max_need, need[q]);
        n_res_max = std::max<uint64_t>(
            n_res_max, rlr::result_k_cap(top_k, static_cast<uint32_t>(std::min<uint64_t>(need[q], 0xFFFFFFFFull)), diversify));
    }
    if (n_live == 0)
        return RLR_OK;
    if (!out || cap < n_res_max)
        return RLR_E_INVALID; // (cap below the result count of a query)
    int32_t st = RLR_OK;
    auto single = [&](uint32_t q) {
        return rlr_engine_search_text_filtered(sc.idx, sc.lex, sc.filter(q), queries_raw ? queries_raw + static_cast<size_t>(q) * dq : nullptr,
                                               dq, tokens ? tokens + token_offsets[q] : nullptr,
                                               static_cast<size_t>(token_offsets[q + 1] - token_offsets[q]), top_k, diversity_factor,
                                               stage, weights, out + static_cast<size_t>(q) * cap, cap, &n_out[q]);
    };
    // the shapes the unscoped batch hands to the single entry point as well
    if (w.embedding == 0.0f || !std::isfinite(w.embedding) || !std::isfinite(w.lexical) || max_need > 1024 || n_queries == 1) {
        for (uint32_t q = 0; q < n_queries; ++q)
            if ((st = single(q)) != RLR_OK)
                return st;
        if (info) {
            info->n_single = n_queries;
            info->n_single_shape = n_queries;
        }
        return RLR_OK;
    }
    const uint32_t P = static_cast<uint32_t>(max_need);
    const uint32_t sub = std::min(text_sub_batch(P, diversify), n_queries);
    std::vector<uint64_t> lrows(static_cast<size_t>(sub) * lcap), rows, lists, round1(sub);
    std::vector<float> lscores(lrows.size()), qn(static_cast<size_t>(sub) * dim), cosv, lcos;
    std::vector<uint32_t> n_lex(sub), got(sub), counts(sub), redo, live;
    std::vector<LexPrep> lexp(sub);
    std::vector<std::vector<Cand>> pools(sub);
    std::vector<char> seen, undecided(sub);
    for (uint32_t q0 = 0; q0 < n_queries; q0 += sub) {
        const uint32_t m = std::min(sub, n_queries - q0);
        bool any_row = false;
        for (uint32_t q = 0; q < m; ++q)
            any_row = any_row || need[q0 + q] != 0;
        if (!any_row)
            continue; // (every scope of this sub-batch is empty)
        // 1. BM25 of every query inside its own filter
        st = sc.bm25(q0, m, tokens, token_offsets, lcap, lrows.data(), lscores.data(), n_lex.data());
        if (st != RLR_OK)
            return st;
        // 2. the queries and the lexical maps, as generic_search prepares them
        if (dq)
            prepare_queries(queries_raw + static_cast<size_t>(q0) * dq, dq, m, dim, qn.data());
        else
            std::fill(qn.begin(), qn.end(), 0.0f);
        uint32_t max_lex = 0;
        uint64_t max_fetch = 0;
        for (uint32_t q = 0; q < m; ++q) {
            const FilteredBackend &be = sc.be(q0 + q);
            lexp[q] = prepare_lexical_in([&be](uint64_t row) { return be.holds(row); }, lrows.data() + static_cast<size_t>(q) * lcap,
                                         lscores.data() + static_cast<size_t>(q) * lcap, n_lex[q]);
            counts[q] = static_cast<uint32_t>(lexp[q].rows.size());
            max_lex = std::max(max_lex, counts[q]);
            round1[q] = std::min<uint64_t>(be.n_rows, need[q0 + q] + counts[q] + 8); // the single call's first fetch
            max_fetch = std::max(max_fetch, round1[q]);
        }
        // 3. one top-k call with the largest fetch (one filter: min(N, need + the longest lexical list + 8))
        const uint32_t fetch = static_cast<uint32_t>(max_fetch);
        rows.assign(static_cast<size_t>(m) * fetch, 0);
        cosv.assign(rows.size(), 0.0f);
        st = sc.topk(q0, qn.data(), m, fetch, rows.data(), cosv.data(), got.data());
        if (st != RLR_OK)
            return st;
        // 4. exact cosines of every query's lexical rows
        lists.assign(static_cast<size_t>(m) * max_lex, 0);
        lcos.assign(lists.size(), 0.0f);
        for (uint32_t q = 0; q < m; ++q)
            std::copy(lexp[q].rows.begin(), lexp[q].rows.end(), lists.begin() + static_cast<size_t>(q) * max_lex);
        st = rlr::score_rows_batch(sc.idx, qn.data(), m, lists.data(), counts.data(), max_lex, lcos.data());
        if (st != RLR_OK)
            return st;
        // 5. blend per query, with its own N and need.  One filter: a query looks at everything it got -- a wider fetch
        // than the single call's changes nothing: where the boundary rule holds, the first `need` candidates are the
        // first `need` of the whole universe, whichever fetch showed it.  A filter per query: at its own first-round
        // fetch only, so its boundary rule decides as the single call's first round does.  (Which queries are handed
        // back -- info->n_single_blend -- depends on this width; the results do not.)
        live.clear();
        for (uint32_t q = 0; q < m; ++q) {
            const uint64_t N = sc.be(q0 + q).n_rows, nd = need[q0 + q];
            pools[q].clear();
            undecided[q] = 0;
            if (N == 0)
                continue;
            const uint32_t look = sc.f ? got[q] : static_cast<uint32_t>(std::min<uint64_t>(got[q], round1[q]));
            undecided[q] = !blend_fetched(w, lexp[q], lcos.data() + static_cast<size_t>(q) * max_lex, rows.data() + static_cast<size_t>(q) * fetch,
                                          cosv.data() + static_cast<size_t>(q) * fetch, look, N, nd, seen, pools[q]);
            if (undecided[q])
                redo.push_back(q0 + q); // the single call widens its fetch
            if (pools[q].size() > nd)
                pools[q].resize(nd);
            if (!undecided[q] && !pools[q].empty())
                live.push_back(q);
        }
        // 6. one MMR over the decided, non-empty pools (generic_search_with_diversity per query)
        if (diversify && (st = mmr_pools(sc.be(0), pools, live, P, top_k, ts.lambda)) != RLR_OK)
            return st;
        for (uint32_t q = 0; q < m; ++q)
            if (!undecided[q])
                emit(pools[q], out + static_cast<size_t>(q0 + q) * cap, cap, &n_out[q0 + q]);
    }
    for (uint32_t q : redo)
        if ((st = single(q)) != RLR_OK)
            return st;
    if (info) {
        info->n_single_blend = static_cast<uint32_t>(redo.size());
        info->n_single = info->n_single_blend;
        info->n_batched = n_live - info->n_single; // (one filter: n_live == n_queries)
    }
    return RLR_OK;
}

} // namespace

extern "C" {

int32_t rlr_engine_search_filtered(rlr_index *idx, const rlr_filter *f, const float *query_raw, uint32_t dq, uint32_t top_k,
                                   const rlr_query_weights *weights, const uint64_t *lex_rows, const float *lex_scores,
                                   uint32_t n_lex, int32_t stage, rlr_search_hit *out, uint32_t cap, uint32_t *n_out)
{
    if (!idx || !f || !n_out || (!query_raw && dq) || (n_lex && (!lex_rows || !lex_scores)))
        return RLR_E_INVALID;
    *n_out = 0;
    FilteredBackend be;
    int32_t st = filtered_backend(idx, f, &be);
    if (st != RLR_OK)
        return st;
    rlr_resolved_weights w;
    rlr_resolve_weights(weights, &w);
    std::vector<Cand> res;
    st = generic_search(be, query_raw, dq, top_k, w, lex_rows, lex_scores, n_lex, stage, res);
    if (st != RLR_OK)
        return st;
    if (!res.empty() && !out)
        return RLR_E_INVALID;
    emit(res, out, cap, n_out);
    return RLR_OK;
}

int32_t rlr_engine_search_with_diversity_filtered(rlr_index *idx, const rlr_filter *f, const float *query_raw, uint32_t dq,
                                                  uint32_t top_k, float diversity_factor, const rlr_query_weights *weights,
                                                  const uint64_t *lex_rows, const float *lex_scores, uint32_t n_lex,
                                                  rlr_search_hit *out, uint32_t cap, uint32_t *n_out)
{
    if (!idx || !f || !n_out || (!query_raw && dq) || (n_lex && (!lex_rows || !lex_scores)))
        return RLR_E_INVALID;
    *n_out = 0;
    if (diversity_factor < 0.0f) diversity_factor = 0.0f; // f32::clamp(0.0, 1.0) (:725); NaN takes the MMR branch
    if (diversity_factor > 1.0f) diversity_factor = 1.0f;
    FilteredBackend be;
    int32_t st = filtered_backend(idx, f, &be);
    if (st != RLR_OK)
        return st;
    rlr_resolved_weights w;
    rlr_resolve_weights(weights, &w);
    std::vector<Cand> picked;
    st = generic_search_with_diversity(be, query_raw, dq, top_k, diversity_factor, w, lex_rows, lex_scores, n_lex, picked);
    if (st != RLR_OK)
        return st;
    if (!picked.empty() && !out)
        return RLR_E_INVALID;
    emit(picked, out, cap, n_out);
    return RLR_OK;
}

int32_t rlr_engine_search_text_filtered(rlr_index *idx, rlr_lexical *lex, const rlr_filter *f, const float *query_raw,
                                        uint32_t dq, const char *query_tokens, size_t tokens_len, uint32_t top_k,
                                        float diversity_factor, int32_t stage, const rlr_query_weights *weights,
                                        rlr_search_hit *out, uint32_t cap, uint32_t *n_out)
{
    if (!idx || !lex || !f || !n_out || (!query_raw && dq) || (tokens_len && !query_tokens))
        return RLR_E_INVALID;
    *n_out = 0;
    const TextSizes ts = text_sizes(top_k, diversity_factor); // the sizes rlr_engine_search_text works with
    std::vector<uint64_t> lrows(ts.lcap);
    std::vector<float> lscores(ts.lcap);
    uint32_t n_lex = 0;
    const int32_t st = rlr_lexical_score_filtered(lex, f, query_tokens, tokens_len, ts.limit, lrows.data(), lscores.data(), &n_lex);
    if (st != RLR_OK)
        return st;
    return ts.diversify ? rlr_engine_search_with_diversity_filtered(idx, f, query_raw, dq, top_k, diversity_factor, weights,
                                                                 lrows.data(), lscores.data(), n_lex, out, cap, n_out)
                     : rlr_engine_search_filtered(idx, f, query_raw, dq, top_k, weights, lrows.data(), lscores.data(), n_lex,
                                                  stage, out, cap, n_out);
}

int32_t rlr_engine_search_with_diversity_batch_filtered(rlr_index *idx, const rlr_filter *f, const float *queries_raw, uint32_t dq,
                                                        uint32_t n_queries, uint32_t top_k, float diversity_factor,
                                                        const rlr_query_weights *weights, rlr_search_hit *out, uint32_t cap,
                                                        uint32_t *n_out)
{
    if (!idx || !f || !n_out || (n_queries && !queries_raw && dq) || (n_queries && cap && !out))
        return RLR_E_INVALID;
    for (uint32_t q = 0; q < n_queries; ++q)
        n_out[q] = 0;
    int32_t st = rlr::filter_check(idx, f); // a stale filter, or one of another index: before any GPU work
    if (st != RLR_OK)
        return st;
    FilteredBackend be;
    st = filtered_backend(idx, f, &be);
    if (st != RLR_OK)
        return st;
    if (n_queries == 0)
        return RLR_OK;
    if (diversity_factor < 0.0f) diversity_factor = 0.0f;
    if (diversity_factor > 1.0f) diversity_factor = 1.0f;
    rlr_resolved_weights w;
    rlr_resolve_weights(weights, &w);
    std::vector<std::vector<Cand>> results;
    // the queries' top-k is ONE rlr_search_topk_filtered call (chunks of up to 8 share a masked pass), the pools' MMR one
    // rlr_mmr_select_batch
    st = generic_search_with_diversity_batch(be, queries_raw, dq, n_queries, top_k, diversity_factor, w, results);
    if (st != RLR_OK)
        return st;
    for (uint32_t q = 0; q < n_queries; ++q)
        emit(results[q], out + static_cast<size_t>(q) * cap, cap, &n_out[q]);
    return RLR_OK;
}

int32_t rlr_engine_search_with_diversity_batch_scoped(rlr_index *idx, const rlr_filter *const *filters, const float *queries_raw,
                                                      uint32_t dq, uint32_t n_queries, uint32_t top_k, float diversity_factor,
                                                      const rlr_query_weights *weights, rlr_search_hit *out, uint32_t cap,
                                                      uint32_t *n_out)
{
    if (!idx || !filters || !n_out || (n_queries && !queries_raw && dq) || (n_queries && cap && !out))
        return RLR_E_INVALID;
    for (uint32_t q = 0; q < n_queries; ++q)
        n_out[q] = 0;
    int32_t st = RLR_OK;
    for (uint32_t q = 0; q < n_queries; ++q) // a null or stale entry, or one of another index: before any GPU work
        if ((st = rlr::filter_check(idx, filters[q])) != RLR_OK)
            return st;
    if (n_queries == 0)
        return RLR_OK;
    if (diversity_factor < 0.0f) diversity_factor = 0.0f;
    if (diversity_factor > 1.0f) diversity_factor = 1.0f;
    rlr_resolved_weights w;
    rlr_resolve_weights(weights, &w);
    // the candidate universe of query q is filters[q]: its size where the one-filter batch has |F|, one
    // rlr_search_topk_scoped call for every query's top-k, the single filtered call where a query runs alone
    struct ScopedBackend {
        rlr_index *idx;
        const rlr_filter *const *filters;
        std::vector<FilteredBackend> one;
        uint32_t dim = 0;
        int32_t topk(const float *queries, uint32_t nq, uint32_t k, uint64_t *rows, float *cos, uint32_t *n) const
        {
            return rlr_search_topk_scoped(idx, filters, queries, nq, k, -1.0f, rows, cos, n);
        }
        int32_t mmr(const uint64_t *pool_rows, const float *pool_scores, const uint32_t *pool_sizes, uint32_t nq, uint32_t P,
                    uint32_t k, float lam, uint32_t *order, uint32_t *n_sel) const
        {
            return one[0].mmr(pool_rows, pool_scores, pool_sizes, nq, P, k, lam, order, n_sel);
        }
    } be{idx, filters, std::vector<FilteredBackend>(n_queries)};
    for (uint32_t q = 0; q < n_queries; ++q)
        if ((st = filtered_backend(idx, filters[q], &be.one[q])) != RLR_OK)
            return st;
    be.dim = be.one[0].dim;
    std::vector<std::vector<Cand>> results;
    st = generic_search_with_diversity_universes(
        be, [&](uint32_t q) { return be.one[q].n_rows; },
        [&](uint32_t q, std::vector<Cand> &res) {
            return generic_search_with_diversity(be.one[q], queries_raw + static_cast<size_t>(q) * dq, dq, top_k, diversity_factor, w,
                                                 nullptr, nullptr, 0, res);
        },
        queries_raw, dq, n_queries, top_k, diversity_factor, w, results);
    if (st != RLR_OK)
        return st;
    for (uint32_t q = 0; q < n_queries; ++q)
        emit(results[q], out + static_cast<size_t>(q) * cap, cap, &n_out[q]);
    return RLR_OK;
}

int32_t rlr_engine_search_text_batch_filtered(rlr_index *idx, rlr_lexical *lex, const rlr_filter *f, const float *queries_raw,
                                              uint32_t dq, uint32_t n_queries, const char *tokens, const uint64_t *token_offsets,
                                              uint32_t top_k, float diversity_factor, int32_t stage,
                                              const rlr_query_weights *weights, rlr_search_hit *out, uint32_t cap, uint32_t *n_out,
                                              rlr_text_batch_info *info)
{
    if (info)
        *info = rlr_text_batch_info{};
    if (!idx || !lex || !f || !text_batch_args(queries_raw, dq, n_queries, tokens, token_offsets, n_out))
        return RLR_E_INVALID;
    int32_t st = rlr::filter_check(idx, f); // a stale filter, or one of another index: before any GPU work
    if (st != RLR_OK)
        return st;
    TextScopes sc{idx, lex, f, nullptr, std::vector<FilteredBackend>(1)};
    if ((st = filtered_backend(idx, f, &sc.one[0])) != RLR_OK)
        return st;
    return text_batch_chain(sc, queries_raw, dq, n_queries, tokens, token_offsets, top_k, diversity_factor, stage, weights, out, cap,
                            n_out, info);
}

int32_t rlr_engine_search_text_batch_scoped(rlr_index *idx, rlr_lexical *lex, const rlr_filter *const *filters,
                                            const float *queries_raw, uint32_t dq, uint32_t n_queries, const char *tokens,
                                            const uint64_t *token_offsets, uint32_t top_k, float diversity_factor, int32_t stage,
                                            const rlr_query_weights *weights, rlr_search_hit *out, uint32_t cap, uint32_t *n_out,
                                            rlr_text_batch_info *info)
{
    if (info)
        *info = rlr_text_batch_info{};
    if (!idx || !lex || !filters || !text_batch_args(queries_raw, dq, n_queries, tokens, token_offsets, n_out))
        return RLR_E_INVALID;
    int32_t st = RLR_OK;
    for (uint32_t q = 0; q < n_queries; ++q) // a null or stale entry, or one of another index: before any GPU work
        if ((st = rlr::filter_check(idx, filters[q])) != RLR_OK)
            return st;
    TextScopes sc{idx, lex, nullptr, filters, std::vector<FilteredBackend>(n_queries)};
    for (uint32_t q = 0; q < n_queries; ++q)
        if ((st = filtered_backend(idx, filters[q], &sc.one[q])) != RLR_OK)
            return st;
    return text_batch_chain(sc, queries_raw, dq, n_queries, tokens, token_offsets, top_k, diversity_factor, stage, weights, out, cap,
                            n_out, info);
}

// Every chunk at or above a cosine (rlr_search_range), with the query normalised as rlr_engine_search does and the hits
// filled as get_embedding_candidates defines them: w_e = 1, no lexical term.
int32_t rlr_engine_search_range(rlr_index *idx, const rlr_filter *f, const float *query_raw, uint32_t dq, float min_cosine,
                                uint32_t cap, rlr_search_hit *out, uint32_t *n_out, uint64_t *n_total_out)
{
    if (!idx || !n_total_out || (!query_raw && dq) || (cap && (!out || !n_out)))
        return RLR_E_INVALID;
    if (n_out)
        *n_out = 0;
    *n_total_out = 0;
    uint32_t dim = 0;
    int32_t st = rlr_index_info(idx, nullptr, &dim, nullptr, nullptr);
    if (st != RLR_OK)
        return st;
    const std::vector<float> q = prepare_query(query_raw, dq, dim);
    std::vector<uint64_t> rows(cap);
    std::vector<float> cosv(cap);
    uint32_t n = 0;
    st = rlr_search_range(idx, f, q.data(), 1, &min_cosine, cap, -1.0f, rows.data(), cosv.data(), &n, n_total_out);
    if (st != RLR_OK)
        return st;
    for (uint32_t i = 0; i < n; ++i) {
        out[i].row = rows[i];
        out[i].score = cosv[i];
        out[i].embedding_score = cosv[i];
        out[i].lexical_score = 0.0f;
        out[i].initial_score = cosv[i];
    }
    if (n_out)
        *n_out = n;
    return RLR_OK;
}

// rlr_engine_search_range for n_queries queries through ONE rlr_search_range_batch call: every query normalised as there,
// the hits of query q filled the same way from out[q * cap] on.
int32_t rlr_engine_search_range_batch(rlr_index *idx, const rlr_filter *f, const float *queries_raw, uint32_t n_queries, uint32_t dq,
                                      const float *min_cosine, uint32_t cap, rlr_search_hit *out, uint32_t *n_out,
                                      uint64_t *n_total_out)
{
    if (!idx || (n_queries && (!n_total_out || !min_cosine || (!queries_raw && dq) || (cap && (!out || !n_out)))))
        return RLR_E_INVALID;
    for (uint32_t q = 0; q < n_queries; ++q) {
        if (n_out)
            n_out[q] = 0;
        n_total_out[q] = 0;
    }
    uint32_t dim = 0;
    int32_t st = rlr_index_info(idx, nullptr, &dim, nullptr, nullptr);
    if (st != RLR_OK)
        return st;
    std::vector<float> qs(static_cast<size_t>(n_queries) * dim);
    for (uint32_t q = 0; q < n_queries; ++q) {
        const std::vector<float> one = prepare_query(queries_raw ? queries_raw + static_cast<size_t>(q) * dq : nullptr, dq, dim);
        std::copy(one.begin(), one.end(), qs.begin() + static_cast<size_t>(q) * dim);
    }
    std::vector<uint64_t> rows(static_cast<size_t>(n_queries) * cap);
    std::vector<float> cosv(static_cast<size_t>(n_queries) * cap);
    std::vector<uint32_t> n(n_queries, 0);
    st = rlr_search_range_batch(idx, f, qs.data(), n_queries, min_cosine, cap, -1.0f, rows.data(), cosv.data(), n.data(), n_total_out);
    if (st != RLR_OK)
        return st;
    for (uint32_t q = 0; q < n_queries; ++q) {
        for (uint32_t i = 0; i < n[q]; ++i) {
            const size_t at = static_cast<size_t>(q) * cap + i;
            out[at].row = rows[at];
            out[at].score = cosv[at];
            out[at].embedding_score = cosv[at];
            out[at].lexical_score = 0.0f;
            out[at].initial_score = cosv[at];
        }
        if (n_out)
            n_out[q] = n[q];
    }
    return RLR_OK;
}

} // extern "C"
