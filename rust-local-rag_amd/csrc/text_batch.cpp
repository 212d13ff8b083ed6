// text_batch.cpp -- rlr_engine_search_text_batch (include/rlr_engine.h): rlr_engine_search_text for many queries at once.
// The host side of the batch: sizes and the gate of the fused kernels exactly as rlr_engine_search_text computes them, the
// queries prepared the same way, sub-batches through rlr::search_hybrid_batch (index_fused.hip) with the BM25 chain of
// rlr::lexical_batch_enqueue (lexical.hip) beside the cosine batch, and every query the batch could not decide re-run alone
// through rlr_engine_search_text.  Compiled with -ffp-contract=off like engine.cpp.
#include "../../include/rlr_engine.h"
#include "../../include/rlr_lexical.h"
#include "engine_host.h"
#include "lexical_internal.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

using namespace rlr_host;

extern "C" {

int32_t rlr_engine_search_text_batch(rlr_index *idx, rlr_lexical *lex, const float *queries_raw, uint32_t dq, uint32_t n_queries,
                                     const char *tokens, const uint64_t *token_offsets, uint32_t top_k, float diversity_factor,
                                     int32_t stage, const rlr_query_weights *weights, rlr_search_hit *out, uint32_t cap,
                                     uint32_t *n_out, rlr_text_batch_info *info)
{
    if (info)
        *info = rlr_text_batch_info{};
    if (!idx || !lex || !text_batch_args(queries_raw, dq, n_queries, tokens, token_offsets, n_out))
        return RLR_E_INVALID;
    if (n_queries == 0)
        return RLR_OK;
    // the sizes rlr_engine_search_text works with
    const TextSizes ts = text_sizes(top_k, diversity_factor);
    const float lambda = ts.lambda;
    const bool diversify = ts.diversify;
    const uint32_t k_seen = ts.k_seen, limit = ts.limit;
    rlr_resolved_weights w;
    rlr_resolve_weights(weights, &w);
    uint64_t N = 0;
    uint32_t dim = 0;
    int32_t st = rlr_index_info(idx, &N, &dim, nullptr, nullptr);
    if (st != RLR_OK || N == 0) // :476-478
        return st;
    const uint64_t initial_k = std::min<uint64_t>(N, static_cast<uint64_t>(k_seen) * 3);             // :544
    const uint64_t need = (diversify || !stage) ? std::min<uint64_t>(initial_k, k_seen) : initial_k; // :667-698
    // (need <= N, and an index holds fewer than 2^32 rows)
    const uint64_t n_res = rlr::result_k_cap(top_k, static_cast<uint32_t>(need), diversify);
    if (!out || cap < n_res)
        return RLR_E_INVALID; // (cap below the result count of a query)
    auto tok = [&](uint32_t q) { return tokens ? tokens + token_offsets[q] : nullptr; };
    auto tok_len = [&](uint32_t q) { return static_cast<size_t>(token_offsets[q + 1] - token_offsets[q]); };
    auto single = [&](uint32_t q) {
        return rlr_engine_search_text(idx, lex, queries_raw ? queries_raw + static_cast<size_t>(q) * dq : nullptr, dq, tok(q),
                                      tok_len(q), top_k, diversity_factor, stage, weights, out + static_cast<size_t>(q) * cap, cap,
                                      &n_out[q]);
    };
    // the shapes the fused kernels cover (the conditions of search_hybrid_begin for the same request)
    const uint32_t n_lex_bound = ts.lcap;
    const uint64_t fetch_full = std::min<uint64_t>(N, need + n_lex_bound + 8);
    const bool fused = w.embedding > 0.0f && std::isfinite(w.embedding) && std::isfinite(w.lexical) && need <= 1024 &&
                       n_lex_bound <= 2048 && fetch_full + n_lex_bound <= 4096 && N <= 0xFFFFFFFFull;
    if (!fused || n_queries == 1) {
        for (uint32_t q = 0; q < n_queries; ++q) {
            st = single(q);
            if (st != RLR_OK)
                return st;
        }
        if (info) {
            info->n_single = n_queries;
            info->n_single_shape = n_queries;
        }
        return RLR_OK;
    }
    const uint32_t nd = static_cast<uint32_t>(need);
    const uint32_t k_cap = static_cast<uint32_t>(n_res);
    const uint32_t sub = text_sub_batch(nd, diversify); // (one GEMM query block; the Gram matrices stay below 256 MB)
    std::vector<float> qs;
    std::vector<uint64_t> rows;
    std::vector<float> cosv, sc, lx;
    std::vector<uint32_t> got, status;
    std::vector<uint8_t> many_terms;
    std::vector<uint32_t> redo_blend, redo_shape;
    for (uint32_t q0 = 0; q0 < n_queries; q0 += sub) {
        const uint32_t m = std::min(sub, n_queries - q0);
        qs.resize(static_cast<size_t>(m) * dim);
        for (uint32_t q = 0; q < m; ++q) {
            const std::vector<float> v = prepare_query(queries_raw ? queries_raw + static_cast<size_t>(q0 + q) * dq : nullptr, dq, dim);
            std::memcpy(qs.data() + static_cast<size_t>(q) * dim, v.data(), dim * sizeof(float));
        }
        rows.assign(static_cast<size_t>(m) * k_cap, 0);
        cosv.assign(rows.size(), 0.0f);
        sc.assign(rows.size(), 0.0f);
        lx.assign(rows.size(), 0.0f);
        got.assign(m, 0);
        status.assign(m, 0);
        many_terms.assign(m, 0);
        struct LexArgs {
            rlr_lexical *lex;
            const char *tokens;
            const uint64_t *offsets;
            uint32_t m, limit;
            uint8_t *many;
            rlr::LexBatchPending lp;
        } la{lex, tokens, token_offsets + q0, m, limit, many_terms.data(), {}};
        st = rlr::search_hybrid_batch(
            idx, qs.data(), m, nd, top_k, lambda, diversify ? 1 : 0, w.embedding, w.lexical, n_lex_bound,
            [](void *a, const rlr::LexBatchSink *sink, void **ready) -> int32_t {
                LexArgs *l = static_cast<LexArgs *>(a);
                const int32_t e = rlr::lexical_batch_enqueue(l->lex, l->m, l->tokens, l->offsets, l->limit, *sink, l->many, &l->lp);
                *ready = l->lp.ready;
                return e;
            },
            &la, rows.data(), cosv.data(), sc.data(), lx.data(), got.data(), status.data());
        rlr::lexical_batch_finish(&la.lp, st == RLR_OK); // (also drops the readers' lock before any single call below)
        if (st != RLR_OK)
            return st;
        for (uint32_t q = 0; q < m; ++q) {
            if (many_terms[q]) {
                redo_shape.push_back(q0 + q);
                continue;
            }
            if (status[q]) {
                redo_blend.push_back(q0 + q);
                continue;
            }
            std::vector<Cand> res(got[q]);
            const size_t b = static_cast<size_t>(q) * k_cap;
            for (uint32_t i = 0; i < got[q]; ++i)
                res[i] = {rows[b + i], sc[b + i], cosv[b + i], lx[b + i]};
            emit(res, out + static_cast<size_t>(q0 + q) * cap, cap, &n_out[q0 + q]);
        }
    }
    // the queries the batch could not decide: alone, through the entry point whose results the batch reproduces
    for (uint32_t q : redo_shape)
        if ((st = single(q)) != RLR_OK)
            return st;
    for (uint32_t q : redo_blend)
        if ((st = single(q)) != RLR_OK)
            return st;
    if (info) {
        info->n_single_shape = static_cast<uint32_t>(redo_shape.size());
        info->n_single_blend = static_cast<uint32_t>(redo_blend.size());
        info->n_single = info->n_single_shape + info->n_single_blend;
        info->n_batched = n_queries - info->n_single;
    }
    return RLR_OK;
}

} // extern "C"
