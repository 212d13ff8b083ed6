// index_grouped.hip -- the searches of include/rlr_gpu.h that answer over documents or thresholds, on the frame of
// index_internal.h: grouped top-k (at most per_doc rows per document), range search (every row at or above a threshold) and
// capped hybrid search, each one query at a time and in chunks of queries behind one shared scan; their gates, their
// workspaces and their C entry points.  No kernel is defined here: the tails are group.hip's and range.hip's.
#include "index_internal.h"
#include "lexical_internal.h"
#include "sort_emit.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <functional>
#include <memory>
#include <mutex>
#include <unordered_map>
#include <vector>

using namespace rlr;

namespace rlr {
namespace {

// floats between the score arrays of two queries of a shared scan
inline uint64_t score_stride(const rlr_index *ix)
{
    return (ix->n_rows + 3) / 4 * 4;
}

// ---- grouped search (rlr_search_topk_grouped): at most per_doc results per document ---------------------------------
// The walk of the contract on the host: `keys` = the exact packed keys of the allowed rows, docs = the whole column (empty:
// no column).  Descending keys are the library's result order; a row is accepted unless per_doc rows of its document are.
uint32_t grouped_walk(std::vector<uint64_t> &keys, const std::vector<uint32_t> &docs, uint32_t k, uint32_t per_doc, uint64_t *res,
                      uint32_t *res_docs)
{
    std::sort(keys.begin(), keys.end(), std::greater<uint64_t>());
    std::unordered_map<uint32_t, uint32_t> taken;
    uint32_t n = 0;
    for (size_t i = 0; i < keys.size() && n < k; ++i) {
        const uint32_t row = 0xFFFFFFFFu - static_cast<uint32_t>(keys[i]);
        const uint32_t d = docs.empty() ? RLR_DOC_NONE : docs[row];
        if (d != RLR_DOC_NONE && taken[d]++ >= per_doc)
            continue;
        res[n] = keys[i];
        res_docs[n] = d;
        n++;
    }
    return n;
}

// Reference-order scores of every allowed row (all rows, or the rows of `f`), copied back with the document column: what
// the exact forms of the grouped and the capped search walk over.  The query is in c->d_query.  list[i] = the i-th allowed
// row, vals[i] = its score, docs = the whole column (empty: no column).
int32_t exact_scores(rlr_index *ix, Ctx *c, const rlr_filter *f, std::vector<uint32_t> &list, std::vector<float> &vals,
                     std::vector<uint32_t> &docs)
{
    hipStream_t s = c->stream;
    const uint32_t n = static_cast<uint32_t>(f ? f->n_allowed : ix->n_rows);
    list.assign(n, 0);
    RLR_TRY(reserve_list(c, n));
    if (f) {
        uint32_t at = 0;
        for (size_t w = 0; w < f->h_mask.size(); ++w)
            for (uint64_t bits = f->h_mask[w]; bits; bits &= bits - 1)
                if (at < n)
                    list[at++] = static_cast<uint32_t>(w * 64 + static_cast<uint32_t>(__builtin_ctzll(bits)));
    } else {
        for (uint32_t i = 0; i < n; ++i)
            list[i] = i;
        RLR_HIP(launch_group_iota(c->d_list.get(), n, s));
    }
    RLR_HIP(launch_score_rows(ix->d_rows.get(), ix->pitch16, ix->dim, ix->dtype, c->d_query.get(), f ? f->d_list.get() : c->d_list.get(), n,
                              c->d_vals.get(), s));
    vals.assign(n, 0.0f);
    docs.assign(ix->d_docs ? ix->n_rows : 0, 0);
    RLR_HIP(hipMemcpyAsync(vals.data(), c->d_vals.get(), static_cast<size_t>(n) * sizeof(float), hipMemcpyDeviceToHost, s));
    if (!docs.empty())
        RLR_HIP(hipMemcpyAsync(docs.data(), ix->d_docs.get(), docs.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    RLR_HIP(hipStreamSynchronize(s));
    return RLR_OK;
}

// The exact form: reference-order scores of every allowed row, copied back, and the walk on the host.  Slow and always
// right.  The query is in c->d_query.
int32_t grouped_exact(rlr_index *ix, Ctx *c, const rlr_filter *f, uint32_t k, uint32_t per_doc, uint64_t *res, uint32_t *res_docs,
                      uint32_t *n_res)
{
    std::vector<uint32_t> list, docs;
    std::vector<float> vals;
    RLR_TRY(exact_scores(ix, c, f, list, vals, docs));
    std::vector<uint64_t> keys(list.size());
    for (size_t i = 0; i < list.size(); ++i)
        keys[i] = pack_result(vals[i], list[i]);
    *n_res = grouped_walk(keys, docs, k, per_doc, res, res_docs);
    return RLR_OK;
}

// The table of a grouped tail holds twice the documents it can meet (one per allowed row at most); > 31: by rule, no table.
uint32_t group_table_bits(uint64_t n_allowed)
{
    uint32_t tab_bits = 10;
    while (tab_bits < 32 && (1ull << tab_bits) < 2 * n_allowed)
        tab_bits++;
    return tab_bits;
}

// The context's grouped-search state for m queries: the document table (ONE key table, a value plane per query), t_g per
// row, the heads' histograms, the states and the candidates -- the single-query buffers, a slice per query.  The order and
// the groupings decide what a failed regrow leaves empty; the error is the caller's to judge (a chunk hands its queries
// back where the memory is short).
hipError_t reserve_group_state(const rlr_index *ix, Ctx *c, uint32_t m, uint32_t per_doc, uint32_t tab_bits)
{
    const size_t slots = static_cast<size_t>(1) << tab_bits, q = m;
    hipError_t e = hipSuccess;
    if (ix->d_docs)
        e = reserve_group(Want{c->d_gkeys, slots}, Want{c->d_gvals, slots * per_doc * q});
    if (e == hipSuccess)
        e = c->d_gtg.reserve(std::max<uint64_t>(q * static_cast<uint32_t>(ix->n_rows), 1024));
    if (e == hipSuccess)
        e = reserve_group(Want{c->d_ghist, q * 2 * kHistBins}, Want{c->d_gstate, q}, Want{c->d_gcand, q * kGroupCap},
                          Want{c->d_gcdoc, q * kGroupCap});
    return e;
}

// What GroupArgs and GroupBatchArgs name alike (a slice per query in the batched form): the column, the call's numbers,
// the grouped state reserve_group_state left and the rows.
template <typename Args>
void fill_group_args(const rlr_index *ix, Ctx *c, uint32_t k, uint32_t per_doc, float two_eps, uint32_t tab_bits, Args *ga)
{
    ga->docs = ix->d_docs.get();
    ga->n = static_cast<uint32_t>(ix->n_rows);
    ga->k = k;
    ga->per_doc = per_doc;
    ga->two_eps = two_eps;
    ga->tab_keys = c->d_gkeys.get();
    ga->tab_vals = c->d_gvals.get();
    ga->tab_bits = tab_bits;
    ga->tg = c->d_gtg.get();
    ga->hist = c->d_ghist.get();
    ga->st = c->d_gstate.get();
    ga->rows = ix->d_rows.get();
    ga->pitch16 = ix->pitch16;
    ga->dim = ix->dim;
    ga->dtype = ix->dtype;
    ga->cand = c->d_gcand.get();
    ga->cand_doc = c->d_gcdoc.get();
    ga->n_cu = ix->n_cu;
}

// Reserve the context's grouped-search state and describe one grouped tail over the scores the scan leaves in c->d_scores
// (the query in c->d_query); out / meta / capped are the caller's.
int32_t make_group_args(rlr_index *ix, Ctx *c, uint32_t k, uint32_t per_doc, float two_eps, uint32_t tab_bits, GroupArgs *out)
{
    RLR_HIP(reserve_group_state(ix, c, 1, per_doc, tab_bits));
    fill_group_args(ix, c, k, per_doc, two_eps, tab_bits, out);
    out->scores = c->d_scores.get();
    out->query = c->d_query.get();
    out->out = nullptr;
    out->meta = nullptr;
    out->ctx_hist = c->d_hist.get();
    return RLR_OK;
}

// The tail of a chunk of m queries behind shared_scan, over the state reserve_group_state left for them; out (c->d_gout) or
// capped is the caller's.
GroupBatchArgs make_group_batch_args(const rlr_index *ix, Ctx *c, uint32_t m, uint32_t k, uint32_t per_doc, float two_eps,
                                     uint32_t tab_bits)
{
    GroupBatchArgs ga{};
    fill_group_args(ix, c, k, per_doc, two_eps, tab_bits, &ga);
    ga.n_queries = m;
    ga.scores = c->d_sample.get();
    ga.score_stride = score_stride(ix);
    ga.queries = c->d_query.get();
    ga.q_pitch = ix->q_pitch;
    return ga;
}

// One grouped query over all rows (f == nullptr) or the rows of `f` (n_allowed > 0); k > 0, per_doc in 1..8.  The scan,
// then group.hip's tail in place of enqueue_query_rest; every hand-off to the exact form is counted (form 1..3).
int32_t grouped_query(rlr_index *ix, Ctx *c, const rlr_filter *f, const float *query, uint32_t k, uint32_t per_doc, float guard_eps,
                      uint64_t *rows_out, float *cos_out, uint32_t *docs_out, uint32_t *n_out)
{
    const uint64_t n_allowed = f ? f->n_allowed : ix->n_rows;
    const SearchPlan p = make_plan(ix, query, 1, static_cast<uint32_t>(std::min<uint64_t>(k, n_allowed)), guard_eps);
    RLR_TRY(ctx_prepare(ix, c, 1, p));
    const uint32_t words = group_out_words(p.k);
    Staged pin;
    RLR_TRY(stage_call(ix, c, query, 1, static_cast<size_t>(words) + 1, /*for_scans=*/false, &pin));
    uint64_t *h_res = pin.h_res, *h_meta = h_res + words;
    hipStream_t s = c->stream;
    const bool timed = ix->profiling;
    uint64_t n_cand = 0;
    uint32_t n_res = 0, form = 0;
    std::vector<uint64_t> ex_res;
    std::vector<uint32_t> ex_docs;
    const uint64_t *res = h_res;
    const uint32_t *res_docs = reinterpret_cast<const uint32_t *>(h_res + p.k);
    const uint32_t tab_bits = group_table_bits(n_allowed);
    if ((f && f->path == 0) || p.k > kGroupKMax || tab_bits > 31 || !group_fits(ix->pitch16, ix->dim, ix->dtype)) {
        form = 3; // by rule: a list-path filter, k beyond the finish, rows beyond the staged re-score
    } else {
        GroupArgs ga;
        RLR_TRY(make_group_args(ix, c, p.k, per_doc, p.two_eps, tab_bits, &ga));
        ga.out = h_res;
        ga.meta = h_meta;
        arm_meta(h_meta, 1);
        // (the masked scan for a filter; without one the scan over the master rows too: no nomination copy, as filtered calls)
        RLR_HIP(enqueue_query_scan(ix, c, 0, timed, f, /*master_rows=*/true));
        RLR_HIP(launch_group_tail(ga, s, timed ? c->ev[2] : nullptr));
        if (timed) {
            RLR_HIP(hipEventRecord(c->ev[3], s));
            RLR_HIP(hipStreamSynchronize(s));
        } else {
            RLR_TRY(wait_results(h_meta, h_res, 1, words, kGroupCap, s, &c->wait_ema));
        }
        RLR_TRY(check_hist_assert(c));
        n_cand = static_cast<uint32_t>(h_meta[0]);
        if (n_cand > kGroupCap) {
            form = 1; // more candidates than the finish holds (or a local list / the table overflowed)
        } else {
            const uint64_t info = h_res[words - 1];
            n_res = static_cast<uint32_t>(info >> 32);
            const uint32_t n_valid = static_cast<uint32_t>(info);
            if (n_res < p.k && n_valid < n_allowed)
                form = 2; // allowed rows with NaN nominations were left out and the answer is short
            if (form == 0 && masked_row_among(f, h_res, n_res))
                form = 2; // a masked row came back
        }
    }
    if (form != 0) {
        ex_res.resize(p.k);
        ex_docs.resize(p.k);
        RLR_TRY(grouped_exact(ix, c, f, p.k, per_doc, ex_res.data(), ex_docs.data(), &n_res));
        res = ex_res.data();
        res_docs = ex_docs.data();
    }
    c->hist_dirty = false;
    *n_out = n_res;
    unpack_results(res, n_res, rows_out, cos_out);
    if (docs_out)
        std::memcpy(docs_out, res_docs, static_cast<size_t>(n_res) * sizeof(uint32_t));
    {
        std::lock_guard<std::mutex> lk(ix->mu);
        ix->grouped_forms[form]++;
    }
    return note_search(ix, c, 1, n_cand, form != 0 ? 1 : 0, timed && form != 3);
}

// ---- the frame of a shared chunk: what the batched grouped, range and capped searches have in common -------------------
// The shared scan of a chunk of m (2..8) queries, uploaded to c->d_query: one pass over the master rows (masked inside a
// filter) leaves query q's nominated scores at c->d_sample + q * score_stride(ix); no histogram.  The caller has reserved
// c->d_sample for m * score_stride(ix) floats, at its own place in its order of reservations.  `gate`: whose gate
// accepted the shape, for the error a refusal is.
int32_t shared_scan(rlr_index *ix, Ctx *c, const rlr_filter *f, uint32_t m, const char *gate)
{
    const uint64_t s_stride = score_stride(ix);
    hipStream_t s = c->stream;
    const ScanArgs sa = scan_args(ix, c->d_query.get(), c->d_sample.get(), nullptr);
    hipError_t e = hipSuccess;
    if (!(f ? launch_scan_masked_multi(sa, f->d_mask.get(), f->n_allowed, ix->q_pitch, m, s_stride, s, &e)
            : launch_scan_multi(sa, ix->q_pitch, m, s_stride, s, &e)))
        return set_error(RLR_E_INTERNAL, "multi-query scan refused a shape the %s gate accepted", gate);
    RLR_HIP(e);
    return RLR_OK;
}

// The bookkeeping of a chunk of m queries that has synchronised, n_back of them handed back: the batch counters of the
// profile, then note_search for the queries decided here.
int32_t note_chunk(rlr_index *ix, Ctx *c, uint32_t m, size_t n_back, uint64_t n_candidates, uint64_t gemm_bytes = 0)
{
    {
        std::lock_guard<std::mutex> lk(ix->mu);
        ix->prof.n_batches += 1;
        ix->prof.n_batch_queries += m;
        ix->prof.n_batch_fallbacks += n_back;
        ix->prof.batch_gemm_bytes += gemm_bytes;
    }
    return note_search(ix, c, m - static_cast<uint32_t>(n_back), n_candidates, 0, /*timed=*/false);
}

// ---- batched grouped search (rlr_search_topk_grouped_batch): the queries of a call share passes over the rows ----------
// The chunk width: the largest w in 2..8 whose workspace -- the key table (4 B a slot), w value planes (8 B x per_doc a
// slot), w t_g arrays (8 B a row) and w score arrays (4 B a row) -- stays at or below the bytes of the index's rows, so the
// state of a search is never larger than what it searches; 0: none fits.
uint32_t grouped_chunk_width(const rlr_index *ix, uint64_t n_allowed, uint32_t per_doc)
{
    const uint64_t n = ix->n_rows, s_stride = score_stride(ix), slots = 1ull << group_table_bits(n_allowed);
    const uint64_t budget = n * row_bytes(ix);
    for (uint64_t w = 8; w >= 2; --w)
        if (4 * slots + w * (8 * per_doc * slots + 8 * n + 4 * s_stride) <= budget)
            return static_cast<uint32_t>(w);
    return 0;
}

// The cost model of the grouped gate and of the capped gate, which grouped_share_wins describes: the three fixed costs, in
// seconds, are the arguments -- one by one per query, shared per chunk, and shared for the chunk's nq queries together
// (each gate multiplies as it always has: the products round differently).
bool share_wins(const rlr_index *ix, const rlr_filter *f, uint32_t nq, uint32_t per_doc, double single_s, double shared_s,
                double queries_s)
{
    const double el = ix->dtype == RLR_F16 ? 2.0 : 4.0;
    const double n = static_cast<double>(ix->n_rows), allowed = static_cast<double>(f ? f->n_allowed : ix->n_rows);
    const double rounds = ix->d_docs ? per_doc : 0.0;
    const double t_single = nq * (single_s + rounds * 2e-6 + allowed * ix->dim * el / 7.3e12 + n * (25e-12 + rounds * 9.5e-12));
    const double rate = nq <= 2 ? 6.45e12 : nq <= 4 ? 6.1e12 : 5.8e12;
    const double t_shared = shared_s + queries_s + allowed * ix->dim * el / rate + nq * n * (20e-12 + rounds * 10e-12);
    return t_single > 1.1 * t_shared;
}

// The gate (rlr_index_set_grouped_sharing mode 0): does a chunk of nq queries through one shared scan and one set of tail
// launches beat the same queries one by one by 10 %?  A cost model in the style of range_share_wins:
//   one by one   per query 77 us (its launches and its own synchronisation) + 2 us per round + the ALLOWED bytes at
//                7.3 TB/s + per row 25 ps and 9.5 ps per round (the tail's passes over the score array, t_g, the ids)
//   shared       80 us (one copy, one synchronisation, one set of launches) + 13 us per query (its collect and finish
//                workgroups) + the allowed bytes at the rate of the Q = 2 / 4 / 8 instance of the shared scan (6.45 / 6.1 /
//                5.8 TB/s) + per row and query 20 ps and 10 ps per round
// The fixed costs and the per-row terms are fitted to tools/bench_grouped_batch.py's cells at 100 k and 1 M rows of 768 f32
// elements (profiles/grouped_batch_bench.json; DESIGN.md "Batched grouped top-k" has the table, the fit and what was NOT
// measured); the four scan rates are the range gate's, borrowed: the cells agree with them but do not separate them from
// the per-row terms.  No measured cell lost with sharing forced, and this model declines none of them.
bool grouped_share_wins(const rlr_index *ix, const rlr_filter *f, uint32_t nq, uint32_t per_doc)
{
    return share_wins(ix, f, nq, per_doc, 77e-6, 80e-6, nq * 13e-6);
}

// The chunk width of a batched grouped or capped call before its gate is asked, 0 by rule: one query, a list-path filter,
// k (clamped to the allowed rows; the capped need) beyond the finish, rows the staged re-score or the shared scans do not
// serve, no width of two within the workspace rule.
uint32_t chunk_width_by_rule(const rlr_index *ix, const rlr_filter *f, uint32_t n_queries, uint64_t k, uint32_t per_doc)
{
    const uint64_t n_allowed = f ? f->n_allowed : ix->n_rows;
    if (n_queries < 2 || (f && f->path == 0) || k > kGroupKMax || group_table_bits(n_allowed) > 31 ||
        !group_fits(ix->pitch16, ix->dim, ix->dtype) || !batch_multi_shape(ix, 2) || ix->n_rows > 0xFFFFFFFFull)
        return 0;
    return std::min(grouped_chunk_width(ix, n_allowed, per_doc), n_queries);
}

// Queries in chunk ci of a call at chunk width w: split evenly over ceil(n_queries / w) chunks (9 -> 5 + 4); w < 2: one
// query a chunk, by rule.
uint32_t chunk_size(uint32_t n_queries, uint32_t w, uint32_t ci)
{
    if (w < 2)
        return 1;
    const uint32_t n_chunks = (n_queries + w - 1) / w;
    return n_queries / n_chunks + (ci < n_queries % n_chunks ? 1u : 0u);
}

// One chunk of m (2..8) queries through ONE shared scan and group.hip's batched tail: the queries staged and uploaded
// once, the scan, one set of tail launches, ONE copy of the chunk's result words and one synchronisation.  The band is the
// plan's f32 band, exactly as in grouped_query; the plan is the chunk's (the largest query norm): a band wider than a
// query's own only adds candidates, the order is decided on the reference-order score.  forms[q]: 0 decided on the device;
// 1 handed back on a capacity (more than kGroupCap candidates, a local list or the table overflowed); 2 handed back because
// the answer is short while allowed rows with NaN nominations exist, a masked row came back, or the chunk's workspace
// could not be reserved.  A handed-back query is answered by grouped_query on the same context, after every decided
// query has been read out of the pinned block (grouped_query stages into it again); its neighbours stay decided.
// c->d_hist is not touched: the shared scans run without a histogram.
int32_t grouped_batch_chunk(rlr_index *ix, Ctx *c, const rlr_filter *f, const float *queries, uint32_t m, uint32_t k, uint32_t per_doc,
                            float guard_eps, uint64_t *rows_out, float *cos_out, uint32_t *docs_out, uint32_t *n_out, uint32_t *forms)
{
    const uint64_t n_allowed = f ? f->n_allowed : ix->n_rows;
    const SearchPlan p = make_plan(ix, queries, m, static_cast<uint32_t>(std::min<uint64_t>(k, n_allowed)), guard_eps);
    RLR_TRY(ctx_prepare(ix, c, m, p));
    const uint32_t words = group_batch_words(p.k), res_words = group_out_words(p.k);
    const size_t n_res = static_cast<size_t>(m) * words;
    Staged pin;
    RLR_TRY(stage_call(ix, c, queries, m, n_res, /*for_scans=*/false, &pin));
    uint64_t *h_res = pin.h_res;
    hipStream_t s = c->stream;
    const uint32_t tab_bits = group_table_bits(n_allowed);
    std::vector<uint32_t> redo;
    uint64_t cand_total = 0;
    // the chunk's workspace, the scan's scores with it: where the memory is short the chunk is handed back
    hipError_t e = reserve_group_state(ix, c, m, per_doc, tab_bits);
    if (e == hipSuccess)
        e = c->d_gout.reserve(n_res);
    if (e == hipSuccess)
        e = c->d_sample.reserve(m * score_stride(ix));
    if (e == hipErrorOutOfMemory) {
        (void)hipGetLastError(); // no error of the call: the queries go one by one, in the single path's smaller workspace
        for (uint32_t q = 0; q < m; ++q) {
            forms[q] = 2;
            redo.push_back(q);
        }
    } else {
        RLR_HIP(e);
        RLR_TRY(shared_scan(ix, c, f, m, "grouped"));
        GroupBatchArgs ga = make_group_batch_args(ix, c, m, p.k, per_doc, p.two_eps, tab_bits);
        ga.out = c->d_gout.get();
        RLR_HIP(launch_group_batch_tail(ga, s));
        RLR_HIP(hipMemcpyAsync(h_res, c->d_gout.get(), n_res * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
        RLR_HIP(hipStreamSynchronize(s));
        for (uint32_t q = 0; q < m; ++q) {
            const uint64_t *r = h_res + static_cast<size_t>(q) * words;
            const uint64_t status = r[words - 1], info = r[res_words - 1];
            const uint32_t n_res_q = static_cast<uint32_t>(info >> 32), n_valid = static_cast<uint32_t>(info);
            if (status > kGroupCap)
                forms[q] = 1;
            else if ((n_res_q < p.k && n_valid < n_allowed) || masked_row_among(f, r, n_res_q))
                forms[q] = 2;
            else
                forms[q] = 0;
            if (forms[q] != 0) {
                redo.push_back(q);
                continue;
            }
            cand_total += status;
            n_out[q] = n_res_q;
            unpack_results(r, n_res_q, rows_out + static_cast<size_t>(q) * k, cos_out + static_cast<size_t>(q) * k);
            if (docs_out)
                std::memcpy(docs_out + static_cast<size_t>(q) * k, r + p.k, static_cast<size_t>(n_res_q) * sizeof(uint32_t));
        }
    }
    c->hist_dirty = false;
    RLR_TRY(note_chunk(ix, c, m, redo.size(), cand_total));
    // (from here on the pinned block and the context are grouped_query's)
    for (uint32_t q : redo)
        RLR_TRY(grouped_query(ix, c, f, queries + static_cast<size_t>(q) * ix->dim, k, per_doc, guard_eps,
                              rows_out + static_cast<size_t>(q) * k, cos_out + static_cast<size_t>(q) * k,
                              docs_out ? docs_out + static_cast<size_t>(q) * k : nullptr, &n_out[q]));
    return RLR_OK;
}

// ---- range search (rlr_search_range): every allowed row scoring at or above a threshold ---------------------------------
// The exact form: reference-order scores of every allowed row, copied back; threshold, count and order on the host.  Slow
// and always right.  The query is in c->d_query.  keys: the first min(n_total, cap) hits in result order.
int32_t range_exact(rlr_index *ix, Ctx *c, const rlr_filter *f, float tau, uint32_t cap, std::vector<uint64_t> &keys, uint64_t *n_total)
{
    std::vector<uint32_t> list, docs;
    std::vector<float> vals;
    RLR_TRY(exact_scores(ix, c, f, list, vals, docs));
    keys.clear();
    uint64_t total = 0;
    for (size_t i = 0; i < list.size(); ++i)
        if (vals[i] >= tau) { // IEEE: a NaN is never a hit, -0 >= +0 holds
            total++;
            if (cap)
                keys.push_back(pack_result(vals[i], list[i]));
        }
    *n_total = total;
    if (keys.size() > cap) {
        std::partial_sort(keys.begin(), keys.begin() + cap, keys.end(), std::greater<uint64_t>());
        keys.resize(cap);
    } else {
        std::sort(keys.begin(), keys.end(), std::greater<uint64_t>());
    }
    return RLR_OK;
}

// One range query over all rows (f == nullptr) or the rows of `f` (n_allowed > 0); tau is a number.  The scan over the
// master rows, then range.hip's tail in place of enqueue_query_rest.  Every query is counted in one form:
//   [0] decided on the device: the finish's ordered keys, or (more than kRangeFinishMax hits, all within cap and the
//       device capacity) one copy of the unordered exact keys and a sort of them here;
//   [1] capacity, n_total > min(cap, RLR_RANGE_DEVICE_MAX) while rows are wanted: n_total is the device's exact count; the
//       rows are the best `cap` of more than `cap` hits, i.e. the top-k answer at k = cap -- taken from the existing top-k
//       path (rlr_search_topk / rlr_search_topk_filtered) while cap <= kLdsSortCap, from the exact form beyond;
//   [2] allowed rows with NaN nominations exist (their exact score could be a number), or a returned row fails the
//       filter's host mask: the exact form;
//   [3] by rule, decided before any workspace is sized: a list-path filter, rows too wide for the staged re-score: the
//       exact form (for a list-path filter that is launch_score_rows over its list).
int32_t range_query(rlr_index *ix, Ctx *c, const rlr_filter *f, const float *query, float tau, uint32_t cap, float guard_eps,
                    uint64_t *rows_out, float *cos_out, uint32_t *n_out, uint64_t *n_total_out)
{
    const uint64_t n_allowed = f ? f->n_allowed : ix->n_rows;
    const bool by_rule = (f && f->path == 0) || !group_fits(ix->pitch16, ix->dim, ix->dtype);
    const SearchPlan p = make_plan(ix, query, 1, 1, guard_eps);
    const uint32_t hit_cap = std::min<uint32_t>(cap, RLR_RANGE_DEVICE_MAX), out_keys = std::min<uint32_t>(cap, kRangeFinishMax);
    const uint32_t words = range_out_words(out_keys);
    if (by_rule)
        RLR_TRY(reserve_queries(ix, c, 1));
    else
        RLR_TRY(ctx_prepare(ix, c, 1, p));
    Staged pin;
    RLR_TRY(stage_call(ix, c, query, 1, static_cast<size_t>(words) + 1, /*for_scans=*/false, &pin));
    uint64_t *h_res = pin.h_res, *h_meta = h_res + words;
    hipStream_t s = c->stream;
    const bool timed = ix->profiling;
    uint32_t form = by_rule ? 3 : 0, n_res = 0;
    uint64_t n_total = 0;
    std::vector<uint64_t> keys;
    const uint64_t *res = h_res;
    if (!by_rule) {
        RLR_HIP(reserve_group(Want{c->d_rstate, 1}, Want{c->d_rhits, std::max<uint32_t>(hit_cap, 1)}));
        RangeArgs ra;
        ra.scores = c->d_scores.get();
        ra.n = static_cast<uint32_t>(ix->n_rows);
        ra.tau = tau;
        ra.two_eps = p.two_eps;
        ra.hit_cap = hit_cap;
        ra.out_keys = out_keys;
        ra.st = c->d_rstate.get();
        ra.rows = ix->d_rows.get();
        ra.pitch16 = ix->pitch16;
        ra.dim = ix->dim;
        ra.dtype = ix->dtype;
        ra.query = c->d_query.get();
        ra.hits = c->d_rhits.get();
        ra.out = h_res;
        ra.meta = h_meta;
        ra.ctx_hist = c->d_hist.get();
        ra.n_cu = ix->n_cu;
        arm_meta(h_meta, 1);
        // (the masked scan for a filter; without one the scan over the master rows too: no nomination copy, as filtered calls)
        RLR_HIP(enqueue_query_scan(ix, c, 0, timed, f, /*master_rows=*/true));
        RLR_HIP(launch_range_tail(ra, s));
        if (timed) {
            RLR_HIP(hipEventRecord(c->ev[2], s));
            RLR_HIP(hipEventRecord(c->ev[3], s));
            RLR_HIP(hipStreamSynchronize(s));
        } else {
            RLR_TRY(wait_results(h_meta, h_res, 1, words, 1, s, &c->wait_ema));
        }
        RLR_TRY(check_hist_assert(c));
        const uint64_t info = h_res[out_keys];
        const uint32_t n_hits = static_cast<uint32_t>(info), n_valid = static_cast<uint32_t>(info >> 32);
        n_total = n_hits;
        if (n_valid < n_allowed) {
            form = 2; // allowed rows with NaN nominations: what they score exactly is not known here
        } else if (cap && n_hits > hit_cap) {
            form = 1;
        } else if (cap && n_hits > out_keys) {
            // beyond the finish, within the device capacity: the exact keys in no order -> one copy, ordered here
            keys.resize(n_hits);
            RLR_HIP(hipMemcpyAsync(keys.data(), c->d_rhits.get(), static_cast<size_t>(n_hits) * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
            RLR_HIP(hipStreamSynchronize(s));
            std::sort(keys.begin(), keys.end(), std::greater<uint64_t>());
            res = keys.data();
            n_res = n_hits;
        } else {
            n_res = cap ? n_hits : 0;
        }
        if (form == 0 && masked_row_among(f, res, n_res))
            form = 2; // a masked row came back
    }
    c->hist_dirty = false;
    {
        std::lock_guard<std::mutex> lk(ix->mu);
        ix->range_forms[form]++;
    }
    *n_total_out = n_total;
    if (form == 1 && cap <= kLdsSortCap) {
        // more hits than cap: the first cap of them are the top-k answer at k = cap (all of them numbers at or above tau)
        if (f)
            return filtered_query(ix, c, f, query, cap, guard_eps, rows_out, cos_out, n_out);
        SearchPlan tp;
        const uint64_t *h = nullptr;
        RLR_TRY(run_search(ix, c, query, 1, cap, guard_eps, nullptr, &tp, &h));
        if (!h)
            return set_error(RLR_E_INTERNAL, "search produced no result buffer");
        *n_out = tp.k;
        unpack_results(h, tp.k, rows_out, cos_out);
        return RLR_OK;
    }
    if (form != 0) {
        RLR_TRY(range_exact(ix, c, f, tau, cap, keys, &n_total));
        *n_total_out = n_total;
        res = keys.data();
        n_res = static_cast<uint32_t>(keys.size());
    }
    if (n_out)
        *n_out = n_res;
    if (n_res)
        unpack_results(res, n_res, rows_out, cos_out);
    return note_search(ix, c, 1, n_total, form != 0 ? 1 : 0, timed && form != 3);
}

// ---- batched range search (rlr_search_range_batch): the queries of a call share passes over the rows ------------------
// Which shared pass serves a chunk of nq queries of this call -- kRangeShareScan: one VALU scan for 2..8 queries
// (scan_multi_kernel, with a mask-path filter scan_masked_multi_kernel), the f32 band; kRangeShareGemm: the nomination
// GEMM in filter mode for 9 or more, and for 2..8 where no shared scan serves the shape, the binary16 band -- or none
// (kRangeShareNone: one by one through range_query, by rule).  f16_ok: the plan's, over all queries of the call.
enum RangeShare : int { kRangeShareNone = -1, kRangeShareScan = 0, kRangeShareGemm = 1 };
RangeShare range_share_path(const rlr_index *ix, const rlr_filter *f, uint32_t nq, bool f16_ok)
{
    if (nq < 2 || (f && f->path == 0) || !group_fits(ix->pitch16, ix->dim, ix->dtype) || ix->n_rows > 0xFFFFFFFFull)
        return kRangeShareNone;
    if (nq <= 8 && batch_multi_shape(ix, nq))
        return kRangeShareScan;
    // (the rows run_batched requires; operands beyond binary16 range keep the f32 paths, as batch_eligible has it)
    if (ix->dim % 128 == 0 && ix->n_rows >= 4096 && f16_ok)
        return kRangeShareGemm;
    return kRangeShareNone;
}

// The auto gate (rlr_index_set_range_sharing mode 0): does the shared path win?  A cost model in the style of
// batch_eligible, from the rates DESIGN.md records (RLR_BATCH_MIN is not consulted):
//   one by one   per query 50 us of launches and its own synchronisation + the ALLOWED bytes at 7.3 TB/s
//   shared scan  40 us (one copy, one synchronisation) + 25 us per query (its collect and finish workgroups) + the allowed
//                bytes at the rate of the Q = 2 / 4 / 8 instance (6.45 / 6.1 / 5.8 TB/s; the middle one interpolated) + 4
//                bytes per row and query for the collect's read of the score arrays at 3 TB/s
//   GEMM         150 us + 1 us per query (its finish workgroup) + per 256 queries one pass over ALL rows (the mask only
//                acts in the finish) at 4.4 TB/s over the row-major rows, 5 TB/s (up to 128 queries) / 2.85 TB/s of
//                binary16 over the image + the result words at 20 GB/s
// and the shared path must win by 10 %.  Fitted to tools/bench_range_batch.py's cells with 0 hits at 100 k and 1 M rows of
// 768 f32 elements (profiles/range_batch_bench.json; DESIGN.md "Batched range search" has the table, the fit and what was
// NOT measured -- among it every shape at which this model declines: no measured cell lost with sharing forced).
bool range_share_wins(const rlr_index *ix, const rlr_filter *f, uint32_t nq, uint32_t cap, RangeShare path)
{
    const double el = ix->dtype == RLR_F16 ? 2.0 : 4.0;
    const double n = static_cast<double>(ix->n_rows), allowed = static_cast<double>(f ? f->n_allowed : ix->n_rows);
    const double t_single = nq * (50e-6 + allowed * ix->dim * el / 7.3e12);
    double t_shared;
    if (path == kRangeShareScan) {
        const double rate = nq <= 2 ? 6.45e12 : nq <= 4 ? 6.1e12 : 5.8e12;
        t_shared = 40e-6 + nq * 25e-6 + allowed * ix->dim * el / rate + nq * n * 4.0 / 3.0e12;
    } else {
        const bool image = ix->image_enabled && ix->d_image.get() && gemm_image_usable(ix->dim);
        const double pass = image ? n * ix->dim * 2.0 / (nq <= 128 ? 5.0e12 : 2.85e12) : n * ix->dim * el / 4.4e12;
        const double words = static_cast<double>(nq) * range_batch_words(std::min<uint32_t>(cap, kRangeFinishMax)) * 8.0;
        t_shared = 150e-6 + nq * 1e-6 + pass * ((nq + 255) / 256) + words / 20e9;
    }
    return t_single > 1.1 * t_shared;
}

// One chunk of m queries through ONE shared pass (path: range_share_path's answer for m) and range.hip's batched tail:
// the queries staged and uploaded once, tau | lo | hi per query computed here once (range_bounds) and uploaded, the pass,
// the tail, ONE copy of the chunk's result words (keys, counts, status) and one synchronisation.  The band: the plan's f32
// band behind the shared scan, exactly as in range_query; behind the GEMM image_two_eps (nomination_eps for the plan's
// norms, scaled by the caller's guard_eps -- the bound run_batched trusts), with d_tau[q] = lo[q].  The plan is the
// chunk's (the largest query norm): a band that is wider than a query's own only adds candidates, membership is decided on
// the reference-order score.  forms[q]: 0 / 1 decided on the device behind the scan / the GEMM, 2 handed back -- a device
// capacity (the GEMM's candidate list, kRangeFinishMax hits while rows are wanted), allowed rows with NaN nominations
// behind the scan, a masked row among the results -- and then answered by range_query on the same context, after every
// decided query has been read out of the pinned block (range_query stages into it again).
// c->d_hist is not touched: the shared scans run without a histogram.
int32_t range_batch_chunk(rlr_index *ix, Ctx *c, const rlr_filter *f, RangeShare path, const float *queries, const float *tau,
                          uint32_t m, uint32_t cap, float guard_eps, uint64_t *rows_out, float *cos_out, uint32_t *n_out,
                          uint64_t *n_total_out, uint32_t *forms)
{
    const uint64_t n_allowed = f ? f->n_allowed : ix->n_rows;
    const uint32_t n = static_cast<uint32_t>(ix->n_rows);
    const SearchPlan p = make_plan(ix, queries, m, 1, guard_eps);
    RLR_TRY(ctx_prepare(ix, c, m, p));
    const uint32_t out_keys = std::min<uint32_t>(cap, kRangeFinishMax), words = range_batch_words(out_keys);
    const size_t n_res = static_cast<size_t>(m) * words;
    Staged pin;
    RLR_TRY(stage_call(ix, c, queries, m, n_res + 2 * static_cast<size_t>(m), /*for_scans=*/false, &pin));
    uint64_t *h_res = pin.h_res;
    float *h_bounds = reinterpret_cast<float *>(h_res + n_res), *h_tau = h_bounds + 3 * static_cast<size_t>(m);
    hipStream_t s = c->stream;
    const float two_eps = path == kRangeShareScan ? p.two_eps : p.two_eps_img;
    for (uint32_t q = 0; q < m; ++q) {
        float *b = h_bounds + 3 * static_cast<size_t>(q);
        b[0] = tau[q];
        range_bounds(tau[q], two_eps, &b[1], &b[2]);
        h_tau[q] = b[1] == b[1] ? b[1] : -__builtin_inff(); // (a bound that is no number takes every row)
    }
    RLR_HIP(reserve_group(Want{c->d_rstate, m}, Want{c->d_rhits, std::max<size_t>(cap ? static_cast<size_t>(m) * kRangeFinishMax : 1, 1)}));
    RLR_HIP(c->d_rbounds.reserve(3 * static_cast<size_t>(m)));
    RLR_HIP(c->d_rout.reserve(n_res));
    RLR_HIP(hipMemcpyAsync(c->d_rbounds.get(), h_bounds, 3 * static_cast<size_t>(m) * sizeof(float), hipMemcpyHostToDevice, s));
    RangeBatchArgs ra{};
    ra.n_queries = m;
    ra.n = n;
    ra.bounds = c->d_rbounds.get();
    ra.cap = cap;
    ra.rows = ix->d_rows.get();
    ra.pitch16 = ix->pitch16;
    ra.dim = ix->dim;
    ra.dtype = ix->dtype;
    ra.queries = c->d_query.get();
    ra.q_pitch = ix->q_pitch;
    ra.hits = c->d_rhits.get();
    ra.out = c->d_rout.get();
    ra.n_cu = ix->n_cu;
    uint64_t gemm_bytes = 0; // the operand the GEMM pass streams, once per chunk (prof.batch_gemm_bytes, as run_batched counts it)
    if (path == kRangeShareScan) {
        RLR_HIP(c->d_sample.reserve(m * score_stride(ix)));
        RLR_HIP(hipMemsetAsync(c->d_rstate.get(), 0, m * sizeof(RangeState), s));
        RLR_TRY(shared_scan(ix, c, f, m, "range"));
        ra.scores = c->d_sample.get();
        ra.score_stride = score_stride(ix);
        ra.st = c->d_rstate.get();
    } else {
        const uint32_t fin_cap = batch_finish_capacity();
        const uint32_t n_qblocks = (m + 255) / 256;
        RLR_HIP(c->d_qfrag.reserve(static_cast<uint64_t>(n_qblocks) * 256 * ix->dim * 2));
        RLR_HIP(c->d_gsync.reserve(256));
        RLR_TRY(batch_arm(c, m, fin_cap, 0, 1, n)); // the states: cap = fin_cap, n_cand = 0
        RLR_HIP(hipMemcpyAsync(c->d_tau.get(), h_tau, m * sizeof(float), hipMemcpyHostToDevice, s));
        const bool use_image = ix->image_enabled && ix->d_image.get() && gemm_image_usable(ix->dim);
        gemm_bytes = static_cast<uint64_t>(n) * ix->dim * ((ix->dtype == RLR_F16 || use_image) ? 2 : 4);
        RLR_HIP(launch_prep_queries(c->d_query.get(), m, ix->q_pitch, ix->dim, use_image ? static_cast<int>(RLR_F16) : ix->dtype,
                                    c->d_qfrag.get(), s));
        RLR_HIP(launch_gemm_nominate(ix->d_rows.get(), ix->pitch16, ix->dim, ix->dtype, 0, n, c->d_qfrag.get(), m, c->d_tau.get(),
                                     c->d_bcand.get(), fin_cap, c->d_bstate.get(), nullptr, 0, use_image ? ix->d_image.get() : nullptr, s,
                                     c->d_gsync.get()));
        ra.cand = c->d_bcand.get();
        ra.cand_stride = fin_cap;
        ra.bst = c->d_bstate.get();
        ra.mask = f ? f->d_mask.get() : nullptr;
    }
    RLR_HIP(launch_range_batch_tail(ra, s));
    RLR_HIP(hipMemcpyAsync(h_res, c->d_rout.get(), n_res * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    RLR_HIP(hipStreamSynchronize(s));
    c->hist_dirty = false;
    std::vector<uint32_t> redo;
    uint64_t hits_total = 0;
    for (uint32_t q = 0; q < m; ++q) {
        const uint64_t *r = h_res + static_cast<size_t>(q) * words;
        const uint32_t n_hits = static_cast<uint32_t>(r[out_keys]), n_valid = static_cast<uint32_t>(r[out_keys] >> 32);
        const uint32_t n_res_q = cap ? std::min(n_hits, out_keys) : 0;
        const bool back = r[out_keys + 1] != kRangeBatchDecided || (path == kRangeShareScan && n_valid < n_allowed) ||
                          masked_row_among(f, r, n_res_q);
        if (back) {
            forms[q] = 2;
            redo.push_back(q);
            continue;
        }
        forms[q] = path == kRangeShareScan ? 0 : 1;
        n_total_out[q] = n_hits;
        hits_total += n_hits;
        if (n_out)
            n_out[q] = n_res_q;
        if (n_res_q)
            unpack_results(r, n_res_q, rows_out + static_cast<size_t>(q) * cap, cos_out + static_cast<size_t>(q) * cap);
    }
    RLR_TRY(note_chunk(ix, c, m, redo.size(), hits_total, gemm_bytes));
    // (from here on the pinned block and the context are range_query's)
    for (uint32_t q : redo)
        RLR_TRY(range_query(ix, c, f, queries + static_cast<size_t>(q) * ix->dim, tau[q], cap, guard_eps,
                            cap ? rows_out + static_cast<size_t>(q) * cap : nullptr, cap ? cos_out + static_cast<size_t>(q) * cap : nullptr,
                            n_out ? &n_out[q] : nullptr, &n_total_out[q]));
    return RLR_OK;
}

// ---- capped hybrid search (rlr_search_capped): at most per_doc results per document, in combined order ---------------
// One pool entry on the host: what the exact form builds and every form hands back.
struct CappedHit {
    uint32_t row, doc;
    float c, e, l;
};

// (combined desc, NaN last, row asc), -0 and +0 tying: the engine's candidate order
bool capped_before(const CappedHit &a, const CappedHit &b)
{
    const bool an = std::isnan(a.c), bn = std::isnan(b.c);
    if (an || bn)
        return an != bn ? bn : a.row < b.row;
    if (a.c != b.c)
        return a.c > b.c;
    return a.row < b.row;
}

// A capped call's workspace: device (c->d_pool) and pinned (c->h_pin: the staged query | the lexical pairs, rows then
// scores as on the device -- one copy | the pool's rows and document ids | the result block).
struct CappedWs {
    uint64_t P, n_lex, q_pitch, k_cap, gram_floats;
    Carver d, h;
    float *gram = d.take<float>(gram_floats), *comb = d.take<float>(P), *cos = d.take<float>(P), *lexv = d.take<float>(P);
    uint32_t *order = d.take<uint32_t>(P);
    float *mmr = d.take<float>(P);
    uint32_t *nsel = d.take<uint32_t>(1), *info = d.take<uint32_t>(7);
    uint32_t *lrow = d.take<uint32_t>(n_lex);
    float *lscore = d.take<float>(n_lex), *lcos = d.take<float>(n_lex);
    float *scratch = d.take<float>(3ull * rlr::kCappedSlots);
    float *h_q = h.take<float>(q_pitch);
    uint32_t *h_lrow = h.take<uint32_t>(n_lex);
    float *h_lscore = h.take<float>(n_lex);
    uint32_t *h_side = h.take<uint32_t>(rlr::capped_side_words(static_cast<uint32_t>(P)));
    uint32_t *h_out = h.take<uint32_t>(block_words(static_cast<uint32_t>(k_cap)));
    char *h_pad = h.take<char>(64);
    CappedWs(float *d_base, void *h_base, uint32_t q_pitch_, uint32_t P_, uint32_t n_lex_, uint32_t k_cap_, bool diversify)
        : P(P_), n_lex(n_lex_), q_pitch(q_pitch_), k_cap(k_cap_), gram_floats(diversify ? static_cast<uint64_t>(P_) * P_ : 0),
          d(d_base), h(h_base) {}
};

// What holds for every query of a capped call: the arguments of the entry point that are not a query's own.
struct CappedBatchCall {
    uint32_t need, k; // need: already min(., |A|)
    float lambda;
    bool diversify;
    float w_e, w_l;
    uint32_t per_doc;
    float guard_eps;
};

// ... and one query of it
struct CappedCall : CappedBatchCall {
    const float *query;
    std::vector<uint32_t> lrow; // the lexical rows inside A, ascending and unique
    std::vector<float> lscore;
    float max_lex;
};

// One query's CappedCall from the arguments of an entry point: what holds for the whole call (bc) and the query's own
// lexical pairs, those inside the filter kept.  q: the query's place in a batched call for the error text, -1 in a call of one.
int32_t make_capped_call(const rlr_index *ix, const rlr_filter *f, const CappedBatchCall &bc, const float *query,
                         const uint64_t *lex_rows, const float *lex_scores, uint64_t n_lex, float max_lex, int64_t q,
                         CappedCall *call)
{
    static_cast<CappedBatchCall &>(*call) = bc;
    call->query = query;
    call->max_lex = max_lex;
    for (uint64_t i = 0; i < n_lex; ++i) {
        if (lex_rows[i] >= ix->n_rows || (i && lex_rows[i] <= lex_rows[i - 1]))
            return q < 0 ? set_error(RLR_E_INVALID, "lex_rows must be ascending, unique and inside the index")
                         : set_error(RLR_E_INVALID, "lex_rows must be ascending, unique and inside the index (query %u)",
                                     static_cast<uint32_t>(q));
        if (f && !filter_holds(f, static_cast<uint32_t>(lex_rows[i])))
            continue; // a lexical row outside the filter is no candidate
        call->lrow.push_back(static_cast<uint32_t>(lex_rows[i]));
        call->lscore.push_back(lex_scores[i]);
    }
    return RLR_OK;
}

// The exact form: reference-order scores of every allowed row, the blend and the walk on the host.  Slow and always
// right.  The query is in c->d_query.  pool: the first `need` accepted rows in order.
int32_t capped_exact(rlr_index *ix, Ctx *c, const rlr_filter *f, const CappedCall &call, std::vector<CappedHit> &pool)
{
    std::vector<uint32_t> list, docs;
    std::vector<float> vals;
    RLR_TRY(exact_scores(ix, c, f, list, vals, docs));
    const uint32_t n = static_cast<uint32_t>(list.size());
    std::vector<CappedHit> all(n);
    size_t lj = 0; // (the allowed rows and the lexical rows both ascend)
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t row = list[i];
        while (lj < call.lrow.size() && call.lrow[lj] < row)
            ++lj;
        const float l = lj < call.lrow.size() && call.lrow[lj] == row ? call.lscore[lj] / call.max_lex : 0.0f;
        const float t0 = call.w_e * vals[i]; // two rounded products, one add (engine_host.h: combine)
        const float t1 = call.w_l * l;
        all[i] = CappedHit{row, docs.empty() ? RLR_DOC_NONE : docs[row], t0 + t1, vals[i], l};
    }
    std::sort(all.begin(), all.end(), capped_before);
    std::unordered_map<uint32_t, uint32_t> taken;
    pool.clear();
    for (size_t i = 0; i < all.size() && pool.size() < call.need; ++i) {
        if (all[i].doc != RLR_DOC_NONE && taken[all[i].doc]++ >= call.per_doc)
            continue;
        pool.push_back(all[i]);
    }
    return RLR_OK;
}

// the per-query checks of capped_query's by-rule test: what sends this query, alone, to the single path
bool capped_query_by_rule(const CappedCall &call)
{
    bool lex_ok = std::isfinite(call.max_lex) && call.max_lex > 0.0f;
    for (size_t i = 0; i < call.lscore.size() && lex_ok; ++i)
        lex_ok = call.lscore[i] >= 0.0f; // (the proof needs w_l * lexn >= 0; NaN compares false)
    return !lex_ok || call.lrow.size() > rlr::kCappedLexMax;
}

// One capped query over all rows (f == nullptr) or the rows of `f` (n_allowed > 0); call.need > 0.  The scan, group.hip's
// tail with the capped finish, then -- diversified -- the Gram and greedy launches in the same enqueue.  Every hand-off to
// the exact form is counted (form 1..3).  *picked: the results are in `hits` (form 0, or no diversification); else `hits` is
// the pool of the exact form and the caller runs the MMR selection over it once the context is back.
int32_t capped_query(rlr_index *ix, Ctx *c, const rlr_filter *f, const CappedCall &call, std::vector<CappedHit> &hits,
                     bool *picked)
{
    const uint64_t n_allowed = f ? f->n_allowed : ix->n_rows;
    const uint32_t need = call.need, n_lex = static_cast<uint32_t>(call.lrow.size());
    const SearchPlan p = make_plan(ix, call.query, 1, need, call.guard_eps);
    RLR_TRY(ctx_prepare(ix, c, 1, p));
    // by rule first: what the exact form answers needs the staged query alone -- no pool, no Gram matrix of need x need
    const uint32_t tab_bits = group_table_bits(n_allowed);
    const bool by_rule = (f && f->path == 0) || need > kGroupKMax || capped_query_by_rule(call) || tab_bits > 31 ||
                         !(call.w_e > 0.0f) || !std::isfinite(call.w_e) || !(call.w_l >= 0.0f) || !std::isfinite(call.w_l) ||
                         !group_fits(ix->pitch16, ix->dim, ix->dtype);
    const uint32_t P = by_rule ? 0 : need;
    const uint32_t k_cap = by_rule ? 0 : rlr::result_k_cap(call.k, P, call.diversify);
    const uint32_t n_lex_ws = by_rule ? 0 : n_lex;
    const CappedWs sizes(nullptr, nullptr, ix->q_pitch, P, n_lex_ws, k_cap, call.diversify);
    RLR_HIP(c->d_pool.reserve(sizes.d.floats()));
    RLR_TRY(reserve_list(c, std::max<uint32_t>(std::max<uint32_t>(P, n_lex_ws), 1)));
    RLR_TRY(pin_reserve(c, sizes.h.bytes));
    const CappedWs ws(c->d_pool.get(), c->h_pin.get(), ix->q_pitch, P, n_lex_ws, k_cap, call.diversify);
    hipStream_t s = c->stream;
    const bool timed = ix->profiling;
    stage_queries(ix, c, call.query, 1, ws.h_q);
    c->h_q_kq = nullptr;
    RLR_HIP(upload_queries(c, ws.h_q, static_cast<size_t>(ix->q_pitch) * sizeof(float), s));
    uint64_t n_cand = 0;
    uint32_t form = 0;
    if (by_rule) {
        form = 3;
    } else {
        rlr::CappedArgs ca;
        ca.w_e = call.w_e;
        ca.w_l = call.w_l;
        ca.eps = p.two_eps * 0.5f;
        ca.n_allowed = static_cast<uint32_t>(n_allowed);
        ca.lrow = ws.lrow;
        ca.lscore = ws.lscore;
        ca.lcos = ws.lcos;
        ca.n_lex = n_lex;
        ca.max_lex = call.max_lex;
        ca.scratch = ws.scratch;
        ca.list = c->d_list.get();
        ca.comb = ws.comb;
        ca.cosv = ws.cos;
        ca.lexv = ws.lexv;
        ca.info = ws.info;
        ca.h_side = ws.h_side;
        ca.k_cap = k_cap;
        ca.h_out = call.diversify ? nullptr : ws.h_out;
        GroupArgs ga;
        RLR_TRY(make_group_args(ix, c, need, call.per_doc, p.two_eps, tab_bits, &ga));
        ga.capped = &ca;
        uint32_t *h_out = ws.h_out;
        h_out[block_done(k_cap)] = kBlockPending; // (the last kernel's last store replaces it: what the wait below polls)
        ws.h_side[0] = 0xFFFFFFFFu;
        if (n_lex) { // the pairs and, behind the scan, their exact cosines
            std::memcpy(ws.h_lrow, call.lrow.data(), static_cast<size_t>(n_lex) * sizeof(uint32_t));
            std::memcpy(ws.h_lscore, call.lscore.data(), static_cast<size_t>(n_lex) * sizeof(float));
            RLR_HIP(hipMemcpyAsync(ws.lrow, ws.h_lrow, static_cast<size_t>(n_lex) * 8, hipMemcpyHostToDevice, s));
        }
        // (the masked scan for a filter; without one the scan over the master rows too: no nomination copy, as grouped calls)
        RLR_HIP(enqueue_query_scan(ix, c, 0, timed, f, /*master_rows=*/true));
        RLR_HIP(launch_score_rows(ix->d_rows.get(), ix->pitch16, ix->dim, ix->dtype, c->d_query.get(), ws.lrow, n_lex, ws.lcos, s));
        RLR_HIP(launch_group_tail(ga, s, timed ? c->ev[2] : nullptr));
        if (call.diversify) {
            RLR_HIP(launch_gram_rows(ix->d_rows.get(), ix->pitch16, ix->dim, ix->dtype, c->d_list.get(), P, ws.gram, 1, s));
            const rlr::MmrEmit emit = mmr_emit(c->d_list.get(), ws.comb, ws.cos, ws.lexv, ws.info, k_cap, h_out);
            RLR_HIP(launch_mmr_greedy(ws.gram, ws.comb, P, call.k, call.lambda, ws.order, ws.mmr, ws.nsel, ws.info, 1, s, &emit));
        }
        if (timed) {
            RLR_HIP(hipEventRecord(c->ev[3], s));
            RLR_HIP(hipStreamSynchronize(s));
        } else {
            RLR_TRY(wait_block(h_out, k_cap, s, &c->wait_ema));
        }
        RLR_TRY(check_hist_assert(c));
        std::vector<uint64_t> r_rows(k_cap);
        std::vector<float> r_cos(k_cap), r_comb(k_cap), r_lex(k_cap);
        uint32_t n_res = 0;
        const uint32_t status = read_block(h_out, k_cap, r_rows.data(), r_cos.data(), r_comb.data(), r_lex.data(), &n_res);
        if (status != 0) {
            form = status == 1 ? 1 : 2; // capacity | undecidable here (a boundary tie, rows that order last are wanted)
        } else {
            // the pool's rows and document ids: written by the finish, ahead of the block's last store on the stream
            const volatile uint32_t *side = ws.h_side;
            auto side_ok = [&]() {
                const uint32_t ns = side[0];
                if (ns > P)
                    return false;
                uint32_t chk = 0;
                for (uint32_t i = 0; i < ns; ++i)
                    chk += result_chk_term(side[2 + i], 2 + i) + result_chk_term(side[2 + P + i], 2 + P + i);
                return chk == side[1];
            };
            if (!side_ok()) {
                RLR_HIP(hipStreamSynchronize(s));
                if (!side_ok())
                    return set_error(RLR_E_INTERNAL, "capped search: the pool's document ids never arrived");
            }
            const uint32_t ns = side[0];
            n_cand = ns;
            hits.resize(n_res);
            for (uint32_t i = 0; i < n_res && form == 0; ++i) {
                const uint32_t row = static_cast<uint32_t>(r_rows[i]);
                uint32_t at = call.diversify ? 0 : i; // (no diversification: result i is pool slot i)
                while (at < ns && side[2 + at] != row)
                    ++at;
                if (at >= ns || (f && !filter_holds(f, row)))
                    form = 2; // a masked row came back (the hazard masked_row_among documents)
                else
                    hits[i] = CappedHit{row, side[2 + P + at], r_comb[i], r_cos[i], r_lex[i]};
            }
        }
    }
    *picked = true;
    if (form != 0) {
        RLR_TRY(capped_exact(ix, c, f, call, hits));
        *picked = !call.diversify;
    }
    c->hist_dirty = false;
    {
        std::lock_guard<std::mutex> lk(ix->mu);
        ix->capped_forms[form]++;
    }
    return note_search(ix, c, 1, n_cand, form != 0 ? 1 : 0, timed && form != 3);
}

// The last step of a capped call, with no context held: an exact form's pool (!picked) goes through mmr_diversify,
// unchanged, then the hits into the caller's arrays.
int32_t capped_deliver(rlr_index *ix, std::vector<CappedHit> &hits, bool picked, uint32_t k, float lambda, uint64_t *rows_out,
                       float *cos_out, float *score_out, float *lex_out, uint32_t *docs_out, uint32_t *n_out)
{
    if (!picked && !hits.empty()) { // the exact form's pool: mmr_diversify over it, unchanged
        const uint32_t P = static_cast<uint32_t>(hits.size());
        std::vector<uint64_t> rows(P);
        std::vector<float> scores(P);
        for (uint32_t i = 0; i < P; ++i) {
            rows[i] = hits[i].row;
            scores[i] = hits[i].c;
        }
        std::vector<uint32_t> order(P);
        uint32_t n_sel = 0;
        RLR_TRY(mmr_single_impl(ix, rows.data(), scores.data(), P, k, lambda, order.data(), nullptr, &n_sel, nullptr, 0));
        std::vector<CappedHit> sel(n_sel);
        for (uint32_t i = 0; i < n_sel; ++i)
            sel[i] = hits[order[i]];
        hits.swap(sel);
    }
    for (size_t i = 0; i < hits.size(); ++i) {
        rows_out[i] = hits[i].row;
        cos_out[i] = hits[i].e;
        score_out[i] = hits[i].c;
        lex_out[i] = hits[i].l;
        if (docs_out)
            docs_out[i] = hits[i].doc;
    }
    *n_out = static_cast<uint32_t>(hits.size());
    return RLR_OK;
}

// ---- batched capped search (rlr_search_capped_batch): the queries of a call share passes over the rows ----------------
// The gate (rlr_index_set_capped_sharing mode 0): does a chunk of nq capped queries through one shared scan, one set of
// tail launches and one Gram / greedy pair beat the same queries one by one by 10 %?  grouped_share_wins' form with
// rounds = per_doc.  BORROWED from the grouped gate, unchanged: the scan rates (7.3 TB/s single, 6.45 / 6.1 / 5.8 TB/s
// shared), the four per-row terms and the 2 us per round.  FITTED to tools/bench_capped_batch.py's cells at 100 k rows,
// top_k = 5 (profiles/capped_batch_bench.json; DESIGN.md "Batched capped search" has the table, the fit and what was NOT
// measured): the three fixed costs.  The cells are whole text requests, so the fixed costs carry the BM25 side too -- one
// by one 160 us a request (its launches, the Gram / greedy pair, the BM25 call and two synchronisations); shared 200 us a
// chunk and 45 us a query (its collect, finish and greedy workgroups, its share of the batched BM25).  A call with
// caller-computed pairs pays less on both sides; the gate does not tell the two apart.
constexpr double kCappedGateSingleUs = 160.0, kCappedGateSharedUs = 200.0, kCappedGateQueryUs = 45.0;
bool capped_share_wins(const rlr_index *ix, const rlr_filter *f, uint32_t nq, uint32_t per_doc)
{
    return share_wins(ix, f, nq, per_doc, kCappedGateSingleUs * 1e-6, kCappedGateSharedUs * 1e-6, nq * kCappedGateQueryUs * 1e-6);
}

// The workspace of one chunk: device (c->d_pool, beside the grouped state) and pinned (c->h_pin).  The lexical pairs lie
// B apart per query (the layout launch_score_rows_batch scores), rows | scores | counts in one region: one upload.  The
// result block (list .. nsel) is one region as well: one copy back.
struct CappedBatchWs {
    uint64_t m, P, B, q_pitch, gram_floats;
    Carver d, h;
    float *gram = d.take<float>(gram_floats), *mmr = d.take<float>(m * P);
    float *scratch = d.take<float>(m * 3ull * rlr::kCappedSlots);
    uint32_t *lrow = d.take<uint32_t>(m * B);
    float *lscore = d.take<float>(m * B);
    uint32_t *lcnt = d.take<uint32_t>(m);
    float *lcos = d.take<float>(m * B);
    uint32_t *list = d.take<uint32_t>(m * P);
    float *comb = d.take<float>(m * P), *cos = d.take<float>(m * P), *lexv = d.take<float>(m * P);
    uint32_t *docs = d.take<uint32_t>(m * P), *order = d.take<uint32_t>(m * P);
    uint32_t *info = d.take<uint32_t>(2 * m), *sizes = d.take<uint32_t>(m), *nsel = d.take<uint32_t>(m);
    float *h_q = h.take<float>(m * q_pitch);
    uint32_t *h_lrow = h.take<uint32_t>(m * B);
    float *h_lscore = h.take<float>(m * B);
    uint32_t *h_lcnt = h.take<uint32_t>(m);
    uint32_t *h_res = h.take<uint32_t>(res_words());
    char *h_pad = h.take<char>(64);
    uint64_t res_words() const { return 6 * m * P + 4 * m; }
    uint64_t lex_words() const { return 2 * m * B + m; }
    CappedBatchWs(float *d_base, void *h_base, uint32_t q_pitch_, uint32_t m_, uint32_t P_, uint32_t B_, bool diversify)
        : m(m_), P(P_), B(B_), q_pitch(q_pitch_), gram_floats(diversify ? static_cast<uint64_t>(m_) * P_ * P_ : 0), d(d_base),
          h(h_base) {}
};

// One chunk of m (2..8) capped queries (calls[q].query = queries + q * dim: consecutive) in ONE enqueue: the queries staged
// and uploaded once and every query's lexical pairs in one copy, the shared scan over the master rows (masked inside a
// filter), launch_score_rows_batch for the exact cosines of all lexical rows, group.hip's batched tail with k = need and
// the capped multi finish, -- diversified -- one batched Gram and one batched greedy launch whose pool sizes are the
// finish's, ONE copy of the chunk's result block and one synchronisation.  The plan is the chunk's (the largest query
// norm): a band wider than a query's own only adds candidates and can only make the boundary rule more cautious; what is
// decided is decided on reference-order scores, so a decided answer is the definition's, as the single path's is.
// forms[q]: 0 decided on the device; 1 handed back on a capacity; 2 handed back as undecidable here (status 2 of the
// finish, a masked row came back, the workspace could not be reserved); 3 by rule for this query alone (it rode the scan
// with an empty lexical slice and its result is not read).  Every query with a non-zero form is answered by capped_query
// on the same context after all decided queries have been read out of the pinned block; its neighbours stay decided.
// hits[q] / picked[q] as capped_query leaves them.  c->d_hist is not touched: the shared scans run without a histogram.
int32_t capped_batch_chunk(rlr_index *ix, Ctx *c, const rlr_filter *f, const float *queries, const CappedCall *calls, uint32_t m,
                           const CappedBatchCall &bc, std::vector<CappedHit> *hits, bool *picked, uint32_t *forms)
{
    const uint64_t n_allowed = f ? f->n_allowed : ix->n_rows;
    const uint32_t n = static_cast<uint32_t>(ix->n_rows), P = bc.need;
    const SearchPlan p = make_plan(ix, queries, m, P, bc.guard_eps);
    RLR_TRY(ctx_prepare(ix, c, m, p));
    uint32_t B = 1;
    for (uint32_t q = 0; q < m; ++q) {
        forms[q] = capped_query_by_rule(calls[q]) ? 3 : 0;
        picked[q] = true;
        if (forms[q] == 0)
            B = std::max<uint32_t>(B, static_cast<uint32_t>(calls[q].lrow.size()));
    }
    const uint32_t k_cap = rlr::result_k_cap(bc.k, P, bc.diversify);
    const uint32_t tab_bits = group_table_bits(n_allowed);
    const CappedBatchWs sizes(nullptr, nullptr, ix->q_pitch, m, P, B, bc.diversify);
    hipStream_t s = c->stream;
    uint64_t cand_total = 0;
    uint32_t n_decided = 0;
    // the chunk's workspace: the grouped state, a slice per query (and ONE key table), and the pool workspace beside it
    hipError_t e = reserve_group_state(ix, c, m, bc.per_doc, tab_bits);
    if (e == hipSuccess)
        e = c->d_sample.reserve(m * score_stride(ix));
    if (e == hipSuccess)
        e = c->d_pool.reserve(sizes.d.floats());
    if (e == hipErrorOutOfMemory) {
        (void)hipGetLastError(); // no error of the call: the queries go one by one, in the single path's smaller workspace
        for (uint32_t q = 0; q < m; ++q)
            if (forms[q] == 0)
                forms[q] = 2;
    } else {
        RLR_HIP(e);
        RLR_TRY(pin_reserve(c, sizes.h.bytes));
        const CappedBatchWs ws(c->d_pool.get(), c->h_pin.get(), ix->q_pitch, m, P, B, bc.diversify);
        stage_queries(ix, c, queries, m, ws.h_q);
        c->h_q_kq = nullptr;
        RLR_HIP(upload_queries(c, ws.h_q, static_cast<size_t>(m) * ix->q_pitch * sizeof(float), s));
        rlr::CappedBatchArgs ca{};
        for (uint32_t q = 0; q < m; ++q) { // (a by-rule query rides with an empty slice)
            const uint32_t nl = forms[q] == 0 ? static_cast<uint32_t>(calls[q].lrow.size()) : 0u;
            uint32_t *hr = ws.h_lrow + static_cast<size_t>(q) * B;
            float *hs = ws.h_lscore + static_cast<size_t>(q) * B;
            if (nl) {
                std::memcpy(hr, calls[q].lrow.data(), static_cast<size_t>(nl) * sizeof(uint32_t));
                std::memcpy(hs, calls[q].lscore.data(), static_cast<size_t>(nl) * sizeof(float));
            }
            std::memset(hr + nl, 0, static_cast<size_t>(B - nl) * sizeof(uint32_t));
            std::memset(hs + nl, 0, static_cast<size_t>(B - nl) * sizeof(float));
            ws.h_lcnt[q] = nl;
            ca.n_lex[q] = nl;
            ca.max_lex[q] = forms[q] == 0 ? calls[q].max_lex : 1.0f;
        }
        RLR_HIP(hipMemcpyAsync(ws.lrow, ws.h_lrow, ws.lex_words() * sizeof(uint32_t), hipMemcpyHostToDevice, s));
        RLR_TRY(shared_scan(ix, c, f, m, "capped"));
        RLR_HIP(launch_score_rows_batch(ix->d_rows.get(), ix->pitch16, ix->dim, ix->dtype, c->d_query.get(), ix->q_pitch, m, ws.lrow, B,
                                        ws.lcos, ws.lcnt, 1, n, s));
        ca.w_e = bc.w_e;
        ca.w_l = bc.w_l;
        ca.eps = p.two_eps * 0.5f;
        ca.n_allowed = static_cast<uint32_t>(n_allowed);
        ca.lrow = ws.lrow;
        ca.lscore = ws.lscore;
        ca.lcos = ws.lcos;
        ca.lex_stride = B;
        ca.scratch = ws.scratch;
        ca.list = ws.list;
        ca.comb = ws.comb;
        ca.cosv = ws.cos;
        ca.lexv = ws.lexv;
        ca.docs = ws.docs;
        ca.info = ws.info;
        ca.sizes = ws.sizes;
        GroupBatchArgs ga = make_group_batch_args(ix, c, m, P, bc.per_doc, p.two_eps, tab_bits);
        ga.capped = &ca;
        RLR_HIP(launch_group_batch_tail(ga, s));
        if (bc.diversify) {
            RLR_HIP(launch_gram_rows(ix->d_rows.get(), ix->pitch16, ix->dim, ix->dtype, ws.list, P, ws.gram, m, s));
            RLR_HIP(launch_mmr_greedy(ws.gram, ws.comb, P, bc.k, bc.lambda, ws.order, ws.mmr, ws.nsel, ws.sizes, m, s));
        }
        RLR_HIP(hipMemcpyAsync(ws.h_res, ws.list, ws.res_words() * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        RLR_HIP(hipStreamSynchronize(s));
        // the result block as the device laid it out: list | comb | cos | lexv | docs | order | info | sizes | nsel
        const size_t plane = static_cast<size_t>(m) * P;
        const uint32_t *r_list = ws.h_res, *r_docs = ws.h_res + 4 * plane, *r_order = ws.h_res + 5 * plane;
        const float *r_comb = reinterpret_cast<const float *>(ws.h_res + plane), *r_cos = reinterpret_cast<const float *>(ws.h_res + 2 * plane);
        const float *r_lex = reinterpret_cast<const float *>(ws.h_res + 3 * plane);
        const uint32_t *r_info = ws.h_res + 6 * plane, *r_nsel = r_info + 3 * static_cast<size_t>(m);
        for (uint32_t q = 0; q < m; ++q) {
            if (forms[q] != 0)
                continue;
            const uint32_t status = r_info[2 * q + 1], n_pool = r_info[2 * q];
            if (status != 0 || n_pool > P) {
                forms[q] = status == 1 ? 1 : 2; // capacity | undecidable here (the boundary rule, rows that order last are wanted)
                continue;
            }
            const size_t base = static_cast<size_t>(q) * P;
            const uint32_t cnt = std::min<uint32_t>(bc.diversify ? r_nsel[q] : n_pool, k_cap);
            std::vector<CappedHit> &out = hits[q];
            out.resize(cnt);
            for (uint32_t i = 0; i < cnt && forms[q] == 0; ++i) {
                const uint32_t o = bc.diversify ? r_order[base + i] : i;
                if (o >= n_pool || (f && !filter_holds(f, r_list[base + o])))
                    forms[q] = 2; // a masked row came back (the hazard masked_row_among documents)
                else
                    out[i] = CappedHit{r_list[base + o], r_docs[base + o], r_comb[base + o], r_cos[base + o], r_lex[base + o]};
            }
            if (forms[q] == 0) {
                cand_total += n_pool;
                n_decided++;
            }
        }
    }
    c->hist_dirty = false;
    RLR_TRY(note_chunk(ix, c, m, m - n_decided, cand_total));
    // (from here on the pinned block and the context are capped_query's)
    for (uint32_t q = 0; q < m; ++q)
        if (forms[q] != 0) {
            hits[q].clear();
            RLR_TRY(capped_query(ix, c, f, calls[q], hits[q], &picked[q]));
        }
    return RLR_OK;
}

// ---- what the entry points of a pair (the one-by-one call and its batched twin) check alike ---------------------------
// The handles, the arguments, the device; every n_out cleared.  Then the caller may return early on an empty row set.
int32_t grouped_entry(rlr_index *ix, const rlr_filter *f, const float *queries, uint32_t n_queries, uint32_t k, uint32_t per_doc,
                      uint64_t *rows_out, float *cos_out, uint32_t *n_out)
{
    RLR_TRY(check_handle(ix));
    if (f)
        RLR_TRY(check_filter(ix, f)); // (a stale filter is refused before any GPU work)
    if (k == 0 || per_doc < 1 || per_doc > RLR_MAX_PER_DOCUMENT)
        return set_error(RLR_E_INVALID, "k must be positive and per_doc in 1..%d (k = %u, per_doc = %u)", RLR_MAX_PER_DOCUMENT, k, per_doc);
    if (n_queries && (!queries || !n_out || !rows_out || !cos_out))
        return set_error(RLR_E_INVALID, "queries / n_out / output buffers are null");
    RLR_TRY(use_device(ix));
    for (uint32_t q = 0; q < n_queries; ++q)
        n_out[q] = 0;
    return RLR_OK;
}

int32_t range_entry(rlr_index *ix, const rlr_filter *f, const float *queries, uint32_t n_queries, const float *tau, uint32_t cap,
                    uint64_t *rows_out, float *cos_out, uint32_t *n_out, uint64_t *n_total_out)
{
    RLR_TRY(check_handle(ix));
    if (f)
        RLR_TRY(check_filter(ix, f)); // (a stale filter is refused before any GPU work)
    if (n_queries && (!queries || !tau || !n_total_out))
        return set_error(RLR_E_INVALID, "queries / tau / n_total_out is null");
    if (n_queries && cap && (!rows_out || !cos_out || !n_out))
        return set_error(RLR_E_INVALID, "output buffers are null (only a count-only call, cap == 0, may leave them out)");
    for (uint32_t q = 0; q < n_queries; ++q)
        if (!(tau[q] == tau[q]))
            return set_error(RLR_E_INVALID, "tau[%u] is NaN", q);
    RLR_TRY(use_device(ix));
    for (uint32_t q = 0; q < n_queries; ++q) {
        if (n_out)
            n_out[q] = 0;
        n_total_out[q] = 0;
    }
    return RLR_OK;
}

} // namespace
} // namespace rlr

extern "C" {

int32_t rlr_search_topk_grouped(rlr_index *ix, const rlr_filter *f, const float *queries, uint32_t n_queries, uint32_t k,
                                uint32_t per_doc, float guard_eps, uint64_t *rows_out, float *cos_out, uint32_t *docs_out, uint32_t *n_out)
{
    RLR_TRY(grouped_entry(ix, f, queries, n_queries, k, per_doc, rows_out, cos_out, n_out));
    if ((f ? f->n_allowed : ix->n_rows) == 0 || n_queries == 0)
        return RLR_OK;
    CtxLease lease(ix);
    RLR_TRY(ctx_acquire(ix, &lease.c));
    StreamDrain drain{lease.c->stream};
    for (uint32_t q = 0; q < n_queries; ++q) // one by one: no coalescer, no nomination copy, no shared pass
        RLR_TRY(grouped_query(ix, lease.c, f, queries + static_cast<size_t>(q) * ix->dim, k, per_doc, guard_eps,
                              rows_out + static_cast<size_t>(q) * k, cos_out + static_cast<size_t>(q) * k,
                              docs_out ? docs_out + static_cast<size_t>(q) * k : nullptr, &n_out[q]));
    drain.armed = false;
    return RLR_OK;
}

int32_t rlr_index_grouped_forms(rlr_index *ix, uint64_t counts[4], int32_t reset)
{
    return read_forms(ix, &rlr_index::grouped_forms, counts, reset);
}

int32_t rlr_search_topk_grouped_batch(rlr_index *ix, const rlr_filter *f, const float *queries, uint32_t n_queries, uint32_t k,
                                      uint32_t per_doc, float guard_eps, uint64_t *rows_out, float *cos_out, uint32_t *docs_out,
                                      uint32_t *n_out)
{
    RLR_TRY(grouped_entry(ix, f, queries, n_queries, k, per_doc, rows_out, cos_out, n_out));
    const uint64_t n_allowed = f ? f->n_allowed : ix->n_rows;
    if (n_allowed == 0 || n_queries == 0)
        return RLR_OK;
    CtxLease lease(ix);
    RLR_TRY(ctx_acquire(ix, &lease.c));
    StreamDrain drain{lease.c->stream};
    // The chunk width w, 0 by rule (chunk_width_by_rule), in mode 1 or where the gate declined.  Then the queries are split
    // evenly (chunk_size); a chunk of one goes by rule as well.
    const int32_t mode = ix->grouped_sharing.load();
    uint32_t w = mode != 1 ? chunk_width_by_rule(ix, f, n_queries, std::min<uint64_t>(k, n_allowed), per_doc) : 0;
    if (w >= 2 && mode == 0 && !grouped_share_wins(ix, f, w, per_doc))
        w = 0;
    uint64_t forms[4] = {0, 0, 0, 0};
    uint32_t chunk_forms[8];
    int32_t rc = RLR_OK;
    for (uint32_t q0 = 0, ci = 0; q0 < n_queries && rc == RLR_OK; ++ci) {
        const uint32_t m = chunk_size(n_queries, w, ci);
        const float *qs = queries + static_cast<size_t>(q0) * ix->dim;
        uint64_t *ro = rows_out + static_cast<size_t>(q0) * k;
        float *co = cos_out + static_cast<size_t>(q0) * k;
        uint32_t *dout = docs_out ? docs_out + static_cast<size_t>(q0) * k : nullptr;
        if (m < 2) {
            rc = grouped_query(ix, lease.c, f, qs, k, per_doc, guard_eps, ro, co, dout, &n_out[q0]);
            forms[3]++;
        } else {
            rc = grouped_batch_chunk(ix, lease.c, f, qs, m, k, per_doc, guard_eps, ro, co, dout, n_out + q0, chunk_forms);
            for (uint32_t i = 0; i < m && rc == RLR_OK; ++i)
                forms[chunk_forms[i]]++;
        }
        q0 += m;
    }
    {
        std::lock_guard<std::mutex> lk(ix->mu);
        for (int i = 0; i < 4; ++i)
            ix->grouped_batch_forms[i] += forms[i];
    }
    RLR_TRY(rc);
    drain.armed = false;
    return RLR_OK;
}

int32_t rlr_index_set_grouped_sharing(rlr_index *ix, int32_t mode)
{
    RLR_TRY(check_handle(ix));
    if (mode < 0 || mode > 2)
        return set_error(RLR_E_INVALID, "grouped sharing mode %d (0 the gate, 1 never, 2 wherever the shape allows)", mode);
    ix->grouped_sharing.store(mode);
    return RLR_OK;
}

int32_t rlr_index_grouped_batch_forms(rlr_index *ix, uint64_t counts[4], int32_t reset)
{
    return read_forms(ix, &rlr_index::grouped_batch_forms, counts, reset);
}

int32_t rlr_search_range(rlr_index *ix, const rlr_filter *f, const float *queries, uint32_t n_queries, const float *tau, uint32_t cap,
                         float guard_eps, uint64_t *rows_out, float *cos_out, uint32_t *n_out, uint64_t *n_total_out)
{
    RLR_TRY(range_entry(ix, f, queries, n_queries, tau, cap, rows_out, cos_out, n_out, n_total_out));
    if ((f ? f->n_allowed : ix->n_rows) == 0 || n_queries == 0)
        return RLR_OK;
    CtxLease lease(ix);
    RLR_TRY(ctx_acquire(ix, &lease.c));
    StreamDrain drain{lease.c->stream};
    for (uint32_t q = 0; q < n_queries; ++q) // one by one: no coalescer, no nomination copy, no shared pass
        RLR_TRY(range_query(ix, lease.c, f, queries + static_cast<size_t>(q) * ix->dim, tau[q], cap, guard_eps,
                            cap ? rows_out + static_cast<size_t>(q) * cap : nullptr, cap ? cos_out + static_cast<size_t>(q) * cap : nullptr,
                            n_out ? &n_out[q] : nullptr, &n_total_out[q]));
    drain.armed = false;
    return RLR_OK;
}

int32_t rlr_index_range_forms(rlr_index *ix, uint64_t counts[4], int32_t reset)
{
    return read_forms(ix, &rlr_index::range_forms, counts, reset);
}

int32_t rlr_search_range_batch(rlr_index *ix, const rlr_filter *f, const float *queries, uint32_t n_queries, const float *tau,
                               uint32_t cap, float guard_eps, uint64_t *rows_out, float *cos_out, uint32_t *n_out,
                               uint64_t *n_total_out)
{
    RLR_TRY(range_entry(ix, f, queries, n_queries, tau, cap, rows_out, cos_out, n_out, n_total_out));
    if ((f ? f->n_allowed : ix->n_rows) == 0 || n_queries == 0)
        return RLR_OK;
    CtxLease lease(ix);
    RLR_TRY(ctx_acquire(ix, &lease.c));
    StreamDrain drain{lease.c->stream};
    // the chunks: up to kBatchMaxQueries queries per GEMM pass, all of 2..8 in one shared scan; anything else one by one
    const int32_t mode = ix->range_sharing.load();
    RangeShare path = kRangeShareNone;
    if (mode != 1 && n_queries >= 2) {
        const bool f16_ok = make_plan(ix, queries, n_queries, 1, guard_eps).f16_ok;
        path = range_share_path(ix, f, n_queries, f16_ok);
        if (path != kRangeShareNone && mode == 0 && !range_share_wins(ix, f, std::min(n_queries, kBatchMaxQueries), cap, path))
            path = kRangeShareNone;
    }
    uint64_t forms[4] = {0, 0, 0, 0};
    std::vector<uint32_t> chunk_forms;
    int32_t rc = RLR_OK;
    for (uint32_t q0 = 0; q0 < n_queries && rc == RLR_OK;) {
        const float *qs = queries + static_cast<size_t>(q0) * ix->dim;
        uint64_t *ro = cap ? rows_out + static_cast<size_t>(q0) * cap : nullptr;
        float *co = cap ? cos_out + static_cast<size_t>(q0) * cap : nullptr;
        if (path == kRangeShareNone) {
            rc = range_query(ix, lease.c, f, qs, tau[q0], cap, guard_eps, ro, co, n_out ? &n_out[q0] : nullptr, &n_total_out[q0]);
            forms[3]++;
            q0 += 1;
            continue;
        }
        const uint32_t m = std::min(kBatchMaxQueries, n_queries - q0);
        chunk_forms.assign(m, 0);
        rc = range_batch_chunk(ix, lease.c, f, path, qs, tau + q0, m, cap, guard_eps, ro, co, n_out ? n_out + q0 : nullptr,
                               n_total_out + q0, chunk_forms.data());
        for (uint32_t i = 0; i < m && rc == RLR_OK; ++i)
            forms[chunk_forms[i]]++;
        q0 += m;
    }
    {
        std::lock_guard<std::mutex> lk(ix->mu);
        for (int i = 0; i < 4; ++i)
            ix->range_batch_forms[i] += forms[i];
    }
    RLR_TRY(rc);
    drain.armed = false;
    return RLR_OK;
}

int32_t rlr_index_set_range_sharing(rlr_index *ix, int32_t mode)
{
    RLR_TRY(check_handle(ix));
    if (mode < 0 || mode > 2)
        return set_error(RLR_E_INVALID, "range sharing mode %d (0 auto, 1 never, 2 wherever the shape allows)", mode);
    ix->range_sharing.store(mode);
    return RLR_OK;
}

int32_t rlr_index_range_batch_forms(rlr_index *ix, uint64_t counts[4], int32_t reset)
{
    return read_forms(ix, &rlr_index::range_batch_forms, counts, reset);
}

int32_t rlr_search_capped(rlr_index *ix, const rlr_filter *f, const float *query, uint32_t need_in, uint32_t k, float lambda,
                          int32_t diversify, float w_embedding, float w_lexical, const uint64_t *lex_rows, const float *lex_scores,
                          uint32_t n_lex, float max_lex, uint32_t per_doc, float guard_eps, uint64_t *rows_out, float *cos_out,
                          float *score_out, float *lex_out, uint32_t *docs_out, uint32_t *n_out)
{
    RLR_TRY(check_handle(ix));
    if (f)
        RLR_TRY(check_filter(ix, f)); // (a stale filter is refused before any GPU work)
    if (per_doc < 1 || per_doc > RLR_MAX_PER_DOCUMENT)
        return set_error(RLR_E_INVALID, "per_doc must be in 1..%d (per_doc = %u)", RLR_MAX_PER_DOCUMENT, per_doc);
    if (!n_out)
        return set_error(RLR_E_INVALID, "n_out is null");
    *n_out = 0;
    const uint64_t n_allowed = f ? f->n_allowed : ix->n_rows;
    if (n_allowed == 0 || need_in == 0)
        return RLR_OK;
    if (!query || !rows_out || !cos_out || !score_out || !lex_out || (n_lex && (!lex_rows || !lex_scores)))
        return set_error(RLR_E_INVALID, "null argument");
    const CappedBatchCall bc{static_cast<uint32_t>(std::min<uint64_t>(need_in, n_allowed)), k, lambda, diversify != 0, w_embedding,
                             w_lexical, per_doc, guard_eps};
    CappedCall call;
    RLR_TRY(make_capped_call(ix, f, bc, query, lex_rows, lex_scores, n_lex, max_lex, -1, &call));
    RLR_TRY(use_device(ix));
    std::vector<CappedHit> hits;
    bool picked = true;
    {
        CtxLease lease(ix);
        RLR_TRY(ctx_acquire(ix, &lease.c));
        StreamDrain drain{lease.c->stream};
        RLR_TRY(capped_query(ix, lease.c, f, call, hits, &picked));
        drain.armed = false;
    }
    return capped_deliver(ix, hits, picked, k, lambda, rows_out, cos_out, score_out, lex_out, docs_out, n_out);
}

int32_t rlr_search_capped_batch(rlr_index *ix, const rlr_filter *f, const float *queries, uint32_t n_queries, uint32_t need_in,
                                uint32_t k, float lambda, int32_t diversify, float w_embedding, float w_lexical,
                                const uint64_t *lex_rows, const float *lex_scores, const uint64_t *lex_offsets, const float *max_lex,
                                uint32_t per_doc, float guard_eps, uint64_t *rows_out, float *cos_out, float *score_out,
                                float *lex_out, uint32_t *docs_out, uint32_t *n_out)
{
    RLR_TRY(check_handle(ix));
    if (f)
        RLR_TRY(check_filter(ix, f)); // (a stale filter is refused before any GPU work)
    if (per_doc < 1 || per_doc > RLR_MAX_PER_DOCUMENT)
        return set_error(RLR_E_INVALID, "per_doc must be in 1..%d (per_doc = %u)", RLR_MAX_PER_DOCUMENT, per_doc);
    if (n_queries && !n_out)
        return set_error(RLR_E_INVALID, "n_out is null");
    for (uint32_t q = 0; q < n_queries; ++q)
        n_out[q] = 0;
    const uint64_t n_allowed = f ? f->n_allowed : ix->n_rows;
    if (n_allowed == 0 || need_in == 0 || n_queries == 0)
        return RLR_OK;
    if (!queries || !rows_out || !cos_out || !score_out || !lex_out || !lex_offsets || !max_lex)
        return set_error(RLR_E_INVALID, "null argument");
    for (uint32_t q = 0; q < n_queries; ++q)
        if (lex_offsets[q + 1] < lex_offsets[q])
            return set_error(RLR_E_INVALID, "lex_offsets must be non-decreasing (query %u)", q);
    if (lex_offsets[n_queries] > lex_offsets[0] && (!lex_rows || !lex_scores))
        return set_error(RLR_E_INVALID, "null argument");
    std::vector<CappedCall> calls(n_queries);
    const CappedBatchCall bc{static_cast<uint32_t>(std::min<uint64_t>(need_in, n_allowed)), k, lambda, diversify != 0, w_embedding,
                             w_lexical, per_doc, guard_eps};
    for (uint32_t q = 0; q < n_queries; ++q) // (no pairs at all: lex_rows may be null, and is not touched)
        RLR_TRY(make_capped_call(ix, f, bc, queries + static_cast<size_t>(q) * ix->dim, lex_rows ? lex_rows + lex_offsets[q] : nullptr,
                                 lex_scores ? lex_scores + lex_offsets[q] : nullptr, lex_offsets[q + 1] - lex_offsets[q], max_lex[q], q,
                                 &calls[q]));
    RLR_TRY(use_device(ix));
    std::vector<std::vector<CappedHit>> hits(n_queries);
    std::unique_ptr<bool[]> picked(new bool[n_queries]);
    uint64_t forms[4] = {0, 0, 0, 0};
    int32_t rc = RLR_OK;
    {
        CtxLease lease(ix);
        RLR_TRY(ctx_acquire(ix, &lease.c));
        StreamDrain drain{lease.c->stream};
        // The chunk width w, 0 by rule for the whole call (chunk_width_by_rule with k = need; weights outside the proof's
        // assumptions), in mode 1 or where the gate declined.  Then the queries are split evenly (chunk_size); a chunk of
        // one goes by rule as well.
        const int32_t mode = ix->capped_sharing.load();
        const bool weights_ok = bc.w_e > 0.0f && std::isfinite(bc.w_e) && bc.w_l >= 0.0f && std::isfinite(bc.w_l);
        uint32_t w = mode != 1 && weights_ok ? chunk_width_by_rule(ix, f, n_queries, bc.need, per_doc) : 0;
        if (w >= 2 && mode == 0 && !capped_share_wins(ix, f, w, per_doc))
            w = 0;
        uint32_t chunk_forms[8];
        bool chunk_picked[8];
        for (uint32_t q0 = 0, ci = 0; q0 < n_queries && rc == RLR_OK; ++ci) {
            const uint32_t m = chunk_size(n_queries, w, ci);
            if (m < 2) {
                bool one = true;
                rc = capped_query(ix, lease.c, f, calls[q0], hits[q0], &one);
                picked[q0] = one;
                forms[3]++;
            } else {
                rc = capped_batch_chunk(ix, lease.c, f, queries + static_cast<size_t>(q0) * ix->dim, calls.data() + q0, m, bc,
                                        hits.data() + q0, chunk_picked, chunk_forms);
                for (uint32_t i = 0; i < m && rc == RLR_OK; ++i) {
                    forms[chunk_forms[i]]++;
                    picked[q0 + i] = chunk_picked[i];
                }
            }
            q0 += m;
        }
        {
            std::lock_guard<std::mutex> lk(ix->mu);
            for (int i = 0; i < 4; ++i)
                ix->capped_batch_forms[i] += forms[i];
        }
        RLR_TRY(rc);
        drain.armed = false;
    }
    // (the contexts are back: the exact forms' pools go through mmr_diversify, as in rlr_search_capped)
    for (uint32_t q = 0; q < n_queries; ++q) {
        const size_t at = static_cast<size_t>(q) * need_in;
        RLR_TRY(capped_deliver(ix, hits[q], picked[q], k, lambda, rows_out + at, cos_out + at, score_out + at, lex_out + at,
                               docs_out ? docs_out + at : nullptr, &n_out[q]));
    }
    return RLR_OK;
}

int32_t rlr_index_set_capped_sharing(rlr_index *ix, int32_t mode)
{
    RLR_TRY(check_handle(ix));
    if (mode < 0 || mode > 2)
        return set_error(RLR_E_INVALID, "capped sharing mode %d (0 the gate, 1 never, 2 wherever the shape allows)", mode);
    ix->capped_sharing.store(mode);
    return RLR_OK;
}

int32_t rlr_index_capped_batch_forms(rlr_index *ix, uint64_t counts[4], int32_t reset)
{
    return read_forms(ix, &rlr_index::capped_batch_forms, counts, reset);
}

int32_t rlr_index_capped_forms(rlr_index *ix, uint64_t counts[4], int32_t reset)
{
    return read_forms(ix, &rlr_index::capped_forms, counts, reset);
}

} // extern "C"
