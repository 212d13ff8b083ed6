// index_fused.hip -- the search chains of include/rlr_gpu.h that end in a blend or MMR on the device, on the frame of
// index_internal.h: MMR over given pools, diversified search (search -> MMR in one enqueue), hybrid search (cosine +
// BM25 blend, one query or many) and the kernels only they launch; the workspace layouts of those chains.
#include "index_internal.h"
#include "filter_internal.h"
#include "lds_select.h"
#include "lexical_internal.h"
#include "pool_prepare.h"
#include "sort_emit.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <new>

using namespace rlr;

namespace rlr {

// ---- search -> MMR without a host round trip (rlr_search_diverse): pool_prepare.h ---------------------------
template <bool FROM_CANDIDATES>
__global__ __launch_bounds__(1024) void pool_prepare_kernel(const uint64_t *__restrict__ packed, const SelectState *__restrict__ st,
                                                            PoolArgs pa)
{
    __shared__ __attribute__((aligned(16))) char s_pool[kPoolLdsBytes];
    pool_prepare_body<FROM_CANDIDATES, false>(packed, FROM_CANDIDATES ? st->n_cand : 0u, FROM_CANDIDATES ? st->cap : 0u, pa, s_pool);
}


// ---- hybrid search without host round trips (rlr_search_hybrid) -------------------------------------------
// The device twin of search_impl's candidate list when lexical (BM25) candidates exist (csrc/engine.cpp;
// rag_engine.rs:505-561): candidates = the `fetch` best rows by cosine UNITED with the lexical rows,
// combined = w_e * cos + w_l * (lex / max_lex) (two rounded products, one add; IEEE division), ordered
// (combined desc, NaN last, row asc), cut to `need`.  Slots [0, fetch) hold the fetched rows, [fetch, fetch + n_lex)
// the lexical rows that were not fetched; one bitonic sort in LDS orders them.  The same boundary rule as the host:
// every unfetched row is non-lexical and scores at most combine(cos of the last fetched row, 0); if the need-th
// candidate does not beat that, info[1] = 2 and the host takes the widening path.
constexpr uint32_t kHybridSlots = 4096, kHybridLexMax = 2048, kHybridSelMax = 2048, kHybridHash = 4096;
constexpr uint32_t kHybridFetchMargin = 32; // rows by cosine fetched beyond `need` (rlr_index::hybrid_fetch_full): room for ties

// What the blend needs to know about the lexical pairs, in device memory: written by the host copy (pairs handed in by
// the caller) or by lex_unpack_kernel (pairs left on the device by a BM25 scoring call).
struct HybridLexHeader {
    uint32_t n_lex;
    float max_lex; // max(lexical scores, f32::EPSILON) (rag_engine.rs:515-519)
};

// A scoring call's result (pack_result(score, row) keys, in any order) -> rows, scores, header.  Rows outside the index
// (a lexical index that ran ahead of the embedding matrix) keep their place but are marked: they still count for
// max_lexical, as in the reference, and never become candidates.  One workgroup (<= kHybridLexMax pairs).
__device__ inline void lex_unpack_body(const uint64_t *__restrict__ packed, const uint32_t *__restrict__ count, uint32_t limit,
                                       uint32_t n_rows, uint32_t *__restrict__ lrow, float *__restrict__ lscore,
                                       HybridLexHeader *__restrict__ hdr)
{
    __shared__ uint32_t s_max;
    if (threadIdx.x == 0)
        s_max = 0;
    __syncthreads();
    if (*count == kLexicalRetry) { // the BM25 selection handed the query back: so does the blend (info[1] = 3)
        if (threadIdx.x == 0) {
            hdr->n_lex = kLexicalRetry;
            hdr->max_lex = 1.0f;
        }
        return;
    }
    const uint32_t n = min(*count, limit);
    uint32_t mx = 0; // largest ordered score key: fold(0.0, f32::max) over the scores (:515-519)
    for (uint32_t i = threadIdx.x; i < n; i += 1024) {
        float sc;
        uint32_t row;
        unpack_result(packed[i], &sc, &row);
        lrow[i] = row < n_rows ? row : 0xFFFFFFFFu;
        lscore[i] = sc;
        mx = max(mx, static_cast<uint32_t>(packed[i] >> 32));
    }
    atomicMax(&s_max, mx);
    __syncthreads();
    if (threadIdx.x == 0) {
        hdr->n_lex = n;
        const float m = s_max ? fmaxf(0.0f, key_score(s_max)) : 0.0f; // NaN scores (key 0) are ignored like f32::max does
        hdr->max_lex = m >= 1.1920929e-07f ? m : 1.1920929e-07f;
    }
}

__global__ __launch_bounds__(1024) void lex_unpack_kernel(const uint64_t *__restrict__ packed, const uint32_t *__restrict__ count,
                                                          uint32_t limit, uint32_t n_rows, uint32_t *__restrict__ lrow,
                                                          float *__restrict__ lscore, HybridLexHeader *__restrict__ hdr)
{
    lex_unpack_body(packed, count, limit, n_rows, lrow, lscore, hdr);
}

// one query per workgroup (rlr_engine_search_text_batch): query q's keys at packed + q * sel_stride, its count at
// count + q * count_stride, its pairs at lrow / lscore + q * bound
__global__ __launch_bounds__(1024) void lex_unpack_batch_kernel(const uint64_t *__restrict__ packed, uint32_t sel_stride,
                                                                const uint32_t *__restrict__ count, uint32_t count_stride,
                                                                uint32_t limit, uint32_t n_rows, uint32_t bound,
                                                                uint32_t *__restrict__ lrow, float *__restrict__ lscore,
                                                                HybridLexHeader *__restrict__ hdr)
{
    const uint32_t q = blockIdx.x;
    lex_unpack_body(packed + static_cast<size_t>(q) * sel_stride, count + static_cast<size_t>(q) * count_stride, limit, n_rows,
                    lrow + static_cast<size_t>(q) * bound, lscore + static_cast<size_t>(q) * bound, hdr + q);
}

__device__ inline void hybrid_pool_body(const uint64_t *__restrict__ packed, uint32_t fetch, uint32_t need, uint32_t n_rows,
                                        float w_e, float w_l, const uint32_t *__restrict__ lrow, const float *__restrict__ lscore,
                                        const float *__restrict__ lcos, const HybridLexHeader *__restrict__ hdr,
                                        float *__restrict__ cand, // 3 x kHybridSlots: combined | cos | lex
                                        uint32_t *__restrict__ list, float *__restrict__ comb, float *__restrict__ cosv,
                                        float *__restrict__ lexv, uint32_t *__restrict__ info, uint32_t k_cap,
                                        uint32_t *__restrict__ h_out) // h_out != null: a search without diversification --
                                                                      // the pool IS the result, emitted here
{
    __shared__ uint64_t s_key[kHybridSlots];   // slot -> (ordered combined score, ~row); 0 = empty
    __shared__ uint64_t s_sel[kHybridSelMax];  // the keys that can be among the first `need`
    __shared__ uint32_t s_slot[kHybridSelMax]; // ... and their slots
    __shared__ uint32_t s_hrow[kHybridHash];   // open-addressing map lexical row + 1 -> its index in the pair list
    __shared__ uint32_t s_hidx[kHybridHash];
    __shared__ uint32_t s_flag[kHybridLexMax]; // lexical pair j was reached by the fetch
    __shared__ uint32_t s_hist[2048];
    __shared__ uint32_t s_pick[3];
    __shared__ uint32_t s_got, s_cand, s_nsel, s_emin;
    __shared__ float s_cneed;
    const uint32_t t = threadIdx.x;
    float *cc = cand, *ce = cand + kHybridSlots, *cl = cand + 2 * kHybridSlots;
    if (hdr->n_lex == kLexicalRetry) { // (uniform) no usable lexical pairs: the host path repeats the BM25 query exactly
        if (threadIdx.x == 0) {
            info[0] = 0;
            info[1] = 3;
        }
        if (h_out)
            hybrid_emit_body(list, comb, cosv, lexv, 0u, 3u, k_cap, h_out);
        return;
    }
    const uint32_t n_lex = min(hdr->n_lex, kHybridLexMax);
    const float max_lex = hdr->max_lex;
    if (t == 0) {
        s_got = 0;
        s_cand = 0;
        s_nsel = 0;
        s_cneed = 0.0f;
        s_emin = 0xFFFFFFFFu;
    }
    for (uint32_t i = t; i < kHybridHash; i += 1024)
        s_hrow[i] = 0;
    for (uint32_t j = t; j < n_lex; j += 1024)
        s_flag[j] = 0;
    __syncthreads();
    for (uint32_t j = t; j < n_lex; j += 1024) {
        const uint32_t row = lrow[j];
        if (row == 0xFFFFFFFFu)
            continue;
        uint32_t h = (row * 2654435761u) >> 20; // 12 bits
        for (;;) {
            const uint32_t old = atomicCAS(&s_hrow[h], 0u, row + 1);
            if (old == 0u) {
                s_hidx[h] = j;
                break;
            }
            h = (h + 1) & (kHybridHash - 1); // rows are unique: never the same key twice
        }
    }
    __syncthreads();
    const bool overflow = packed[0] == ~0ull;
    const uint32_t total = fetch + n_lex;
    for (uint32_t i = t; i < fetch; i += 1024) {
        const uint64_t p = overflow ? 0ull : packed[i];
        uint64_t key = 0;
        if (p != 0) { // valid entries are a prefix (in no particular order), padding zeros behind
            const uint32_t row = 0xFFFFFFFFu - static_cast<uint32_t>(p & 0xFFFFFFFFull);
            const float e = key_score(static_cast<uint32_t>(p >> 32));
            atomicMin(&s_emin, static_cast<uint32_t>(p >> 32)); // the smallest fetched cosine (NaN orders lowest)
            float l = 0.0f;
            uint32_t h = (row * 2654435761u) >> 20;
            for (;;) {
                const uint32_t hr = s_hrow[h];
                if (hr == 0u)
                    break;
                if (hr == row + 1) {
                    const uint32_t j = s_hidx[h];
                    l = lscore[j] / max_lex;
                    s_flag[j] = 1;
                    break;
                }
                h = (h + 1) & (kHybridHash - 1);
            }
            const float t0 = w_e * e;
            const float t1 = w_l * l;
            const float c = t0 + t1;
            cc[i] = c;
            ce[i] = e;
            cl[i] = l;
            key = (static_cast<uint64_t>(score_key(c == 0.0f ? 0.0f : c)) << 32) | (p & 0xFFFFFFFFull); // -0 ties with +0
            atomicAdd(&s_got, 1u);
        }
        s_key[i] = key;
    }
    __syncthreads();
    for (uint32_t j = t; j < n_lex; j += 1024) {
        uint64_t key = 0;
        const uint32_t slot = fetch + j;
        const uint32_t row = lrow[j];
        if (row != 0xFFFFFFFFu && !s_flag[j]) { // a lexical row the fetch did not reach
            const float e = lcos[j];
            const float l = lscore[j] / max_lex;
            const float t0 = w_e * e;
            const float t1 = w_l * l;
            const float c = t0 + t1;
            cc[slot] = c;
            ce[slot] = e;
            cl[slot] = l;
            key = (static_cast<uint64_t>(score_key(c == 0.0f ? 0.0f : c)) << 32) | (0xFFFFFFFFu - row);
            atomicAdd(&s_cand, 1u);
        }
        s_key[slot] = key;
    }
    __syncthreads();
    const uint32_t got = s_got, n_cand = got + s_cand, n_pool = min(n_cand, need);
    // a lower edge that between need and need + 32 of the full keys reach (the passes of the radix select stop as soon as a
    // bin decides that much), then those are ranked.  [It was the need-th largest 32-bit SCORE in three fixed passes and
    // everything at or above it: a score shared by thousands of candidates flooded the rank sort and sent the query to the
    // host path -- the row half of the key splits such a class here.]
    uint64_t key_lo = 0;
    if (n_cand > need)
        key_lo = lds_kth_key64(s_key, total, need, s_hist, s_pick, 1024, /*slack=*/32);
    for (uint32_t i = t; i < total; i += 1024) {
        const uint64_t v = s_key[i];
        if (v != 0 && v >= key_lo) {
            const uint32_t at = atomicAdd(&s_nsel, 1u);
            if (at < kHybridSelMax) {
                s_sel[at] = v;
                s_slot[at] = i;
            }
        }
    }
    __syncthreads();
    const uint32_t n_sel = s_nsel;
    const bool flood = n_sel > kHybridSelMax; // (cannot happen with the select above; kept as the guard of s_sel's capacity)
    if (!flood)
        for (uint32_t i = t; i < n_sel; i += 1024) {
            const uint64_t mine = s_sel[i];
            const uint32_t rank = lds_rank_desc(s_sel, n_sel, mine); // keys are unique (the row is part of the key)
            if (rank < n_pool) {
                const uint32_t slot = s_slot[i];
                list[rank] = 0xFFFFFFFFu - static_cast<uint32_t>(mine & 0xFFFFFFFFull);
                comb[rank] = cc[slot];
                cosv[rank] = ce[slot];
                lexv[rank] = cl[slot];
                if (rank == need - 1)
                    s_cneed = cc[slot];
            }
        }
    for (uint32_t r = n_pool + t; r < need; r += 1024) { // unused slots: a valid row, never read by the greedy kernel
        list[r] = 0;
        comb[r] = 0.0f;
        cosv[r] = 0.0f;
        lexv[r] = 0.0f;
    }
    __syncthreads();
    if (t == 0) {
        uint32_t status = overflow ? 1u : flood ? 2u : 0u;
        if (!status && got < n_rows && got > 0) {
            const float t0 = w_e * key_score(s_emin); // the smallest fetched cosine bounds every unfetched (non-lexical) row
            const float t1 = w_l * 0.0f;
            const float c_tail = t0 + t1;
            const bool ok = n_cand >= need && (c_tail != c_tail || s_cneed > c_tail);
            if (!ok)
                status = 2u;
        }
        info[0] = status ? 0u : n_pool;
        info[1] = status;
        s_pick[0] = status;
    }
    if (h_out) { // (list .. lexv were stored by this workgroup's own threads in front of the barrier above)
        __syncthreads();
        const uint32_t status = s_pick[0];
        hybrid_emit_body(list, comb, cosv, lexv, status ? 0u : min(n_pool, k_cap), status, k_cap, h_out);
    }
}

__global__ __launch_bounds__(1024) void hybrid_pool_kernel(const uint64_t *__restrict__ packed, uint32_t fetch, uint32_t need,
                                                           uint32_t n_rows, float w_e, float w_l,
                                                           const uint32_t *__restrict__ lrow, const float *__restrict__ lscore,
                                                           const float *__restrict__ lcos,
                                                           const HybridLexHeader *__restrict__ hdr,
                                                           float *__restrict__ cand, uint32_t *__restrict__ list,
                                                           float *__restrict__ comb, float *__restrict__ cosv,
                                                           float *__restrict__ lexv, uint32_t *__restrict__ info,
                                                           uint32_t k_cap, uint32_t *__restrict__ h_out)
{
    hybrid_pool_body(packed, fetch, need, n_rows, w_e, w_l, lrow, lscore, lcos, hdr, cand, list, comb, cosv, lexv, info, k_cap,
                     h_out);
}

// hybrid_pool_kernel for many queries (rlr_engine_search_text_batch), one workgroup each: query q's fetched keys at
// packed + q * fetch, pairs at + q * bound, header q, pool at + q * need; info[2q .. 2q + 1] = (pool size, status), and
// sizes[q] = the pool size again (the stride-1 array the batched greedy kernel reads)
__global__ __launch_bounds__(1024) void hybrid_pool_batch_kernel(const uint64_t *__restrict__ packed, uint32_t fetch, uint32_t need,
                                                                 uint32_t n_rows, float w_e, float w_l, uint32_t bound,
                                                                 const uint32_t *__restrict__ lrow, const float *__restrict__ lscore,
                                                                 const float *__restrict__ lcos,
                                                                 const HybridLexHeader *__restrict__ hdr, float *__restrict__ cand,
                                                                 uint32_t *__restrict__ list, float *__restrict__ comb,
                                                                 float *__restrict__ cosv, float *__restrict__ lexv,
                                                                 uint32_t *__restrict__ info, uint32_t *__restrict__ sizes)
{
    const uint32_t q = blockIdx.x;
    const size_t lo = static_cast<size_t>(q) * bound, po = static_cast<size_t>(q) * need;
    hybrid_pool_body(packed + static_cast<size_t>(q) * fetch, fetch, need, n_rows, w_e, w_l, lrow + lo, lscore + lo, lcos + lo,
                     hdr + q, cand + static_cast<size_t>(q) * 3 * kHybridSlots, list + po, comb + po, cosv + po, lexv + po,
                     info + 2 * q, 0u, nullptr);
    if (threadIdx.x == 0) // (thread 0 wrote info itself)
        sizes[q] = info[2 * q];
}

} // namespace rlr

namespace {

// ---- workspace layouts, each ONE list of regions over a Carver (index_internal.h) ----------------------------------
// The results of an MMR call over m pools of P: order | mmr | n, contiguous on the device and in pinned memory -- one
// copy of words() words moves them.
struct MmrResults {
    uint32_t *order;
    float *mmr;
    uint32_t *n;
    MmrResults(Carver &w, uint64_t m, uint64_t P)
        : order(w.take<uint32_t>(m * P)), mmr(w.take<float>(m * P)), n(w.take<uint32_t>(m)) {}
    static uint64_t words(uint64_t m, uint64_t P) { return 2 * m * P + m; }
};

// Device side (c->d_pool) of an MMR call over m pools of P.
struct MmrWs {
    uint64_t m, P, unused_head; // floats in front that no kernel reads (the single-pool call once gathered its pool there)
    Carver d;
    float *head = d.take<float>(unused_head), *gram = d.take<float>(m * P * P), *scores = d.take<float>(m * P);
    MmrResults res{d, m, P};
    uint32_t *sizes = d.take<uint32_t>(m), *pad = d.take<uint32_t>(8);
    MmrWs(float *base, uint32_t m_, uint32_t P_, uint64_t head_ = 0) : m(m_), P(P_), unused_head(head_), d(base) {}
};

// Pinned side (c->h_pin) of a batched MMR call: the row list upload_list stages at the head of the buffer | scores |
// sizes | the results.  Reserved as a whole BEFORE upload_list enqueues its copy, so that the buffer
// is never reallocated under a transfer.
struct MmrStaging {
    uint64_t m, P;
    Carver h;
    char *list = h.take<char>(m * P * 8 + 64);
    float *scores = h.take<float>(m * P);
    uint32_t *sizes = h.take<uint32_t>(m + 4);
    MmrResults res{h, m, P};
    char *pad = h.take<char>(64);
    MmrStaging(void *base, uint32_t m_, uint32_t P_) : m(m_), P(P_), h(base) {}
};

// rlr_search_diverse: device (c->d_pool) and pinned (c->h_pin: the staged query | the result block).
struct DiverseWs {
    uint64_t P, dim, q_pitch, k_cap;
    Carver d, h;
    float *unused = d.take<float>(P * dim); // (the Gram kernel reads the pool rows in place)
    float *gram = d.take<float>(P * P), *comb = d.take<float>(P), *cos = d.take<float>(P);
    uint32_t *order = d.take<uint32_t>(P);
    float *mmr = d.take<float>(P);
    uint32_t *nsel = d.take<uint32_t>(1), *info = d.take<uint32_t>(7);
    float *h_q = h.take<float>(q_pitch);
    uint32_t *h_out = h.take<uint32_t>(block_words(static_cast<uint32_t>(k_cap)));
    char *h_pad = h.take<char>(64);
    DiverseWs(float *d_base, void *h_base, const rlr_index *ix, uint32_t P_, uint32_t k_cap_)
        : P(P_), dim(ix->dim), q_pitch(ix->q_pitch), k_cap(k_cap_), d(d_base), h(h_base) {}
};

// A hybrid search: hybrid_begin_impl lays it out, the ticket carries it to hybrid_finish_impl.  Header, lexical rows and
// scores are adjacent on the device and in pinned memory (h_lex): host-supplied pairs travel in one copy.
struct HybridWs {
    uint64_t P, n_lex_bound, q_pitch, k_cap;
    Carver d, h;
    float *gram = d.take<float>(P * P), *comb = d.take<float>(P), *cos = d.take<float>(P), *lexv = d.take<float>(P);
    uint32_t *order = d.take<uint32_t>(P);
    float *mmr = d.take<float>(P);
    uint32_t *nsel = d.take<uint32_t>(1), *info = d.take<uint32_t>(7);
    HybridLexHeader *hdr = d.take<HybridLexHeader>(1);
    uint32_t *lrow = d.take<uint32_t>(2 * n_lex_bound); // the rows, then their scores: lscore()
    float *lcos = d.take<float>(n_lex_bound);
    float *cand = d.take<float>(3ull * kHybridSlots);                                    // blend candidates: combined | cos | lex
    float *h_q = h.take<float>(q_pitch);
    uint32_t *h_lex = h.take<uint32_t>(2 + 2 * n_lex_bound), *h_out = h.take<uint32_t>(block_words(static_cast<uint32_t>(k_cap)));
    char *h_pad = h.take<char>(64);
    HybridWs(float *d_base, void *h_base, uint32_t q_pitch_, uint32_t P_, uint32_t bound, uint32_t k_cap_)
        : P(P_), n_lex_bound(bound), q_pitch(q_pitch_), k_cap(k_cap_), d(d_base), h(h_base) {}
    HybridWs() : HybridWs(nullptr, nullptr, 0, 0, 0, 0) {}
    // The scores of n_lex pairs sit right behind their rows.  Pairs left on the device by the BM25 kernels use every slot
    // (n_lex = n_lex_bound: the LexSink of begin and the blend of finish agree by construction); host-supplied pairs
    // (n_lex <= n_lex_bound) are packed the same way in h_lex, so that header | rows | scores is one copy.
    float *lscore(uint32_t n_lex) const { return reinterpret_cast<float *>(lrow + n_lex); }
    static float *h_lscore(uint32_t *h_lex, uint32_t n_lex) { return reinterpret_cast<float *>(h_lex + 2 + n_lex); }
    static size_t lex_copy_bytes(uint32_t n_lex) { return sizeof(HybridLexHeader) + static_cast<size_t>(n_lex) * 8; }
};

// The per-query results of search_hybrid_batch (Q x P each, then per-query words): the same list on the device and in
// pinned memory, moved in one copy of words() words.
struct HybridBatchRes {
    uint32_t *list;
    float *comb, *cos, *lexv;
    uint32_t *order;
    float *mmr;
    uint32_t *nsel, *sizes, *info;
    HybridBatchRes(Carver &w, uint64_t Q, uint64_t P)
        : list(w.take<uint32_t>(Q * P)), comb(w.take<float>(Q * P)), cos(w.take<float>(Q * P)), lexv(w.take<float>(Q * P)),
          order(w.take<uint32_t>(Q * P)), mmr(w.take<float>(Q * P)), nsel(w.take<uint32_t>(Q)), sizes(w.take<uint32_t>(Q)),
          info(w.take<uint32_t>(2 * Q)) {}
    static uint64_t words(uint64_t Q, uint64_t P) { return 6 * Q * P + 4 * Q; }
};

// search_hybrid_batch, device side (c->d_pool)
struct HybridBatchWs {
    uint64_t Q, fetch, P, bound, q_pitch, gram_floats;
    Carver d;
    uint64_t *packed = d.take<uint64_t>(Q * fetch); // the fetched keys of every query
    float *q = d.take<float>(Q * q_pitch);
    uint32_t *lrow = d.take<uint32_t>(Q * bound);
    float *lscore = d.take<float>(Q * bound), *lcos = d.take<float>(Q * bound);
    HybridLexHeader *hdr = d.take<HybridLexHeader>(Q);
    float *cand = d.take<float>(Q * 3 * kHybridSlots);
    HybridBatchRes res{d, Q, P};
    float *gram = d.take<float>(gram_floats);
    HybridBatchWs(float *base, const rlr_index *ix, uint64_t Q_, uint32_t fetch_, uint32_t P_, uint32_t bound_, bool diversify)
        : Q(Q_), fetch(fetch_), P(P_), bound(bound_), q_pitch(ix->q_pitch), gram_floats(diversify ? Q_ * P_ * P_ : 0), d(base) {}
};

// search_hybrid_batch, pinned side (c->h_pin): fetched keys | queries | the results.  Laid out only once the cosine batch,
// which stages through the same buffer, is back.
struct HybridBatchPin {
    uint64_t Q, fetch, P, q_pitch;
    Carver h;
    uint64_t *packed = h.take<uint64_t>(Q * fetch);
    float *q = h.take<float>(Q * q_pitch);
    HybridBatchRes res{h, Q, P};
    char *pad = h.take<char>(64);
    HybridBatchPin(void *base, const rlr_index *ix, uint64_t Q_, uint32_t fetch_, uint32_t P_)
        : Q(Q_), fetch(fetch_), P(P_), q_pitch(ix->q_pitch), h(base) {}
};

} // namespace

namespace rlr {

rlr::MmrEmit mmr_emit(const uint32_t *list, const float *comb, const float *cosv, const float *lexv, const uint32_t *info,
                      uint32_t k_cap, uint32_t *h_out)
{
    return rlr::MmrEmit{list, comb, cosv, lexv, info, k_cap, h_out};
}

int32_t mmr_single_impl(rlr_index *ix, const uint64_t *pool_rows, const float *pool_scores, uint32_t P, uint32_t k,
                        float lambda, uint32_t *order_out, float *mmr_out, uint32_t *n_out, const void *d_matrix,
                        uint64_t n_matrix)
{
    RLR_TRY(check_handle(ix));
    if (!n_out)
        return set_error(RLR_E_INVALID, "n_out is null");
    *n_out = 0;
    if (P == 0)
        return RLR_OK; // `if candidates.is_empty() { return vec![] }`
    if (!pool_rows || !pool_scores || !order_out)
        return set_error(RLR_E_INVALID, "null argument");
    if (P > 4096)
        return set_error(RLR_E_INVALID, "pool of %u exceeds the supported 4096 candidates", P);
    RLR_TRY(use_device(ix));
    CtxLease lease(ix);
    RLR_TRY(ctx_acquire(ix, &lease.c));
    Ctx *c = lease.c;
    hipStream_t s = c->stream;
    RLR_TRY(upload_list(ix, c, pool_rows, P, d_matrix ? n_matrix : ~0ull));
    const uint64_t head = static_cast<uint64_t>(P) * ix->dim;
    RLR_HIP(c->d_pool.reserve(MmrWs(nullptr, 1, P, head).d.floats()));
    const MmrWs ws(c->d_pool.get(), 1, P, head);
    const bool timed = ix->profiling;
    RLR_HIP(hipMemcpyAsync(ws.scores, pool_scores, static_cast<size_t>(P) * sizeof(float), hipMemcpyHostToDevice, s));
    if (timed) RLR_HIP(hipEventRecord(c->ev[0], s));
    RLR_HIP(launch_gram_rows(d_matrix ? d_matrix : ix->d_rows.get(), ix->pitch16, ix->dim, ix->dtype, c->d_list.get(), P, ws.gram, 1, s));
    RLR_HIP(launch_mmr_greedy(ws.gram, ws.scores, P, k, lambda, ws.res.order, ws.res.mmr, ws.res.n, nullptr, 1, s));
    if (timed) RLR_HIP(hipEventRecord(c->ev[1], s));
    RLR_TRY(pin_reserve(c, (MmrResults::words(1, P) + 3) * 4));
    Carver pin(c->h_pin.get()); // (upload_list's copy out of it is ahead on the stream)
    const MmrResults h(pin, 1, P);
    RLR_HIP(hipMemcpyAsync(h.order, ws.res.order, MmrResults::words(1, P) * 4, hipMemcpyDeviceToHost, s));
    RLR_HIP(hipStreamSynchronize(s));
    if (timed)
        note_mmr(ix, c, 1);
    const uint32_t n_sel = h.n[0];
    for (uint32_t i = 0; i < n_sel; ++i) {
        order_out[i] = h.order[i];
        if (mmr_out)
            mmr_out[i] = h.mmr[i];
    }
    *n_out = n_sel;
    return RLR_OK;
}

} // namespace rlr

extern "C" {

int32_t rlr_mmr_select(rlr_index *ix, const uint64_t *pool_rows, const float *pool_scores, uint32_t P, uint32_t k,
                       float lambda, uint32_t *order_out, float *mmr_out, uint32_t *n_out)
{
    return mmr_single_impl(ix, pool_rows, pool_scores, P, k, lambda, order_out, mmr_out, n_out, nullptr, 0);
}

int32_t rlr_search_diverse(rlr_index *ix, const float *query, uint32_t pool, uint32_t k, float lambda, float w_embedding,
                           float w_lexical, float guard_eps, uint64_t *rows_out, float *cos_out, float *score_out,
                           uint32_t *n_out, int32_t *fallback)
{
    RLR_TRY(check_handle(ix));
    if (!n_out || !fallback)
        return set_error(RLR_E_INVALID, "n_out / fallback is null");
    *n_out = 0;
    *fallback = 0;
    if (ix->n_rows == 0 || pool == 0)
        return RLR_OK;
    if (!query || !rows_out || !cos_out || !score_out)
        return set_error(RLR_E_INVALID, "null argument");
    const uint32_t n = static_cast<uint32_t>(ix->n_rows);
    const uint32_t need = std::min<uint32_t>(n, pool);
    const uint32_t fetch = static_cast<uint32_t>(std::min<uint64_t>(n, static_cast<uint64_t>(need) + 8));
    if (need > rlr::kPoolMax || !(w_embedding > 0.0f) || !(w_lexical >= 0.0f) || !std::isfinite(w_lexical)) {
        *fallback = 1; // outside what the fused kernels cover: the caller's two-call path handles it
        return RLR_OK;
    }
    if (coalesce_hands_back(ix, need)) {
        *fallback = 1; // the two-call path's rlr_search_topk shares a pass with concurrent callers
        return RLR_OK;
    }
    RLR_TRY(use_device(ix));
    CtxLease lease(ix);
    RLR_TRY(ctx_acquire(ix, &lease.c));
    Ctx *c = lease.c;
    hipStream_t s = c->stream;
    const SearchPlan p = make_plan(ix, query, 1, fetch, guard_eps);
    RLR_TRY(ctx_prepare(ix, c, 1, p));
    count_f16_fallbacks(ix, p, 1, false);
    const uint32_t P = need;
    const uint32_t k_cap = rlr::result_k_cap(k, P, true);
    const DiverseWs sizes(nullptr, nullptr, ix, P, k_cap);
    RLR_HIP(c->d_pool.reserve(sizes.d.floats()));
    RLR_TRY(reserve_list(c, P));
    RLR_TRY(pin_reserve(c, sizes.h.bytes));
    const DiverseWs ws(c->d_pool.get(), c->h_pin.get(), ix, P, k_cap);
    uint32_t *h_out = ws.h_out;
    h_out[block_done(k_cap)] = kBlockPending; // (the greedy kernel's last store replaces it: what the wait below polls)
    stage_queries(ix, c, query, 1, ws.h_q);
    const bool timed = ix->profiling;
    RLR_HIP(stage_queries_for_scans(ix, c, ws.h_q, static_cast<size_t>(ix->q_pitch) * sizeof(float), s));
    uint64_t *d_meta = c->d_out.get() + fetch;
    const bool from_candidates = fetch <= 512; // (the band of a larger fetch rarely fits 1024)
    const PoolArgs pa{fetch, need, n, w_embedding, w_lexical, c->d_list.get(), ws.comb, ws.cos, ws.info};
    bool pool_done = false; // (the fused tail's finish builds the pool itself: one launch and ~13 us of config 2's chain less)
    RLR_HIP(enqueue_query(ix, c, 0, p, c->d_out.get(), d_meta, timed, /*emit=*/!from_candidates, from_candidates ? &pa : nullptr,
                          &pool_done));
    if (timed) RLR_HIP(hipEventRecord(c->bev[0], s));
    if (!pool_done) {
        if (from_candidates)
            hipLaunchKernelGGL(rlr::pool_prepare_kernel<true>, dim3(1), dim3(1024), 0, s, c->d_packed.get(), c->d_state.get(), pa);
        else
            hipLaunchKernelGGL(rlr::pool_prepare_kernel<false>, dim3(1), dim3(1024), 0, s, c->d_out.get(), c->d_state.get(), pa);
        RLR_HIP(hipGetLastError());
    }
    RLR_HIP(launch_gram_rows(ix->d_rows.get(), ix->pitch16, ix->dim, ix->dtype, c->d_list.get(), P, ws.gram, 1, s));
    const rlr::MmrEmit emit = mmr_emit(c->d_list.get(), ws.comb, ws.cos, nullptr, ws.info, k_cap, h_out);
    RLR_HIP(launch_mmr_greedy(ws.gram, ws.comb, P, k, lambda, ws.order, ws.mmr, ws.nsel, ws.info, 1, s, &emit));
    if (timed) RLR_HIP(hipEventRecord(c->bev[1], s));
    if (timed)
        RLR_HIP(hipStreamSynchronize(s)); // (the events are read below)
    else
        RLR_TRY(wait_block(h_out, k_cap, s, &c->wait_ema));
    RLR_TRY(check_hist_assert(c));
    c->hist_dirty = false;
    (void)note_search(ix, c, 1, 0, 0, timed, /*mmr_chain=*/true);
    *fallback = static_cast<int32_t>(read_block(h_out, k_cap, rows_out, cos_out, score_out, nullptr, n_out));
    return RLR_OK;
}

// where the lexical pairs of a hybrid search come from
struct HybridLexSrc {
    const uint64_t *h_rows = nullptr; // host pairs: ascending unique rows inside the index ...
    const float *h_scores = nullptr;
    uint32_t n_host = 0;
    float max_lex = 1.1920929e-07f;
    const rlr::LexPending *dev = nullptr; // ... or a BM25 call's result still on the device (null + n_host 0: no pairs)
};

} // extern "C"

namespace rlr {

// A hybrid search between its two enqueues: the scan / select / re-score / sort part is on the stream (it does not
// depend on the lexical pairs, only on an upper bound of their number), the blend and everything behind it follows in
// search_hybrid_finish.  In between the caller enqueues the BM25 kernels on their own stream: the device runs them
// beside the scan, and the host's launch calls for both overlap the scan instead of preceding it.
struct HybridTicket {
    rlr_index *ix;
    CtxLease lease;
    uint32_t n, need, fetch, k, k_cap;
    float lambda, w_e, w_l;
    int32_t diversify;
    bool timed;
    // begin hands the lexical side of it to the BM25 kernels (LexSink), finish blends from the same object.  It points into
    // c->d_pool and c->h_pin: the ticket holds the context's lease, and nothing may reserve() / pin_reserve() on this context
    // between begin and finish.
    HybridWs ws;
    explicit HybridTicket(rlr_index *i) : ix(i), lease(i) {}
};

static int32_t hybrid_begin_impl(rlr_index *ix, const float *query, uint32_t need_in, uint32_t k, float lambda, int32_t diversify,
                                 float w_embedding, float w_lexical, uint32_t n_lex_bound, float guard_eps, HybridTicket **out,
                                 int32_t *fallback, int32_t (*behind_scan)(void *, const LexSink *) = nullptr,
                                 void *behind_scan_arg = nullptr)
{
    *out = nullptr;
    *fallback = 0;
    RLR_TRY(check_handle(ix));
    if (!query)
        return set_error(RLR_E_INVALID, "null argument");
    const uint32_t n = static_cast<uint32_t>(ix->n_rows);
    const uint32_t need = std::min<uint32_t>(n, need_in);
    const uint64_t fetch_full = std::min<uint64_t>(n, static_cast<uint64_t>(need) + n_lex_bound + 8);
    const uint64_t fetch64 = ix->hybrid_fetch_full ? fetch_full : std::min<uint64_t>(fetch_full, static_cast<uint64_t>(need) + kHybridFetchMargin);
    if (n == 0 || need == 0 || need > kPoolMax || n_lex_bound > kHybridLexMax || fetch_full + n_lex_bound > kHybridSlots ||
        !(w_embedding > 0.0f) || !std::isfinite(w_embedding) || !std::isfinite(w_lexical)) {
        *fallback = 1; // outside what the fused kernels cover: the caller's host path handles it
        return RLR_OK;
    }
    if (coalesce_hands_back(ix, need)) {
        *fallback = 1; // the host path's rlr_search_topk shares a pass with concurrent callers
        return RLR_OK;
    }
    const uint32_t fetch = static_cast<uint32_t>(fetch64);
    RLR_TRY(use_device(ix));
    std::unique_ptr<HybridTicket> t(new (std::nothrow) HybridTicket(ix));
    if (!t)
        return set_error(RLR_E_OOM, "host allocation failed");
    RLR_TRY(ctx_acquire(ix, &t->lease.c));
    Ctx *c = t->lease.c;
    hipStream_t s = c->stream;
    // unordered: the blend orders fetched and lexical rows together -- it needs the fetched SET and its minimum
    const SearchPlan p = make_plan(ix, query, 1, fetch, guard_eps, /*unordered=*/true);
    RLR_TRY(ctx_prepare(ix, c, 1, p));
    count_f16_fallbacks(ix, p, 1, false);
    const uint32_t P = need;
    const uint32_t k_cap = result_k_cap(k, P, diversify != 0);
    const HybridWs sizes(nullptr, nullptr, ix->q_pitch, P, n_lex_bound, k_cap);
    RLR_HIP(c->d_pool.reserve(sizes.d.floats()));
    RLR_TRY(reserve_list(c, P));
    RLR_TRY(pin_reserve(c, sizes.h.bytes));
    t->ws = HybridWs(c->d_pool.get(), c->h_pin.get(), ix->q_pitch, P, n_lex_bound, k_cap);
    const HybridWs &ws = t->ws;
    t->n = n;
    t->need = need;
    t->fetch = fetch;
    t->k = k;
    t->k_cap = k_cap;
    t->lambda = lambda;
    t->w_e = w_embedding;
    t->w_l = w_lexical;
    t->diversify = diversify;
    t->timed = ix->profiling;
    stage_queries(ix, c, query, 1, ws.h_q);
    StreamDrain drain{s};
    RLR_HIP(stage_queries_for_scans(ix, c, ws.h_q, static_cast<size_t>(ix->q_pitch) * sizeof(float), s));
    uint64_t *d_meta = c->d_out.get() + fetch;
    // the scan first; then whatever the caller runs beside it (the BM25 chain on its own stream: about as long as scan +
    // select + re-score + sort, so it must not wait for the host to have launched those -- it used to start 39 us behind the
    // scan and was the critical path by as much); then the four launches that wait for the scan anyway
    RLR_HIP(enqueue_query_scan(ix, c, 0, t->timed));
    if (behind_scan) {
        LexSink sink; // (pairs that stay on the device fill every slot)
        sink.d_header = ws.hdr;
        sink.d_rows = ws.lrow;
        sink.d_scores = ws.lscore(n_lex_bound);
        sink.n_bound = n_lex_bound;
        sink.n_index_rows = n;
        RLR_TRY(behind_scan(behind_scan_arg, &sink));
    }
    RLR_HIP(enqueue_query_rest(ix, c, 0, p, c->d_out.get(), d_meta, t->timed));
    if (t->timed) RLR_HIP(hipEventRecord(c->bev[0], s));
    drain.armed = false;
    *out = t.release();
    return RLR_OK;
}

// always consumes the ticket
static int32_t hybrid_finish_impl(HybridTicket *ticket, const HybridLexSrc &src, uint64_t *rows_out, float *cos_out,
                                  float *score_out, float *lex_out, uint32_t *n_out, int32_t *fallback)
{
    std::unique_ptr<HybridTicket> t(ticket);
    rlr_index *ix = t->ix;
    Ctx *c = t->lease.c;
    hipStream_t s = c->stream;
    *n_out = 0;
    *fallback = 0;
    StreamDrain drain{s};
    const HybridWs &ws = t->ws;
    const uint32_t n_lex = src.dev ? static_cast<uint32_t>(ws.n_lex_bound) : src.n_host;
    if (n_lex > ws.n_lex_bound || !rows_out || !cos_out || !score_out || !lex_out)
        return set_error(RLR_E_INVALID, "hybrid search: bad arguments");
    const uint32_t P = t->need, k_cap = t->k_cap, n = t->n;
    float *d_lscore = ws.lscore(n_lex);
    uint32_t *h_lex = ws.h_lex, *h_out = ws.h_out;
    h_out[block_done(k_cap)] = kBlockPending; // (the last kernel's last store replaces it: what the wait below polls)
    if (src.dev) { // the BM25 kernels ran beside the scan on their own stream: join, then unpack their result
        RLR_HIP(hipStreamWaitEvent(s, static_cast<hipEvent_t>(src.dev->ready), 0));
        if (!src.dev->unpacked) { // (begin's LexSink: the scoring stream has done it in front of `ready`)
            hipLaunchKernelGGL(lex_unpack_kernel, dim3(1), dim3(1024), 0, s, src.dev->d_packed, src.dev->d_count,
                               std::min(n_lex, src.dev->limit), n, ws.lrow, d_lscore, ws.hdr);
            RLR_HIP(hipGetLastError());
        }
    } else {
        for (uint32_t i = 0; i < n_lex; ++i)
            if (src.h_rows[i] >= n || (i && src.h_rows[i] <= src.h_rows[i - 1]))
                return set_error(RLR_E_INVALID, "lex_rows must be ascending, unique and inside the index");
        h_lex[0] = n_lex;
        h_lex[1] = __builtin_bit_cast(uint32_t, src.max_lex);
        for (uint32_t i = 0; i < n_lex; ++i)
            h_lex[2 + i] = static_cast<uint32_t>(src.h_rows[i]);
        if (n_lex)
            std::memcpy(HybridWs::h_lscore(h_lex, n_lex), src.h_scores, static_cast<size_t>(n_lex) * sizeof(float));
        RLR_HIP(hipMemcpyAsync(ws.hdr, h_lex, HybridWs::lex_copy_bytes(n_lex), hipMemcpyHostToDevice, s));
    }
    RLR_HIP(launch_score_rows(ix->d_rows.get(), ix->pitch16, ix->dim, ix->dtype, c->d_query.get(), ws.lrow, n_lex, ws.lcos, s,
                              src.dev ? &ws.hdr->n_lex : nullptr, n));
    const bool pool_emits = !t->diversify; // (without diversification the blend kernel emits by itself)
    hipLaunchKernelGGL(hybrid_pool_kernel, dim3(1), dim3(1024), 0, s, c->d_out.get(), t->fetch, t->need, n, t->w_e, t->w_l, ws.lrow,
                       d_lscore, ws.lcos, ws.hdr, ws.cand, c->d_list.get(), ws.comb, ws.cos, ws.lexv, ws.info, k_cap,
                       pool_emits ? h_out : static_cast<uint32_t *>(nullptr));
    RLR_HIP(hipGetLastError());
    if (t->diversify) {
        RLR_HIP(launch_gram_rows(ix->d_rows.get(), ix->pitch16, ix->dim, ix->dtype, c->d_list.get(), P, ws.gram, 1, s));
        const MmrEmit emit = mmr_emit(c->d_list.get(), ws.comb, ws.cos, ws.lexv, ws.info, k_cap, h_out);
        RLR_HIP(launch_mmr_greedy(ws.gram, ws.comb, P, t->k, t->lambda, ws.order, ws.mmr, ws.nsel, ws.info, 1, s, &emit));
    }
    if (t->timed) RLR_HIP(hipEventRecord(c->bev[1], s));
    if (t->timed) {
        drain.armed = false;
        RLR_HIP(hipStreamSynchronize(s)); // (the events are read below)
    } else {
        RLR_TRY(wait_block(h_out, k_cap, s, &c->wait_ema)); // (a failure leaves the drain guard armed)
        drain.armed = false;
    }
    RLR_TRY(check_hist_assert(c));
    c->hist_dirty = false;
    (void)note_search(ix, c, 1, 0, 0, t->timed, /*mmr_chain=*/true);
    *fallback = static_cast<int32_t>(read_block(h_out, k_cap, rows_out, cos_out, score_out, lex_out, n_out));
    return RLR_OK;
}

void launch_lex_unpack(const uint64_t *d_packed, const uint32_t *d_count, uint32_t limit, const LexSink &sink, void *stream)
{
    // (tried: the event recorded by this launch itself, hipExtLaunchKernelGGL's stop event, instead of a marker packet behind
    // it -- the join on the search's stream resumed 3 us earlier under the profiler, nothing measurable without it)
    hipLaunchKernelGGL(lex_unpack_kernel, dim3(1), dim3(1024), 0, static_cast<hipStream_t>(stream), d_packed, d_count, limit,
                       sink.n_index_rows, sink.d_rows, sink.d_scores, static_cast<HybridLexHeader *>(sink.d_header));
}

int32_t search_hybrid_begin(rlr_index *ix, const float *query, uint32_t need, uint32_t k, float lambda, int32_t diversify,
                            float w_embedding, float w_lexical, uint32_t n_lex_bound, float guard_eps, HybridTicket **ticket,
                            int32_t *fallback, int32_t (*behind_scan)(void *, const LexSink *), void *behind_scan_arg)
{
    return hybrid_begin_impl(ix, query, need, k, lambda, diversify, w_embedding, w_lexical, n_lex_bound, guard_eps, ticket,
                             fallback, behind_scan, behind_scan_arg);
}

int32_t search_hybrid_finish(HybridTicket *ticket, const LexPending *lex, uint64_t *rows_out, float *cos_out, float *score_out,
                             float *lex_out, uint32_t *n_out, int32_t *fallback)
{
    HybridLexSrc src;
    if (lex && lex->limit)
        src.dev = lex; // else: no lexical pair at all -- the blend degenerates to w_e * cos + w_l * 0
    return hybrid_finish_impl(ticket, src, rows_out, cos_out, score_out, lex_out, n_out, fallback);
}

void search_hybrid_abort(HybridTicket *ticket)
{
    if (!ticket)
        return;
    (void)hipStreamSynchronize(ticket->lease.c->stream);
    delete ticket;
}

void launch_lex_unpack_batch(const uint64_t *d_sel, uint32_t sel_stride, const uint32_t *d_count, uint32_t count_stride,
                             uint32_t nq, uint32_t limit, const LexBatchSink &sink, void *stream)
{
    hipLaunchKernelGGL(lex_unpack_batch_kernel, dim3(nq), dim3(1024), 0, static_cast<hipStream_t>(stream), d_sel, sel_stride,
                       d_count, count_stride, limit, sink.n_index_rows, sink.bound, sink.d_rows, sink.d_scores,
                       static_cast<HybridLexHeader *>(sink.d_headers));
}

int32_t search_hybrid_batch(rlr_index *ix, const float *queries, uint32_t nq, uint32_t need_in, uint32_t k, float lambda,
                            int32_t diversify, float w_embedding, float w_lexical, uint32_t n_lex_bound,
                            int32_t (*lex_launch)(void *, const LexBatchSink *, void **ready), void *lex_arg, uint64_t *rows_out,
                            float *cos_out, float *score_out, float *lex_out, uint32_t *n_out, uint32_t *status)
{
    RLR_TRY(check_handle(ix));
    const uint32_t n = static_cast<uint32_t>(ix->n_rows);
    const uint32_t need = std::min<uint32_t>(n, need_in);
    if (nq == 0 || n == 0 || need == 0 || need > kPoolMax || n_lex_bound == 0 || n_lex_bound > kHybridLexMax || !lex_launch ||
        !queries || !rows_out || !cos_out || !score_out || !lex_out || !n_out || !status || !(w_embedding > 0.0f) ||
        !std::isfinite(w_embedding) || !std::isfinite(w_lexical))
        return set_error(RLR_E_INVALID, "batched hybrid search: arguments outside the fused kernels");
    const uint32_t fetch = static_cast<uint32_t>(std::min<uint64_t>(n, static_cast<uint64_t>(need) + kHybridFetchMargin));
    if (fetch + n_lex_bound > kHybridSlots)
        return set_error(RLR_E_INVALID, "batched hybrid search: %u fetched + %u lexical rows exceed the blend's slots", fetch, n_lex_bound);
    RLR_TRY(use_device(ix));
    CtxLease lease(ix);
    RLR_TRY(ctx_acquire(ix, &lease.c));
    Ctx *c = lease.c;
    hipStream_t s = c->stream;
    const uint32_t P = need, B = n_lex_bound;
    const uint32_t k_cap = result_k_cap(k, P, diversify != 0);
    const uint64_t Q = nq;
    RLR_HIP(c->d_pool.reserve(HybridBatchWs(nullptr, ix, Q, fetch, P, B, diversify != 0).d.floats()));
    const HybridBatchWs ws(c->d_pool.get(), ix, Q, fetch, P, B, diversify != 0);
    // whatever goes wrong from here on: the BM25 chain (another stream, writing into this workspace) and this stream must
    // be drained before the context goes back
    StreamDrain drain{s};
    // 1. the BM25 chain on the lexical index' stream, into this workspace
    LexBatchSink sink;
    sink.d_rows = ws.lrow;
    sink.d_scores = ws.lscore;
    sink.d_headers = ws.hdr;
    sink.bound = B;
    sink.n_index_rows = n;
    void *ready = nullptr;
    RLR_TRY(lex_launch(lex_arg, &sink, &ready));
    drain.also = static_cast<hipEvent_t>(ready);
    // 2. beside it: the fetch of every query, the batched top-k (GEMM / shared scan / per-query pipeline as the planner picks);
    //    its overflow handling needs the host, hence the first synchronisation
    SearchPlan p;
    const uint64_t *h = nullptr;
    RLR_TRY(run_search(ix, c, queries, nq, fetch, -1.0f, nullptr, &p, &h));
    if (!h || p.k != fetch)
        return set_error(RLR_E_INTERNAL, "batched hybrid search: the cosine batch produced no result");
    // (the fetch goes through the host on purpose: run_search's single-query pipelines -- the planner's choice for batches
    // too small for a shared pass -- write their results straight into pinned host memory, not into c->d_out, so the host
    // copy is the one place every path leaves them; Q x fetch x 8 bytes each way)
    std::vector<uint64_t> fetched(h, h + Q * fetch); // (the pinned buffer is re-laid out below)
    RLR_TRY(pin_reserve(c, HybridBatchPin(nullptr, ix, Q, fetch, P).h.bytes));
    const HybridBatchPin pin(c->h_pin.get(), ix, Q, fetch, P);
    const size_t b_packed = Q * fetch * sizeof(uint64_t), b_q = Q * ix->q_pitch * sizeof(float);
    std::memcpy(pin.packed, fetched.data(), b_packed);
    pad_queries(ix, queries, nq, pin.q);
    RLR_HIP(hipMemcpyAsync(ws.packed, pin.packed, b_packed, hipMemcpyHostToDevice, s));
    RLR_HIP(hipMemcpyAsync(ws.q, pin.q, b_q, hipMemcpyHostToDevice, s));
    // 3. join the BM25 chain; exact cosines of the lexical rows, blend, order, cut -- one workgroup per query
    RLR_HIP(hipStreamWaitEvent(s, static_cast<hipEvent_t>(ready), 0));
    RLR_HIP(launch_score_rows_batch(ix->d_rows.get(), ix->pitch16, ix->dim, ix->dtype, ws.q, ix->q_pitch, nq, ws.lrow, B, ws.lcos,
                                    reinterpret_cast<const uint32_t *>(ws.hdr), 2, n, s));
    const HybridBatchRes &d = ws.res, &r = pin.res;
    hipLaunchKernelGGL(hybrid_pool_batch_kernel, dim3(nq), dim3(1024), 0, s, ws.packed, fetch, P, n, w_embedding, w_lexical, B,
                       ws.lrow, ws.lscore, ws.lcos, ws.hdr, ws.cand, d.list, d.comb, d.cos, d.lexv, d.info, d.sizes);
    RLR_HIP(hipGetLastError());
    // 4. MMR over every pool at once
    if (diversify) {
        RLR_HIP(launch_gram_rows(ix->d_rows.get(), ix->pitch16, ix->dim, ix->dtype, d.list, P, ws.gram, nq, s));
        RLR_HIP(launch_mmr_greedy(ws.gram, d.comb, P, k, lambda, d.order, d.mmr, d.nsel, d.sizes, nq, s));
    }
    RLR_HIP(hipMemcpyAsync(r.list, d.list, HybridBatchRes::words(Q, P) * 4, hipMemcpyDeviceToHost, s));
    RLR_HIP(hipStreamSynchronize(s));
    drain.armed = false;
    for (uint32_t q = 0; q < nq; ++q) {
        status[q] = r.info[2 * q + 1];
        n_out[q] = 0;
        if (status[q])
            continue;
        const size_t base = static_cast<size_t>(q) * P, ob = static_cast<size_t>(q) * k_cap;
        const uint32_t cnt = std::min<uint32_t>(diversify ? r.nsel[q] : r.info[2 * q], k_cap);
        for (uint32_t i = 0; i < cnt; ++i) {
            const size_t o = base + (diversify ? r.order[base + i] : i);
            rows_out[ob + i] = r.list[o];
            cos_out[ob + i] = r.cos[o];
            score_out[ob + i] = r.comb[o];
            lex_out[ob + i] = r.lexv[o];
        }
        n_out[q] = cnt;
    }
    return RLR_OK;
}

} // namespace rlr

extern "C" {

int32_t rlr_search_hybrid(rlr_index *ix, const float *query, uint32_t need, uint32_t k, float lambda, int32_t diversify,
                          float w_embedding, float w_lexical, const uint64_t *lex_rows, const float *lex_scores, uint32_t n_lex,
                          float max_lex, float guard_eps, uint64_t *rows_out, float *cos_out, float *score_out, float *lex_out,
                          uint32_t *n_out, int32_t *fallback)
{
    RLR_TRY(check_handle(ix));
    if (!n_out || !fallback)
        return set_error(RLR_E_INVALID, "n_out / fallback is null");
    *n_out = 0;
    *fallback = 0;
    if (ix->n_rows == 0 || need == 0)
        return RLR_OK;
    if (!query || !rows_out || !cos_out || !score_out || !lex_out || (n_lex && (!lex_rows || !lex_scores)))
        return set_error(RLR_E_INVALID, "null argument");
    rlr::HybridTicket *t = nullptr;
    RLR_TRY(rlr::hybrid_begin_impl(ix, query, need, k, lambda, diversify, w_embedding, w_lexical, n_lex, guard_eps, &t, fallback));
    if (*fallback)
        return RLR_OK;
    HybridLexSrc src;
    src.h_rows = lex_rows;
    src.h_scores = lex_scores;
    src.n_host = n_lex;
    src.max_lex = max_lex;
    return rlr::hybrid_finish_impl(t, src, rows_out, cos_out, score_out, lex_out, n_out, fallback);
}

// Batched MMR over P-strided pools.  The pool rows either live in the index (pool_rows != null:
// gathered to f32 here) or are already in device memory as n_queries x P x dim f32 values
// (d_values != null: the sharded path, after the winner-row exchange).
// d_matrix != null: pool_rows are slots of that matrix (n_matrix raw rows in the index' own dtype and pitch, e.g. the
// receive buffer of the cross-shard winner-row exchange) instead of rows of the index.
static int32_t mmr_batch_impl(rlr_index *ix, const uint64_t *pool_rows, const float *d_values, const float *pool_scores,
                              const uint32_t *pool_sizes, uint32_t n_queries, uint32_t P, uint32_t k, float lambda,
                              uint32_t *order_out, float *mmr_out, uint32_t *n_out, const void *d_matrix = nullptr,
                              uint64_t n_matrix = 0)
{
    RLR_TRY(check_handle(ix));
    if (n_queries == 0)
        return RLR_OK;
    if ((!pool_rows && !d_values) || !pool_scores || !pool_sizes || !order_out || !n_out)
        return set_error(RLR_E_INVALID, "null argument");
    if (P == 0) {
        for (uint32_t q = 0; q < n_queries; ++q)
            n_out[q] = 0;
        return RLR_OK;
    }
    if (P > 1024)
        return set_error(RLR_E_INVALID, "batched MMR supports pools of at most 1024 candidates (got %u)", P);
    RLR_TRY(use_device(ix));
    CtxLease lease(ix);
    RLR_TRY(ctx_acquire(ix, &lease.c));
    Ctx *c = lease.c;
    hipStream_t s = c->stream;
    // queries per pass: the workspace (gram m x P x P + scores / order / mmr) is capped at ~3 GB.  All queries of a
    // pass run their greedy chains concurrently, one wavefront each, so the more queries per pass the better the
    // chip is filled: at 64 per pass (the first version) 1024 pools took 16 rounds of gather + Gram + greedy + sync.
    const uint64_t per_query = static_cast<uint64_t>(P) * P + 3ull * P + 2;
    const uint32_t QC = static_cast<uint32_t>(std::max<uint64_t>(64, std::min<uint64_t>(4096, (3ull << 30) / 4 / std::max<uint64_t>(per_query, 1))));
    std::vector<uint64_t> rows_chunk;
    for (uint32_t q0 = 0; q0 < n_queries; q0 += QC) {
        const uint32_t m = std::min(QC, n_queries - q0);
        const uint32_t n_list = m * P;
        for (uint32_t q = 0; q < m; ++q)
            if (pool_sizes[q0 + q] > P)
                return set_error(RLR_E_INVALID, "pool_sizes[%u] = %u exceeds P = %u", q0 + q, pool_sizes[q0 + q], P);
        RLR_TRY(pin_reserve(c, MmrStaging(nullptr, m, P).h.bytes));
        if (pool_rows) {
            // unused slots (j >= pool_sizes[q]) gather row 0: never read by the greedy kernel
            bool all_full = true;
            for (uint32_t q = 0; q < m && all_full; ++q)
                all_full = pool_sizes[q0 + q] == P;
            const uint64_t *src_rows = pool_rows + static_cast<size_t>(q0) * P;
            if (!all_full) { // (full pools are taken as they stand: no 8 n_list-byte fill + copy in front of every batch)
                rows_chunk.assign(n_list, 0);
                for (uint32_t q = 0; q < m; ++q)
                    std::memcpy(rows_chunk.data() + static_cast<size_t>(q) * P, pool_rows + static_cast<size_t>(q0 + q) * P,
                                pool_sizes[q0 + q] * sizeof(uint64_t));
                src_rows = rows_chunk.data();
            }
            RLR_TRY(upload_list(ix, c, src_rows, n_list, d_matrix ? n_matrix : ~0ull));
        }
        RLR_HIP(c->d_pool.reserve(MmrWs(nullptr, m, P).d.floats()));
        const MmrWs ws(c->d_pool.get(), m, P);
        const MmrStaging h(c->h_pin.get(), m, P);
        std::memcpy(h.scores, pool_scores + static_cast<size_t>(q0) * P, static_cast<size_t>(n_list) * sizeof(float));
        std::memcpy(h.sizes, pool_sizes + q0, m * sizeof(uint32_t));
        RLR_HIP(hipMemcpyAsync(ws.scores, h.scores, static_cast<size_t>(n_list) * sizeof(float), hipMemcpyHostToDevice, s));
        RLR_HIP(hipMemcpyAsync(ws.sizes, h.sizes, m * sizeof(uint32_t), hipMemcpyHostToDevice, s));
        const bool timed = ix->profiling;
        if (timed) RLR_HIP(hipEventRecord(c->ev[0], s));
        if (pool_rows) // the Gram kernel reads the index rows through the list: no gathered copy
            RLR_HIP(launch_gram_rows(d_matrix ? d_matrix : ix->d_rows.get(), ix->pitch16, ix->dim, ix->dtype, c->d_list.get(), P, ws.gram, m, s));
        else
            RLR_HIP(launch_gram(d_values + static_cast<size_t>(q0) * P * ix->dim, P, ix->dim, ws.gram, m, s));
        RLR_HIP(launch_mmr_greedy(ws.gram, ws.scores, P, k, lambda, ws.res.order, ws.res.mmr, ws.res.n, ws.sizes, m, s));
        if (timed) RLR_HIP(hipEventRecord(c->ev[1], s));
        RLR_HIP(hipMemcpyAsync(h.res.order, ws.res.order, MmrResults::words(m, P) * 4, hipMemcpyDeviceToHost, s));
        RLR_HIP(hipStreamSynchronize(s));
        if (timed)
            note_mmr(ix, c, m);
        for (uint32_t q = 0; q < m; ++q) {
            const uint32_t ns = h.res.n[q];
            n_out[q0 + q] = ns;
            std::memcpy(order_out + static_cast<size_t>(q0 + q) * P, h.res.order + static_cast<size_t>(q) * P, ns * sizeof(uint32_t));
            if (mmr_out)
                std::memcpy(mmr_out + static_cast<size_t>(q0 + q) * P, h.res.mmr + static_cast<size_t>(q) * P, ns * sizeof(float));
        }
    }
    return RLR_OK;
}

int32_t rlr_mmr_select_batch(rlr_index *ix, const uint64_t *pool_rows, const float *pool_scores,
                             const uint32_t *pool_sizes, uint32_t n_queries, uint32_t P, uint32_t k, float lambda,
                             uint32_t *order_out, float *mmr_out, uint32_t *n_out)
{
    if (n_queries && !pool_rows)
        return set_error(RLR_E_INVALID, "null argument");
    return mmr_batch_impl(ix, pool_rows, nullptr, pool_scores, pool_sizes, n_queries, P, k, lambda, order_out, mmr_out, n_out);
}

int32_t rlr_mmr_select_values(rlr_index *ix, const void *d_values, const float *pool_scores, const uint32_t *pool_sizes,
                              uint32_t n_queries, uint32_t P, uint32_t k, float lambda, uint32_t *order_out,
                              float *mmr_out, uint32_t *n_out)
{
    if (n_queries && !d_values)
        return set_error(RLR_E_INVALID, "null argument");
    return mmr_batch_impl(ix, nullptr, static_cast<const float *>(d_values), pool_scores, pool_sizes, n_queries, P, k, lambda,
                          order_out, mmr_out, n_out);
}

int32_t rlr_mmr_select_staged(rlr_index *ix, const void *d_staged, uint64_t n_staged, const uint64_t *pool_slots,
                              const float *pool_scores, const uint32_t *pool_sizes, uint32_t n_queries, uint32_t P, uint32_t k,
                              float lambda, uint32_t *order_out, float *mmr_out, uint32_t *n_out)
{
    if (n_queries && (!d_staged || !pool_slots || n_staged == 0))
        return set_error(RLR_E_INVALID, "null argument");
    // one large pool: the single-pool kernels (up to 4096).  P is only the stride, which one pool does not use, so a
    // small pool in a wide slot list goes the same way
    if (n_queries == 1 && pool_sizes && (pool_sizes[0] > 1024 || P > 1024)) {
        if (pool_sizes[0] > P)
            return set_error(RLR_E_INVALID, "pool_sizes[0] = %u exceeds P = %u", pool_sizes[0], P);
        return mmr_single_impl(ix, pool_slots, pool_scores, pool_sizes[0], k, lambda, order_out, mmr_out, n_out, d_staged,
                               n_staged);
    }
    return mmr_batch_impl(ix, pool_slots, nullptr, pool_scores, pool_sizes, n_queries, P, k, lambda, order_out, mmr_out, n_out,
                          d_staged, n_staged);
}

} // extern "C"

namespace rlr {
// rlr_score_rows for nq queries with a list each: queries, lists and counts go up in one copy, launch_score_rows_batch
// scores every list (the reference-order dot product of rlr_score_rows per pair), one copy back, one synchronisation.
int32_t score_rows_batch(rlr_index *ix, const float *queries, uint32_t nq, const uint64_t *rows, const uint32_t *counts,
                         uint32_t stride, float *cos_out)
{
    RLR_TRY(check_handle(ix));
    if (nq == 0 || stride == 0)
        return RLR_OK;
    if (!queries || !rows || !counts || !cos_out)
        return set_error(RLR_E_INVALID, "null argument");
    RLR_TRY(use_device(ix));
    CtxLease lease(ix);
    RLR_TRY(ctx_acquire(ix, &lease.c));
    Ctx *c = lease.c;
    // [queries nq x q_pitch | lists nq x stride | counts nq | cosines nq x stride], 32-bit words, on both sides
    const size_t w_q = static_cast<size_t>(nq) * ix->q_pitch, w_list = static_cast<size_t>(nq) * stride;
    const size_t w_in = w_q + w_list + nq, w_all = w_in + w_list;
    RLR_TRY(pin_reserve(c, w_all * 4));
    RLR_HIP(c->d_pool.reserve(w_all));
    float *h_q = static_cast<float *>(c->h_pin.get());
    uint32_t *h_list = reinterpret_cast<uint32_t *>(h_q + w_q), *h_cnt = h_list + w_list;
    pad_queries(ix, queries, nq, h_q);
    for (uint32_t q = 0; q < nq; ++q) {
        if (counts[q] > stride)
            return set_error(RLR_E_INVALID, "list %u holds %u rows, the stride is %u", q, counts[q], stride);
        h_cnt[q] = counts[q];
        for (uint32_t i = 0; i < stride; ++i) {
            const uint64_t r = i < counts[q] ? rows[static_cast<size_t>(q) * stride + i] : 0;
            if (r >= ix->n_rows)
                return set_error(RLR_E_RANGE, "row %llu out of range (%llu rows)", static_cast<unsigned long long>(r),
                                 static_cast<unsigned long long>(ix->n_rows));
            h_list[static_cast<size_t>(q) * stride + i] = static_cast<uint32_t>(r);
        }
    }
    float *d_q = c->d_pool.get();
    const uint32_t *d_list = reinterpret_cast<const uint32_t *>(d_q + w_q), *d_cnt = d_list + w_list;
    float *d_cos = d_q + w_in;
    RLR_HIP(hipMemcpyAsync(d_q, h_q, w_in * 4, hipMemcpyHostToDevice, c->stream));
    RLR_HIP(launch_score_rows_batch(ix->d_rows.get(), ix->pitch16, ix->dim, ix->dtype, d_q, ix->q_pitch, nq, d_list, stride, d_cos, d_cnt, 1,
                                    static_cast<uint32_t>(ix->n_rows), c->stream));
    float *h_cos = reinterpret_cast<float *>(h_cnt + nq);
    RLR_HIP(hipMemcpyAsync(h_cos, d_cos, w_list * 4, hipMemcpyDeviceToHost, c->stream));
    RLR_HIP(hipStreamSynchronize(c->stream));
    for (uint32_t q = 0; q < nq; ++q)
        std::memcpy(cos_out + static_cast<size_t>(q) * stride, h_cos + static_cast<size_t>(q) * stride, counts[q] * sizeof(float));
    return RLR_OK;
}
} // namespace rlr
