// range.hip -- the tail of a range search (include/rlr_gpu.h, "Range search"): every allowed row whose reference-order
// score is at or above a threshold tau, and how many there are, from the nominated scores the scan left.
//
// With a = nominated score, e = reference-order score, |a - e| <= eps, and two floats lo <= tau - 2 eps, hi >= tau + 2 eps
// (range_bounds, kernels.h; DESIGN.md "Range search" has the argument):
//   e >= tau  =>  a >= tau - eps >= lo : every hit is a candidate
//   a >= hi   =>  e >= tau             : a sure hit (count-only mode counts it without a re-score)
//   a <  lo   =>  e <  tau             : a sure miss
//   clear      the two state words.
//   collect    each workgroup owns one contiguous chunk of rows and walks it in tiles of kRangeTile rows; the candidates
//              of a tile (never more than the tile has rows: the LDS list cannot overflow, however dense the hits) are
//              re-scored in reference order (staged_dot.h), membership is decided on the exact score, the hits take their
//              slots by ONE atomic per tile.  n_hits counts every hit, beyond the key capacity too.
//   finish     one workgroup: up to kRangeFinishMax keys ordered and written to the pinned block with the counts and the
//              completion word; with more hits, or in count-only mode, the counts alone.
// An order between workgroups comes from the order of launches on one stream, never from a flag (the rule of tail.hip).
// Keys are unique per row, so the emitted order does not depend on which workgroup wrote first.
#include "../../include/rlr_gpu.h"
#include "common.h"
#include "kernels.h"
#include "sort_emit.h"
#include "staged_dot.h"

#include <algorithm>

namespace rlr {

namespace {

constexpr uint32_t kRangeBlock = 256;
constexpr uint32_t kRangeTile = 512; // rows of one tile = entries of the workgroup's candidate list
// the tile's two lists and five counters, behind the staging area of group_shape (at most 56 KB): under 64 KB together
constexpr size_t kRangeListBytes = kRangeTile * (sizeof(uint64_t) + sizeof(uint32_t)) + 8 * sizeof(uint32_t);
static_assert(56 * 1024 + kRangeListBytes <= 64 * 1024, "LDS of range_collect_kernel");

struct RangeDev {
    const float *scores;
    uint32_t n;
    float tau, lo, hi;
    uint32_t hit_cap, out_keys;
    RangeState *st;
    const float4 *rows;
    uint32_t pitch16, dim;
    const float *query;
    uint64_t *hits;
    uint64_t *out;
    uint64_t *meta;
    uint32_t *ctx_hist;
    uint32_t cpb;
    uint32_t lists_off; // bytes of the staging area (a multiple of 16): where the tile's lists begin in LDS
};

__global__ __launch_bounds__(64) void range_clear_kernel(RangeDev a)
{
    if (threadIdx.x == 0) {
        a.st->n_hits = 0;
        a.st->n_valid = 0;
    }
}

template <bool F16>
__global__ __launch_bounds__(kRangeBlock) void range_collect_kernel(RangeDev a)
{
    // All LDS is dynamic: statics would precede the staging area unpadded and take its 16-byte alignment (the products are
    // written and read as float4).  Layout: query | cpb rows of products | hit keys | candidate rows | five counters.
    extern __shared__ __attribute__((aligned(16))) float s_mem[];
    uint64_t *s_key = reinterpret_cast<uint64_t *>(reinterpret_cast<char *>(s_mem) + a.lists_off);
    uint32_t *s_row = reinterpret_cast<uint32_t *>(s_key + kRangeTile);
    uint32_t &s_cnt = s_row[kRangeTile], &s_hcnt = s_row[kRangeTile + 1], &s_base = s_row[kRangeTile + 2];
    uint32_t &s_valid = s_row[kRangeTile + 3], &s_sure = s_row[kRangeTile + 4];
    const uint32_t tid = threadIdx.x;
    if (tid == 0) {
        s_valid = 0;
        s_sure = 0;
    }
    const uint64_t chunk = (static_cast<uint64_t>(a.n) + gridDim.x - 1) / gridDim.x;
    const uint64_t r_lo = min(blockIdx.x * chunk, static_cast<uint64_t>(a.n)), r_hi = min(r_lo + chunk, static_cast<uint64_t>(a.n));
    const bool count_only = a.hit_cap == 0;
    const uint32_t q_floats = (a.dim + 7) & ~7u;
    float *s_q = s_mem;
    float *s_p = s_mem + q_floats;
    uint32_t valid = 0, sure = 0;
    bool staged = false;
    for (uint64_t t0 = r_lo; t0 < r_hi; t0 += kRangeTile) { // (uniform)
        __syncthreads(); // the previous tile's lists and products have been read
        if (tid == 0) {
            s_cnt = 0;
            s_hcnt = 0;
        }
        __syncthreads();
        const uint64_t t1 = min(t0 + kRangeTile, r_hi);
        for (uint64_t r = t0 + tid; r < t1; r += kRangeBlock) {
            const float s = a.scores[r];
            if (score_key(s) == 0u)
                continue; // masked, or a NaN nomination: not counted, the host compares n_valid with the allowed rows
            valid++;
            if (count_only && s >= a.hi) {
                sure++;
                continue;
            }
            if (!(s < a.lo)) // (a bound that is no number takes every row)
                s_row[atomicAdd(&s_cnt, 1u)] = static_cast<uint32_t>(r); // at most t1 - t0 <= kRangeTile entries
        }
        __syncthreads();
        const uint32_t found = s_cnt;
        if (found == 0)
            continue; // (uniform)
        if (!staged) {
            for (uint32_t i = tid; i < q_floats; i += kRangeBlock)
                s_q[i] = i < a.dim ? a.query[i] : 0.0f;
            staged = true;
            __syncthreads();
        }
        for (uint32_t g0 = 0; g0 < found; g0 += a.cpb) {
            const uint32_t c = min(a.cpb, found - g0);
            if (g0)
                __syncthreads(); // the chains of the previous group have left s_p
            const float e = staged_reference_dot<F16, kRangeBlock>(a.rows, a.pitch16, a.dim, s_q, s_p, s_row + g0, c, tid);
            if (tid < c && e >= a.tau) // membership on the exact score; a NaN is never a hit
                s_key[atomicAdd(&s_hcnt, 1u)] = pack_result(e, s_row[g0 + tid]);
        }
        __syncthreads();
        const uint32_t hits = s_hcnt;
        if (hits == 0)
            continue; // (uniform)
        if (tid == 0)
            s_base = atomicAdd(&a.st->n_hits, hits);
        __syncthreads();
        const uint32_t base = s_base;
        for (uint32_t i = tid; i < hits; i += kRangeBlock)
            if (base + i < a.hit_cap) // (n_hits <= n < 2^32: the sum cannot wrap)
                a.hits[base + i] = s_key[i];
    }
    if (valid)
        atomicAdd(&s_valid, valid);
    if (sure)
        atomicAdd(&s_sure, sure);
    __syncthreads();
    if (tid == 0) {
        if (s_valid)
            atomicAdd(&a.st->n_valid, s_valid);
        if (s_sure)
            atomicAdd(&a.st->n_hits, s_sure);
    }
}

__global__ __launch_bounds__(1024) void range_finish_kernel(RangeDev a)
{
    __shared__ uint64_t s[kRangeFinishMax];
    __shared__ uint32_t s_hist[2048]; // (sort_emit_rows' select paths; not reached with k = out_keys >= n_hits)
    __shared__ uint32_t s_chk;
    const uint32_t tid = threadIdx.x;
    for (uint32_t i = tid; i < kHistBins; i += 1024)
        a.ctx_hist[i] = 0; // the scan counted its scores into the context's digit-1 histogram; nothing here read it
    const uint32_t n_hits = a.st->n_hits, n_valid = a.st->n_valid;
    if (tid == 0)
        s_chk = 0;
    __syncthreads();
    const bool emit = a.hit_cap != 0 && n_hits != 0 && n_hits <= a.out_keys; // (uniform)
    if (emit) {
        sort_emit_rows(a.hits, n_hits, a.out_keys, a.out, a.out_keys, false, s, s_hist, &s_chk);
    } else {
        for (uint32_t i = tid; i < a.out_keys; i += 1024)
            a.out[i] = 0ull; // (whatever an earlier call left there would enter the host's checksum)
    }
    if (tid == 0) {
        const uint64_t info = static_cast<uint64_t>(n_hits) | (static_cast<uint64_t>(n_valid) << 32);
        a.out[a.out_keys] = info;
        if (info)
            atomicAdd(&s_chk, result_chk_term(info, a.out_keys));
    }
    __threadfence_system();
    __syncthreads();
    if (tid == 0)
        *a.meta = (static_cast<uint64_t>(s_chk) << 32) | (emit ? 1u : 0u); // (low half 0 / 1: never the pending pattern)
}

} // namespace

hipError_t launch_range_tail(const RangeArgs &a, hipStream_t s)
{
    uint32_t cpb;
    size_t staging;
    if (a.n == 0 || !(a.tau == a.tau) || a.out_keys > kRangeFinishMax || a.out_keys > a.hit_cap ||
        !group_shape(a.pitch16, a.dim, a.dtype, &cpb, &staging))
        return hipErrorInvalidValue;
    RangeDev d;
    d.scores = a.scores;
    d.n = a.n;
    d.tau = a.tau;
    range_bounds(a.tau, a.two_eps, &d.lo, &d.hi);
    d.hit_cap = a.hit_cap;
    d.out_keys = a.out_keys;
    d.st = a.st;
    d.rows = static_cast<const float4 *>(a.rows);
    d.pitch16 = a.pitch16;
    d.dim = a.dim;
    d.query = a.query;
    d.hits = a.hits;
    d.out = a.out;
    d.meta = a.meta;
    d.ctx_hist = a.ctx_hist;
    d.cpb = cpb;
    d.lists_off = static_cast<uint32_t>(staging);
    const size_t lds = staging + kRangeListBytes;
    // the workgroups re-score what they find: a small corpus is spread over more (partly idle) workgroups than its scores
    // need, as in group.hip's collect
    const uint32_t max_blocks = static_cast<uint32_t>(std::max(a.n_cu, 1)) * 8;
    const uint64_t n64 = a.n; // (n + 31 may pass 2^32)
    const uint32_t collect_blocks = static_cast<uint32_t>(std::max<uint64_t>(1, std::min<uint64_t>((n64 + 31) / 32, max_blocks)));
    hipLaunchKernelGGL(range_clear_kernel, dim3(1), dim3(64), 0, s, d);
    if (a.dtype == RLR_F16)
        hipLaunchKernelGGL(range_collect_kernel<true>, dim3(collect_blocks), dim3(kRangeBlock), lds, s, d);
    else
        hipLaunchKernelGGL(range_collect_kernel<false>, dim3(collect_blocks), dim3(kRangeBlock), lds, s, d);
    hipLaunchKernelGGL(range_finish_kernel, dim3(1), dim3(1024), 0, s, d);
    return hipGetLastError();
}

// ---- the batched tail (rlr_search_range_batch; kernels.h "RangeBatchArgs") -------------------------------------------
// Several queries behind ONE pass over the rows.  Per query the arithmetic and the decisions are those of the kernels
// above: candidates a >= lo, membership on the reference-order score e >= tau, sure hits a >= hi counted without a re-score
// in count-only mode, n_hits counting every hit.  Two sources of candidates:
//   shared scan   range_collect_multi_kernel: range_collect_kernel with blockIdx.y selecting the query (its score array,
//                 bounds, state and key buffer); then range_batch_finish_kernel only orders and emits.
//   GEMM          the nomination GEMM appended every (a, row) with a >= lo[q] to query q's list; one workgroup per query of
//                 range_batch_finish_kernel walks the list in chunks of kRangeChunk: mask test, sure hits, the rest into an
//                 LDS row list that is re-scored in groups of cpb with the query staged once.  The hit counters live in
//                 LDS: no state words in global memory, nothing to clear.
// Per-query key capacity: kRangeFinishMax when rows are wanted (lower than the single path's min(cap, RLR_RANGE_DEVICE_MAX):
// with more hits the query is handed back).  The finish's LDS is used twice -- staging area + row list while it re-scores,
// the sort's key array + histogram afterwards -- and stays under 64 KB either way.
namespace {

constexpr uint32_t kRangeChunk = 1024; // candidates of the GEMM's list looked at per round = entries of the finish's row list
constexpr size_t kRangeSortBytes = kRangeFinishMax * sizeof(uint64_t) + 2048 * sizeof(uint32_t);
static_assert(56 * 1024 + kRangeChunk * sizeof(uint32_t) + 64 <= 64 * 1024, "LDS of range_batch_finish_kernel (re-score)");
static_assert(kRangeSortBytes + 64 <= 64 * 1024, "LDS of range_batch_finish_kernel (sort)");

struct RangeBatchDev {
    uint32_t n;
    const float *scores;
    size_t score_stride;
    const uint64_t *cand;
    uint32_t cand_stride;
    const SelectState *bst;
    const uint64_t *mask;
    const float *bounds;
    uint32_t cap, hit_keys, out_keys;
    RangeState *st;
    const float4 *rows;
    uint32_t pitch16, dim;
    const float *queries;
    uint32_t q_pitch;
    uint64_t *hits;
    uint64_t *out;
    uint32_t cpb;
    uint32_t lists_off;
};

template <bool F16>
__global__ __launch_bounds__(kRangeBlock) void range_collect_multi_kernel(RangeBatchDev a)
{
    // range_collect_kernel, query blockIdx.y: same LDS layout, same tile walk
    extern __shared__ __attribute__((aligned(16))) float s_mem[];
    uint64_t *s_key = reinterpret_cast<uint64_t *>(reinterpret_cast<char *>(s_mem) + a.lists_off);
    uint32_t *s_row = reinterpret_cast<uint32_t *>(s_key + kRangeTile);
    uint32_t &s_cnt = s_row[kRangeTile], &s_hcnt = s_row[kRangeTile + 1], &s_base = s_row[kRangeTile + 2];
    uint32_t &s_valid = s_row[kRangeTile + 3], &s_sure = s_row[kRangeTile + 4];
    const uint32_t tid = threadIdx.x, q = blockIdx.y;
    const float *scores = a.scores + static_cast<size_t>(q) * a.score_stride;
    const float *query = a.queries + static_cast<size_t>(q) * a.q_pitch;
    const float tau = a.bounds[3 * q], lo = a.bounds[3 * q + 1], hi = a.bounds[3 * q + 2];
    RangeState *st = a.st + q;
    uint64_t *hits = a.hits + static_cast<size_t>(q) * a.hit_keys;
    if (tid == 0) {
        s_valid = 0;
        s_sure = 0;
    }
    const uint64_t chunk = (static_cast<uint64_t>(a.n) + gridDim.x - 1) / gridDim.x;
    const uint64_t r_lo = min(blockIdx.x * chunk, static_cast<uint64_t>(a.n)), r_hi = min(r_lo + chunk, static_cast<uint64_t>(a.n));
    const bool count_only = a.cap == 0;
    const uint32_t q_floats = (a.dim + 7) & ~7u;
    float *s_q = s_mem;
    float *s_p = s_mem + q_floats;
    uint32_t valid = 0, sure = 0;
    bool staged = false;
    for (uint64_t t0 = r_lo; t0 < r_hi; t0 += kRangeTile) { // (uniform)
        __syncthreads(); // the previous tile's lists and products have been read
        if (tid == 0) {
            s_cnt = 0;
            s_hcnt = 0;
        }
        __syncthreads();
        const uint64_t t1 = min(t0 + kRangeTile, r_hi);
        for (uint64_t r = t0 + tid; r < t1; r += kRangeBlock) {
            const float s = scores[r];
            if (score_key(s) == 0u)
                continue; // masked, or a NaN nomination: not counted, the host compares n_valid with the allowed rows
            valid++;
            if (count_only && s >= hi) {
                sure++;
                continue;
            }
            if (!(s < lo)) // (a bound that is no number takes every row)
                s_row[atomicAdd(&s_cnt, 1u)] = static_cast<uint32_t>(r); // at most t1 - t0 <= kRangeTile entries
        }
        __syncthreads();
        const uint32_t found = s_cnt;
        if (found == 0)
            continue; // (uniform)
        if (!staged) {
            for (uint32_t i = tid; i < q_floats; i += kRangeBlock)
                s_q[i] = i < a.dim ? query[i] : 0.0f;
            staged = true;
            __syncthreads();
        }
        for (uint32_t g0 = 0; g0 < found; g0 += a.cpb) {
            const uint32_t c = min(a.cpb, found - g0);
            if (g0)
                __syncthreads(); // the chains of the previous group have left s_p
            const float e = staged_reference_dot<F16, kRangeBlock>(a.rows, a.pitch16, a.dim, s_q, s_p, s_row + g0, c, tid);
            if (tid < c && e >= tau) // membership on the exact score; a NaN is never a hit
                s_key[atomicAdd(&s_hcnt, 1u)] = pack_result(e, s_row[g0 + tid]);
        }
        __syncthreads();
        const uint32_t n_new = s_hcnt;
        if (n_new == 0)
            continue; // (uniform)
        if (tid == 0)
            s_base = atomicAdd(&st->n_hits, n_new);
        __syncthreads();
        const uint32_t base = s_base;
        for (uint32_t i = tid; i < n_new; i += kRangeBlock)
            if (base + i < a.hit_keys) // (n_hits <= n < 2^32: the sum cannot wrap; hit_keys = 0 in count-only mode)
                hits[base + i] = s_key[i];
    }
    if (valid)
        atomicAdd(&s_valid, valid);
    if (sure)
        atomicAdd(&s_sure, sure);
    __syncthreads();
    if (tid == 0) {
        if (s_valid)
            atomicAdd(&st->n_valid, s_valid);
        if (s_sure)
            atomicAdd(&st->n_hits, s_sure);
    }
}

template <bool F16>
__global__ __launch_bounds__(1024) void range_batch_finish_kernel(RangeBatchDev a)
{
    // Dynamic LDS, used twice: query | cpb rows of products | kRangeChunk candidate rows, then keys | histogram of the sort.
    extern __shared__ __attribute__((aligned(16))) float s_mem[];
    __shared__ uint32_t s_cnt, s_hcnt, s_sure, s_chk;
    const uint32_t tid = threadIdx.x, q = blockIdx.x;
    const float tau = a.bounds[3 * q], hi = a.bounds[3 * q + 2];
    uint64_t *hits = a.hits + static_cast<size_t>(q) * a.hit_keys;
    uint64_t *o = a.out + static_cast<size_t>(q) * (a.out_keys + 2);
    const bool count_only = a.cap == 0;
    uint32_t n_hits = 0, n_valid = 0, status = kRangeBatchDecided;
    if (tid == 0) {
        s_hcnt = 0;
        s_sure = 0;
        s_chk = 0;
    }
    if (a.cand) {
        const uint32_t n_raw = a.bst[q].n_cand; // (uniform from here on)
        if ((n_raw & 0x80000000u) != 0 || n_raw > a.cand_stride) {
            status = kRangeBatchCandidates;
        } else {
            const uint64_t *cand = a.cand + static_cast<size_t>(q) * a.cand_stride;
            const float *query = a.queries + static_cast<size_t>(q) * a.q_pitch;
            const uint32_t q_floats = (a.dim + 7) & ~7u;
            float *s_q = s_mem;
            float *s_p = s_mem + q_floats;
            uint32_t *s_row = reinterpret_cast<uint32_t *>(reinterpret_cast<char *>(s_mem) + a.lists_off);
            for (uint32_t i = tid; i < q_floats; i += 1024)
                s_q[i] = i < a.dim ? query[i] : 0.0f;
            for (uint32_t c0 = 0; c0 < n_raw; c0 += kRangeChunk) {
                __syncthreads(); // the previous round's list and products have been read (first round: the query is staged)
                if (tid == 0)
                    s_cnt = 0;
                __syncthreads();
                if (c0 + tid < n_raw) {
                    const uint64_t w = cand[c0 + tid];
                    const uint32_t row = 0xFFFFFFFFu - static_cast<uint32_t>(w);
                    const bool allowed = row < a.n && (!a.mask || ((a.mask[row >> 6] >> (row & 63)) & 1ull));
                    if (allowed) {
                        if (count_only && key_score(static_cast<uint32_t>(w >> 32)) >= hi)
                            atomicAdd(&s_sure, 1u); // a >= hi => e >= tau
                        else
                            s_row[atomicAdd(&s_cnt, 1u)] = row; // at most kRangeChunk entries
                    }
                }
                __syncthreads();
                const uint32_t found = s_cnt;
                for (uint32_t g0 = 0; g0 < found; g0 += a.cpb) {
                    const uint32_t c = min(a.cpb, found - g0);
                    if (g0)
                        __syncthreads(); // the chains of the previous group have left s_p
                    const float e = staged_reference_dot<F16, 1024>(a.rows, a.pitch16, a.dim, s_q, s_p, s_row + g0, c, tid);
                    if (tid < c && e >= tau) { // membership on the exact score; a NaN is never a hit
                        const uint32_t slot = atomicAdd(&s_hcnt, 1u);
                        if (slot < a.hit_keys)
                            hits[slot] = pack_result(e, s_row[g0 + tid]);
                    }
                }
            }
            __syncthreads();
            n_hits = s_hcnt + s_sure;
        }
    } else {
        n_hits = a.st[q].n_hits;
        n_valid = a.st[q].n_valid;
    }
    if (status == kRangeBatchDecided && !count_only && n_hits > a.hit_keys)
        status = kRangeBatchHits;
    __syncthreads(); // the re-score is done with the LDS the sort takes; this workgroup's keys are in `hits`
    if (status == kRangeBatchDecided && !count_only && n_hits != 0) {
        uint64_t *s = reinterpret_cast<uint64_t *>(s_mem);
        uint32_t *s_hist = reinterpret_cast<uint32_t *>(s + kRangeFinishMax);
        sort_emit_rows(hits, n_hits, a.hit_keys, o, a.out_keys, false, s, s_hist, &s_chk);
    } else {
        for (uint32_t i = tid; i < a.out_keys; i += 1024)
            o[i] = 0ull;
    }
    if (tid == 0) {
        o[a.out_keys] = static_cast<uint64_t>(n_hits) | (static_cast<uint64_t>(n_valid) << 32);
        o[a.out_keys + 1] = status;
    }
}

} // namespace

hipError_t launch_range_batch_tail(const RangeBatchArgs &a, hipStream_t s)
{
    uint32_t cpb;
    size_t staging;
    if (a.n == 0 || a.n_queries == 0 || (a.scores != nullptr) == (a.cand != nullptr) || !a.bounds || !a.out ||
        (a.scores && (!a.st || a.score_stride < a.n || a.n_queries > 65535)) || (a.cand && !a.bst) || (a.cap && !a.hits) ||
        !group_shape(a.pitch16, a.dim, a.dtype, &cpb, &staging))
        return hipErrorInvalidValue;
    RangeBatchDev d;
    d.n = a.n;
    d.scores = a.scores;
    d.score_stride = a.score_stride;
    d.cand = a.cand;
    d.cand_stride = a.cand_stride;
    d.bst = a.bst;
    d.mask = a.mask;
    d.bounds = a.bounds;
    d.cap = a.cap;
    d.hit_keys = a.cap ? kRangeFinishMax : 0;
    d.out_keys = std::min<uint32_t>(a.cap, kRangeFinishMax);
    d.st = a.st;
    d.rows = static_cast<const float4 *>(a.rows);
    d.pitch16 = a.pitch16;
    d.dim = a.dim;
    d.queries = a.queries;
    d.q_pitch = a.q_pitch;
    d.hits = a.hits;
    d.out = a.out;
    d.cpb = cpb;
    d.lists_off = static_cast<uint32_t>(staging);
    if (a.scores) {
        const size_t lds = staging + kRangeListBytes;
        const uint32_t max_blocks = static_cast<uint32_t>(std::max(a.n_cu, 1)) * 8;
        const uint64_t n64 = a.n;
        const uint32_t collect_blocks = static_cast<uint32_t>(std::max<uint64_t>(1, std::min<uint64_t>((n64 + 31) / 32, max_blocks)));
        if (a.dtype == RLR_F16)
            hipLaunchKernelGGL(range_collect_multi_kernel<true>, dim3(collect_blocks, a.n_queries), dim3(kRangeBlock), lds, s, d);
        else
            hipLaunchKernelGGL(range_collect_multi_kernel<false>, dim3(collect_blocks, a.n_queries), dim3(kRangeBlock), lds, s, d);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess)
            return e;
    }
    const size_t lds = std::max(staging + kRangeChunk * sizeof(uint32_t), kRangeSortBytes);
    if (a.dtype == RLR_F16)
        hipLaunchKernelGGL(range_batch_finish_kernel<true>, dim3(a.n_queries), dim3(1024), lds, s, d);
    else
        hipLaunchKernelGGL(range_batch_finish_kernel<false>, dim3(a.n_queries), dim3(1024), lds, s, d);
    return hipGetLastError();
}

} // namespace rlr
