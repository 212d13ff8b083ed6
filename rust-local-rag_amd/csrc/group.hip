// group.hip -- the tail of a grouped search (include/rlr_gpu.h, "Grouped top-k"): the best k rows with at most per_doc
// of any one document, selected on the device from the nominated scores the scan left and the document column.
//
// With a = nominated score, e = reference-order score, |a - e| <= eps (DESIGN.md "Grouped top-k" has the proof):
//   rounds     j = 1..per_doc, one launch each: every document's j-th largest packed key (score key << 32 | ~row) by a
//              64-bit atomicMax into an open-addressing table keyed by document id, over the keys strictly below its
//              (j-1)-th.  Integer maxima: the table is the same whatever order the workgroups run in.  Runs of equal ids
//              inside a wave are reduced first, so a document of consecutive rows costs one atomic per wave.
//   heads      t_g (the per_doc-th value, 0 for a smaller group) per row, and the digit-1 histogram of the heads: the
//              rows among their group's best per_doc by nomination (every untagged row is one).
//   refine     digit 2 of the heads inside the bin of the k-th head.
//   collect    rows with a >= max(t_g, U) - 2 eps, U = the floor of the k-th head's 22-bit bin; each workgroup re-scores
//              what it found in reference order (staged_dot.h).
//   finish     one workgroup: exact order, rank inside the group, accept below per_doc, emit the first k.
// A capped hybrid search (rlr_search_capped) runs the same launches with k = the pool size and capped_finish_kernel as its
// finish: the candidates united with the lexical rows, blended, ranked inside the group in COMBINED order (below).
// A batched grouped search (rlr_search_topk_grouped_batch) runs ONE set of these launches for a chunk of up to 8 queries
// behind a shared scan, with one key table for the chunk and a value plane per query ("the batched tail", below); a
// batched capped search (rlr_search_capped_batch) runs that tail with capped_finish_multi_kernel as its finish.
// An order between workgroups comes from the order of launches on one stream, never from a flag (the rule of tail.hip);
// inside a launch the table is only touched by atomics, between launches by plain loads.
#include "../../include/rlr_gpu.h"
#include "common.h"
#include "kernels.h"
#include "select_dev.h"
#include "sort_emit.h"
#include "staged_dot.h"

#include <algorithm>

namespace rlr {

namespace {

constexpr uint32_t kGroupBlock = 256;
constexpr uint32_t kGroupLocalCap = 1024; // candidates one workgroup keeps for its own re-score
constexpr uint32_t kNoSlot = 0xFFFFFFFFu;
static_assert(kGroupBlock == kSelThreads, "find_rank_bin is written for 256 threads");

struct GroupDev {
    const float *scores;
    const uint32_t *docs;
    uint32_t n, k, per_doc;
    float two_eps;
    uint32_t *tab_keys;
    uint64_t *tab_vals;
    uint32_t tab_bits;
    uint64_t *tg;
    uint32_t *hist;
    GroupState *st;
    const float4 *rows;
    uint32_t pitch16, dim;
    const float *query;
    uint64_t *cand;
    uint32_t *cand_doc;
    uint64_t *out;
    uint64_t *meta;
    uint32_t *ctx_hist;
    uint32_t cpb;
};

__device__ inline uint32_t group_hash(uint32_t id, uint32_t bits)
{
    return (id * 0x9E3779B1u) >> (32u - bits); // multiplicative: ids that differ in any bit spread over the table
}

// the slot of `id`, claimed if it has none yet (launches that insert touch the keys with atomics only)
__device__ inline uint32_t group_insert(uint32_t *keys, uint32_t bits, uint32_t id)
{
    const uint32_t mask = (1u << bits) - 1u;
    uint32_t h = group_hash(id, bits);
    for (uint32_t probes = 0; probes <= mask; ++probes) {
        // (an agent-scope load first: the rows of a large document find its slot without a read-modify-write on one address)
        uint32_t old = __hip_atomic_load(&keys[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (old == RLR_DOC_NONE)
            old = atomicCAS(&keys[h], RLR_DOC_NONE, id);
        if (old == RLR_DOC_NONE || old == id)
            return h;
        h = (h + 1u) & mask;
    }
    return kNoSlot;
}

// the slot of `id` in a table no launch is inserting into, kNoSlot if it has none
__device__ inline uint32_t group_find(const uint32_t *keys, uint32_t bits, uint32_t id)
{
    const uint32_t mask = (1u << bits) - 1u;
    uint32_t h = group_hash(id, bits);
    for (uint32_t probes = 0; probes <= mask; ++probes) {
        const uint32_t key = keys[h];
        if (key == id)
            return h;
        if (key == RLR_DOC_NONE)
            return kNoSlot;
        h = (h + 1u) & mask;
    }
    return kNoSlot;
}

__device__ inline uint64_t shfl_up_u64(uint64_t v, uint32_t d)
{
    const uint32_t lo = __shfl_up(static_cast<uint32_t>(v), d, 64), hi = __shfl_up(static_cast<uint32_t>(v >> 32), d, 64);
    return (static_cast<uint64_t>(hi) << 32) | lo;
}

__global__ __launch_bounds__(kGroupBlock) void group_clear_kernel(GroupDev a)
{
    const uint32_t stride = gridDim.x * kGroupBlock, t0 = blockIdx.x * kGroupBlock + threadIdx.x;
    const uint32_t slots = a.docs ? 1u << a.tab_bits : 0u;
    for (uint32_t i = t0; i < slots; i += stride)
        a.tab_keys[i] = RLR_DOC_NONE;
    const uint64_t n_vals = static_cast<uint64_t>(slots) * a.per_doc;
    for (uint64_t i = t0; i < n_vals; i += stride)
        a.tab_vals[i] = 0ull;
    for (uint32_t i = t0; i < 2u * kHistBins; i += stride)
        a.hist[i] = 0u;
    if (t0 == 0) {
        a.st->n_cand = 0;
        a.st->n_valid = 0;
        a.st->flags = 0;
        a.st->u_bits = 0;
    }
}

// Round j (0-based): tab_vals[slot][j] = the largest packed key of the slot's document below tab_vals[slot][j - 1].
// A wave takes 64 consecutive rows at a time; lanes of one run of equal ids combine their keys by a segmented maximum
// and the last lane of the run issues the one atomic.  (A lane that meets an equal id beyond its run's start only adds
// keys of the same document: still that document's maximum.)
template <bool FIRST>
__global__ __launch_bounds__(kGroupBlock) void group_round_kernel(GroupDev a, uint32_t j)
{
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t n_words = a.n / 64 + ((a.n & 63) != 0 ? 1u : 0u);
    const uint32_t waves = gridDim.x * (kGroupBlock / 64);
    for (uint64_t w = blockIdx.x * (kGroupBlock / 64) + (threadIdx.x >> 6); w < n_words; w += waves) { // (wave-uniform)
        const uint64_t row = w * 64 + lane;
        const bool in = row < a.n;
        const uint32_t id = in ? a.docs[row] : RLR_DOC_NONE;
        const uint32_t key = in ? score_key(a.scores[row]) : 0u;
        const bool act = id != RLR_DOC_NONE && key != 0u;
        uint64_t v = act ? (static_cast<uint64_t>(key) << 32) | (0xFFFFFFFFu - static_cast<uint32_t>(row)) : 0ull;
        uint32_t slot = kNoSlot;
        if (!FIRST && act) {
            slot = group_find(a.tab_keys, a.tab_bits, id);
            const uint64_t bound = slot != kNoSlot ? a.tab_vals[static_cast<uint64_t>(slot) * a.per_doc + j - 1] : 0ull;
            if (!(v < bound))
                v = 0ull; // taken by an earlier round (or the document has no slot: the table overflowed, flagged)
        }
#pragma unroll
        for (uint32_t d = 1; d < 64; d <<= 1) {
            const uint64_t ov = shfl_up_u64(v, d);
            const uint32_t oid = __shfl_up(id, d, 64);
            if (lane >= d && oid == id && ov > v)
                v = ov;
        }
        const uint32_t next_id = __shfl_down(id, 1, 64);
        const bool tail = lane == 63 || next_id != id;
        if (tail && id != RLR_DOC_NONE && v != 0ull) {
            if (FIRST)
                slot = group_insert(a.tab_keys, a.tab_bits, id);
            else if (slot == kNoSlot)
                slot = group_find(a.tab_keys, a.tab_bits, id);
            if (slot != kNoSlot) {
                // The value only grows during a launch, so whatever a load sees is a lower bound of the final maximum: a
                // key at or below it cannot be that maximum and needs no atomic.  (200 000 scattered rows of ONE document
                // were 200 000 read-modify-writes on one address, 2 ms a round, before this test.)
                unsigned long long *p = reinterpret_cast<unsigned long long *>(&a.tab_vals[static_cast<uint64_t>(slot) * a.per_doc + j]);
                if (__hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < v)
                    atomicMax(p, static_cast<unsigned long long>(v));
            } else {
                atomicOr(&a.st->flags, 2u);
            }
        }
    }
}

// is the row a head -- among its group's best per_doc by nomination?  (tg = 0 for a smaller group and an untagged row)
__device__ inline bool group_is_head(uint32_t key, uint32_t row, uint64_t tg)
{
    return key != 0u && ((static_cast<uint64_t>(key) << 32) | (0xFFFFFFFFu - row)) >= tg;
}

// (the bodies of heads, refine and collect are shared with the batched tail below: one GroupDev per query)
__device__ inline void group_heads_body(const GroupDev &a)
{
    __shared__ uint32_t s_hist[kHistBins];
    __shared__ uint32_t s_valid;
    for (uint32_t i = threadIdx.x; i < kHistBins; i += kGroupBlock)
        s_hist[i] = 0;
    if (threadIdx.x == 0)
        s_valid = 0;
    __syncthreads();
    const uint32_t stride = gridDim.x * kGroupBlock;
    uint32_t valid = 0;
    for (uint64_t r = blockIdx.x * kGroupBlock + threadIdx.x; r < a.n; r += stride) { // (64-bit: r + stride may pass 2^32)
        const uint32_t row = static_cast<uint32_t>(r);
        const uint32_t key = score_key(a.scores[row]);
        uint64_t tg = 0ull;
        if (key != 0u && a.docs) {
            const uint32_t id = a.docs[row];
            if (id != RLR_DOC_NONE) {
                const uint32_t slot = group_find(a.tab_keys, a.tab_bits, id);
                // (no slot: the table overflowed, the flag is set and the host discards this pass)
                tg = slot != kNoSlot ? a.tab_vals[static_cast<uint64_t>(slot) * a.per_doc + a.per_doc - 1] : 0ull;
            }
        }
        a.tg[row] = tg;
        if (key != 0u) {
            valid++;
            if (group_is_head(key, row, tg))
                atomicAdd(&s_hist[key >> 21], 1u);
        }
    }
    if (valid)
        atomicAdd(&s_valid, valid);
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < kHistBins; i += kGroupBlock) {
        const uint32_t c = s_hist[i];
        if (c)
            atomicAdd(&a.hist[i], c);
    }
    if (threadIdx.x == 0 && s_valid)
        atomicAdd(&a.st->n_valid, s_valid);
}

__global__ __launch_bounds__(kGroupBlock) void group_heads_kernel(GroupDev a)
{
    group_heads_body(a);
}

// digit 2 (key bits 20..10) of the heads whose digit 1 is the k-th head's
__device__ inline void group_refine_body(const GroupDev &a)
{
    __shared__ uint32_t s_hist[kHistBins];
    uint32_t bin1, k2, in_bin;
    find_rank_bin(a.hist, a.k, &bin1, &k2, &in_bin);
    if (in_bin == 0)
        return; // fewer than k heads: no threshold (uniform)
    for (uint32_t i = threadIdx.x; i < kHistBins; i += kGroupBlock)
        s_hist[i] = 0;
    __syncthreads();
    const uint32_t stride = gridDim.x * kGroupBlock;
    for (uint64_t r = blockIdx.x * kGroupBlock + threadIdx.x; r < a.n; r += stride) {
        const uint32_t row = static_cast<uint32_t>(r);
        const uint32_t key = score_key(a.scores[row]);
        if ((key >> 21) == bin1 && group_is_head(key, row, a.tg[row]))
            atomicAdd(&s_hist[(key >> 10) & (kHistBins - 1)], 1u);
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < kHistBins; i += kGroupBlock) {
        const uint32_t c = s_hist[i];
        if (c)
            atomicAdd(&a.hist[kHistBins + i], c);
    }
}

__global__ __launch_bounds__(kGroupBlock) void group_refine_kernel(GroupDev a)
{
    group_refine_body(a);
}

template <bool F16>
__device__ inline void group_collect_body(const GroupDev &a)
{
    extern __shared__ __attribute__((aligned(16))) float s_mem[];
    __shared__ uint32_t s_row[kGroupLocalCap];
    __shared__ uint32_t s_cnt, s_base;
    const uint32_t tid = threadIdx.x;
    // U: the floor of the 22-bit bin of the k-th head, -inf with fewer than k heads
    uint32_t bin1, k2, in_bin, bin2 = 0, r2;
    find_rank_bin(a.hist, a.k, &bin1, &k2, &in_bin);
    __syncthreads(); // (find_rank_bin's LDS words are reused by the second search)
    if (in_bin != 0)
        find_rank_bin(a.hist + kHistBins, k2, &bin2, &r2);
    const uint32_t floor_key = in_bin != 0 ? (bin1 << 21) | (bin2 << 10) : 0u;
    float u = floor_key ? key_score(floor_key) : -__builtin_inff();
    if (!(u == u))
        u = -__builtin_inff(); // (the bin of -inf decodes to a NaN pattern)
    if (tid == 0) {
        s_cnt = 0;
        if (blockIdx.x == 0)
            a.st->u_bits = __builtin_bit_cast(uint32_t, u); // (the capped finish bounds the rows left behind with it)
    }
    __syncthreads();
    const uint64_t chunk = (static_cast<uint64_t>(a.n) + gridDim.x - 1) / gridDim.x;
    const uint64_t lo = min(blockIdx.x * chunk, static_cast<uint64_t>(a.n)), hi = min(lo + chunk, static_cast<uint64_t>(a.n));
    for (uint64_t r = lo + tid; r < hi; r += kGroupBlock) {
        const uint32_t row = static_cast<uint32_t>(r);
        const float s = a.scores[row];
        if (score_key(s) == 0u)
            continue;
        const uint32_t tkey = static_cast<uint32_t>(a.tg[row] >> 32);
        const float t = tkey ? key_score(tkey) : -__builtin_inff();
        const float thr = fmaxf(t, u) - a.two_eps;
        if (!(s < thr)) { // (a band so wide that the threshold is no number takes every row)
            const uint32_t l = atomicAdd(&s_cnt, 1u);
            if (l < kGroupLocalCap)
                s_row[l] = row;
        }
    }
    __syncthreads();
    const uint32_t found = s_cnt;
    if (found == 0)
        return; // (uniform)
    if (tid == 0) {
        s_base = atomicAdd(&a.st->n_cand, found);
        if (found > kGroupLocalCap)
            atomicOr(&a.st->flags, 1u);
    }
    const uint32_t q_floats = (a.dim + 7) & ~7u;
    float *s_q = s_mem;
    float *s_p = s_mem + q_floats;
    for (uint32_t i = tid; i < q_floats; i += kGroupBlock)
        s_q[i] = i < a.dim ? a.query[i] : 0.0f;
    __syncthreads();
    const uint32_t base = s_base;
    const uint32_t cnt = min(found, kGroupLocalCap);
    for (uint32_t g0 = 0; g0 < cnt; g0 += a.cpb) {
        const uint32_t c = min(a.cpb, cnt - g0);
        if (g0)
            __syncthreads(); // the chains of the previous group have left s_p
        const float sc = staged_reference_dot<F16, kGroupBlock>(a.rows, a.pitch16, a.dim, s_q, s_p, s_row + g0, c, tid);
        const uint32_t slot = base + g0 + tid;
        if (tid < c && slot < kGroupCap) {
            const uint32_t row = s_row[g0 + tid];
            a.cand[slot] = pack_result(sc, row);
            a.cand_doc[slot] = a.docs ? a.docs[row] : RLR_DOC_NONE;
        }
    }
}

template <bool F16>
__global__ __launch_bounds__(kGroupBlock) void group_collect_kernel(GroupDev a)
{
    group_collect_body<F16>(a);
}

// The body of a finish, one workgroup of 1024 threads over n_raw <= kGroupCap re-scored candidates: the candidates in exact
// order, each one's rank inside its group, the accepted ones compacted, the first k and their document ids into `out` behind
// them, then the n_valid | n_out << 32 word.  *s_chk and *s_nacc are zero on entry (set before a barrier the caller need
// not add: the first one here follows); *s_chk receives the checksum terms of every word written.
__device__ inline void group_finish_body(const uint64_t *cand, const uint32_t *cand_doc, uint32_t n_raw, uint32_t n_valid, uint32_t k,
                                         uint32_t per_doc, uint64_t *out, uint64_t *s_pk, uint32_t *s_doc, uint32_t *s_acc,
                                         uint32_t *s_outdoc, uint32_t *s_chk, uint32_t *s_nacc)
{
    const uint32_t tid = threadIdx.x;
    for (uint32_t i = tid; i < n_raw; i += 1024) {
        s_pk[i] = cand[i];
        s_doc[i] = cand_doc[i];
    }
    for (uint32_t i = tid; i <= kGroupKMax; i += 1024)
        s_outdoc[i] = 0;
    __syncthreads();
    for (uint32_t i = tid; i < n_raw; i += 1024) {
        const uint64_t mine = s_pk[i];
        const uint32_t d = s_doc[i];
        uint32_t ahead = 0;
        if (d != RLR_DOC_NONE)
            for (uint32_t j = 0; j < n_raw; ++j)
                ahead += (s_pk[j] > mine && s_doc[j] == d) ? 1u : 0u;
        s_acc[i] = ahead < per_doc ? 1u : 0u;
    }
    __syncthreads();
    for (uint32_t i = tid; i < n_raw; i += 1024) {
        if (!s_acc[i])
            continue;
        const uint64_t mine = s_pk[i];
        uint32_t pos = 0;
        for (uint32_t j = 0; j < n_raw; ++j)
            pos += (s_acc[j] && s_pk[j] > mine) ? 1u : 0u;
        atomicAdd(s_nacc, 1u);
        if (pos < k) {
            out[pos] = mine;
            s_outdoc[pos] = s_doc[i];
            atomicAdd(s_chk, result_chk_term(mine, pos));
        }
    }
    __syncthreads();
    const uint32_t n_out = min(*s_nacc, k);
    for (uint32_t i = n_out + tid; i < k; i += 1024)
        out[i] = 0ull;
    const uint32_t doc_words = (k + 1) / 2;
    for (uint32_t w = tid; w < doc_words; w += 1024) {
        const uint64_t word = static_cast<uint64_t>(s_outdoc[2 * w]) | (static_cast<uint64_t>(s_outdoc[2 * w + 1]) << 32);
        out[k + w] = word;
        if (word)
            atomicAdd(s_chk, result_chk_term(word, k + w));
    }
    if (tid == 0) {
        const uint64_t info = static_cast<uint64_t>(n_valid) | (static_cast<uint64_t>(n_out) << 32);
        out[k + doc_words] = info;
        if (info)
            atomicAdd(s_chk, result_chk_term(info, k + doc_words));
    }
}

// One workgroup: group_finish_body over the context's candidates into the pinned block, then the completion word.
__global__ __launch_bounds__(1024) void group_finish_kernel(GroupDev a)
{
    __shared__ uint64_t s_pk[kGroupCap];
    __shared__ uint32_t s_doc[kGroupCap];
    __shared__ uint32_t s_acc[kGroupCap];
    __shared__ uint32_t s_outdoc[kGroupKMax + 1];
    __shared__ uint32_t s_chk, s_nacc;
    const uint32_t tid = threadIdx.x;
    for (uint32_t i = tid; i < kHistBins; i += 1024)
        a.ctx_hist[i] = 0; // the scan counted its scores into the context's digit-1 histogram; nothing here read it
    const uint32_t n_raw = a.st->n_cand, flags = a.st->flags, n_valid = a.st->n_valid;
    if (tid == 0) {
        s_chk = 0;
        s_nacc = 0;
    }
    if (flags != 0 || n_raw > kGroupCap) { // (uniform) the host takes the exact path
        if (tid == 0)
            *a.meta = 0xFFFFFFFFull;
        return;
    }
    group_finish_body(a.cand, a.cand_doc, n_raw, n_valid, a.k, a.per_doc, a.out, s_pk, s_doc, s_acc, s_outdoc, &s_chk, &s_nacc);
    __threadfence_system();
    __syncthreads();
    if (tid == 0)
        *a.meta = (static_cast<uint64_t>(s_chk) << 32) | n_raw; // (n_raw <= kGroupCap: never the pending pattern)
}

// ---- the finish of a capped hybrid search (rlr_search_capped; DESIGN.md "Capped hybrid search") ----------------------
// -0 and +0 combined scores tie: the row decides
__device__ inline uint32_t capped_comb_key(float c)
{
    return score_key(c == 0.0f ? 0.0f : c);
}

// The key of a combined score that no row the collect left behind can exceed, for a group whose per_doc-th nominated value
// is t (-inf: a smaller group, an untagged row).  Such a row has a < fmaxf(t, u) - 2 eps in the collect's own arithmetic and
// |a - e| <= eps, so e < (that threshold) + eps; the sum below is rounded to nearest and then stepped up once, so it is no
// smaller than the real sum, and rounding is monotone: combined(e) <= combined(bound).  0: the threshold is -inf, the
// collect left no row of this group behind.  ~0: the bound is no number -- nothing can be decided against it.
__device__ inline uint32_t capped_bound_key(float t, float u, float two_eps, float eps, float w_e, float w_l)
{
    const float thr = fmaxf(t, u) - two_eps;
    if (thr == -__builtin_inff())
        return 0u;
    float eb = thr + eps;
    if (!(eb == eb))
        return 0xFFFFFFFFu;
    if (eb == 0.0f)
        eb = 0.0f; // (-0 steps up from +0)
    if (eb != __builtin_inff()) {
        const uint32_t b = __builtin_bit_cast(uint32_t, eb);
        eb = __builtin_bit_cast(float, (b & 0x80000000u) ? b - 1u : b + 1u);
    }
    const float t0 = w_e * eb;
    const float t1 = w_l * 0.0f;
    const float cb = t0 + t1;
    return cb == cb ? capped_comb_key(cb) : 0xFFFFFFFFu;
}

// One workgroup in place of group_finish_kernel.  Entries [0, n_raw) are the re-scored grouped candidates, entries
// [n_raw, n_raw + n_lex) the lexical rows no candidate is (a lexical row that is a candidate is blended where it sits:
// once).  combined = w_e * cos + w_l * lexn in the arithmetic of pool_prepare.h; every entry is ranked inside its document
// by (combined, row), entries ranked below per_doc are accepted, the accepted ones are ordered and the first `need` become
// the pool.  LDS: kCappedSlots (= kGroupCap + kCappedLexMax = 4096) entries x 16 B + kCappedLexMax flags = 72 KB.
// status 1: more candidates or lexical rows than that (or the collect / the table overflowed); status 2: the boundary rule
// below cannot decide, or rows that order last (NaN) would be needed to fill the pool.
//
// The boundary rule.  Every row outside the union is non-lexical and bounded by capped_bound_key of its group.  A group is
// closed when per_doc of its entries lie STRICTLY above its bound: whatever it left behind is capped out.  The bound of
// every other group with rows left behind (untagged rows and groups without an entry have t <= u: the bound of u covers
// them) must lie strictly below the need-th accepted entry: the walk ends before it reaches such a row.  If the collect
// left no row behind (n_raw == n_valid) there is nothing to bound.
//
// The body over one query's view (the batched tail runs it once per query of a chunk: capped_finish_multi_kernel): `a` as
// the finish of that query sees it, `c` its lexical pairs, scratch and pool, pool_doc (may be null) the pool's document
// ids in device memory, c.h_side (may be null) the pinned side block.  Returns the status, *n_pool_out the pool size and
// *side_out the checksum of the side block's values, all uniform, behind a barrier.
__device__ inline uint32_t capped_finish_body(const GroupDev &a, const CappedArgs &c, uint32_t *pool_doc, uint32_t *n_pool_out,
                                              uint32_t *side_out)
{
    __shared__ uint64_t s_key[kCappedSlots];
    __shared__ uint32_t s_doc[kCappedSlots];
    __shared__ uint32_t s_acc[kCappedSlots];
    __shared__ uint32_t s_flag[kCappedLexMax]; // lexical pair j is one of the candidates
    __shared__ uint32_t s_nacc, s_nan, s_req, s_tkey, s_status, s_side;
    const uint32_t tid = threadIdx.x;
    const uint32_t n_raw = a.st->n_cand, flags = a.st->flags, n_valid = a.st->n_valid;
    const float u = __builtin_bit_cast(float, a.st->u_bits);
    const uint32_t need = a.k, m = a.per_doc, n_lex = min(c.n_lex, kCappedLexMax);
    float *cc = c.scratch, *ce = c.scratch + kCappedSlots, *cl = c.scratch + 2 * kCappedSlots;
    if (tid == 0) {
        s_nacc = 0;
        s_nan = 0;
        s_req = 0;
        s_tkey = 0;
        s_side = 0;
    }
    const bool capacity = flags != 0 || n_raw > kGroupCap || c.n_lex > kCappedLexMax; // (uniform)
    const bool all_collected = n_raw == n_valid;
    if (!capacity) {
        const uint32_t total = n_raw + n_lex;
        for (uint32_t j = tid; j < n_lex; j += 1024)
            s_flag[j] = 0;
        __syncthreads();
        for (uint32_t i = tid; i < n_raw; i += 1024) {
            const uint64_t p = a.cand[i];
            const uint32_t row = 0xFFFFFFFFu - static_cast<uint32_t>(p);
            const float e = key_score(static_cast<uint32_t>(p >> 32));
            float l = 0.0f;
            uint32_t lo = 0, hi = n_lex;
            while (lo < hi) { // the lexical rows ascend
                const uint32_t mid = (lo + hi) >> 1;
                if (c.lrow[mid] < row)
                    lo = mid + 1;
                else
                    hi = mid;
            }
            if (lo < n_lex && c.lrow[lo] == row) {
                l = c.lscore[lo] / c.max_lex;
                s_flag[lo] = 1;
            }
            const float t0 = c.w_e * e;
            const float t1 = c.w_l * l;
            const float cmb = t0 + t1;
            cc[i] = cmb;
            ce[i] = e;
            cl[i] = l;
            if (cmb == cmb) {
                s_key[i] = (static_cast<uint64_t>(capped_comb_key(cmb)) << 32) | (p & 0xFFFFFFFFull);
            } else { // orders last: only wanted when the numbers run out, and then the exact form answers
                s_key[i] = 0ull;
                s_nan = 1;
            }
            s_doc[i] = a.cand_doc[i];
        }
        __syncthreads();
        for (uint32_t j = tid; j < n_lex; j += 1024) {
            const uint32_t slot = n_raw + j;
            uint64_t key = 0ull;
            uint32_t d = RLR_DOC_NONE;
            if (!s_flag[j]) {
                const uint32_t row = c.lrow[j];
                const float e = c.lcos[j];
                const float l = c.lscore[j] / c.max_lex;
                const float t0 = c.w_e * e;
                const float t1 = c.w_l * l;
                const float cmb = t0 + t1;
                cc[slot] = cmb;
                ce[slot] = e;
                cl[slot] = l;
                if (cmb == cmb) {
                    key = (static_cast<uint64_t>(capped_comb_key(cmb)) << 32) | (0xFFFFFFFFu - row);
                    d = a.docs ? a.docs[row] : RLR_DOC_NONE;
                } else {
                    s_nan = 1;
                }
            }
            s_key[slot] = key;
            s_doc[slot] = d;
        }
        __syncthreads();
        if (tid == 0 && !all_collected) {
            const uint32_t kb = capped_bound_key(-__builtin_inff(), u, a.two_eps, c.eps, c.w_e, c.w_l);
            if (kb != 0u)
                atomicMax(&s_req, kb);
        }
        for (uint32_t i = tid; i < total; i += 1024) {
            const uint64_t mine = s_key[i];
            const uint32_t d = s_doc[i];
            uint32_t ahead = 0;
            if (mine != 0ull && d != RLR_DOC_NONE) {
                uint32_t kb = 0u;
                if (!all_collected) {
                    const uint32_t slot = group_find(a.tab_keys, a.tab_bits, d);
                    const uint32_t tkey =
                        slot != kNoSlot ? static_cast<uint32_t>(a.tab_vals[static_cast<uint64_t>(slot) * m + m - 1] >> 32) : 0u;
                    kb = capped_bound_key(tkey ? key_score(tkey) : -__builtin_inff(), u, a.two_eps, c.eps, c.w_e, c.w_l);
                }
                uint32_t above = 0;
                for (uint32_t j = 0; j < total; ++j) {
                    const uint64_t kj = s_key[j];
                    const bool same = s_doc[j] == d && kj != 0ull;
                    ahead += (same && kj > mine) ? 1u : 0u;
                    above += (same && static_cast<uint32_t>(kj >> 32) > kb) ? 1u : 0u;
                }
                if (kb != 0u && above < m)
                    atomicMax(&s_req, kb); // an open group with rows left behind
            }
            s_acc[i] = (mine != 0ull && ahead < m) ? 1u : 0u;
        }
        __syncthreads();
        for (uint32_t i = tid; i < total; i += 1024) {
            if (!s_acc[i])
                continue;
            const uint64_t mine = s_key[i];
            uint32_t pos = 0;
            for (uint32_t j = 0; j < total; ++j)
                pos += (s_acc[j] && s_key[j] > mine) ? 1u : 0u;
            atomicAdd(&s_nacc, 1u);
            if (pos < need) {
                const uint32_t row = 0xFFFFFFFFu - static_cast<uint32_t>(mine), d = s_doc[i];
                c.list[pos] = row;
                c.comb[pos] = cc[i];
                c.cosv[pos] = ce[i];
                c.lexv[pos] = cl[i];
                if (pool_doc)
                    pool_doc[pos] = d;
                if (c.h_side) {
                    c.h_side[2 + pos] = row;
                    c.h_side[2 + need + pos] = d;
                    atomicAdd(&s_side, result_chk_term(row, 2 + pos) + result_chk_term(d, 2 + need + pos));
                }
                if (pos == need - 1)
                    s_tkey = static_cast<uint32_t>(mine >> 32);
            }
        }
    }
    __syncthreads();
    const uint32_t n_acc = s_nacc, n_pool = min(n_acc, need);
    if (tid == 0) {
        uint32_t status = capacity ? 1u : 0u;
        if (!status && s_req != 0u && !(n_acc >= need && s_tkey > s_req))
            status = 2u; // a row left behind may tie with, or precede, the last entry that counts
        if (!status && n_acc < need && (n_valid < c.n_allowed || s_nan != 0u))
            status = 2u; // the numbers ran out: the rows that order last are wanted
        c.info[0] = status ? 0u : n_pool;
        c.info[1] = status;
        s_status = status;
    }
    for (uint32_t r = n_pool + tid; r < need; r += 1024) { // unused slots: a valid row, never read by the greedy kernel
        c.list[r] = 0;
        c.comb[r] = 0.0f;
        c.cosv[r] = 0.0f;
        c.lexv[r] = 0.0f;
        if (pool_doc)
            pool_doc[r] = RLR_DOC_NONE;
    }
    __threadfence_system();
    __syncthreads();
    *n_pool_out = n_pool;
    *side_out = s_side;
    return s_status;
}

// One workgroup in place of group_finish_kernel: the body over the context's single query, then the pinned side block's
// header and -- without diversification -- the result block.
__global__ __launch_bounds__(1024) void capped_finish_kernel(GroupDev a, CappedArgs c)
{
    const uint32_t tid = threadIdx.x;
    for (uint32_t i = tid; i < kHistBins; i += 1024)
        a.ctx_hist[i] = 0; // the scan counted its scores into the context's digit-1 histogram; nothing here read it
    uint32_t n_pool, s_side;
    const uint32_t status = capped_finish_body(a, c, nullptr, &n_pool, &s_side);
    if (tid == 0) {
        c.h_side[1] = status ? 0u : s_side;
        __threadfence_system();
        c.h_side[0] = status ? 0u : n_pool;
    }
    if (c.h_out)
        hybrid_emit_body(c.list, c.comb, c.cosv, c.lexv, status ? 0u : min(n_pool, c.k_cap), status, c.k_cap, c.h_out);
}

__global__ __launch_bounds__(kGroupBlock) void group_iota_kernel(uint32_t *__restrict__ list, uint32_t n)
{
    for (uint32_t i = blockIdx.x * kGroupBlock + threadIdx.x; i < n; i += gridDim.x * kGroupBlock)
        list[i] = i;
}

// ---- the batched tail (rlr_search_topk_grouped_batch; kernels.h "GroupBatchArgs") -------------------------------------
// A chunk of 2..8 queries behind ONE shared scan and one set of launches: clear, per_doc rounds, heads, refine, collect,
// finish.  Per query the arithmetic and the decisions are those of the kernels above.  The document table is where the
// sharing pays: the allowed rows and the column are the same for every query, so the chunk has ONE key table (inserted
// once, in round 1, from any query's active row) and a value plane per query.  A round reads a wave's document ids once,
// works out the runs of equal ids once, probes the table once per lane and then runs the segmented maximum and the guarded
// atomicMax per query on that query's plane.  A row whose score is NaN for query q (a masked row is NaN for all) has key
// 0 and is skipped for q only.  Heads, refine and collect take their query from blockIdx.y and run the single-query bodies
// over that query's slice (group_view); the finish is one workgroup per query.  The rules of the file hold: the table is
// touched by atomics only inside a launch and by plain loads between launches, no workgroup waits for another, order
// comes from the order of launches on one stream, integer maxima make the table independent of workgroup order.
struct GroupBatchDev {
    uint32_t n_queries;
    const float *scores;
    size_t score_stride;
    const uint32_t *docs;
    uint32_t n, k, per_doc;
    float two_eps;
    uint32_t *tab_keys;
    uint64_t *tab_vals;
    uint32_t tab_bits;
    uint64_t *tg;
    uint32_t *hist;
    GroupState *st;
    const float4 *rows;
    uint32_t pitch16, dim;
    const float *queries;
    uint32_t q_pitch;
    uint64_t *cand;
    uint32_t *cand_doc;
    uint64_t *out;
    uint32_t out_words; // group_batch_words(k)
    uint32_t cpb;
};

// query q's slice of the chunk as the single-query bodies take it (meta / ctx_hist: not used by them)
__device__ inline GroupDev group_view(const GroupBatchDev &a, uint32_t q)
{
    GroupDev d;
    d.scores = a.scores + static_cast<size_t>(q) * a.score_stride;
    d.docs = a.docs;
    d.n = a.n;
    d.k = a.k;
    d.per_doc = a.per_doc;
    d.two_eps = a.two_eps;
    d.tab_keys = a.tab_keys;
    d.tab_vals = a.tab_vals + ((static_cast<uint64_t>(q) << a.tab_bits) * a.per_doc);
    d.tab_bits = a.tab_bits;
    d.tg = a.tg + static_cast<uint64_t>(q) * a.n;
    d.hist = a.hist + static_cast<size_t>(q) * 2u * kHistBins;
    d.st = a.st + q;
    d.rows = a.rows;
    d.pitch16 = a.pitch16;
    d.dim = a.dim;
    d.query = a.queries + static_cast<size_t>(q) * a.q_pitch;
    d.cand = a.cand + static_cast<size_t>(q) * kGroupCap;
    d.cand_doc = a.cand_doc + static_cast<size_t>(q) * kGroupCap;
    d.out = a.out + static_cast<size_t>(q) * a.out_words;
    d.meta = nullptr;
    d.ctx_hist = nullptr;
    d.cpb = a.cpb;
    return d;
}

__global__ __launch_bounds__(kGroupBlock) void group_clear_multi_kernel(GroupBatchDev a)
{
    const uint32_t stride = gridDim.x * kGroupBlock, t0 = blockIdx.x * kGroupBlock + threadIdx.x;
    const uint32_t slots = a.docs ? 1u << a.tab_bits : 0u;
    for (uint32_t i = t0; i < slots; i += stride)
        a.tab_keys[i] = RLR_DOC_NONE;
    const uint64_t n_vals = static_cast<uint64_t>(slots) * a.per_doc * a.n_queries;
    for (uint64_t i = t0; i < n_vals; i += stride)
        a.tab_vals[i] = 0ull;
    for (uint32_t i = t0; i < a.n_queries * 2u * kHistBins; i += stride)
        a.hist[i] = 0u;
    if (t0 < a.n_queries) {
        a.st[t0].n_cand = 0;
        a.st[t0].n_valid = 0;
        a.st[t0].flags = 0;
        a.st[t0].u_bits = 0;
    }
}

// Round j (0-based) for every query of the chunk: plane q's tab_vals[slot][j] = the largest packed key of the slot's
// document below its tab_vals[slot][j - 1], by query q's scores.  group_round_kernel's wave walk; what does not depend on
// the query is done once per wave: the document ids, which lanes below share a lane's id (`same`, bit d for distance d),
// the run's last lane, and the lane's slot (looked up, or claimed in round 1, when the first query needs it).
template <bool FIRST>
__global__ __launch_bounds__(kGroupBlock) void group_round_multi_kernel(GroupBatchDev a, uint32_t j)
{
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t n_words = a.n / 64 + ((a.n & 63) != 0 ? 1u : 0u);
    const uint32_t waves = gridDim.x * (kGroupBlock / 64);
    const uint64_t plane = (1ull << a.tab_bits) * a.per_doc;
    for (uint64_t w = blockIdx.x * (kGroupBlock / 64) + (threadIdx.x >> 6); w < n_words; w += waves) { // (wave-uniform)
        const uint64_t row = w * 64 + lane;
        const bool in = row < a.n;
        const uint32_t id = in ? a.docs[row] : RLR_DOC_NONE;
        uint32_t same = 0;
#pragma unroll
        for (uint32_t d = 1; d < 64; d <<= 1) {
            const uint32_t oid = __shfl_up(id, d, 64);
            if (lane >= d && oid == id)
                same |= d;
        }
        const uint32_t next_id = __shfl_down(id, 1, 64);
        const bool tail = (lane == 63 || next_id != id) && id != RLR_DOC_NONE;
        uint32_t slot = kNoSlot;
        bool probed = false;
        for (uint32_t q = 0; q < a.n_queries; ++q) { // (uniform: every lane takes every shuffle)
            const uint32_t key = in ? score_key(a.scores[static_cast<size_t>(q) * a.score_stride + row]) : 0u;
            const bool act = id != RLR_DOC_NONE && key != 0u;
            uint64_t v = act ? (static_cast<uint64_t>(key) << 32) | (0xFFFFFFFFu - static_cast<uint32_t>(row)) : 0ull;
            uint64_t *vals = a.tab_vals + q * plane;
            if (!FIRST && act) {
                if (!probed) {
                    slot = group_find(a.tab_keys, a.tab_bits, id);
                    probed = true;
                }
                const uint64_t bound = slot != kNoSlot ? vals[static_cast<uint64_t>(slot) * a.per_doc + j - 1] : 0ull;
                if (!(v < bound))
                    v = 0ull; // taken by an earlier round (or the document has no slot: the table overflowed, flagged)
            }
#pragma unroll
            for (uint32_t d = 1; d < 64; d <<= 1) {
                const uint64_t ov = shfl_up_u64(v, d);
                if ((same & d) != 0u && ov > v)
                    v = ov;
            }
            if (tail && v != 0ull) {
                if (!probed) {
                    slot = FIRST ? group_insert(a.tab_keys, a.tab_bits, id) : group_find(a.tab_keys, a.tab_bits, id);
                    probed = true;
                }
                if (slot != kNoSlot) {
                    // (the guard of group_round_kernel: a key at or below what a load sees cannot be the maximum)
                    unsigned long long *p = reinterpret_cast<unsigned long long *>(&vals[static_cast<uint64_t>(slot) * a.per_doc + j]);
                    if (__hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < v)
                        atomicMax(p, static_cast<unsigned long long>(v));
                } else {
                    atomicOr(&a.st[q].flags, 2u);
                }
            }
        }
    }
}

__global__ __launch_bounds__(kGroupBlock) void group_heads_multi_kernel(GroupBatchDev a)
{
    group_heads_body(group_view(a, blockIdx.y));
}

__global__ __launch_bounds__(kGroupBlock) void group_refine_multi_kernel(GroupBatchDev a)
{
    group_refine_body(group_view(a, blockIdx.y));
}

template <bool F16>
__global__ __launch_bounds__(kGroupBlock) void group_collect_multi_kernel(GroupBatchDev a)
{
    group_collect_body<F16>(group_view(a, blockIdx.y));
}

// One workgroup per query: group_finish_body into the query's slice of the device result block, then its status word.
// (c->d_hist is not touched: the shared scans run without a histogram.)
__global__ __launch_bounds__(1024) void group_finish_multi_kernel(GroupBatchDev a)
{
    __shared__ uint64_t s_pk[kGroupCap];
    __shared__ uint32_t s_doc[kGroupCap];
    __shared__ uint32_t s_acc[kGroupCap];
    __shared__ uint32_t s_outdoc[kGroupKMax + 1];
    __shared__ uint32_t s_chk, s_nacc;
    const uint32_t tid = threadIdx.x, q = blockIdx.x;
    const GroupState *st = a.st + q;
    uint64_t *out = a.out + static_cast<size_t>(q) * a.out_words;
    const uint32_t n_raw = st->n_cand, flags = st->flags, n_valid = st->n_valid;
    if (tid == 0) {
        s_chk = 0;
        s_nacc = 0;
    }
    if (flags != 0 || n_raw > kGroupCap) { // (uniform) the host hands the query to the single-query path
        for (uint32_t i = tid; i + 1 < a.out_words; i += 1024)
            out[i] = 0ull;
        if (tid == 0)
            out[a.out_words - 1] = kGroupBatchBack;
        return;
    }
    group_finish_body(a.cand + static_cast<size_t>(q) * kGroupCap, a.cand_doc + static_cast<size_t>(q) * kGroupCap, n_raw, n_valid, a.k,
                      a.per_doc, out, s_pk, s_doc, s_acc, s_outdoc, &s_chk, &s_nacc);
    if (tid == 0)
        out[a.out_words - 1] = n_raw;
}

// The finish of a batched capped search (rlr_search_capped_batch): one workgroup per query, capped_finish_body over the
// query's view -- its candidates, state, t_g slice and value plane as the collect left them (group_view), its lexical
// slice and max_lex, its slice of the scratch and of the pool planes.  Nothing is shared between two workgroups but the
// read-only key table, the column and the per-call scalars.  A non-zero status leaves pool size 0 in info and in sizes:
// the Gram and greedy launches behind it do nothing for that query.  (c->d_hist is not touched: the shared scans run
// without a histogram.)
__global__ __launch_bounds__(1024) void capped_finish_multi_kernel(GroupBatchDev a, CappedBatchArgs b)
{
    const uint32_t q = blockIdx.x, need = a.k;
    const GroupDev v = group_view(a, q);
    CappedArgs c;
    c.w_e = b.w_e;
    c.w_l = b.w_l;
    c.eps = b.eps;
    c.n_allowed = b.n_allowed;
    c.lrow = b.lrow + static_cast<size_t>(q) * b.lex_stride;
    c.lscore = b.lscore + static_cast<size_t>(q) * b.lex_stride;
    c.lcos = b.lcos + static_cast<size_t>(q) * b.lex_stride;
    c.n_lex = b.n_lex[q];
    c.max_lex = b.max_lex[q];
    c.scratch = b.scratch + static_cast<size_t>(q) * 3u * kCappedSlots;
    c.list = b.list + static_cast<size_t>(q) * need;
    c.comb = b.comb + static_cast<size_t>(q) * need;
    c.cosv = b.cosv + static_cast<size_t>(q) * need;
    c.lexv = b.lexv + static_cast<size_t>(q) * need;
    c.info = b.info + 2u * q;
    c.h_side = nullptr;
    c.k_cap = 0;
    c.h_out = nullptr;
    uint32_t n_pool, side;
    const uint32_t status = capped_finish_body(v, c, b.docs + static_cast<size_t>(q) * need, &n_pool, &side);
    if (threadIdx.x == 0)
        b.sizes[q] = status ? 0u : n_pool;
}

} // namespace

// the staging of collect's re-score: the query and cpb rows of products (tail.hip's layout, under what is left of the
// 64 KB beside the local candidate list and the bin search's words); range.hip stages its re-score the same way
bool group_shape(uint32_t pitch16, uint32_t dim, int dtype, uint32_t *cpb_out, size_t *staging_out)
{
    const size_t q_bytes = static_cast<size_t>((dim + 7) & ~7u) * sizeof(float);
    const size_t row_bytes = q_bytes + 16;
    if (pitch16 * (dtype == RLR_F16 ? 8u : 4u) < ((dim + 7) & ~7u))
        return false;
    constexpr size_t budget = 56 * 1024;
    uint32_t cpb = 8;
    while (cpb > 1 && q_bytes + cpb * row_bytes > budget)
        cpb >>= 1;
    if (q_bytes + cpb * row_bytes > budget)
        return false;
    *cpb_out = cpb;
    *staging_out = q_bytes + cpb * row_bytes;
    return true;
}

bool group_fits(uint32_t pitch16, uint32_t dim, int dtype)
{
    uint32_t cpb;
    size_t staging;
    return group_shape(pitch16, dim, dtype, &cpb, &staging);
}

hipError_t launch_group_tail(const GroupArgs &a, hipStream_t s, hipEvent_t after_rounds)
{
    uint32_t cpb;
    size_t staging;
    if (a.n == 0 || a.k == 0 || a.k > kGroupKMax || a.per_doc == 0 || a.per_doc > RLR_MAX_PER_DOCUMENT || a.tab_bits < 1 ||
        a.tab_bits > 31 || !group_shape(a.pitch16, a.dim, a.dtype, &cpb, &staging) || (a.capped && a.capped->n_lex > kCappedLexMax))
        return hipErrorInvalidValue;
    GroupDev d;
    d.scores = a.scores;
    d.docs = a.docs;
    d.n = a.n;
    d.k = a.k;
    d.per_doc = a.per_doc;
    d.two_eps = a.two_eps;
    d.tab_keys = a.tab_keys;
    d.tab_vals = a.tab_vals;
    d.tab_bits = a.tab_bits;
    d.tg = a.tg;
    d.hist = a.hist;
    d.st = a.st;
    d.rows = static_cast<const float4 *>(a.rows);
    d.pitch16 = a.pitch16;
    d.dim = a.dim;
    d.query = a.query;
    d.cand = a.cand;
    d.cand_doc = a.cand_doc;
    d.out = a.out;
    d.meta = a.meta;
    d.ctx_hist = a.ctx_hist;
    d.cpb = cpb;
    const uint32_t max_blocks = static_cast<uint32_t>(std::max(a.n_cu, 1)) * 8;
    const uint32_t row_blocks = std::max<uint32_t>(1, std::min<uint32_t>((a.n + kGroupBlock - 1) / kGroupBlock, max_blocks));
    const uint64_t slots = a.docs ? 1ull << a.tab_bits : 0ull;
    const uint32_t clear_blocks = static_cast<uint32_t>(
        std::max<uint64_t>(2u * kHistBins / kGroupBlock, std::min<uint64_t>((slots * a.per_doc + kGroupBlock - 1) / kGroupBlock, max_blocks)));
    hipLaunchKernelGGL(group_clear_kernel, dim3(clear_blocks), dim3(kGroupBlock), 0, s, d);
    if (a.docs) {
        hipLaunchKernelGGL(group_round_kernel<true>, dim3(row_blocks), dim3(kGroupBlock), 0, s, d, 0u);
        for (uint32_t j = 1; j < a.per_doc; ++j)
            hipLaunchKernelGGL(group_round_kernel<false>, dim3(row_blocks), dim3(kGroupBlock), 0, s, d, j);
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess)
        return e;
    if (after_rounds && (e = hipEventRecord(after_rounds, s)) != hipSuccess)
        return e;
    hipLaunchKernelGGL(group_heads_kernel, dim3(row_blocks), dim3(kGroupBlock), 0, s, d);
    hipLaunchKernelGGL(group_refine_kernel, dim3(row_blocks), dim3(kGroupBlock), 0, s, d);
    // the workgroups re-score what they find, cpb candidates at a time: a small corpus is spread over more (partly idle)
    // workgroups than its scores need, as in tail.hip's stage 1
    const uint32_t collect_blocks =
        std::max<uint32_t>(1, std::min<uint32_t>(std::max<uint32_t>(row_blocks, (a.n + 31) / 32), max_blocks));
    if (a.dtype == RLR_F16)
        hipLaunchKernelGGL(group_collect_kernel<true>, dim3(collect_blocks), dim3(kGroupBlock), staging, s, d);
    else
        hipLaunchKernelGGL(group_collect_kernel<false>, dim3(collect_blocks), dim3(kGroupBlock), staging, s, d);
    if (a.capped)
        hipLaunchKernelGGL(capped_finish_kernel, dim3(1), dim3(1024), 0, s, d, *a.capped);
    else
        hipLaunchKernelGGL(group_finish_kernel, dim3(1), dim3(1024), 0, s, d);
    return hipGetLastError();
}

hipError_t launch_group_batch_tail(const GroupBatchArgs &a, hipStream_t s)
{
    uint32_t cpb;
    size_t staging;
    if (a.n == 0 || a.n_queries < 2 || a.n_queries > 8 || a.k == 0 || a.k > kGroupKMax || a.per_doc == 0 ||
        a.per_doc > RLR_MAX_PER_DOCUMENT || a.tab_bits < 1 || a.tab_bits > 31 || a.score_stride < a.n || !a.scores ||
        (!a.out && !a.capped) || !group_shape(a.pitch16, a.dim, a.dtype, &cpb, &staging))
        return hipErrorInvalidValue;
    if (a.capped) {
        const CappedBatchArgs &b = *a.capped;
        if (!b.scratch || !b.list || !b.comb || !b.cosv || !b.lexv || !b.docs || !b.info || !b.sizes)
            return hipErrorInvalidValue;
        for (uint32_t q = 0; q < a.n_queries; ++q)
            if (b.n_lex[q] > kCappedLexMax || b.n_lex[q] > b.lex_stride || (b.n_lex[q] && (!b.lrow || !b.lscore || !b.lcos)))
                return hipErrorInvalidValue;
    }
    GroupBatchDev d;
    d.n_queries = a.n_queries;
    d.scores = a.scores;
    d.score_stride = a.score_stride;
    d.docs = a.docs;
    d.n = a.n;
    d.k = a.k;
    d.per_doc = a.per_doc;
    d.two_eps = a.two_eps;
    d.tab_keys = a.tab_keys;
    d.tab_vals = a.tab_vals;
    d.tab_bits = a.tab_bits;
    d.tg = a.tg;
    d.hist = a.hist;
    d.st = a.st;
    d.rows = static_cast<const float4 *>(a.rows);
    d.pitch16 = a.pitch16;
    d.dim = a.dim;
    d.queries = a.queries;
    d.q_pitch = a.q_pitch;
    d.cand = a.cand;
    d.cand_doc = a.cand_doc;
    d.out = a.out;
    d.out_words = group_batch_words(a.k);
    d.cpb = cpb;
    // the launch shapes of launch_group_tail; heads, refine and collect with the query in the grid's y
    const uint32_t max_blocks = static_cast<uint32_t>(std::max(a.n_cu, 1)) * 8;
    const uint32_t row_blocks = std::max<uint32_t>(1, std::min<uint32_t>((a.n + kGroupBlock - 1) / kGroupBlock, max_blocks));
    const uint64_t slots = a.docs ? 1ull << a.tab_bits : 0ull;
    const uint32_t clear_blocks = static_cast<uint32_t>(std::max<uint64_t>(
        a.n_queries * 2u * kHistBins / kGroupBlock, std::min<uint64_t>((slots * a.per_doc * a.n_queries + kGroupBlock - 1) / kGroupBlock, max_blocks)));
    hipLaunchKernelGGL(group_clear_multi_kernel, dim3(clear_blocks), dim3(kGroupBlock), 0, s, d);
    if (a.docs) {
        hipLaunchKernelGGL(group_round_multi_kernel<true>, dim3(row_blocks), dim3(kGroupBlock), 0, s, d, 0u);
        for (uint32_t j = 1; j < a.per_doc; ++j)
            hipLaunchKernelGGL(group_round_multi_kernel<false>, dim3(row_blocks), dim3(kGroupBlock), 0, s, d, j);
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess)
        return e;
    hipLaunchKernelGGL(group_heads_multi_kernel, dim3(row_blocks, a.n_queries), dim3(kGroupBlock), 0, s, d);
    hipLaunchKernelGGL(group_refine_multi_kernel, dim3(row_blocks, a.n_queries), dim3(kGroupBlock), 0, s, d);
    const uint32_t collect_blocks =
        std::max<uint32_t>(1, std::min<uint32_t>(std::max<uint32_t>(row_blocks, (a.n + 31) / 32), max_blocks));
    if (a.dtype == RLR_F16)
        hipLaunchKernelGGL(group_collect_multi_kernel<true>, dim3(collect_blocks, a.n_queries), dim3(kGroupBlock), staging, s, d);
    else
        hipLaunchKernelGGL(group_collect_multi_kernel<false>, dim3(collect_blocks, a.n_queries), dim3(kGroupBlock), staging, s, d);
    if (a.capped)
        hipLaunchKernelGGL(capped_finish_multi_kernel, dim3(a.n_queries), dim3(1024), 0, s, d, *a.capped);
    else
        hipLaunchKernelGGL(group_finish_multi_kernel, dim3(a.n_queries), dim3(1024), 0, s, d);
    return hipGetLastError();
}

hipError_t launch_group_iota(uint32_t *list, uint32_t n, hipStream_t s)
{
    if (n == 0)
        return hipSuccess;
    hipLaunchKernelGGL(group_iota_kernel, dim3(std::min<uint32_t>((n + kGroupBlock - 1) / kGroupBlock, 4096)), dim3(kGroupBlock), 0, s, list, n);
    return hipGetLastError();
}

} // namespace rlr
