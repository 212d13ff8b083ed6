// docs.hip -- the per-row document column (include/rlr_gpu.h, "Document column"): which rows belong to a set of
// documents, as a filter's mask words and ascending row list, and its complement as the keep list of a deletion --
// all decided on the device from 4 bytes per row.
//
// Three kinds of launch, none of which waits for another workgroup (the rule of tail.hip: an order between workgroups
// comes from the order of launches on one stream, never from a flag):
//   docs_mask_kernel     one workgroup per kDocsRowsPerGroup rows: membership of every row, one __ballot per 64 rows
//                        IS the mask word (64-bit on gfx950); the popcounts add up to one count per workgroup.
//   docs_scan_kernel     exclusive scan of kDocsSumsPerGroup counts per workgroup, in place, and the sum of each tile;
//                        a second launch scans the tile sums.
//   docs_scatter_kernel  one workgroup per kDocsRowsPerGroup rows again: re-reads its mask words and writes the row
//                        numbers of the set bits (or, inverted, of the clear bits from `first_row` on) at
//                        group offset + words before + lane prefix.
//
// Scan hierarchy (tests/test_gpu_documents.py derives its row counts from these three lines):
//   level 0: a workgroup covers kDocsRowsPerGroup = 4096 rows (64 mask words, 16 per wave) -> one count
//   level 1: a scan workgroup covers kDocsSumsPerGroup = 1024 counts = 4 194 304 rows -> one tile sum
//   level 2: ONE scan workgroup covers up to kDocsSumsPerGroup = 1024 tile sums = 2^32 rows (an index holds < 2^32)
#include "../../include/rlr_gpu.h"
#include "common.h"
#include "kernels.h"

#include <algorithm>

namespace rlr {

namespace {

constexpr uint32_t kDocsBlock = 256;                                      // threads of every workgroup here
constexpr uint32_t kDocsWordsPerWave = 16;                                // mask words (runs of 64 rows) a wave owns
constexpr uint32_t kDocsWordsPerGroup = kDocsWordsPerWave * (kDocsBlock / kWave); // 64
static_assert(kDocsWordsPerGroup * 64 == kDocsRowsPerGroup, "kernels.h states the rows of a workgroup");
static_assert(kDocsSumsPerGroup == 4 * kDocsBlock, "a scan thread owns four consecutive sums");

// is `id` one of the n sorted, distinct ids at `set`?  (a branch-free lower bound; n >= 1)
__device__ inline bool docs_member(const uint32_t *set, uint32_t n, uint32_t id)
{
    uint32_t lo = 0, len = n;
    while (len > 1) {
        const uint32_t half = len >> 1;
        lo += set[lo + half - 1] < id ? half : 0;
        len -= half;
    }
    return set[lo] == id;
}

// Mask words and per-workgroup counts of {r : col[r] in docs}.  LDS_SET: the ids are staged in LDS first
// (n_docs <= kDocsLdsMax), else every probe of the binary search goes to global memory (the set is shared by all
// workgroups: it stays in L2).
template <bool LDS_SET>
__global__ __launch_bounds__(kDocsBlock) void docs_mask_kernel(const uint32_t *__restrict__ col, uint32_t n_rows,
                                                               const uint32_t *__restrict__ docs, uint32_t n_docs,
                                                               uint64_t *__restrict__ mask, uint32_t *__restrict__ counts)
{
    __shared__ uint32_t s_set[LDS_SET ? kDocsLdsMax : 1];
    __shared__ uint32_t s_cnt[kDocsBlock / kWave];
    if (LDS_SET) {
        for (uint32_t i = threadIdx.x; i < n_docs; i += kDocsBlock)
            s_set[i] = docs[i];
        __syncthreads();
    }
    const uint32_t *set = LDS_SET ? s_set : docs;
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t n_words = (n_rows + 63) / 64;
    const uint32_t w0 = blockIdx.x * kDocsWordsPerGroup + wave * kDocsWordsPerWave;
    uint32_t cnt = 0;
    for (uint32_t i0 = 0; i0 < kDocsWordsPerWave; i0 += 4) { // four loads in flight per wave, then four votes
        if (w0 + i0 >= n_words)                              // (wave-uniform)
            break;
        uint32_t id[4];
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) {
            // a lane past the last row reads nothing and votes 0: the ragged last word gets its zero tail by predicate
            const uint64_t row = static_cast<uint64_t>(w0 + i0 + j) * 64 + lane;
            id[j] = row < n_rows ? col[row] : RLR_DOC_NONE; // one coalesced 256 B load per word
        }
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) {
            const uint32_t w = w0 + i0 + j;
            const bool member = id[j] != RLR_DOC_NONE && docs_member(set, n_docs, id[j]);
            const uint64_t word = __ballot(member);
            if (lane == 0 && w < n_words)
                mask[w] = word;
            cnt += static_cast<uint32_t>(__popcll(word));
        }
    }
    if (lane == 0)
        s_cnt[wave] = cnt;
    __syncthreads();
    if (threadIdx.x == 0)
        counts[blockIdx.x] = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
}

// inclusive sum over the wave's lanes
__device__ inline uint32_t wave_inclusive_sum(uint32_t v, uint32_t lane)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t up = __shfl_up(v, d, 64);
        if (lane >= static_cast<uint32_t>(d))
            v += up;
    }
    return v;
}

// v[tile * kDocsSumsPerGroup ..) := its exclusive scan (within the tile); tile_sums[tile] := the tile's sum.
__global__ __launch_bounds__(kDocsBlock) void docs_scan_kernel(uint32_t *__restrict__ v, uint32_t n, uint32_t *__restrict__ tile_sums)
{
    __shared__ uint32_t s_wave[kDocsBlock / kWave];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t base = blockIdx.x * kDocsSumsPerGroup + threadIdx.x * 4;
    uint32_t x[4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
        x[j] = base + j < n ? v[base + j] : 0u;
    const uint32_t mine = x[0] + x[1] + x[2] + x[3];
    const uint32_t incl = wave_inclusive_sum(mine, lane);
    if (lane == 63)
        s_wave[wave] = incl;
    __syncthreads();
    uint32_t before = incl - mine;
    for (uint32_t w = 0; w < wave; ++w)
        before += s_wave[w];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (base + j < n)
            v[base + j] = before;
        before += x[j];
    }
    if (threadIdx.x == kDocsBlock - 1)
        tile_sums[blockIdx.x] = before; // (the last thread's running sum has reached the tile's total)
}

// The rows of the mask's set bits, ascending, at list[set bits before the row].  offsets = the scanned counts of the
// mask launch (one per workgroup), tile_offsets = the scanned tile sums (null when one tile covers every workgroup).
// invert != 0: the rows >= first_row whose bit is CLEAR instead, at list[(row - first_row) - set bits before the row]
// (every set bit lies at or after first_row: the caller passes the first set bit's row).
__global__ __launch_bounds__(kDocsBlock) void docs_scatter_kernel(const uint64_t *__restrict__ mask, uint32_t n_rows,
                                                                  const uint32_t *__restrict__ offsets,
                                                                  const uint32_t *__restrict__ tile_offsets, int invert,
                                                                  uint32_t first_row, uint32_t *__restrict__ list)
{
    __shared__ uint32_t s_wave[kDocsBlock / kWave];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t n_words = (n_rows + 63) / 64;
    const uint32_t w0 = blockIdx.x * kDocsWordsPerGroup + wave * kDocsWordsPerWave;
    // lane i < 16 holds word w0 + i of this wave and the set bits of the wave's words before it
    const uint32_t wl = w0 + lane;
    const uint64_t my_word = lane < kDocsWordsPerWave && wl < n_words ? mask[wl] : 0ull;
    const uint32_t my_cnt = static_cast<uint32_t>(__popcll(my_word));
    const uint32_t incl = wave_inclusive_sum(my_cnt, lane);
    if (lane == 63)
        s_wave[wave] = incl;
    __syncthreads();
    uint32_t base = offsets[blockIdx.x] + (tile_offsets ? tile_offsets[blockIdx.x / kDocsSumsPerGroup] : 0u);
    for (uint32_t w = 0; w < wave; ++w)
        base += s_wave[w];
    const uint32_t excl = incl - my_cnt;
    for (uint32_t i = 0; i < kDocsWordsPerWave; ++i) {
        const uint32_t w = w0 + i; // (wave-uniform)
        if (w >= n_words)
            break;
        const uint64_t word = __shfl(my_word, i, 64);
        const uint32_t before_word = base + __shfl(excl, i, 64);
        // set bits of this word below my lane (v_mbcnt over the two halves of the word)
        const uint32_t below = __builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(word >> 32),
                                                         __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(word), 0u));
        const uint64_t row = static_cast<uint64_t>(w) * 64 + lane;
        const bool set = (word >> lane) & 1ull;
        if (!invert) {
            if (set)
                list[before_word + below] = static_cast<uint32_t>(row);
        } else if (!set && row < n_rows && row >= first_row) {
            list[static_cast<uint32_t>(row) - first_row - (before_word + below)] = static_cast<uint32_t>(row);
        }
    }
}

__global__ __launch_bounds__(kDocsBlock) void docs_fill_kernel(uint32_t *__restrict__ col, uint64_t n, uint32_t doc)
{
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kDocsBlock;
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * kDocsBlock + threadIdx.x; i < n; i += stride)
        col[i] = doc;
}

__global__ __launch_bounds__(kDocsBlock) void docs_gather_kernel(const uint32_t *__restrict__ col, const uint32_t *__restrict__ keep,
                                                                 uint64_t n, uint32_t *__restrict__ out)
{
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kDocsBlock;
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * kDocsBlock + threadIdx.x; i < n; i += stride)
        out[i] = col[keep[i]];
}

uint32_t docs_ew_blocks(uint64_t n)
{
    return static_cast<uint32_t>(std::min<uint64_t>((n + kDocsBlock - 1) / kDocsBlock, 4096));
}

} // namespace

uint32_t docs_groups(uint32_t n_rows)
{
    return static_cast<uint32_t>((static_cast<uint64_t>(n_rows) + kDocsRowsPerGroup - 1) / kDocsRowsPerGroup);
}

uint32_t docs_tiles(uint32_t n_groups)
{
    return (n_groups + kDocsSumsPerGroup - 1) / kDocsSumsPerGroup;
}

hipError_t launch_docs_mask(const uint32_t *col, uint32_t n_rows, const uint32_t *docs, uint32_t n_docs, uint64_t *mask,
                            uint32_t *counts, hipStream_t s)
{
    if (n_rows == 0 || n_docs == 0)
        return hipErrorInvalidValue;
    const dim3 grid(docs_groups(n_rows)), block(kDocsBlock);
    if (n_docs <= kDocsLdsMax)
        hipLaunchKernelGGL(docs_mask_kernel<true>, grid, block, 0, s, col, n_rows, docs, n_docs, mask, counts);
    else
        hipLaunchKernelGGL(docs_mask_kernel<false>, grid, block, 0, s, col, n_rows, docs, n_docs, mask, counts);
    return hipGetLastError();
}

hipError_t launch_docs_scan(uint32_t *counts, uint32_t n_groups, uint32_t *tile_sums, uint32_t *total, hipStream_t s)
{
    const uint32_t tiles = docs_tiles(n_groups);
    if (n_groups == 0 || tiles > kDocsSumsPerGroup)
        return hipErrorInvalidValue; // (2^32 rows: an index never holds that many)
    if (tiles == 1) {
        hipLaunchKernelGGL(docs_scan_kernel, dim3(1), dim3(kDocsBlock), 0, s, counts, n_groups, total);
        return hipGetLastError();
    }
    hipLaunchKernelGGL(docs_scan_kernel, dim3(tiles), dim3(kDocsBlock), 0, s, counts, n_groups, tile_sums);
    hipLaunchKernelGGL(docs_scan_kernel, dim3(1), dim3(kDocsBlock), 0, s, tile_sums, tiles, total);
    return hipGetLastError();
}

hipError_t launch_docs_scatter(const uint64_t *mask, uint32_t n_rows, const uint32_t *offsets, const uint32_t *tile_offsets,
                               int invert, uint32_t first_row, uint32_t *list, hipStream_t s)
{
    if (n_rows == 0)
        return hipSuccess;
    const uint32_t groups = docs_groups(n_rows);
    hipLaunchKernelGGL(docs_scatter_kernel, dim3(groups), dim3(kDocsBlock), 0, s, mask, n_rows, offsets,
                       docs_tiles(groups) > 1 ? tile_offsets : nullptr, invert, first_row, list);
    return hipGetLastError();
}

hipError_t launch_docs_fill(uint32_t *col, uint64_t n, uint32_t doc, hipStream_t s)
{
    if (n == 0)
        return hipSuccess;
    hipLaunchKernelGGL(docs_fill_kernel, dim3(docs_ew_blocks(n)), dim3(kDocsBlock), 0, s, col, n, doc);
    return hipGetLastError();
}

hipError_t launch_docs_gather(const uint32_t *col, const uint32_t *keep, uint64_t n, uint32_t *out, hipStream_t s)
{
    if (n == 0)
        return hipSuccess;
    hipLaunchKernelGGL(docs_gather_kernel, dim3(docs_ew_blocks(n)), dim3(kDocsBlock), 0, s, col, keep, n, out);
    return hipGetLastError();
}

} // namespace rlr
