// index.hip -- the C ABI of include/rlr_gpu.h: device-resident chunk-embedding matrix,
// per-call search contexts (stream + workspace), and the kernel pipeline of a single query
//   scan (+digit-1 histogram) -> tail stage 1 -> tail stage 2 (tail.hip: select, reference-order re-score, sort, results
//   and a completion word straight into pinned host memory), or above 4 M rows the four specialised launches
//   hist2_find1 -> collect_find2 -> rescore_staged -> sort_emit; batches of queries go through the matrix cores (gemm.hip).
// This file defines the frame index_internal.h declares; the search chains that end in a blend or MMR on the device are
// in index_fused.hip, grouped, range and capped search in index_grouped.hip.
// There is no CPU compute path in this file: without a HIP device every compute entry
// point fails with RLR_E_NO_DEVICE.
#include "index_internal.h"
#include "lds_select.h"
#include "sort_emit.h"
#include "lexical_internal.h"
#include "filter_internal.h"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <memory>
#include <new>
#include <thread>
#include <vector>

#include <time.h>

using namespace rlr;

namespace {

thread_local char g_err[512] = "";

} // namespace

namespace rlr {
// the thread-local message behind rlr_last_error(), for this file and the other translation units of the library
int32_t set_error(int32_t code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}
} // namespace rlr

namespace rlr {
bool poison_mode()
{
    static const bool poison = [] {
        const char *v = getenv("RLR_POISON_ALLOC");
        return v && v[0] == '1';
    }();
    return poison;
}

hipError_t dev_malloc(void **p, size_t bytes)
{
    const bool poison = poison_mode();
    hipError_t e = hipMalloc(p, bytes);
    if (e != hipSuccess)
        (void)hipGetLastError(); // reported through the return value; do not leave it for a later launch check to find
    if (e == hipSuccess && poison && bytes) {
        e = hipMemset(*p, 0xFF, bytes);
        if (e == hipSuccess)
            e = hipDeviceSynchronize();
    }
    return e;
}

int32_t use_device(const rlr_index *ix)
{
    RLR_HIP(hipSetDevice(ix->device));
    return RLR_OK;
}

int32_t pin_reserve(Ctx *c, size_t bytes)
{
    RLR_HIP(c->h_pin.reserve(std::max<size_t>(bytes, 1 << 16)));
    return RLR_OK;
}

int32_t reserve_queries(const rlr_index *ix, Ctx *c, uint32_t nq)
{
    if (c->d_state.capacity() >= nq)
        return RLR_OK;
    RLR_HIP(reserve_group(Want{c->d_query, static_cast<size_t>(nq) * ix->q_pitch}, Want{c->d_state, nq}));
    // the fused tail's counters (n_work, done, flags) are zero between two queries; on the context's stream, like the histograms
    const hipError_t e = hipMemsetAsync(c->d_state.get(), 0, static_cast<size_t>(nq) * sizeof(SelectState), c->stream);
    if (e != hipSuccess)
        c->d_state.reset(); // (states that were never cleared: the next call rebuilds the group)
    RLR_HIP(e);
    return RLR_OK;
}

// c->d_cand / c->d_packed for cap candidates
static int32_t reserve_cand(Ctx *c, uint32_t cap)
{
    RLR_HIP(reserve_group(Want{c->d_cand, cap}, Want{c->d_packed, cap}));
    return RLR_OK;
}

static void ctx_free(Ctx *c)
{
    if (!c)
        return;
    for (auto &e : c->ev)
        if (e) (void)hipEventDestroy(e);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    for (auto &e : c->bev)
        if (e) (void)hipEventDestroy(e);
    delete c; // (the buffers free themselves)
}

int32_t ctx_acquire(rlr_index *ix, Ctx **out)
{
    {
        std::unique_lock<std::mutex> lk(ix->mu);
        for (;;) {
            if (!ix->free_ctx.empty()) {
                Ctx *c = ix->free_ctx.back(); // the most recently released one
                ix->free_ctx.pop_back();
                lk.unlock();
                if (c->hist_dirty) { // a previous call failed half way: restore the zero-histogram invariant
                    (void)hipStreamSynchronize(c->stream);
                    // (on the context's own stream: the null stream does not order against a non-blocking one)
                    if (hipMemsetAsync(c->d_hist.get(), 0, 2 * kHistBins * sizeof(uint32_t), c->stream) == hipSuccess &&
                        (!c->d_state.get() || hipMemsetAsync(c->d_state.get(), 0, c->d_state.capacity() * sizeof(SelectState), c->stream) ==
                                            hipSuccess))
                        c->hist_dirty = false;
                }
                *out = c;
                return RLR_OK;
            }
            if (ix->ctx_made < ix->ctx_cap) {
                ix->ctx_made++;
                break;
            }
            ix->ctx_cv.wait(lk);
        }
    }
    auto give_up = [ix](Ctx *c) {
        ctx_free(c);
        {
            std::lock_guard<std::mutex> lk(ix->mu);
            ix->ctx_made--;
        }
        ix->ctx_cv.notify_one();
    };
    Ctx *c = new (std::nothrow) Ctx();
    if (!c) {
        give_up(nullptr);
        return set_error(RLR_E_OOM, "host allocation failed");
    }
    hipError_t e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    for (int i = 0; i < 4 && e == hipSuccess; ++i)
        e = hipEventCreate(&c->ev[i]);
    for (int i = 0; i < 5 && e == hipSuccess; ++i)
        e = hipEventCreate(&c->bev[i]);
    if (e == hipSuccess)
        e = c->d_hist.reserve(2 * kHistBins);
    // The zero-histogram invariant is established ON THE CONTEXT'S STREAM: a null-stream hipMemset of device
    // memory may return before it has run, and a non-blocking stream is not ordered against the null stream --
    // the first scan's histogram atomics could then land before the fill and be wiped (a rare wrong threshold
    // on the first search of a fresh context, caught by the multi-shard fuzz with five contexts starting at once).
    if (e == hipSuccess)
        e = hipMemsetAsync(c->d_hist.get(), 0, 2 * kHistBins * sizeof(uint32_t), c->stream);
    if (e == hipSuccess && rlr::poison_mode()) {
        e = c->h_assert.reserve(64);
        if (e == hipSuccess)
            *static_cast<uint32_t *>(c->h_assert.get()) = 0;
    }
    if (e == hipSuccess)
        e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) {
        give_up(c);
        return set_error(RLR_E_HIP, "context setup failed: %s", hipGetErrorString(e));
    }
    *out = c;
    return RLR_OK;
}

void ctx_release(rlr_index *ix, Ctx *c)
{
    {
        std::lock_guard<std::mutex> lk(ix->mu);
        ix->free_ctx.push_back(c);
    }
    ix->ctx_cv.notify_one();
}

int32_t check_handle(const rlr_index *ix)
{
    if (!ix)
        return set_error(RLR_E_INVALID, "null index handle");
    return RLR_OK;
}

static int32_t ensure_rows(rlr_index *ix, uint64_t want_rows)
{
    if (want_rows <= ix->cap_rows)
        return RLR_OK;
    if (want_rows > 0xFFFFFFF0ull)
        return set_error(RLR_E_INVALID, "an index shard holds at most 2^32-16 rows");
    uint64_t cap = std::max<uint64_t>(want_rows, ix->cap_rows + ix->cap_rows / 2);
    cap = std::max<uint64_t>(cap, 1024);
    DevBuf<char> n;
    hipError_t e = n.reserve(cap * row_bytes(ix));
    if (e != hipSuccess && cap > want_rows) {
        cap = want_rows;
        e = n.reserve(cap * row_bytes(ix));
    }
    if (e != hipSuccess)
        return set_error(RLR_E_OOM, "allocation of %llu rows x %zu B failed: %s",
                         static_cast<unsigned long long>(cap), row_bytes(ix), hipGetErrorString(e));
    DevBuf<uint32_t> nd; // the document column moves with the rows
    if (ix->d_docs && nd.reserve(cap) != hipSuccess)
        return set_error(RLR_E_OOM, "allocation of the document column for %llu rows failed", static_cast<unsigned long long>(cap));
    if (ix->d_rows.get() && ix->n_rows) {
        hipError_t ce = hipMemcpy(n.get(), ix->d_rows.get(), ix->n_rows * row_bytes(ix), hipMemcpyDeviceToDevice);
        if (ce == hipSuccess)
            ce = hipStreamSynchronize(nullptr); // a device-to-device copy may return before it has run
        if (ce == hipSuccess && ix->d_docs) {
            ce = hipMemcpyAsync(nd.get(), ix->d_docs.get(), ix->n_rows * sizeof(uint32_t), hipMemcpyDeviceToDevice, nullptr);
            if (ce == hipSuccess)
                ce = hipStreamSynchronize(nullptr);
        }
        if (ce != hipSuccess)
            return set_error(RLR_E_HIP, "moving the rows into the larger allocation failed: %s", hipGetErrorString(ce));
    }
    if (ix->d_docs)
        ix->d_docs = std::move(nd);
    ix->d_rows = std::move(n); // (frees the old rows)
    ix->cap_rows = cap;
    return RLR_OK;
}

// (Re)build the 8-bit nomination copy for rows >= first_row; the error / scale maxima only ever grow between
// full rebuilds (a delete keeps the old maxima: conservative).
static int32_t sync_q8(rlr_index *ix, uint64_t first_row)
{
    if (!ix->q8_enabled)
        return RLR_OK;
    const uint64_t want = std::max<uint64_t>(std::max<uint64_t>(ix->cap_rows, ix->n_rows), 1);
    if (ix->d_q8_scale.capacity() < want) {
        RLR_HIP(reserve_group(Want{ix->d_q8, want * ix->dim}, Want{ix->d_q8_scale, want}));
        first_row = 0;
    }
    RLR_HIP(ix->d_q8_stats.reserve(4));
    if (first_row == 0)
        RLR_HIP(hipMemset(ix->d_q8_stats.get(), 0, 4 * sizeof(uint32_t)));
    RLR_HIP(launch_q8_build(ix->d_rows.get(), ix->pitch16, ix->dim, ix->dtype, static_cast<uint32_t>(first_row),
                            static_cast<uint32_t>(ix->n_rows), ix->d_q8.get(), ix->d_q8_scale.get(), ix->d_q8_stats.get(), nullptr));
    uint32_t h[4] = {0, 0, 0, 0};
    RLR_HIP(hipMemcpy(h, ix->d_q8_stats.get(), sizeof(h), hipMemcpyDeviceToHost));
    std::memcpy(&ix->q8_delta, &h[0], 4);
    std::memcpy(&ix->q8_scale_max, &h[1], 4);
    ix->q8_has_inf = h[2] != 0;
    return RLR_OK;
}

// (Re)build the nomination image for every tile that holds a row >= first_row.
static int32_t sync_image(rlr_index *ix, uint64_t first_row)
{
    RLR_TRY(sync_q8(ix, first_row));
    if (!ix->image_enabled)
        return RLR_OK;
    const size_t need = image_bytes(ix->dim, std::max<uint64_t>(ix->cap_rows, ix->n_rows));
    if (ix->d_image.capacity() < need) {
        RLR_HIP(ix->d_image.reserve(std::max<size_t>(need, 256)));
        first_row = 0; // fresh buffer: every tile has to be written
    }
    const uint32_t t0 = static_cast<uint32_t>(first_row / 256);
    const uint32_t t1 = static_cast<uint32_t>((ix->n_rows + 255) / 256);
    RLR_HIP(launch_build_image(ix->d_rows.get(), ix->pitch16, ix->dim, ix->dtype, static_cast<uint32_t>(ix->n_rows), t0, t1,
                               ix->d_image.get(), nullptr));
    RLR_HIP(hipStreamSynchronize(nullptr));
    return RLR_OK;
}

// does any of the n values lie outside binary16 range (|x| > 65504, Inf included)?  NaN does not count: a NaN operand
// makes the reference's score NaN as well, which orders last on every path.
static bool beyond_f16(const float *v, uint32_t n)
{
    for (uint32_t i = 0; i < n; ++i)
        if (std::fabs(v[i]) > 65504.0f)
            return true;
    return false;
}

// a vector with an element beyond binary16 range has a sum of squares above 65504^2 -- the cheap test in front of the
// element-wise one (row sums of squares come from an f32 reduction: the ingest test leaves it 0.1 % of slack)
constexpr double kF16MaxSq = 65504.0 * 65504.0;

// Copy host rows in, normalise (optionally) and store them at row `first`.
static int32_t ingest(rlr_index *ix, const float *rows, uint64_t n, uint64_t first, int normalize)
{
    if (n == 0)
        return RLR_OK;
    const uint64_t chunk_rows = std::max<uint64_t>(1, (64ull << 20) / (static_cast<uint64_t>(ix->dim) * 4));
    DevBuf<float> stage, norm;
    const uint64_t cr = std::min(chunk_rows, n);
    RLR_HIP(stage.reserve(cr * ix->dim));
    hipError_t e = norm.reserve(cr);
    if (e != hipSuccess)
        return set_error(RLR_E_OOM, "staging allocation failed");
    float *const d_stage = stage.get(), *const d_norm = norm.get();
    int32_t st = RLR_OK;
    std::vector<float> h_norm;
    for (uint64_t r0 = 0; r0 < n && st == RLR_OK; r0 += cr) {
        const uint64_t m = std::min(cr, n - r0);
        e = hipMemcpy(d_stage, rows + r0 * ix->dim, m * ix->dim * sizeof(float), hipMemcpyHostToDevice);
        if (e == hipSuccess)
            e = launch_normalize_store(d_stage, static_cast<uint32_t>(m), ix->dim, normalize,
                                       static_cast<char *>(ix->d_rows.get()) + (first + r0) * row_bytes(ix), ix->pitch16,
                                       ix->dtype, d_norm, nullptr);
        if (e == hipSuccess)
            e = hipStreamSynchronize(nullptr);
        if (e == hipSuccess && !normalize) {
            // rows stored as given: remember the largest norm (NaN rows order last anyway; they do not widen the band)
            h_norm.resize(m);
            e = hipMemcpy(h_norm.data(), d_norm, m * sizeof(float), hipMemcpyDeviceToHost);
            for (uint64_t i = 0; i < m && e == hipSuccess; ++i) {
                if (h_norm[i] > ix->max_row_sumsq)
                    ix->max_row_sumsq = h_norm[i];
                if (ix->dtype == RLR_F32 && !ix->f16_overflow && h_norm[i] > 0.999 * kF16MaxSq &&
                    beyond_f16(rows + (r0 + i) * ix->dim, ix->dim))
                    ix->f16_overflow = true;
            }
        }
        if (e != hipSuccess)
            st = set_error(RLR_E_HIP, "row ingest failed: %s", hipGetErrorString(e));
    }
    return st;
}

// ---- waiting for a query without the stream's completion signal ------------------------------------------------
// The last kernel of a pipeline writes the query's candidate count into pinned host memory behind a system-scope fence
// (sort_emit.h), so "the count has left kMetaPending" means "the k results are in host memory".  hipStreamSynchronize
// learns the same thing from the queue's completion signal, which the ROCm runtime waits for in the kernel driver
// (interrupt + wake-up: ~15-20 us between the end of the last kernel and the return, measured as device idle time
// between two searches of a C loop); polling the word takes ~1 us.  RLR_WAIT: "hybrid" (default) polls, but sleeps
// through the first two thirds of a wait that took more than 1.5 ms last time -- a 4.4 ms scan does not burn a core --,
// "spin" always polls from the start, "block" is hipStreamSynchronize.
namespace {

enum WaitMode { kWaitHybrid = 0, kWaitSpin = 1, kWaitBlock = 2 };

WaitMode wait_mode()
{
    static const WaitMode m = [] {
        const char *v = getenv("RLR_WAIT");
        if (v && v[0] == 's')
            return kWaitSpin;
        if (v && v[0] == 'b')
            return kWaitBlock;
        return kWaitHybrid;
    }();
    return m;
}

inline void cpu_relax()
{
#if defined(__x86_64__) || defined(__i386__)
    __builtin_ia32_pause();
#else
    __asm__ __volatile__("" ::: "memory");
#endif
}

// Wait until `complete()` holds -- it reads pinned host words the device writes last (and may check them against the
// data they cover).  The stream is queried every ~1000 polls: an error, or a drained stream with the words still
// incomplete (a kernel that never ran), ends the wait.
template <typename Complete>
int32_t wait_polling(Complete &&complete, hipStream_t s, WaitEma *c, uint32_t key)
{
    using clk = std::chrono::steady_clock;
    const WaitMode mode = wait_mode();
    if (mode == kWaitBlock) {
        RLR_HIP(hipStreamSynchronize(s));
        return RLR_OK;
    }
    const auto t0 = clk::now();
    bool slept = false;
    if (c && c->key != key) {
        c->key = key;
        c->us = 0.0;
    }
    // (only waits of milliseconds: a timed sleep comes back 50-150 us late often enough that at 0.5 ms per query the
    // hybrid form measured 589 us per call where polling from the start took 565 and hipStreamSynchronize 570)
    if (mode == kWaitHybrid && c && c->us > 1500.0) {
        const double sleep_us = 0.7 * c->us - 150.0;
        if (sleep_us > 20.0) {
            timespec ts;
            clock_gettime(CLOCK_MONOTONIC, &ts);
            const long add = static_cast<long>(sleep_us * 1000.0);
            ts.tv_sec += (ts.tv_nsec + add) / 1000000000L;
            ts.tv_nsec = (ts.tv_nsec + add) % 1000000000L;
            (void)clock_nanosleep(CLOCK_MONOTONIC, TIMER_ABSTIME, &ts, nullptr);
            slept = true;
        }
    }
    uint32_t polls = 0;
    for (;;) {
        std::atomic_thread_fence(std::memory_order_acquire);
        if (complete())
            break;
        if ((++polls & 0x3FFu) == 0) {
            const hipError_t e = hipStreamQuery(s);
            if (e == hipSuccess) {
                // drained: everything the kernels stored is on its way; give it a moment, then it is an error
                bool ok = false;
                for (int spin = 0; spin < 100000 && !ok; ++spin) {
                    std::atomic_thread_fence(std::memory_order_acquire);
                    ok = complete();
                    cpu_relax();
                }
                if (ok)
                    break;
                return set_error(RLR_E_INTERNAL, "the stream drained but a completion word was never written");
            }
            if (e != hipErrorNotReady)
                return set_error(RLR_E_HIP, "stream failed while a search was in flight: %s", hipGetErrorString(e));
        }
        if (polls > 8192 && (polls & 0xFF) == 0)
            std::this_thread::yield(); // a long wait: more waiters than cores must not starve the threads that feed the GPU
        cpu_relax();
    }
    std::atomic_thread_fence(std::memory_order_acquire);
    if (c) {
        const double us = std::chrono::duration<double, std::micro>(clk::now() - t0).count();
        if (slept && polls == 0) // the words were there when the sleep ended: it was too long (a smaller corpus than last time)
            c->us *= 0.5;
        else
            c->us = c->us == 0.0 ? us : 0.75 * c->us + 0.25 * us;
    }
    return RLR_OK;
}

} // namespace

int32_t wait_block(const volatile uint32_t *h_out, uint32_t k_cap, hipStream_t s, WaitEma *c)
{
    return wait_polling(
        [&]() {
            if (h_out[block_done(k_cap)] != kBlockDone)
                return false;
            const uint32_t n = h_out[block_n(k_cap)], status = h_out[block_status(k_cap)];
            if (n > k_cap)
                return false;
            uint32_t chk = 0;
            for (uint32_t b = 0; b < kBlockPlanes; ++b)
                for (uint32_t i = 0; i < n; ++i)
                    chk += result_chk_term(h_out[block_value(k_cap, b, i)], block_value(k_cap, b, i));
            return block_chk_tail(chk, n, status, k_cap) == h_out[block_chk(k_cap)];
        },
        s, c, 0x40000000u);
}

uint32_t read_block(const uint32_t *h_out, uint32_t k_cap, uint64_t *rows_out, float *cos_out, float *score_out, float *lex_out,
                    uint32_t *n_out)
{
    const uint32_t n = h_out[block_n(k_cap)], status = h_out[block_status(k_cap)];
    if (status != 0)
        return status;
    for (uint32_t i = 0; i < n; ++i) {
        rows_out[i] = h_out[block_value(k_cap, kBlockRow, i)];
        cos_out[i] = __builtin_bit_cast(float, h_out[block_value(k_cap, kBlockCos, i)]);
        score_out[i] = __builtin_bit_cast(float, h_out[block_value(k_cap, kBlockComb, i)]);
        if (lex_out)
            lex_out[i] = __builtin_bit_cast(float, h_out[block_value(k_cap, kBlockLex, i)]);
    }
    *n_out = n;
    return 0;
}

int32_t wait_results(const volatile uint64_t *meta, const volatile uint64_t *res, uint32_t nq, uint32_t k, uint32_t limit,
                            hipStream_t s, WaitEma *c)
{
    uint32_t verified = nq; // queries [verified, nq) are complete (the last one finishes last)
    return wait_polling(
        [&]() {
            while (verified > 0) {
                const uint32_t q = verified - 1;
                const uint64_t m = meta[q];
                if (m == kMetaPending)
                    return false;
                if (res && static_cast<uint32_t>(m) <= limit) { // (an overflowed query emits only its marker: nothing to verify)
                    uint32_t chk = 0;
                    const volatile uint64_t *r = res + static_cast<size_t>(q) * k;
                    for (uint32_t i = 0; i < k; ++i) {
                        const uint64_t w = r[i];
                        if (w)
                            chk += result_chk_term(w, i);
                    }
                    if (chk != static_cast<uint32_t>(m >> 32))
                        return false;
                }
                verified--;
            }
            return true;
        },
        s, c, nq);
}

// ---- query upload -----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void stage_query_kernel(const float4 *__restrict__ src, float4 *__restrict__ dst, uint32_t n16)
{
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n16; i += gridDim.x * 256)
        dst[i] = src[i];
}

hipError_t upload_queries(Ctx *c, const float *h_q, size_t q_bytes, hipStream_t s)
{
    if (q_bytes > (64u << 10) || (q_bytes & 15) || (reinterpret_cast<uintptr_t>(h_q) & 15))
        return hipMemcpyAsync(c->d_query.get(), h_q, q_bytes, hipMemcpyHostToDevice, s);
    const uint32_t n16 = static_cast<uint32_t>(q_bytes / 16);
    hipLaunchKernelGGL(rlr::stage_query_kernel, dim3(std::min<uint32_t>((n16 + 255) / 256, 8)), dim3(256), 0, s,
                       reinterpret_cast<const float4 *>(h_q), reinterpret_cast<float4 *>(c->d_query.get()), n16);
    return hipGetLastError();
}

// ---- the search pipeline ------------------------------------------------------------
// The guard bands are error bounds for unit-norm operands; every term of them is linear in |row| * |query|.
// Rows stored with normalize_on_device = 0 and queries the caller did not normalise widen the band by that
// product (norms rounded up); unit-norm data -- the reference's invariant, rag_engine.rs:359 / :494 -- gives 1.
// sum of squares in binary64 with eight independent partial sums: the value only feeds an upper bound with its own slack, so
// the order is free -- and one dependent chain per query was 0.2 ms of host time in front of every 256-query batch of 768-d
// queries (1.2 ms in front of config 5's 1024 x 1024-d), more than the whole select-and-finish tail.
static double sumsq_f64(const float *v, uint32_t n)
{
    double a[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    uint32_t i = 0;
    for (; i + 8 <= n; i += 8)
        for (int j = 0; j < 8; ++j)
            a[j] += static_cast<double>(v[i + j]) * v[i + j];
    for (; i < n; ++i)
        a[0] += static_cast<double>(v[i]) * v[i];
    return ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]));
}

// The plan's band factors for this call's queries: p->scale (above), p->norm_sum (nomination_eps) and p->f16_ok.
static void plan_bands(const rlr_index *ix, const float *queries, uint32_t nq, SearchPlan *p)
{
    double qmax = 0.0;
    bool f16_ok = !(ix->dtype == RLR_F32 && ix->f16_overflow);
    for (uint32_t q = 0; q < nq; ++q) {
        const double s2 = sumsq_f64(queries + static_cast<size_t>(q) * ix->dim, ix->dim);
        if (s2 > qmax) // (a NaN query compares false: its scores are NaN and order last whatever the band)
            qmax = s2;
        if (f16_ok && s2 > kF16MaxSq && beyond_f16(queries + static_cast<size_t>(q) * ix->dim, ix->dim))
            f16_ok = false;
    }
    const double qn = std::sqrt(qmax), rn = std::sqrt(static_cast<double>(ix->max_row_sumsq));
    const double f = qn * rn * 1.000002;
    p->scale = !(f > 1.0001) ? 1.0f : std::isfinite(f) ? static_cast<float>(f) : 3.0e38f;
    // unit-norm operands give exactly 2, so the unit-norm band is unchanged
    const double sum = qn + rn;
    p->norm_sum = !(sum > 2.0001) ? 2.0f : sum * 1.000002 < 3.0e38 ? static_cast<float>(sum * 1.000002) : 3.0e38f;
    p->f16_ok = f16_ok;
}

int32_t ctx_prepare(rlr_index *ix, Ctx *c, uint32_t nq, const SearchPlan &p)
{
    c->no_f16 = !p.f16_ok;
    RLR_TRY(reserve_queries(ix, c, nq));
    RLR_HIP(c->d_scores.reserve(std::max<uint64_t>(ix->n_rows, 4)));
    RLR_TRY(reserve_cand(c, p.cap));
    RLR_HIP(c->d_out.reserve(static_cast<uint64_t>(nq) * p.k + nq)); // results + per-query counts
    return RLR_OK;
}

// Debug assertion (RLR_POISON_ALLOC=1 runs only): every single-query pipeline relies on "the histograms are zero on
// entry" -- established at context creation and re-established by the previous query's re-score kernel, which is only
// stream-order-safe.  A second stream, a reordered launch or a skipped clear would break it silently (a wrong threshold,
// not a crash); this kernel runs in front of every scan in the poisoned test runs and counts non-zero bins into a
// pinned host word that the host checks at the call's synchronisation.
__global__ __launch_bounds__(256) void hist_assert_zero_kernel(const uint32_t *__restrict__ hist, uint32_t n,
                                                               uint32_t *__restrict__ flag)
{
    uint32_t bad = 0;
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256)
        bad += hist[i] != 0;
    if (bad)
        atomicAdd(flag, bad);
}

// device-side: sort the re-scored candidates (<= kLdsSortCap) and emit the best k (sort_emit.h).
__global__ __launch_bounds__(1024) void sort_emit_kernel(uint64_t *__restrict__ packed, const SelectState *__restrict__ st,
                                                         uint64_t *__restrict__ out, uint32_t k,
                                                         uint64_t *__restrict__ meta, bool unordered)
{
    __shared__ uint64_t s[4096];
    __shared__ uint32_t s_hist[2048];
    sort_emit_body(packed, st->n_cand, st->cap, out, k, meta, unordered, s, s_hist);
}

// Exchange-step merge: one workgroup per query orders the world x k packed partial
// results the all-gather delivered and emits the global top-k.  Shards are ascending row ranges,
// so (score desc, global row asc) is the same tie rule every shard already applied.
struct MergeBases {
    uint64_t base[16];
};


__global__ __launch_bounds__(1024) void merge_topk_kernel(const uint64_t *__restrict__ gathered, uint32_t world,
                                                         uint32_t n_queries, uint32_t k, MergeBases bases,
                                                         uint64_t *__restrict__ rows_out, float *__restrict__ cos_out,
                                                         uint32_t *__restrict__ n_out, uint64_t *__restrict__ flag_out)
{
    __shared__ uint64_t s[8192];
    __shared__ uint32_t s_valid;
    __shared__ uint32_t s_valid_overflow;
    __shared__ uint32_t s_chk;
    const uint32_t q = blockIdx.x;
    const uint32_t n = world * k;
    uint32_t n_pad = 1;
    while (n_pad < n)
        n_pad <<= 1;
    if (threadIdx.x == 0) {
        s_valid = 0;
        s_valid_overflow = 0;
        s_chk = 0;
    }
    __syncthreads();
    uint32_t valid = 0;
    for (uint32_t i = threadIdx.x; i < n_pad; i += 1024) {
        uint64_t v = 0;
        if (i < n) {
            const uint32_t r = i / k, j = i - r * k;
            const uint64_t p = gathered[(static_cast<size_t>(r) * n_queries + q) * k + j];
            if (p == ~0ull) {
                s_valid_overflow = 1u; // a shard's guard band overflowed: this query has to be redone everywhere
            } else if (p != 0) {
                const uint64_t local = 0xFFFFFFFFull - (p & 0xFFFFFFFFull);
                const uint64_t glob = bases.base[r] + local;
                v = (p & 0xFFFFFFFF00000000ull) | (0xFFFFFFFFull - glob);
                valid++;
            }
        }
        s[i] = v;
    }
    atomicAdd(&s_valid, valid);
    __syncthreads();
    // Every partial list arrives sorted (score desc, row asc; zeros behind) -- that is how sort_emit leaves it -- so an entry's
    // place in the merged order is its index in its own list plus, for every other list, the number of entries there that
    // are greater: world - 1 binary searches of log2(k) steps instead of a sort (a rank sort of the 800 keys of a world-8
    // merge walked ~45 us, a bitonic network of 1024 took ~25 us; this takes ~2).  Keys are unique (the global row is in
    // the low word).  Lists that are NOT sorted (a caller's own data) take the network below.
    __shared__ uint32_t s_unsorted;
    if (threadIdx.x == 0)
        s_unsorted = 0;
    __syncthreads();
    for (uint32_t i = threadIdx.x; i + 1 < n; i += 1024)
        if ((i + 1) % k != 0 && s[i] < s[i + 1])
            s_unsorted = 1u;
    __syncthreads();
    if (!s_unsorted) {
        const uint32_t m_out = min(s_valid, k);
        for (uint32_t i = threadIdx.x; i < n; i += 1024) {
            const uint64_t mine = s[i];
            if (mine == 0)
                continue;
            const uint32_t r = i / k;
            uint32_t rank = i - r * k;
            for (uint32_t o = 0; o < world && rank < k; ++o) {
                if (o == r)
                    continue;
                const uint64_t *lst = s + o * k;
                uint32_t lo = 0, hi = k; // first position whose entry is not greater than `mine`
                while (lo < hi) {
                    const uint32_t mid = (lo + hi) >> 1;
                    if (lst[mid] > mine)
                        lo = mid + 1;
                    else
                        hi = mid;
                }
                rank += lo;
            }
            if (rank < m_out) {
                const uint64_t row = 0xFFFFFFFFull - (mine & 0xFFFFFFFFull);
                const float cs = key_score(static_cast<uint32_t>(mine >> 32));
                rows_out[static_cast<size_t>(q) * k + rank] = row;
                cos_out[static_cast<size_t>(q) * k + rank] = cs;
                atomicAdd(&s_chk, result_chk_term(row, rank) + result_chk_term(__builtin_bit_cast(uint32_t, cs), rank + k));
            }
        }
        for (uint32_t i = m_out + threadIdx.x; i < k; i += 1024) { // (the padding behind fewer than k results)
            const float cs = key_score(0u);
            rows_out[static_cast<size_t>(q) * k + i] = ~0ull;
            cos_out[static_cast<size_t>(q) * k + i] = cs;
            atomicAdd(&s_chk, result_chk_term(~0ull, i) + result_chk_term(__builtin_bit_cast(uint32_t, cs), i + k));
        }
        __threadfence_system();
        __syncthreads();
        if (threadIdx.x == 0) {
            const uint32_t cnt = s_valid_overflow ? 0xFFFFFFFFu : m_out;
            n_out[q] = cnt;
            if (flag_out)
                flag_out[q] = (static_cast<uint64_t>(s_chk) << 32) | cnt;
        }
        return;
    } else
    for (uint32_t kk = 2; kk <= n_pad; kk <<= 1) {
        for (uint32_t j = kk >> 1; j > 0; j >>= 1) {
            for (uint32_t i = threadIdx.x; i < n_pad; i += 1024) {
                const uint32_t ixj = i ^ j;
                if (ixj > i) {
                    const uint64_t a = s[i], b = s[ixj];
                    const bool desc = (i & kk) == 0;
                    if (desc ? (a < b) : (a > b)) {
                        s[i] = b;
                        s[ixj] = a;
                    }
                }
            }
            __syncthreads();
        }
    }
    const uint32_t m = min(s_valid, k);
    for (uint32_t i = threadIdx.x; i < k; i += 1024) {
        const uint64_t v = i < m ? s[i] : 0ull;
        const uint64_t row = i < m ? 0xFFFFFFFFull - (v & 0xFFFFFFFFull) : ~0ull;
        const float cs = key_score(static_cast<uint32_t>(v >> 32));
        rows_out[static_cast<size_t>(q) * k + i] = row;
        cos_out[static_cast<size_t>(q) * k + i] = cs;
        atomicAdd(&s_chk, result_chk_term(row, i) + result_chk_term(__builtin_bit_cast(uint32_t, cs), i + k));
    }
    // count | checksum << 32 last, behind a system-scope fence: a host that pre-set the word to kMetaPending polls it and
    // verifies the checksum over the rows and scores it finds in its memory (sort_emit.h: the word can overtake them)
    __threadfence_system();
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t cnt = s_valid_overflow ? 0xFFFFFFFFu : m;
        n_out[q] = cnt;
        if (flag_out)
            flag_out[q] = (static_cast<uint64_t>(s_chk) << 32) | cnt;
    }
}

// The large-candidate path's finish (a guard band that outgrew the 4096-entry LDS sort: dense score distributions under
// the 8-bit nomination, k in the thousands): the k best of n exactly re-scored keys in global memory by one workgroup --
// radix select of the k-th key over the L2-resident list (3-6 passes, histograms in LDS), the winners gathered into LDS,
// sorted, emitted.  One launch where a global bitonic network took log^2(n) of them.
__global__ __launch_bounds__(1024) void topk_global_kernel(const uint64_t *__restrict__ keys, const SelectState *__restrict__ st,
                                                           uint32_t cap, uint64_t *__restrict__ out, uint32_t k)
{
    __shared__ uint64_t s[4096];
    __shared__ uint32_t s_hist[2048];
    __shared__ uint32_t s_pick[3];
    __shared__ uint32_t s_n;
    const uint32_t n = min(st->n_cand, cap);
    if (threadIdx.x == 0)
        s_n = 0;
    __syncthreads();
    uint64_t kth = 0;
    if (n > k)
        kth = lds_kth_key64(keys, n, k, s_hist, s_pick, 1024); // (the helper only needs a pointer; keys are unique)
    for (uint32_t i = threadIdx.x; i < n; i += 1024) {
        const uint64_t v = keys[i];
        if (v >= kth && v != 0) {
            const uint32_t at = atomicAdd(&s_n, 1u);
            if (at < 4096)
                s[at] = v;
        }
    }
    __syncthreads();
    const uint32_t m = min(s_n, 4096u);
    uint32_t n_pad = 1;
    while (n_pad < m)
        n_pad <<= 1;
    for (uint32_t i = m + threadIdx.x; i < n_pad; i += 1024)
        s[i] = 0;
    __syncthreads();
    for (uint32_t kk = 2; kk <= n_pad; kk <<= 1)
        for (uint32_t j = kk >> 1; j > 0; j >>= 1) {
            for (uint32_t i = threadIdx.x; i < n_pad; i += 1024) {
                const uint32_t ixj = i ^ j;
                if (ixj > i) {
                    const uint64_t a = s[i], b = s[ixj];
                    const bool desc = (i & kk) == 0;
                    if (desc ? (a < b) : (a > b)) {
                        s[i] = b;
                        s[ixj] = a;
                    }
                }
            }
            __syncthreads();
        }
    for (uint32_t i = threadIdx.x; i < k; i += 1024)
        out[i] = i < m ? s[i] : 0ull;
}

__global__ void emit_kernel(const uint64_t *__restrict__ packed, uint32_t n, uint64_t *__restrict__ out, uint32_t k)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < k)
        out[i] = i < n ? packed[i] : 0ull;
}

// The list path of a filtered search: the reference-order scores of the filter's rows as sortable keys, zero padding up
// to the power of two the sort / select behind it works on; the count goes where topk_global_kernel reads it.
__global__ __launch_bounds__(256) void pack_list_kernel(const float *__restrict__ vals, const uint32_t *__restrict__ list, uint32_t n,
                                                        uint64_t *__restrict__ packed, uint32_t n_pad, SelectState *__restrict__ st)
{
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n_pad; i += gridDim.x * 256)
        packed[i] = i < n ? pack_result(vals[i], list[i]) : 0ull;
    if (blockIdx.x == 0 && threadIdx.x == 0)
        st->n_cand = n;
}

// f32 rows with an up-to-date image and the opt-in set: the nomination scan reads the binary16 image
static bool scan_over_image(const rlr_index *ix, const Ctx *c)
{
    return ix->image_scan && ix->image_enabled && ix->d_image.get() && ix->dtype == RLR_F32 && !(c && c->no_f16);
}

// ||q||_2 per staged query, rounded up (only the 8-bit nomination band needs it)
static void stage_query_norms(const rlr_index *ix, Ctx *c, const float *queries, uint32_t nq)
{
    if (!ix->q8_enabled)
        return;
    c->q_norm.resize(nq);
    for (uint32_t q = 0; q < nq; ++q) {
        const double s2 = sumsq_f64(queries + static_cast<size_t>(q) * ix->dim, ix->dim);
        c->q_norm[q] = std::isfinite(s2) ? static_cast<float>(std::sqrt(s2) * 1.000001) : 1.0f;
    }
}

// f32 rows with an up-to-date 8-bit copy: the nomination scan reads one byte per element
static bool scan_over_q8(const rlr_index *ix)
{
    return ix->q8_enabled && ix->d_q8.get() && !ix->q8_has_inf;
}

// bytes per element the single-query nomination scan streams (profile accounting)
static uint64_t scan_bytes_per_element(const rlr_index *ix, const Ctx *c)
{
    return scan_over_q8(ix) ? 1 : (ix->dtype == RLR_F16 || scan_over_image(ix, c)) ? 2 : 4;
}

ScanArgs scan_args(const rlr_index *ix, const float *query, float *scores, uint32_t *hist)
{
    ScanArgs sa;
    sa.rows = ix->d_rows.get();
    sa.query = query;
    sa.scores = scores;
    sa.hist = hist;
    sa.n_rows = static_cast<uint32_t>(ix->n_rows);
    sa.dim = ix->dim;
    sa.pitch16 = ix->pitch16;
    sa.dtype = ix->dtype;
    sa.n_cu = ix->n_cu;
    sa.variant = ix->scan_variant;
    return sa;
}

// Will this index's single-query scans take their query in the kernel arguments?  (Then nothing is uploaded in front of
// them: workgroup 0 of the scan leaves the query in the context's device buffer for the kernels behind it.)
static bool scans_take_host_query(const rlr_index *ix, const Ctx *c, const float *h_q)
{
    if (scan_over_q8(ix) || scan_over_image(ix, c) || ix->n_rows == 0)
        return false;
    ScanArgs sa = scan_args(ix, nullptr, nullptr, nullptr);
    sa.query_host = h_q;
    return launch_scan_takes_host_query(sa);
}

hipError_t stage_queries_for_scans(const rlr_index *ix, Ctx *c, const float *h_q, size_t q_bytes, hipStream_t s)
{
    c->h_q_kq = scans_take_host_query(ix, c, h_q) ? h_q : nullptr;
    return c->h_q_kq ? hipSuccess : upload_queries(c, h_q, q_bytes, s);
}

// band for 8-bit-nominated scores of a query of norm q_norm (Cauchy-Schwarz on the stored row error norms)
static float q8_two_eps(const rlr_index *ix, float q_norm, float guard_eps)
{
    const float dflt = rlr_default_guard_eps(ix->dim);
    const float scale = guard_eps > dflt ? guard_eps / dflt : 1.0f;
    const float qn = q_norm * 1.0001f + 1e-30f;
    return 2.0f * (ix->q8_delta * qn + q8_arith_eps(ix->dim, ix->q8_scale_max, qn) + dflt) * scale;
}

// band for image-nominated scores: the nomination bound for the plan's norms, scaled like the caller scaled guard_eps
// (eps = the caller's guard_eps, or the default, times p.scale)
static float image_two_eps(const rlr_index *ix, float eps, const SearchPlan &p)
{
    const float dflt = rlr_default_guard_eps(ix->dim) * p.scale;
    const float scale = eps > dflt ? eps / dflt : 1.0f;
    return 2.0f * nomination_eps(ix->dim, ix->dtype, p.scale, p.norm_sum) * scale;
}

void count_f16_fallbacks(rlr_index *ix, const SearchPlan &p, uint32_t nq, bool batch_f16)
{
    if (p.f16_ok || !(batch_f16 || scan_over_image(ix, nullptr)))
        return;
    std::lock_guard<std::mutex> lk(ix->mu);
    ix->prof.n_f16_range_fallbacks += nq;
}

int32_t check_hist_assert(Ctx *c)
{
    uint32_t *h = static_cast<uint32_t *>(c->h_assert.get());
    if (h && *h) {
        const uint32_t n = *h;
        *h = 0;
        return set_error(RLR_E_INTERNAL, "zero-histogram invariant violated: %u non-zero bins in front of a scan", n);
    }
    return RLR_OK;
}

// ---- the frame every search entry point is built on (index_internal.h) ----------------------------------------------
SearchPlan make_plan(const rlr_index *ix, const float *queries, uint32_t nq, uint32_t k, float guard_eps, bool unordered)
{
    SearchPlan p;
    p.k = static_cast<uint32_t>(std::min<uint64_t>(k, ix->n_rows));
    plan_bands(ix, queries, nq, &p);
    const float eps = (guard_eps >= 0.0f ? guard_eps : rlr_default_guard_eps(ix->dim)) * p.scale;
    p.two_eps = 2.0f * eps;
    p.two_eps_img = image_two_eps(ix, eps, p);
    p.cap = kLdsSortCap;
    p.unordered = unordered;
    return p;
}

void pad_queries(const rlr_index *ix, const float *queries, uint32_t nq, float *h_q)
{
    if (ix->q_pitch != ix->dim)
        std::memset(h_q, 0, static_cast<size_t>(nq) * ix->q_pitch * sizeof(float));
    for (uint32_t q = 0; q < nq; ++q)
        std::memcpy(h_q + static_cast<size_t>(q) * ix->q_pitch, queries + static_cast<size_t>(q) * ix->dim, ix->dim * sizeof(float));
}

void stage_queries(const rlr_index *ix, Ctx *c, const float *queries, uint32_t nq, float *h_q)
{
    pad_queries(ix, queries, nq, h_q);
    stage_query_norms(ix, c, queries, nq);
    c->hist_dirty = true;
}

int32_t stage_call(rlr_index *ix, Ctx *c, const float *queries, uint32_t nq, size_t res_words, bool for_scans, Staged *out)
{
    const size_t q_bytes = static_cast<size_t>(nq) * ix->q_pitch * sizeof(float);
    RLR_TRY(pin_reserve(c, q_bytes + res_words * sizeof(uint64_t)));
    out->h_q = static_cast<float *>(c->h_pin.get());
    out->h_res = reinterpret_cast<uint64_t *>(static_cast<char *>(c->h_pin.get()) + q_bytes);
    stage_queries(ix, c, queries, nq, out->h_q);
    c->h_q_kq = nullptr;
    if (for_scans)
        RLR_HIP(stage_queries_for_scans(ix, c, out->h_q, q_bytes, c->stream));
    else
        RLR_HIP(upload_queries(c, out->h_q, q_bytes, c->stream));
    return RLR_OK;
}

void arm_meta(uint64_t *h_meta, uint32_t nq)
{
    if (wait_mode() != kWaitBlock)
        for (uint32_t q = 0; q < nq; ++q)
            h_meta[q] = kMetaPending;
}

static hipError_t add_stage_ms(Ctx *c, StageMs *t)
{
    float a = 0, b = 0, d = 0;
    hipError_t e = hipEventElapsedTime(&a, c->ev[0], c->ev[1]);
    if (e == hipSuccess)
        e = hipEventElapsedTime(&b, c->ev[1], c->ev[2]);
    if (e == hipSuccess)
        e = hipEventElapsedTime(&d, c->ev[2], c->ev[3]);
    t->scan += a;
    t->select += b;
    t->rescore += d;
    t->total += a + b + d;
    return e;
}

void note_mmr(rlr_index *ix, Ctx *c, uint32_t n_queries)
{
    float ms = 0;
    (void)hipEventElapsedTime(&ms, c->ev[0], c->ev[1]);
    std::lock_guard<std::mutex> lk(ix->mu);
    ix->prof.n_mmr += n_queries;
    ix->prof.mmr_ms += ms;
}

int32_t note_search(rlr_index *ix, Ctx *c, uint32_t nq, uint64_t n_candidates, uint64_t n_retries, bool timed,
                    bool mmr_chain, const StageMs *summed)
{
    StageMs t;
    float mmr_ms = 0;
    hipError_t e = hipSuccess;
    if (timed && summed)
        t = *summed;
    else if (timed)
        e = add_stage_ms(c, &t);
    if (timed && mmr_chain && hipEventElapsedTime(&mmr_ms, c->bev[0], c->bev[1]) != hipSuccess)
        mmr_ms = 0;
    std::unique_lock<std::mutex> lk(ix->mu);
    ix->prof.n_searches += nq;
    ix->prof.n_candidates += n_candidates;
    ix->prof.n_retries += n_retries;
    if (timed) {
        ix->prof.n_scan_launches += nq;
        ix->prof.scan_ms += t.scan;
        ix->prof.select_ms += t.select;
        ix->prof.rescore_ms += t.rescore;
        ix->prof.total_ms += t.total + mmr_ms;
        ix->prof.scan_bytes += static_cast<uint64_t>(nq) * ix->n_rows * ix->dim * scan_bytes_per_element(ix, c);
        if (mmr_chain) {
            ix->prof.n_mmr += nq;
            ix->prof.mmr_ms += mmr_ms;
        }
    }
    lk.unlock();
    RLR_HIP(e);
    return RLR_OK;
}

hipError_t enqueue_query_scan(rlr_index *ix, Ctx *c, uint32_t qi, bool timed, const rlr_filter *f, bool master_rows)
{
    hipStream_t s = c->stream;
    hipError_t e;
    const uint32_t n = static_cast<uint32_t>(ix->n_rows);
    uint32_t *hist1 = c->d_hist.get();
    const float *dq = c->d_query.get() + static_cast<size_t>(qi) * ix->q_pitch;

    if (c->h_assert) {
        hipLaunchKernelGGL(rlr::hist_assert_zero_kernel, dim3(4), dim3(256), 0, s, c->d_hist.get(), 2u * kHistBins,
                           static_cast<uint32_t *>(c->h_assert.get()));
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    if (timed && (e = hipEventRecord(c->ev[0], s)) != hipSuccess) return e;
    ScanArgs sa = scan_args(ix, dq, c->d_scores.get(), hist1);
    sa.query_host = c->h_q_kq ? c->h_q_kq + static_cast<size_t>(qi) * ix->q_pitch : nullptr;
    const bool q8 = !f && !master_rows && scan_over_q8(ix);
    const bool img = !f && !master_rows && !q8 && scan_over_image(ix, c);
    if (f)
        e = launch_scan_masked(sa, f->d_mask.get(), f->n_allowed, s);
    else if (q8)
        e = launch_q8_scan(ix->d_q8.get(), ix->d_q8_scale.get(), n, ix->dim, dq, c->d_scores.get(), hist1, ix->n_cu, s);
    else if (img)
        e = launch_scan_image(ix->d_image.get(), n, ix->dim, dq, c->d_scores.get(), hist1, ix->n_cu, s);
    else
        e = launch_scan(sa, s);
    if (e != hipSuccess) return e;
    if (timed && (e = hipEventRecord(c->ev[1], s)) != hipSuccess) return e;
    return hipSuccess;
}

hipError_t enqueue_query_rest(rlr_index *ix, Ctx *c, uint32_t qi, const SearchPlan &p, uint64_t *d_out_q, uint64_t *d_meta_q,
                              bool timed, bool emit, const PoolArgs *pool, bool *pool_done, bool master_scan)
{
    if (pool_done)
        *pool_done = false;
    hipStream_t s = c->stream;
    hipError_t e;
    const uint32_t n = static_cast<uint32_t>(ix->n_rows);
    uint32_t *hist1 = c->d_hist.get(), *hist2 = c->d_hist.get() + kHistBins;
    SelectState *st = c->d_state.get() + qi;
    const float *dq = c->d_query.get() + static_cast<size_t>(qi) * ix->q_pitch;
    // (master_scan: the scores in front of this tail came from the master rows whatever copies the index keeps -- the masked scan)
    const bool q8 = !master_scan && scan_over_q8(ix);
    const bool img = !master_scan && !q8 && scan_over_image(ix, c);
    const float band = q8 ? q8_two_eps(ix, qi < c->q_norm.size() ? c->q_norm[qi] : 1.0f, p.two_eps * 0.5f)
                          : (img ? p.two_eps_img : p.two_eps);
    // Up to a few million rows the k-th score's digit-1 bin holds a few hundred scores and the tail's one-pass (DIRECT)
    // mode applies: 15 + 8 us at 1.25 M rows where the four launches took 30 + three launch boundaries.  At 10 M rows the
    // bin holds thousands, both forms make two passes over the 40 MB of scores, and the four specialised kernels win
    // (31 us against 15 + 27: their histogram / collect passes run at a third of the registers and LDS).
    const bool fused = ix->fused_tail < 0 ? ix->n_rows <= 4000000ull : ix->fused_tail != 0;
    if (fused && p.cap <= kLdsSortCap && tail_fits(ix->pitch16, ix->dim, ix->dtype)) {
        // two launches (tail.hip): bin search + collect + re-score (or the digit-2 histogram of a crowded bin), then sort + emit
        TailArgs ta;
        ta.scores = c->d_scores.get();
        ta.n = n;
        ta.hist = c->d_hist.get();
        ta.st = st;
        ta.k = p.k;
        ta.cap = p.cap;
        ta.two_eps = band;
        ta.rows = ix->d_rows.get();
        ta.pitch16 = ix->pitch16;
        ta.dim = ix->dim;
        ta.dtype = ix->dtype;
        ta.query = dq;
        ta.packed = c->d_packed.get();
        ta.out = emit ? d_out_q : nullptr;
        ta.meta = d_meta_q;
        ta.unordered = p.unordered;
        ta.pool = emit ? nullptr : pool;
        ta.direct_max = ta.pool ? std::min<uint32_t>(ix->tail_direct_max, 1024u) : ix->tail_direct_max;
        ta.n_cu = ix->n_cu;
        if (pool_done)
            *pool_done = ta.pool != nullptr;
        if ((e = launch_tail_stage1(ta, s)) != hipSuccess) return e;
        if (timed && (e = hipEventRecord(c->ev[2], s)) != hipSuccess) return e;
        if ((e = launch_tail_stage2(ta, s)) != hipSuccess) return e;
        if (timed && (e = hipEventRecord(c->ev[3], s)) != hipSuccess) return e;
        return hipSuccess;
    }
    if ((e = launch_hist2_find1(c->d_scores.get(), n, hist1, hist2, st, p.k, p.cap, ix->n_cu, s)) != hipSuccess) return e;
    if ((e = launch_collect_find2(c->d_scores.get(), n, hist2, st, band, c->d_cand.get(), ix->n_cu, s)) != hipSuccess)
        return e;
    if (timed && (e = hipEventRecord(c->ev[2], s)) != hipSuccess) return e;
    const uint32_t n_max = std::min<uint32_t>(p.cap, kLdsSortCap);
    if (!launch_rescore_staged(ix->d_rows.get(), ix->pitch16, ix->dim, ix->dtype, dq, c->d_cand.get(), st, c->d_packed.get(), n_max,
                               c->d_hist.get(), s, &e)) {
        // rows too large for the staged layout: one lane per candidate, then clear the histograms
        if ((e = launch_rescore(ix->d_rows.get(), ix->pitch16, ix->dim, ix->dtype, dq, c->d_cand.get(), st, c->d_packed.get(), n_max, s)) !=
            hipSuccess)
            return e;
        e = hipMemsetAsync(c->d_hist.get(), 0, 2 * kHistBins * sizeof(uint32_t), s);
    }
    if (e != hipSuccess) return e;
    if (emit) { // (a caller that orders the re-scored candidates itself -- pool_prepare_kernel<true> -- skips this launch)
        hipLaunchKernelGGL(rlr::sort_emit_kernel, dim3(1), dim3(1024), 0, s, c->d_packed.get(), st, d_out_q, p.k, d_meta_q, p.unordered);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    if (timed && (e = hipEventRecord(c->ev[3], s)) != hipSuccess) return e;
    return hipSuccess;
}

hipError_t enqueue_query(rlr_index *ix, Ctx *c, uint32_t qi, const SearchPlan &p, uint64_t *d_out_q, uint64_t *d_meta_q,
                         bool timed, bool emit, const PoolArgs *pool, bool *pool_done)
{
    const hipError_t e = enqueue_query_scan(ix, c, qi, timed);
    return e != hipSuccess ? e : enqueue_query_rest(ix, c, qi, p, d_out_q, d_meta_q, timed, emit, pool, pool_done);
}

// The ending of the exact paths (big_query, the filtered list path): the k best of the exactly scored keys in d_packed
// (cap slots, zero padded) into d_out.
static hipError_t enqueue_order_emit(uint64_t *d_packed, const SelectState *st, uint32_t cap, uint32_t n_valid, uint64_t *d_out,
                                     uint32_t k, hipStream_t s)
{
    if (k <= kLdsSortCap) {
        // second level: the exact keys (st->n_cand of them) are selected and sorted by one workgroup
        hipLaunchKernelGGL(rlr::topk_global_kernel, dim3(1), dim3(1024), 0, s, d_packed, st, cap, d_out, k);
    } else {
        const hipError_t e = launch_sort_desc(d_packed, cap, s);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(rlr::emit_kernel, dim3((k + 255) / 256), dim3(256), 0, s, d_packed, n_valid, d_out, k);
    }
    return hipGetLastError();
}

// Large-candidate path for one query whose band overflowed the LDS sort (massive ties /
// duplicated chunks, or k > kLdsSortCap).  Re-uses the scores still resident from the scan
// only when the query was the last one scanned; otherwise re-scans.
static int32_t big_query(rlr_index *ix, Ctx *c, uint32_t qi, const SearchPlan &p, uint32_t n_cand, bool rescan,
                         uint64_t *d_out_q)
{
    hipStream_t s = c->stream;
    const uint32_t n = static_cast<uint32_t>(ix->n_rows);
    const uint32_t cap = next_pow2(std::max<uint32_t>(n_cand, p.k));
    SearchPlan big = p;
    big.cap = cap;
    RLR_TRY(reserve_cand(c, cap));
    SelectState *st = c->d_state.get() + qi;
    const float *dq = c->d_query.get() + static_cast<size_t>(qi) * ix->q_pitch;
    if (rescan)
        RLR_HIP(launch_scan(scan_args(ix, dq, c->d_scores.get(), nullptr), s));
    // key_lo is still valid in the state; reset the counter and the capacity
    SelectState h;
    RLR_HIP(hipMemcpyAsync(&h, st, sizeof(h), hipMemcpyDeviceToHost, s));
    RLR_HIP(hipStreamSynchronize(s));
    h.n_cand = 0;
    h.cap = cap;
    RLR_HIP(hipMemcpyAsync(st, &h, sizeof(h), hipMemcpyHostToDevice, s));
    RLR_HIP(launch_collect(c->d_scores.get(), n, st, c->d_cand.get(), ix->n_cu, s));
    hipError_t e = hipSuccess;
    const bool second_level = p.k <= kLdsSortCap;
    // (the staged kernel writes the n_cand keys only; the global sort below needs the zero padding up to `cap` that the
    // one-lane kernel writes)
    const bool staged = second_level && launch_rescore_staged(ix->d_rows.get(), ix->pitch16, ix->dim, ix->dtype, dq, c->d_cand.get(), st,
                                                              c->d_packed.get(), cap, nullptr, s, &e);
    RLR_HIP(e);
    if (!staged) // rows too large for the staged layout, or k beyond the one-workgroup finish
        RLR_HIP(launch_rescore(ix->d_rows.get(), ix->pitch16, ix->dim, ix->dtype, dq, c->d_cand.get(), st, c->d_packed.get(), cap, s));
    RLR_HIP(enqueue_order_emit(c->d_packed.get(), st, cap, n_cand, d_out_q, p.k, s));
    RLR_HIP(hipStreamSynchronize(s));
    return RLR_OK;
}

// ---- batched (matrix-core) pipeline ---------------------------------------------------
bool batch_multi_shape(const rlr_index *ix, uint32_t nq, bool coalesced)
{
    if (coalesced && ix->dtype == RLR_F16)
        return nq <= 8 && ix->pitch16 % 32 == 0 && ix->pitch16 / 32 <= 4 && ix->pitch16 * 8 == ix->dim;
    return nq <= 8 && ix->dtype == RLR_F32 && ix->pitch16 % 64 == 0 && ix->pitch16 / 64 <= 4 && ix->pitch16 * 4 == ix->dim;
}

static bool batch_eligible(const rlr_index *ix, uint32_t nq, uint32_t k, bool f16_ok = true, bool coalesced = false)
{
    if (nq < 2 || ix->dim % 128 != 0 || ix->n_rows < 4096 || k * 8 > batch_finish_capacity())
        return false;
    // operands beyond binary16 range: only the f32 shared scan may nominate
    if (!f16_ok && !(batch_multi_shape(ix, nq, coalesced) && !(ix->image_enabled && ix->d_image.get())))
        return false;
    if (ix->batch_min > 0)
        return nq >= ix->batch_min;
    // Cost model from the measured rates: a single-query pipeline streams the
    // rows at ~6.5 TB/s plus ~60 us of fixed cost; a batch of up to 256 queries costs one GEMM pass
    // (~3.7 TB/s over the row-major matrix, ~3 TB/s of binary16 over the nomination image) plus
    // ~0.8 ms for the sample, the per-query selects and the finish kernels.
    const double row_bytes = static_cast<double>(ix->n_rows) * ix->dim * (ix->dtype == RLR_F16 ? 2.0 : 4.0);
    // the single-query scan streams the 8-bit copy / the binary16 image when those are switched on
    const double scan_bytes = static_cast<double>(ix->n_rows) * ix->dim * static_cast<double>(scan_bytes_per_element(ix, nullptr));
    const double t_single = 60e-6 + scan_bytes / 6.2e12;
    const bool image = ix->image_enabled && ix->d_image.get();
    // (over the image, batches of <= 128 queries take the resident-query kernel: ~5 TB/s of binary16)
    const double pass = image ? static_cast<double>(ix->n_rows) * ix->dim * 2.0 / (nq <= 128 ? 5.0e12 : 3.0e12)
                              : row_bytes / 3.7e12;
    const bool multi = batch_multi_shape(ix, nq, coalesced) && !image;
    if (multi) // one VALU pass for all of them + the per-query selects over the materialised scores
        return nq * t_single > 0.3e-3 + row_bytes / 5.5e12 + nq * (static_cast<double>(ix->n_rows) * 12.0 / 3.0e12);
    const double t_batch = 0.8e-3 + pass * ((nq + 255) / 256);
    return nq * t_single > t_batch;
}

int32_t batch_arm(Ctx *c, uint32_t nq, uint32_t fin_cap, uint64_t s_stride, uint32_t rank, uint64_t n)
{
    hipStream_t s = c->stream;
    // (the status words of h_batch start behind d_bstate.capacity() states: all five or none)
    RLR_HIP(reserve_group(Want{c->d_tau, nq}, Want{c->d_bstate, nq}, Want{c->d_bhist, static_cast<size_t>(nq) * 2 * kHistBins},
                          Want{c->d_bstatus, nq}, Want{c->h_batch, static_cast<size_t>(nq) * (sizeof(SelectState) + sizeof(uint32_t))}));
    RLR_HIP(c->d_bcand.reserve(static_cast<uint64_t>(nq) * fin_cap));
    RLR_HIP(c->d_sample.reserve(static_cast<uint64_t>(nq) * s_stride));
    SelectState *h_st = static_cast<SelectState *>(c->h_batch.get());
    for (uint32_t i = 0; i < nq; ++i) {
        std::memset(&h_st[i], 0, sizeof(SelectState));
        h_st[i].k = static_cast<uint32_t>(std::min<uint64_t>(rank, n));
        h_st[i].cap = fin_cap;
    }
    RLR_HIP(hipMemcpyAsync(c->d_bstate.get(), h_st, nq * sizeof(SelectState), hipMemcpyHostToDevice, s));
    RLR_HIP(hipMemsetAsync(c->d_bhist.get(), 0, static_cast<size_t>(nq) * 2 * kHistBins * sizeof(uint32_t), s));
    RLR_HIP(hipMemsetAsync(c->d_bstatus.get(), 0xFF, static_cast<size_t>(nq) * sizeof(uint32_t), s));
    return RLR_OK;
}

// The end of a batched run: the per-query finish (band, reference-order re-score, order, emit) over the candidates the
// select and the nomination left, then ONE copy of the status words (and of the results, when h_res_out is given) and one
// synchronisation.  h_status[q] != 0: the finish handed query q back.  n_cand_out (optional): the candidates the select
// collected per query (the rows at or above its floor), fetched with the same synchronisation.
static int32_t batch_finish(rlr_index *ix, Ctx *c, const float *dq, uint32_t nq, uint32_t k, float two_eps, uint64_t *d_out,
                            std::vector<uint32_t> &h_status, uint64_t *h_res_out, std::vector<uint32_t> *n_cand_out = nullptr)
{
    hipStream_t s = c->stream;
    uint32_t *h_stat = reinterpret_cast<uint32_t *>(static_cast<SelectState *>(c->h_batch.get()) + c->d_bstate.capacity());
    RLR_HIP(launch_batch_finish(ix->d_rows.get(), ix->pitch16, ix->dim, ix->dtype, dq, ix->q_pitch, nq, c->d_bcand.get(), batch_finish_capacity(),
                                c->d_bstate.get(), k, two_eps, d_out, c->d_bstatus.get(), s));
    if (ix->profiling) RLR_HIP(hipEventRecord(c->ev[3], s));
    RLR_HIP(hipMemcpyAsync(h_stat, c->d_bstatus.get(), nq * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    if (h_res_out) // the batch's results ride on the same synchronisation (queries handed back are fetched again by the caller)
        RLR_HIP(hipMemcpyAsync(h_res_out, d_out, static_cast<size_t>(nq) * k * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    SelectState *h_st = static_cast<SelectState *>(c->h_batch.get());
    if (n_cand_out)
        RLR_HIP(hipMemcpyAsync(h_st, c->d_bstate.get(), nq * sizeof(SelectState), hipMemcpyDeviceToHost, s));
    RLR_HIP(hipStreamSynchronize(s));
    h_status.assign(h_stat, h_stat + nq);
    if (n_cand_out) {
        n_cand_out->resize(nq);
        for (uint32_t q = 0; q < nq; ++q)
            (*n_cand_out)[q] = h_st[q].n_cand;
    }
    return RLR_OK;
}

// Runs queries [q0, q0+nq) (already staged in c->d_query) through the GEMM nomination pipeline
// and leaves k packed results per query in d_out; h_status[q] != 0 marks queries the caller must
// re-run through the single-query pipeline.
static int32_t run_batched(rlr_index *ix, Ctx *c, uint32_t q0, uint32_t nq, const SearchPlan &p, uint64_t *d_out,
                    std::vector<uint32_t> &h_status, uint64_t *h_res_out, bool coalesced = false)
{
    hipStream_t s = c->stream;
    const uint32_t n = static_cast<uint32_t>(ix->n_rows);
    const uint32_t fin_cap = batch_finish_capacity();
    const uint32_t n_qblocks = (nq + 255) / 256;
    // 2..8 queries over f32 rows: one VALU pass over the rows for all of them (scan_multi_kernel) instead of the
    // matrix-core pipeline -- about the cost of a single scan, scores in wavefront order (the tight f32 band)
    const bool use_multi = batch_multi_shape(ix, nq, coalesced) && !(ix->image_enabled && ix->d_image.get());
    const float eps_nom = use_multi ? 0.5f * p.two_eps : nomination_eps(ix->dim, ix->dtype, p.scale, p.norm_sum);
    const float two_eps = 2.0f * eps_nom;
    // Sample rows [0, S): the floor for the rest of the corpus is the sample's rank-th score, and S is large enough that
    // the expected number of later rows above it (rank * N / S) stays well inside the per-query candidate capacity.
    // rank = k needs no check afterwards (k sample rows sit at or above the floor) but a sample of k * N * 2.5 / capacity
    // rows, four times what rank = k / 4 has to materialise and radix-select per query.  With rank = k / 4 the count of
    // rows above the floor spreads more (relative deviation 1 / sqrt(rank): 3.3 k +- 0.65 k at rank 25 against a capacity
    // of 8192), and the finish hands a query back when its k-th nominated score lies under the floor's rank
    // (batch_band_kernel; essentially never: it takes fewer than k rows where ~3 k are expected).
    uint32_t rank = std::max<uint32_t>(std::min<uint32_t>(p.k, 16), p.k / 4);
    uint64_t S = (static_cast<uint64_t>(rank) * n * 5 / 2 + fin_cap - 1) / fin_cap;
    S = std::max<uint64_t>(S, std::min<uint64_t>(n, 65536));
    S = (S + 255) / 256 * 256;
    if (S * 2 >= n || use_multi) {
        S = n;
        rank = p.k; // the sample is the corpus: its k-th score is the k-th score
    } else {
        // fewer than k rows above the floor <=> the sample holds `rank` of the corpus' best k - 1 rows, a Poisson(k S / N)
        // count: keep the rank six deviations above that mean (it matters when the 65 536-row minimum makes the sample a
        // large part of a small corpus; at 10 M rows the mean is 0.8)
        const double mean_in_sample = static_cast<double>(p.k) * static_cast<double>(S) / n;
        const uint32_t safe = static_cast<uint32_t>(std::ceil(mean_in_sample + 6.0 * std::sqrt(mean_in_sample) + 6.0));
        rank = std::min<uint32_t>(p.k, std::max(rank, safe));
        static const uint32_t forced = getenv("RLR_BATCH_RANK_FORCE") ? static_cast<uint32_t>(atoi(getenv("RLR_BATCH_RANK_FORCE"))) : 0;
        if (forced) // tests: a rank low enough that queries ARE handed back (too few candidates, or a band below the floor)
            rank = std::min<uint32_t>(p.k, forced);
    }
    const uint64_t s_stride = (S + 3) / 4 * 4;

    // workspace
    const uint64_t qfrag_bytes = static_cast<uint64_t>(n_qblocks) * 256 * ix->dim * 2;
    RLR_HIP(c->d_qfrag.reserve(qfrag_bytes));
    RLR_HIP(c->d_gsync.reserve(256));
    RLR_TRY(batch_arm(c, nq, fin_cap, s_stride, rank, S));

    const float *dq = c->d_query.get() + static_cast<size_t>(q0) * ix->q_pitch;
    const bool timed = ix->profiling;
    if (timed) RLR_HIP(hipEventRecord(c->bev[0], s));
    const bool use_image = ix->image_enabled && ix->d_image.get() && gemm_image_usable(ix->dim);
    const void *image = use_image ? ix->d_image.get() : nullptr;
    // the image stores k in natural order (like binary16 rows); only the direct f32-row loads permute it
    if (use_multi) {
        const ScanArgs sa = scan_args(ix, dq, c->d_sample.get(), nullptr);
        hipError_t e = hipSuccess;
        // (binary16 rows: the same band -- the widening is exact and the products and sums are f32 as in the single-query scan)
        if (!(ix->dtype == RLR_F16 ? launch_scan_multi_f16(sa, ix->q_pitch, nq, s_stride, s, &e)
                                   : launch_scan_multi(sa, ix->q_pitch, nq, s_stride, s, &e)))
            return set_error(RLR_E_INTERNAL, "multi-query scan refused a shape its gate accepted");
        RLR_HIP(e);
    } else {
        RLR_HIP(launch_prep_queries(dq, nq, ix->q_pitch, ix->dim, use_image ? static_cast<int>(RLR_F16) : ix->dtype, c->d_qfrag.get(), s));
        // 1. nominated scores of the sample rows, materialised
        RLR_HIP(launch_gemm_nominate(ix->d_rows.get(), ix->pitch16, ix->dim, ix->dtype, 0, static_cast<uint32_t>(S), c->d_qfrag.get(), nq,
                                     nullptr, nullptr, 0, nullptr, c->d_sample.get(), s_stride, image, s));
    }
    if (timed) RLR_HIP(hipEventRecord(c->bev[1], s));
    // 2. per-query k-th score of the sample -> threshold; the sample's own candidates
    RLR_HIP(launch_batch_select(c->d_sample.get(), static_cast<uint32_t>(S), s_stride, nq, c->d_bhist.get(), c->d_bstate.get(), two_eps,
                                c->d_tau.get(), c->d_bcand.get(), fin_cap, ix->n_cu, s));
    if (timed) RLR_HIP(hipEventRecord(c->bev[2], s));
    const uint32_t rest_begin = static_cast<uint32_t>(S);
    // 3. the rest of the corpus, filtered in the GEMM epilogue
    if (timed) RLR_HIP(hipEventRecord(c->bev[4], s));
    RLR_HIP(launch_gemm_nominate(ix->d_rows.get(), ix->pitch16, ix->dim, ix->dtype, rest_begin, n, c->d_qfrag.get(), nq,
                                 c->d_tau.get(), c->d_bcand.get(), fin_cap, c->d_bstate.get(), nullptr, 0, image, s, c->d_gsync.get()));
    if (timed) RLR_HIP(hipEventRecord(c->bev[3], s));
    // 4. per-query finish: band, reference-order re-score, order, emit
    RLR_TRY(batch_finish(ix, c, dq, nq, p.k, two_eps, d_out, h_status, h_res_out));
    uint64_t fallbacks = 0;
    for (uint32_t v : h_status)
        fallbacks += v != 0;
    {
        std::lock_guard<std::mutex> lk(ix->mu);
        ix->prof.n_batches += 1;
        ix->prof.n_batch_queries += nq;
        ix->prof.n_batch_fallbacks += fallbacks;
        if (!use_image && !use_multi && nq >= 16 && ix->dtype == RLR_F32 && gemm_image_usable(ix->dim))
            ix->prof.n_batches_without_image += 1; // (an image would have halved the bytes this batch streamed)
        if (timed) {
            float prep = 0, sel = 0, g2 = 0, fin = 0;
            (void)hipEventElapsedTime(&prep, c->bev[0], c->bev[1]);
            (void)hipEventElapsedTime(&sel, c->bev[1], c->bev[2]);
            (void)hipEventElapsedTime(&g2, c->bev[2], c->bev[3]);
            (void)hipEventElapsedTime(&fin, c->bev[3], c->ev[3]);
            ix->prof.batch_gemm_ms += prep + g2; // prep is ~us; both GEMM launches are in here
            ix->prof.batch_other_ms += sel + fin;
            const uint64_t opb = (ix->dtype == RLR_F16 || use_image) ? 2 : 4;
            ix->prof.batch_gemm_bytes += static_cast<uint64_t>(n) * ix->dim * opb;
            ix->prof.batch_gemm_flops += 2.0 * nq * static_cast<double>(n) * ix->dim;
            if (!use_multi && rest_begin < n) {
                float mainp = 0;
                (void)hipEventElapsedTime(&mainp, c->bev[4], c->bev[3]);
                ix->prof.batch_main_ms += mainp;
                ix->prof.batch_main_bytes += static_cast<uint64_t>(n - rest_begin) * ix->dim * opb;
                ix->prof.batch_main_flops += 2.0 * nq * static_cast<double>(n - rest_begin) * ix->dim;
            }
        }
    }
    return RLR_OK;
}

int32_t run_search(rlr_index *ix, Ctx *c, const float *queries, uint32_t nq, uint32_t k_req, float guard_eps,
                   uint64_t *d_out_user, SearchPlan *plan_out, const uint64_t **h_results, bool coalesced,
                   uint32_t *n_handed_back)
{
    if (n_handed_back)
        *n_handed_back = 0;
    const SearchPlan p = make_plan(ix, queries, nq, k_req, guard_eps);
    *plan_out = p;
    if (h_results)
        *h_results = nullptr;
    if (p.k == 0 || nq == 0)
        return RLR_OK;
    RLR_TRY(ctx_prepare(ix, c, nq, p));
    const size_t n_res = static_cast<size_t>(nq) * p.k;
    uint64_t *d_out = d_out_user ? d_out_user : c->d_out.get();
    uint64_t *d_meta = c->d_out.get() + n_res; // per-query candidate counts, right behind the context's results

    // stage queries (zero padded to the row pitch); the matrix-core pipeline reads them from device memory
    const bool batched = batch_eligible(ix, nq, p.k, p.f16_ok, coalesced);
    Staged pin;
    RLR_TRY(stage_call(ix, c, queries, nq, n_res + nq, /*for_scans=*/!batched, &pin));
    uint64_t *h_res = pin.h_res, *h_meta = h_res + n_res;
    hipStream_t s = c->stream;
    if (!batched)
        count_f16_fallbacks(ix, p, nq, batch_eligible(ix, nq, p.k));

    const bool timed = ix->profiling;
    StageMs per_query_ms; // (profiling several queries: summed query by query)
    uint64_t n_cand_total = 0, n_retry = 0;
    auto fetch_results = [&](size_t first, size_t count) -> int32_t { // packed results -> pinned host
        if (!d_out_user && count)
            RLR_HIP(hipMemcpyAsync(h_res + first, c->d_out.get() + first, count * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
        return RLR_OK;
    };

    if (batched) {
        // matrix-core path in runs of <= kBatchMaxQueries; queries it hands back (overflow, or
        // fewer than k finite candidates) go through the single-query pipeline below.
        std::vector<uint32_t> redo;
        std::vector<uint32_t> status;
        for (uint32_t q0 = 0; q0 < nq; q0 += kBatchMaxQueries) {
            const uint32_t m = std::min(kBatchMaxQueries, nq - q0);
            RLR_TRY(run_batched(ix, c, q0, m, p, d_out + static_cast<size_t>(q0) * p.k, status,
                                d_out_user ? nullptr : h_res + static_cast<size_t>(q0) * p.k, coalesced));
            for (uint32_t i = 0; i < m; ++i)
                if (status[i] != 0)
                    redo.push_back(q0 + i);
        }
        if (n_handed_back)
            *n_handed_back = static_cast<uint32_t>(redo.size());
        for (uint32_t q : redo) {
            RLR_HIP(enqueue_query(ix, c, q, p, d_out + static_cast<size_t>(q) * p.k, d_meta + q, false));
            RLR_HIP(hipMemcpyAsync(h_meta + q, d_meta + q, sizeof(uint64_t), hipMemcpyDeviceToHost, s));
            RLR_HIP(hipStreamSynchronize(s));
            const uint32_t nc = static_cast<uint32_t>(h_meta[q]);
            if (nc > p.cap || nc > kLdsSortCap) {
                n_retry++;
                RLR_TRY(big_query(ix, c, q, p, nc, /*rescan=*/false, d_out + static_cast<size_t>(q) * p.k));
            }
        }
        if (!redo.empty()) { // (their results changed after the batch's own copy)
            RLR_TRY(fetch_results(0, n_res));
            RLR_HIP(hipStreamSynchronize(s));
        }
        c->hist_dirty = false;
        if (h_results)
            *h_results = h_res;
        return note_search(ix, c, nq, 0, n_retry, /*timed=*/false);
    }

    // Host-bound results: the last kernel of each pipeline writes its k packed results and the candidate
    // count straight into the pinned (device-mapped) host buffer -- no D2H copy operation on the stream.
    const bool host_direct = !d_out_user;
    uint64_t *q_out = host_direct ? h_res : d_out;
    uint64_t *q_meta = h_meta; // the candidate count always goes straight to the host (the overflow check needs it)
    arm_meta(h_meta, nq);
    if (!timed || nq == 1) {
        // (with profiling on, a single query's four events are read after the one final sync)
        for (uint32_t q = 0; q < nq; ++q)
            RLR_HIP(enqueue_query(ix, c, q, p, q_out + static_cast<size_t>(q) * p.k, q_meta + q, timed));
    } else {
        // one query at a time so the four events can be read back per query
        for (uint32_t q = 0; q < nq; ++q) {
            RLR_HIP(enqueue_query(ix, c, q, p, q_out + static_cast<size_t>(q) * p.k, q_meta + q, true));
            RLR_HIP(hipStreamSynchronize(s));
            RLR_HIP(add_stage_ms(c, &per_query_ms));
        }
    }
    if (timed)
        RLR_HIP(hipStreamSynchronize(s)); // (the events are read below)
    else
        RLR_TRY(wait_results(h_meta, host_direct ? h_res : nullptr, nq, p.k, std::min<uint32_t>(p.cap, kLdsSortCap), s,
                             &c->wait_ema));
    RLR_TRY(check_hist_assert(c));
    // band overflow -> large-candidate path (rare: massive exact ties, or k > 4096)
    bool refetch = false;
    for (uint32_t q = 0; q < nq; ++q) {
        const uint32_t nc = static_cast<uint32_t>(h_meta[q]);
        n_cand_total += nc;
        if (nc > p.cap || nc > kLdsSortCap) {
            n_retry++;
            RLR_TRY(big_query(ix, c, q, p, nc, /*rescan=*/nq > 1, q_out + static_cast<size_t>(q) * p.k));
            refetch = !host_direct;
        }
    }
    if (refetch)
        RLR_HIP(hipStreamSynchronize(s));
    c->hist_dirty = false;
    if (h_results)
        *h_results = h_res;
    // (a single profiled query's events are read here, after the one final synchronisation)
    return note_search(ix, c, nq, n_cand_total, n_retry, timed, /*mmr_chain=*/false, nq > 1 ? &per_query_ms : nullptr);
}

int32_t reserve_list(Ctx *c, uint32_t n)
{
    const uint32_t cap = std::max<uint32_t>(next_pow2(n), 1024);
    RLR_HIP(reserve_group(Want{c->d_list, cap}, Want{c->d_vals, cap}));
    return RLR_OK;
}

int32_t upload_list(rlr_index *ix, Ctx *c, const uint64_t *rows, uint32_t n, uint64_t bound)
{
    if (bound == ~0ull)
        bound = ix->n_rows;
    RLR_TRY(reserve_list(c, n));
    RLR_TRY(pin_reserve(c, static_cast<size_t>(n) * 8 + 64));
    uint32_t *h = static_cast<uint32_t *>(c->h_pin.get());
    for (uint32_t i = 0; i < n; ++i) {
        if (rows[i] >= bound)
            return set_error(RLR_E_RANGE, "row %llu out of range (%llu rows)", static_cast<unsigned long long>(rows[i]),
                             static_cast<unsigned long long>(bound));
        h[i] = static_cast<uint32_t>(rows[i]);
    }
    RLR_HIP(hipMemcpyAsync(c->d_list.get(), h, static_cast<size_t>(n) * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    return RLR_OK;
}

void unpack_results(const uint64_t *__restrict__ src, uint32_t take, uint64_t *__restrict__ ro, float *cos_out)
{
    uint32_t *__restrict__ co = reinterpret_cast<uint32_t *>(cos_out);
    for (uint32_t i = 0; i < take; ++i) {
        const uint64_t w = src[i];
        const uint32_t key = static_cast<uint32_t>(w >> 32);
        const uint32_t neg = static_cast<uint32_t>(static_cast<int32_t>(key) >> 31);        // all ones: key of a value >= +0
        const uint32_t bits = key ^ (0xFFFFFFFFu ^ (neg & 0x7FFFFFFFu));                     // key_score(): & 0x7FFFFFFF or ~
        co[i] = key == 0u ? 0x7FC00000u : bits;
        ro[i] = 0xFFFFFFFFu - static_cast<uint32_t>(w);
    }
}

// rlr_search_topk on a context of its own (n_rows > 0, k > 0)
static int32_t search_topk_host(rlr_index *ix, const float *queries, uint32_t n_queries, uint32_t k, float guard_eps, uint64_t *rows_out,
                         float *cos_out, uint32_t *n_out)
{
    CtxLease lease(ix);
    RLR_TRY(ctx_acquire(ix, &lease.c));
    Ctx *c = lease.c;
    SearchPlan p;
    const uint64_t *h = nullptr;
    RLR_TRY(run_search(ix, c, queries, n_queries, k, guard_eps, nullptr, &p, &h));
    if (!h)
        return set_error(RLR_E_INTERNAL, "search produced no result buffer");
    for (uint32_t q = 0; q < n_queries; ++q) {
        n_out[q] = p.k;
        unpack_results(h + static_cast<size_t>(q) * p.k, p.k, rows_out + static_cast<size_t>(q) * k, cos_out + static_cast<size_t>(q) * k);
    }
    return RLR_OK;
}

// ---- filtered search (rlr_search_topk_filtered) ---------------------------------------------------------------------
// Fewer allowed rows than this: the list path (reference-order scores of every allowed row, then a sort or a select).
// From here on: the masked scan and the unfiltered tail.  Measured on the MI355X at 1 M x 768 f32, k = 100, scattered rows
// (tools/bench_filtered.py, DESIGN.md "Row filters"): list / scan 42 / 50 us at 256 rows, 56 / 60 at 8192, 69 / 66 at
// 16 384, 134 / 87 at 65 536 -- the crossover lies near 12 k rows; rounded down to a power of two.
constexpr uint64_t kFilterListMax = 8192;
constexpr uint64_t kFilterListBatchEntries = 1u << 20; // list-path workspace of one run of queries: keys (queries x padded rows) at most
constexpr uint64_t kFilterListBatchQueries = 256;    // ... and queries enqueued back to back behind one synchronisation at most

int32_t check_filter(const rlr_index *ix, const rlr_filter *f)
{
    if (!f)
        return set_error(RLR_E_INVALID, "null filter handle");
    if (f->ix != ix)
        return set_error(RLR_E_INVALID, "the filter was made for another index");
    if (f->mutations != ix->mutations.load(std::memory_order_acquire))
        return set_error(RLR_E_INVALID, "stale filter: the index was mutated after the filter was made (rows may have been renumbered)");
    return RLR_OK;
}

// The list path, and the exact fall-back of the masked scan: every allowed row scored in reference order (no nomination,
// no band), the keys sorted -- or, for k <= 4096, the k best selected and sorted by one workgroup.  The query is in
// c->d_query; p.k <= n_allowed.  The k packed results end up in h_res.
static int32_t filtered_exact_enqueue(rlr_index *ix, Ctx *c, const rlr_filter *f, const SearchPlan &p, uint32_t qi, float *d_vals,
                                      uint64_t *d_packed, uint32_t cap, uint64_t *d_out)
{
    hipStream_t s = c->stream;
    const uint32_t n = static_cast<uint32_t>(f->n_allowed);
    SelectState *st = c->d_state.get() + qi;
    RLR_HIP(launch_score_rows(ix->d_rows.get(), ix->pitch16, ix->dim, ix->dtype, c->d_query.get() + static_cast<size_t>(qi) * ix->q_pitch,
                              f->d_list.get(), n, d_vals, s));
    hipLaunchKernelGGL(rlr::pack_list_kernel, dim3(std::min<uint32_t>((cap + 255) / 256, 1024)), dim3(256), 0, s, d_vals,
                       f->d_list.get(), n, d_packed, cap, st);
    RLR_HIP(hipGetLastError());
    RLR_HIP(enqueue_order_emit(d_packed, st, cap, n, d_out, p.k, s));
    return RLR_OK;
}

static int32_t filtered_exact(rlr_index *ix, Ctx *c, const rlr_filter *f, const SearchPlan &p, uint64_t *h_res)
{
    hipStream_t s = c->stream;
    const uint32_t n = static_cast<uint32_t>(f->n_allowed);
    const uint32_t cap = next_pow2(std::max<uint32_t>(n, p.k));
    RLR_TRY(reserve_list(c, n));
    RLR_TRY(reserve_cand(c, cap));
    RLR_TRY(filtered_exact_enqueue(ix, c, f, p, 0, c->d_vals.get(), c->d_packed.get(), cap, c->d_out.get()));
    RLR_HIP(hipMemcpyAsync(h_res, c->d_out.get(), static_cast<size_t>(p.k) * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    RLR_HIP(hipStreamSynchronize(s));
    return RLR_OK;
}

bool filter_holds(const rlr_filter *f, uint32_t row)
{
    return row < f->index_rows && ((f->h_mask[row >> 6] >> (row & 63)) & 1ull);
}

bool masked_row_among(const rlr_filter *f, const uint64_t *keys, uint32_t n)
{
    for (uint32_t i = 0; f && i < n; ++i)
        if (!filter_holds(f, 0xFFFFFFFFu - static_cast<uint32_t>(keys[i])))
            return true;
    return false;
}

int32_t filtered_query(rlr_index *ix, Ctx *c, const rlr_filter *f, const float *query, uint32_t k, float guard_eps,
                       uint64_t *rows_out, float *cos_out, uint32_t *n_out)
{
    // k is clamped to the allowed rows BEFORE the plan: the histogram of a masked scan counts n_allowed scores
    const SearchPlan p = make_plan(ix, query, 1, static_cast<uint32_t>(std::min<uint64_t>(k, f->n_allowed)), guard_eps);
    RLR_TRY(ctx_prepare(ix, c, 1, p));
    Staged pin;
    RLR_TRY(stage_call(ix, c, query, 1, static_cast<size_t>(p.k) + 1, /*for_scans=*/false, &pin));
    uint64_t *h_res = pin.h_res, *h_meta = h_res + p.k;
    hipStream_t s = c->stream;
    const bool timed = ix->profiling;
    uint64_t n_cand = 0, n_retry = 0;
    if (f->path == 0) {
        RLR_TRY(filtered_exact(ix, c, f, p, h_res));
    } else {
        arm_meta(h_meta, 1);
        RLR_HIP(enqueue_query_scan(ix, c, 0, timed, f));
        RLR_HIP(enqueue_query_rest(ix, c, 0, p, h_res, h_meta, timed, true, nullptr, nullptr, /*master_scan=*/true));
        if (timed)
            RLR_HIP(hipStreamSynchronize(s));
        else
            RLR_TRY(wait_results(h_meta, h_res, 1, p.k, std::min<uint32_t>(p.cap, kLdsSortCap), s, &c->wait_ema));
        RLR_TRY(check_hist_assert(c));
        n_cand = static_cast<uint32_t>(h_meta[0]);
        if (n_cand > p.cap || n_cand > kLdsSortCap) {
            // band overflow (massive ties, k > 4096): the large-candidate path over the masked scores still resident
            n_retry++;
            RLR_TRY(big_query(ix, c, 0, p, static_cast<uint32_t>(n_cand), /*rescan=*/false, h_res));
        }
        if (masked_row_among(f, h_res, p.k)) { // a masked row came back: the exact path
            n_retry++;
            RLR_TRY(filtered_exact(ix, c, f, p, h_res));
        }
    }
    c->hist_dirty = false;
    *n_out = p.k;
    unpack_results(h_res, p.k, rows_out, cos_out);
    return note_search(ix, c, 1, n_cand, n_retry, timed && f->path != 0);
}

int32_t read_forms(rlr_index *ix, uint64_t (rlr_index::*forms)[4], uint64_t counts[4], int32_t reset)
{
    RLR_TRY(check_handle(ix));
    std::lock_guard<std::mutex> lk(ix->mu);
    for (int i = 0; i < 4; ++i) {
        if (counts)
            counts[i] = (ix->*forms)[i];
        if (reset)
            (ix->*forms)[i] = 0;
    }
    return RLR_OK;
}

namespace {

// ---- several queries, inside one filter or a filter each: one shared masked pass ------------------------------------
// Can a query over `f` join a shared pass at all?  Its filter is on the masked-scan path and holds at least k rows (one
// plan, one rank k for the whole chunk), the rows are a shape the kernel serves and k leaves the finish its band.
bool masked_query_joins(const rlr_index *ix, const rlr_filter *f, uint32_t k)
{
    return f->path == 1 && k <= f->n_allowed && batch_multi_shape(ix, 2) && k * 8 <= batch_finish_capacity();
}

// Does a chunk of nq (2..8) queries, query q inside fs[q], take ONE shared masked pass -- with one_filter (every fs[q] the
// same object; k already clamped to its allowed rows) scan_masked_multi_kernel over that filter, else
// scan_masked_scopes_kernel over the union of the scopes?  Every query must be able to join.  RLR_BATCH_MIN decides when
// set.  Else a cost model over the ALLOWED bytes A_q, fitted to the calls measured at 1 M x 768 f32, k = 100:
//   one by one   per query 45 us of launches and its own synchronisation + its OWN A_q / 6.5 TB/s
//                (measured 0.050 / 0.10 / 0.28 / 0.50 ms per query at 0.01 / 0.1 / 0.5 / 1.0 of the rows)
//   shared       100 us for the batched select, the finish and the one synchronisation, 6 us per query and million rows
//                (the select reads an n_rows-long score array per query, sentinels included, whatever the filter allows)
//                and one pass over the bytes of the union at the rate of the Q = 2 / 4 / 8 instance
// and the shared pass must win by 10 %.
// One filter (tools/bench_filtered.py --queries against the parent build, natural and with the pass forced; DESIGN.md
// "Several queries inside one filter" has the table and what was NOT measured): the union is the filter, the pass runs
// at 6.5 / 6.0 / 4.1 TB/s (eight queries are VALU-bound; measured 0.106 / 0.112 / 0.142 ms at 0.01, 0.55 / 0.62 / 0.88
// with every row allowed).  Two queries over a hundredth of the rows measured 3-5 % SLOWER shared and stay one by one,
// as the model has it.
// A filter per query: the union is estimated as min(n_rows, sum of |F_q|) -- exact for disjoint scopes, an upper bound
// otherwise (identical scopes are overestimated nq-fold, which only makes the gate decline earlier) -- so that no call
// popcounts ORed masks.  The pass rates are refitted to the forced leg of tools/bench_scoped.py (MI355X, 1 M x 768 f32,
// k = 100; DESIGN.md "Queries with different scopes in one pass" has the table and what was NOT measured), (whole call -
// fixed costs) per byte of the union, the slower of the disjoint and the overlapping scope sets: 5.5 / 4.8 / 3.8 TB/s --
// a unit reads Q mask words and branches per query and row.  With these no measured configuration is slower than one by
// one, and the gate declines three that the forced pass won: two random halves (20 %: the estimate, every row, exceeds
// the union, three quarters) and 4 / 8 disjoint eighths (9 / 15 %: the one-by-one side, 104 us per query, is below the
// 118 us measured through the Python layer).  The model errs to the parent's path.
bool filtered_batch_eligible(const rlr_index *ix, const rlr_filter *const *fs, uint32_t nq, uint32_t k, bool one_filter)
{
    if (nq < 2 || nq > 8)
        return false;
    for (uint32_t q = 0; q < nq; ++q)
        if (!masked_query_joins(ix, fs[q], k))
            return false;
    if (ix->batch_min > 0)
        return nq >= ix->batch_min;
    double t_single = 0.0, union_rows = 0.0;
    if (one_filter) {
        union_rows = static_cast<double>(fs[0]->n_allowed);
        t_single = nq * (45e-6 + union_rows * ix->dim * 4.0 / 6.5e12);
    } else {
        for (uint32_t q = 0; q < nq; ++q) {
            t_single += 45e-6 + static_cast<double>(fs[q]->n_allowed) * ix->dim * 4.0 / 6.5e12;
            union_rows += static_cast<double>(fs[q]->n_allowed);
        }
        union_rows = std::min(static_cast<double>(ix->n_rows), union_rows);
    }
    const double pass_rate = one_filter ? (nq <= 2 ? 6.5e12 : nq <= 4 ? 6.0e12 : 4.1e12) : (nq <= 2 ? 5.5e12 : nq <= 4 ? 4.8e12 : 3.8e12);
    const double t_shared = 100e-6 + nq * (static_cast<double>(ix->n_rows) * 6e-12) + union_rows * ix->dim * 4.0 / pass_rate;
    return t_single > 1.1 * t_shared;
}

// A chunk of m (2..8) queries, query q inside fs[q], through ONE masked pass (the gate's one_filter says which): the
// queries staged and uploaded once, the pass into c->d_sample (the "sample" is the whole score array: rank = k, as
// run_batched's use_multi branch), the batched select and finish, one result copy and one synchronisation.  k is clamped
// to the smallest scope, so one plan serves the chunk (a filter each: k <= every |F_q| already).  Query q's score array
// is the same whichever pass wrote it.  The hazards filtered_query closes are closed per query: a result holding a row
// its OWN filter masks (k reached allowed rows whose nominated score is NaN: threshold key 0) and a query the finish
// handed back (band overflow, mass ties) are re-run by filtered_query inside that filter -- never by an unfiltered path.
// c->d_hist is not touched (the select's histograms are c->d_bhist, cleared in front of every use).
int32_t masked_batch(rlr_index *ix, Ctx *c, const rlr_filter *const *fs, bool one_filter, const float *queries, uint32_t m,
                     uint32_t k, float guard_eps, uint64_t *rows_out, float *cos_out, uint32_t *n_out)
{
    uint64_t k_plan = k, sum_rows = 0;
    const uint64_t *masks[8] = {};
    for (uint32_t q = 0; q < m; ++q) {
        k_plan = std::min<uint64_t>(k_plan, fs[q]->n_allowed);
        sum_rows += fs[q]->n_allowed;
        masks[q] = fs[q]->d_mask.get();
    }
    const SearchPlan p = make_plan(ix, queries, m, static_cast<uint32_t>(k_plan), guard_eps);
    RLR_TRY(ctx_prepare(ix, c, m, p));
    const size_t n_res = static_cast<size_t>(m) * p.k;
    Staged pin;
    RLR_TRY(stage_call(ix, c, queries, m, n_res, /*for_scans=*/false, &pin));
    uint64_t *h_res = pin.h_res;
    hipStream_t s = c->stream;
    const uint64_t n = ix->n_rows;
    const uint64_t s_stride = (n + 3) / 4 * 4;
    const float two_eps = p.two_eps; // the summation-order band: 2 x (0.5 x two_eps), as run_batched's shared scan
    RLR_TRY(batch_arm(c, m, batch_finish_capacity(), s_stride, p.k, n));
    const bool timed = ix->profiling;
    if (timed) RLR_HIP(hipEventRecord(c->bev[0], s));
    hipError_t e = hipSuccess;
    const ScanArgs sa = scan_args(ix, c->d_query.get(), c->d_sample.get(), nullptr);
    if (one_filter) {
        if (!launch_scan_masked_multi(sa, masks[0], fs[0]->n_allowed, ix->q_pitch, m, s_stride, s, &e))
            return set_error(RLR_E_INTERNAL, "masked multi-query scan refused a shape its gate accepted");
    } else if (!launch_scan_masked_scopes(sa, masks, std::min<uint64_t>(n, sum_rows), ix->q_pitch, m, s_stride, s, &e)) {
        return set_error(RLR_E_INTERNAL, "masked multi-scope scan refused a shape its gate accepted");
    }
    RLR_HIP(e);
    if (timed) RLR_HIP(hipEventRecord(c->bev[1], s));
    RLR_HIP(launch_batch_select(c->d_sample.get(), static_cast<uint32_t>(n), s_stride, m, c->d_bhist.get(), c->d_bstate.get(), two_eps, c->d_tau.get(),
                                c->d_bcand.get(), batch_finish_capacity(), ix->n_cu, s));
    std::vector<uint32_t> status, n_cand;
    RLR_TRY(batch_finish(ix, c, c->d_query.get(), m, p.k, two_eps, c->d_out.get(), status, h_res, &n_cand));
    c->hist_dirty = false;
    std::vector<uint32_t> redo;
    uint64_t n_cand_total = 0; // of the queries served here, as filtered_query reports its own
    for (uint32_t q = 0; q < m; ++q) {
        if (status[q] != 0 || masked_row_among(fs[q], h_res + static_cast<size_t>(q) * p.k, p.k)) {
            redo.push_back(q);
            continue;
        }
        n_out[q] = p.k;
        n_cand_total += n_cand[q];
        unpack_results(h_res + static_cast<size_t>(q) * p.k, p.k, rows_out + static_cast<size_t>(q) * k, cos_out + static_cast<size_t>(q) * k);
    }
    {
        float scan_ms = 0;
        uint64_t union_rows = one_filter ? fs[0]->n_allowed : 0;
        if (timed) {
            (void)hipEventElapsedTime(&scan_ms, c->bev[0], c->bev[1]);
            // the rows the pass read: a filter each, the exact union (profiling is off by default; no call pays this otherwise)
            for (size_t w = 0; !one_filter && w < fs[0]->h_mask.size(); ++w) {
                uint64_t any = 0;
                for (uint32_t q = 0; q < m; ++q)
                    any |= fs[q]->h_mask[w];
                union_rows += static_cast<uint64_t>(__builtin_popcountll(any));
            }
        }
        std::lock_guard<std::mutex> lk(ix->mu);
        ix->prof.n_batches += 1;
        ix->prof.n_batch_queries += m;
        ix->prof.n_batch_fallbacks += redo.size();
        ix->prof.n_searches += m - redo.size(); // (a query handed back is counted by filtered_query)
        ix->prof.n_candidates += n_cand_total;
        if (timed) {
            ix->prof.scan_ms += scan_ms;
            ix->prof.scan_bytes += union_rows * ix->dim * 4;
        }
    }
    // (from here on the pinned buffer and the context are filtered_query's)
    for (uint32_t q : redo)
        RLR_TRY(filtered_query(ix, c, fs[q], queries + static_cast<size_t>(q) * ix->dim, k, guard_eps, rows_out + static_cast<size_t>(q) * k,
                               cos_out + static_cast<size_t>(q) * k, &n_out[q]));
    return RLR_OK;
}

// The list path for a run of m >= 2 queries: score -> pack -> select of every query enqueued back to back on per-query
// slices of the workspace, then one result copy and one synchronisation.  Same kernels, same results as filtered_exact.
int32_t filtered_list_batch(rlr_index *ix, Ctx *c, const rlr_filter *f, const float *queries, uint32_t m, uint32_t k,
                            float guard_eps, uint64_t *rows_out, float *cos_out, uint32_t *n_out)
{
    const SearchPlan p = make_plan(ix, queries, m, static_cast<uint32_t>(std::min<uint64_t>(k, f->n_allowed)), guard_eps);
    RLR_TRY(ctx_prepare(ix, c, m, p));
    const size_t n_res = static_cast<size_t>(m) * p.k;
    Staged pin;
    RLR_TRY(stage_call(ix, c, queries, m, n_res, /*for_scans=*/false, &pin));
    uint64_t *h_res = pin.h_res;
    hipStream_t s = c->stream;
    const uint32_t cap = next_pow2(std::max<uint32_t>(static_cast<uint32_t>(f->n_allowed), p.k));
    RLR_TRY(reserve_list(c, m * cap));
    RLR_TRY(reserve_cand(c, next_pow2(m * cap)));
    for (uint32_t q = 0; q < m; ++q)
        RLR_TRY(filtered_exact_enqueue(ix, c, f, p, q, c->d_vals.get() + static_cast<size_t>(q) * cap, c->d_packed.get() + static_cast<size_t>(q) * cap,
                                       cap, c->d_out.get() + static_cast<size_t>(q) * p.k));
    RLR_HIP(hipMemcpyAsync(h_res, c->d_out.get(), n_res * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    RLR_HIP(hipStreamSynchronize(s));
    c->hist_dirty = false;
    for (uint32_t q = 0; q < m; ++q) {
        n_out[q] = p.k;
        unpack_results(h_res + static_cast<size_t>(q) * p.k, p.k, rows_out + static_cast<size_t>(q) * k, cos_out + static_cast<size_t>(q) * k);
    }
    return note_search(ix, c, m, 0, 0, /*timed=*/false);
}

int32_t filter_finish(rlr_index *ix, std::vector<uint64_t> &&mask, rlr_filter **out)
{
    std::unique_ptr<rlr_filter> f(new (std::nothrow) rlr_filter());
    if (!f)
        return set_error(RLR_E_OOM, "host allocation failed");
    f->ix = ix;
    f->index_rows = ix->n_rows;
    f->mutations = ix->mutations.load(std::memory_order_acquire);
    f->h_mask = std::move(mask);
    std::vector<uint32_t> list;
    for (size_t w = 0; w < f->h_mask.size(); ++w)
        for (uint64_t m = f->h_mask[w]; m; m &= m - 1)
            list.push_back(static_cast<uint32_t>(w * 64 + static_cast<uint32_t>(__builtin_ctzll(m))));
    f->n_allowed = list.size();
    f->path = f->n_allowed < kFilterListMax ? 0 : 1;
    CtxLease lease(ix);
    RLR_TRY(ctx_acquire(ix, &lease.c));
    hipStream_t s = lease.c->stream;
    hipError_t e = f->d_mask.reserve(std::max<size_t>(f->h_mask.size(), 1));
    if (e == hipSuccess)
        e = f->d_list.reserve(std::max<size_t>(list.size(), 1));
    // uploaded on a stream and waited for: the searches that read them run on other, non-blocking streams
    if (e == hipSuccess && !f->h_mask.empty())
        e = hipMemcpyAsync(f->d_mask.get(), f->h_mask.data(), f->h_mask.size() * sizeof(uint64_t), hipMemcpyHostToDevice, s);
    if (e == hipSuccess && !list.empty())
        e = hipMemcpyAsync(f->d_list.get(), list.data(), list.size() * sizeof(uint32_t), hipMemcpyHostToDevice, s);
    if (e == hipSuccess)
        e = hipStreamSynchronize(s);
    if (e != hipSuccess)
        return set_error(e == hipErrorOutOfMemory ? RLR_E_OOM : RLR_E_HIP, "filter upload failed: %s", hipGetErrorString(e));
    *out = f.release();
    return RLR_OK;
}

int32_t filter_create_check(rlr_index *ix, rlr_filter **out)
{
    if (!out)
        return set_error(RLR_E_INVALID, "out is null");
    *out = nullptr;
    if (rlr_device_count() <= 0)
        return set_error(RLR_E_NO_DEVICE, "no HIP device is visible (this library has no CPU path)");
    RLR_TRY(check_handle(ix));
    return use_device(ix);
}

// ---- document column (rlr_index_set_documents ... rlr_index_delete_documents; kernels in docs.hip) ------------------
int32_t docs_entry_check(const rlr_index *ix)
{
    if (rlr_device_count() <= 0)
        return set_error(RLR_E_NO_DEVICE, "no HIP device is visible (this library has no CPU path)");
    RLR_TRY(check_handle(ix));
    return use_device(ix);
}

// the column, created on first use with every row in no document
int32_t ensure_docs(rlr_index *ix)
{
    if (ix->d_docs)
        return RLR_OK;
    RLR_HIP(ix->d_docs.reserve(std::max<uint64_t>(std::max<uint64_t>(ix->cap_rows, ix->n_rows), 1)));
    hipError_t e = launch_docs_fill(ix->d_docs.get(), ix->n_rows, RLR_DOC_NONE, nullptr);
    if (e == hipSuccess)
        e = hipStreamSynchronize(nullptr);
    if (e != hipSuccess)
        ix->d_docs.reset();
    RLR_HIP(e);
    return RLR_OK;
}

// the caller's ids sorted and distinct (what the membership search of docs.hip takes)
int32_t docs_set(const uint32_t *docs, uint32_t n_docs, std::vector<uint32_t> *set)
{
    if (n_docs && !docs)
        return set_error(RLR_E_INVALID, "docs is null");
    set->assign(docs, docs + n_docs);
    std::sort(set->begin(), set->end());
    set->erase(std::unique(set->begin(), set->end()), set->end());
    if (!set->empty() && set->back() == RLR_DOC_NONE)
        return set_error(RLR_E_INVALID, "RLR_DOC_NONE is not a document");
    return RLR_OK;
}

// The device side of one "rows of these documents" pass: the uploaded id set and the counts the scan works on,
// laid out [one count per workgroup of the mask launch | one sum per scan tile | the total].
struct DocsPass {
    DevBuf<uint32_t> d_set, d_scan;
    uint32_t groups = 0, tiles = 0;
    uint32_t *counts() const { return d_scan.get(); }
    uint32_t *tile_sums() const { return d_scan.get() + groups; }
    uint32_t *total() const { return d_scan.get() + groups + tiles; }
};

// Mark the rows of `set` (non-empty; the index has a column and rows) in d_mask, scan the per-workgroup counts and
// wait: *n_marked = rows marked; h_mask (nullable) receives the mask words.  The scanned counts stay in `pass` for the
// scatter launches.
int32_t docs_mark(rlr_index *ix, hipStream_t s, const std::vector<uint32_t> &set, uint64_t *d_mask, DocsPass *pass,
                  uint64_t *h_mask, uint32_t *n_marked)
{
    const uint32_t N = static_cast<uint32_t>(ix->n_rows);
    pass->groups = docs_groups(N);
    pass->tiles = docs_tiles(pass->groups);
    RLR_HIP(pass->d_set.reserve(set.size()));
    RLR_HIP(pass->d_scan.reserve(static_cast<size_t>(pass->groups) + pass->tiles + 1));
    RLR_HIP(hipMemcpyAsync(pass->d_set.get(), set.data(), set.size() * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    RLR_HIP(launch_docs_mask(ix->d_docs.get(), N, pass->d_set.get(), static_cast<uint32_t>(set.size()), d_mask, pass->counts(), s));
    if (h_mask)
        RLR_HIP(hipMemcpyAsync(h_mask, d_mask, static_cast<size_t>((N + 63ull) / 64) * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    RLR_HIP(launch_docs_scan(pass->counts(), pass->groups, pass->tile_sums(), pass->total(), s));
    RLR_HIP(hipMemcpyAsync(n_marked, pass->total(), sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    RLR_HIP(hipStreamSynchronize(s));
    return RLR_OK;
}

// one bounce-buffer step of a deletion on the document column: rows keep[0 .. m) move to [dst_first, dst_first + m)
hipError_t compact_docs_step(rlr_index *ix, const uint32_t *d_keep, uint64_t m, uint64_t dst_first, uint32_t *d_bounce, hipStream_t s)
{
    hipError_t e = launch_docs_gather(ix->d_docs.get(), d_keep, m, d_bounce, s);
    if (e == hipSuccess)
        e = hipMemcpyAsync(ix->d_docs.get() + dst_first, d_bounce, m * sizeof(uint32_t), hipMemcpyDeviceToDevice, s);
    return e;
}

// ---- coalescer: concurrent single-query calls served from shared passes (rlr_index_set_coalescing) ----------------
// A caller that finds no coalescer pipeline running and nothing pending runs today's single-query pipeline at once
// (after linger_us, if set, as the leader of a group others may join meanwhile).  A caller that arrives while one runs
// joins the oldest open group of its guard band, or opens one as its leader.  A group is sealed when it is full or when
// it gets a pipeline slot -- a retiring pipeline hands its slot to the oldest pending group.  The leader runs the group
// as one multi-query call (run_search -> run_batched: one shared pass, the per-query selects, the finish; queries whose
// band overflows are re-run on the single-query pipeline inside it) and copies each member's prefix into the member's
// buffers.  Everything waits on one condition variable: no polling.
constexpr int kCoalesceInflight = 1; // coalescer pipelines per index (coalescing)

// Would two concurrent single-query calls with this k share a pass?  (Everything else runs today's path at once.)
bool coalesce_eligible(const rlr_index *ix, uint32_t k)
{
    return !ix->image_enabled && !ix->q8_enabled && batch_multi_shape(ix, 2, true) &&
           batch_eligible(ix, 2, std::min<uint64_t>(k, ix->n_rows), true, true);
}

// co_mu held: a retiring pipeline hands its slot to the oldest pending group without one
void coalesce_retire(rlr_index *ix)
{
    ix->co_running--;
    for (auto &g : ix->co_pending)
        if (!g->go && ix->co_running < kCoalesceInflight) {
            g->go = true;
            g->sealed = true;
            ix->co_running++;
        }
    ix->co_cv.notify_all();
}

// the group's queries as one call; every member's results written or g->status set
void coalesce_run(rlr_index *ix, CoalesceGroup *g, float guard_eps)
{
    const uint32_t nq = static_cast<uint32_t>(g->members.size());
    uint32_t kmax = 0;
    for (const CoalesceMember *m : g->members)
        kmax = std::max(kmax, m->k);
    int32_t st = RLR_OK;
    uint32_t handed = 0;
    bool ran = false;
    {
        std::vector<float> qs;
        try {
            qs.resize(static_cast<size_t>(nq) * ix->dim);
        } catch (const std::bad_alloc &) {
            st = set_error(RLR_E_OOM, "host allocation failed");
        }
        for (uint32_t i = 0; st == RLR_OK && i < nq; ++i)
            std::memcpy(qs.data() + static_cast<size_t>(i) * ix->dim, g->members[i]->query, ix->dim * sizeof(float));
        CtxLease lease(ix);
        if (st == RLR_OK)
            st = ctx_acquire(ix, &lease.c);
        SearchPlan p;
        const uint64_t *h = nullptr;
        if (st == RLR_OK)
            st = run_search(ix, lease.c, qs.data(), nq, kmax, guard_eps, nullptr, &p, &h, /*coalesced=*/true, &handed);
        if (st == RLR_OK && !h)
            st = set_error(RLR_E_INTERNAL, "search produced no result buffer");
        if (st == RLR_OK) {
            ran = true;
            for (uint32_t i = 0; i < nq; ++i) {
                CoalesceMember *m = g->members[i];
                const uint32_t take = std::min(m->k, p.k); // a prefix of the group's top-kmax: the order is total
                *m->n_out = take;
                unpack_results(h + static_cast<size_t>(i) * p.k, take, m->rows_out, m->cos_out);
            }
        }
    }
    std::lock_guard<std::mutex> lk(ix->co_mu);
    g->status = st;
    if (st != RLR_OK)
        snprintf(g->msg, sizeof(g->msg), "%s", g_err);
    if (ran) {
        rlr_coalesce_stats &s = ix->co_stats;
        s.n_groups += 1;
        s.n_grouped_queries += nq;
        s.group_size[nq] += 1;
        s.n_groups_f16 += ix->dtype == RLR_F16;
        s.n_handed_back += handed;
    }
}

int32_t coalesced_search(rlr_index *ix, const float *query, uint32_t k, float guard_eps, uint64_t *rows_out, float *cos_out,
                         uint32_t *n_out)
{
    uint32_t key;
    std::memcpy(&key, &guard_eps, sizeof(key));
    CoalesceMember me{query, k, rows_out, cos_out, n_out};
    std::unique_lock<std::mutex> lk(ix->co_mu);
    ix->co_stats.n_calls += 1;
    const uint32_t cap = std::min<uint32_t>(ix->co_max.load(std::memory_order_relaxed), 8);
    for (const std::shared_ptr<CoalesceGroup> &open : ix->co_pending) {
        if (open->sealed || open->key != key)
            continue;
        std::shared_ptr<CoalesceGroup> g = open; // (the leader drops the group from co_pending before it runs it)
        g->members.push_back(&me);
        if (g->members.size() >= g->cap) {
            g->sealed = true;
            ix->co_cv.notify_all(); // a lingering leader launches now
        }
        ix->co_cv.wait(lk, [&] { return g->done; });
        if (g->status != RLR_OK)
            return set_error(g->status, "%s", g->msg);
        return RLR_OK;
    }
    const bool idle = ix->co_running < kCoalesceInflight && ix->co_pending.empty();
    const uint32_t linger_us = ix->co_linger_us;
    if (idle && linger_us == 0) { // nobody to wait for: today's pipeline at once
        ix->co_running++;
        ix->co_stats.n_solo += 1;
        lk.unlock();
        const int32_t st = search_topk_host(ix, query, 1, k, guard_eps, rows_out, cos_out, n_out);
        lk.lock();
        coalesce_retire(ix);
        return st;
    }
    auto g = std::make_shared<CoalesceGroup>();
    g->key = key;
    g->cap = std::max<uint32_t>(cap, 1);
    g->members.push_back(&me);
    g->sealed = g->cap <= 1;
    ix->co_pending.push_back(g);
    const auto deadline = std::chrono::steady_clock::now() + std::chrono::microseconds(linger_us);
    for (;;) {
        if (g->go)
            break;
        // a free slot: a group opened while the index was busy takes it at once, a lingering one once it is full or
        // its linger is over
        const bool ready = !idle || g->sealed || std::chrono::steady_clock::now() >= deadline;
        if (ix->co_running < kCoalesceInflight && ready) {
            g->go = true;
            ix->co_running++;
            break;
        }
        if (idle && !g->sealed && ix->co_running < kCoalesceInflight) {
            // (the deadline is steady; the wait itself is a system_clock one -- pthread_cond_timedwait, which the thread
            // sanitizer's runtime intercepts, where a steady_clock wait becomes pthread_cond_clockwait)
            const auto left = deadline - std::chrono::steady_clock::now();
            ix->co_cv.wait_until(lk, std::chrono::system_clock::now() +
                                         std::chrono::duration_cast<std::chrono::system_clock::duration>(left));
        } else
            ix->co_cv.wait(lk);
    }
    g->sealed = true;
    ix->co_pending.erase(std::find(ix->co_pending.begin(), ix->co_pending.end(), g));
    int32_t st;
    if (g->members.size() == 1) { // nobody joined: today's pipeline
        ix->co_stats.n_solo += 1;
        lk.unlock();
        st = search_topk_host(ix, query, 1, k, guard_eps, rows_out, cos_out, n_out);
        lk.lock();
        g->status = st;
    } else {
        lk.unlock();
        coalesce_run(ix, g.get(), guard_eps);
        lk.lock();
        st = g->status;
    }
    g->done = true;
    coalesce_retire(ix); // (notifies the members too)
    return st;
}

} // namespace

bool coalesce_hands_back(rlr_index *ix, uint32_t k)
{
    if (ix->co_max.load(std::memory_order_relaxed) < 2 || !coalesce_eligible(ix, k))
        return false;
    std::lock_guard<std::mutex> lk(ix->co_mu);
    ix->co_stats.n_engine_handbacks += 1;
    return true;
}

} // namespace rlr

// =====================================================================================
// C ABI
// =====================================================================================
extern "C" {

int32_t rlr_version(void)
{
    return RLR_VERSION;
}

int32_t rlr_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess)
        return 0;
    return n;
}

const char *rlr_last_error(void)
{
    return g_err;
}

float rlr_default_guard_eps(uint32_t dim)
{
    // |seq_sum - tree_sum| <= (dim + reduction depth) * 2^-24 * sum|x_i y_i| <= that * |x||y|
    // for unit-norm operands; 64 covers the 12-deep lane chain + 6 DPP levels with margin,
    // and the final 1/16 absorbs norms that are 1 +- a few ulp.
    return (static_cast<float>(dim) + 64.0f) * 5.9604645e-8f * 1.0625f;
}

int32_t rlr_index_create(uint32_t dim, int32_t dtype, int32_t device_id, rlr_index **out)
{
    if (!out)
        return set_error(RLR_E_INVALID, "out is null");
    *out = nullptr;
    if (dim == 0 || dim > kMaxDim)
        return set_error(RLR_E_INVALID, "dim must be in [1, %u]", kMaxDim);
    if (dtype != RLR_F32 && dtype != RLR_F16)
        return set_error(RLR_E_INVALID, "unknown dtype %d", dtype);
    int n_dev = rlr_device_count();
    if (n_dev <= 0)
        return set_error(RLR_E_NO_DEVICE, "no HIP device is visible (this library has no CPU path)");
    if (device_id < 0 || device_id >= n_dev)
        return set_error(RLR_E_NO_DEVICE, "device %d out of range (%d visible)", device_id, n_dev);
    rlr_index *ix = new (std::nothrow) rlr_index();
    if (!ix)
        return set_error(RLR_E_OOM, "host allocation failed");
    ix->dim = dim;
    ix->dtype = dtype;
    ix->device = device_id;
    const uint32_t elem = dtype == RLR_F16 ? 2 : 4;
    ix->pitch16 = (dim * elem + 15) / 16;
    ix->q_pitch = ix->pitch16 * (16 / elem);
    hipDeviceProp_t prop;
    if (hipSetDevice(device_id) != hipSuccess || hipGetDeviceProperties(&prop, device_id) != hipSuccess) {
        delete ix;
        return set_error(RLR_E_HIP, "cannot query device %d", device_id);
    }
    ix->n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    if (const char *v = getenv("RLR_SCAN_VARIANT"))
        ix->scan_variant = static_cast<int>(strtol(v, nullptr, 0));
    if (const char *v = getenv("RLR_TAIL"))
        ix->fused_tail = v[0] != '0' ? 1 : 0;
    if (const char *v = getenv("RLR_TAIL_DIRECT_MAX"))
        ix->tail_direct_max = static_cast<uint32_t>(std::min<unsigned long>(strtoul(v, nullptr, 0), 4096));
    if (const char *v = getenv("RLR_HYBRID_FETCH"))
        ix->hybrid_fetch_full = !strcmp(v, "full");
    if (const char *v = getenv("RLR_BATCH_MIN"))
        ix->batch_min = static_cast<uint32_t>(strtoul(v, nullptr, 0));
    if (const char *v = getenv("RLR_COMPACT_CHUNK_ROWS"))
        ix->compact_chunk_rows = strtoull(v, nullptr, 0);
    if (const char *v = getenv("RLR_MAX_CONTEXTS"))
        ix->ctx_cap = static_cast<int>(std::min<long>(std::max<long>(strtol(v, nullptr, 0), 1), 64));
    *out = ix;
    return RLR_OK;
}

int32_t rlr_index_destroy(rlr_index *ix)
{
    if (!ix)
        return RLR_OK;
    (void)hipSetDevice(ix->device);
    (void)hipDeviceSynchronize();
    for (Ctx *c : ix->free_ctx)
        ctx_free(c);
    delete ix; // (the rows and the nomination copies free themselves)
    return RLR_OK;
}

int32_t rlr_index_info(const rlr_index *ix, uint64_t *n_rows, uint32_t *dim, int32_t *dtype, int32_t *device_id)
{
    RLR_TRY(check_handle(ix));
    if (n_rows) *n_rows = ix->n_rows;
    if (dim) *dim = ix->dim;
    if (dtype) *dtype = ix->dtype;
    if (device_id) *device_id = ix->device;
    return RLR_OK;
}

int32_t rlr_index_reserve(rlr_index *ix, uint64_t n_rows)
{
    RLR_TRY(check_handle(ix));
    RLR_TRY(use_device(ix));
    return ensure_rows(ix, n_rows);
}

int32_t rlr_index_upload(rlr_index *ix, const float *rows, uint64_t n_rows, int32_t normalize_on_device)
{
    RLR_TRY(check_handle(ix));
    ix->mutations.fetch_add(1, std::memory_order_acq_rel); // (row filters made before this call are stale from here on)
    if (n_rows && !rows)
        return set_error(RLR_E_INVALID, "rows is null");
    RLR_TRY(use_device(ix));
    ix->n_rows = 0;
    ix->d_docs.reset(); // (new rows: the document column goes with the old ones)
    ix->max_row_sumsq = 1.0f;
    ix->f16_overflow = false;
    RLR_TRY(ensure_rows(ix, n_rows));
    RLR_TRY(ingest(ix, rows, n_rows, 0, normalize_on_device));
    ix->n_rows = n_rows;
    return sync_image(ix, 0);
}

int32_t rlr_index_append(rlr_index *ix, const float *rows, uint64_t n_rows, int32_t normalize_on_device,
                         uint64_t *first_row_out)
{
    RLR_TRY(check_handle(ix));
    ix->mutations.fetch_add(1, std::memory_order_acq_rel); // (row filters made before this call are stale from here on)
    if (n_rows && !rows)
        return set_error(RLR_E_INVALID, "rows is null");
    RLR_TRY(use_device(ix));
    const uint64_t first = ix->n_rows;
    RLR_TRY(ensure_rows(ix, first + n_rows));
    RLR_TRY(ingest(ix, rows, n_rows, first, normalize_on_device));
    if (ix->d_docs && n_rows) { // the new rows belong to no document until the host tags them
        RLR_HIP(launch_docs_fill(ix->d_docs.get() + first, n_rows, RLR_DOC_NONE, nullptr));
        RLR_HIP(hipStreamSynchronize(nullptr));
    }
    ix->n_rows = first + n_rows;
    if (first_row_out)
        *first_row_out = first;
    return sync_image(ix, first);
}

int32_t rlr_index_delete_rows(rlr_index *ix, const uint64_t *rows, uint64_t n)
{
    RLR_TRY(check_handle(ix));
    if (n == 0)
        return RLR_OK;
    if (!rows)
        return set_error(RLR_E_INVALID, "rows is null");
    ix->mutations.fetch_add(1, std::memory_order_acq_rel); // (deletion renumbers rows: a filter made before it names other rows now)
    RLR_TRY(use_device(ix));
    const uint64_t N = ix->n_rows;
    std::vector<uint8_t> dead(N, 0);
    for (uint64_t i = 0; i < n; ++i) {
        if (rows[i] >= N)
            return set_error(RLR_E_RANGE, "row %llu out of range (index holds %llu rows)",
                             static_cast<unsigned long long>(rows[i]), static_cast<unsigned long long>(N));
        dead[rows[i]] = 1;
    }
    uint64_t first_dead = 0;
    while (first_dead < N && !dead[first_dead])
        ++first_dead;
    std::vector<uint32_t> keep;
    keep.reserve(N - first_dead);
    for (uint64_t r = first_dead; r < N; ++r)
        if (!dead[r])
            keep.push_back(static_cast<uint32_t>(r));
    // stable in-place compaction through a bounce buffer: destination rows
    // [first_dead + i0, first_dead + i1) only overwrite rows below every source still to move.
    const uint64_t chunk = std::max<uint64_t>(1, (256ull << 20) / row_bytes(ix));
    DevBuf<uint8_t> bounce;
    DevBuf<uint32_t> keep_dev, docs_bounce;
    const uint64_t cr = std::min<uint64_t>(chunk, std::max<size_t>(keep.size(), 1));
    RLR_HIP(bounce.reserve(cr * row_bytes(ix)));
    hipError_t e = keep_dev.reserve(cr);
    if (e == hipSuccess && ix->d_docs)
        e = docs_bounce.reserve(cr);
    if (e != hipSuccess)
        return set_error(RLR_E_OOM, "compaction buffer allocation failed");
    void *const d_bounce = bounce.get();
    uint32_t *const d_keep = keep_dev.get();
    int32_t st = RLR_OK;
    for (uint64_t i0 = 0; i0 < keep.size() && st == RLR_OK; i0 += cr) {
        const uint64_t m = std::min<uint64_t>(cr, keep.size() - i0);
        e = hipMemcpy(d_keep, keep.data() + i0, m * sizeof(uint32_t), hipMemcpyHostToDevice);
        if (e == hipSuccess)
            e = launch_compact_rows(ix->d_rows.get(), d_bounce, ix->pitch16, d_keep, static_cast<uint32_t>(m), nullptr);
        if (e == hipSuccess)
            e = hipMemcpyAsync(static_cast<char *>(ix->d_rows.get()) + (first_dead + i0) * row_bytes(ix), d_bounce,
                               m * row_bytes(ix), hipMemcpyDeviceToDevice, nullptr);
        if (e == hipSuccess && ix->d_docs) // the document column is compacted through the same keep list
            e = compact_docs_step(ix, d_keep, m, first_dead + i0, docs_bounce.get(), nullptr);
        if (e == hipSuccess)
            e = hipStreamSynchronize(nullptr);
        if (e != hipSuccess)
            st = set_error(RLR_E_HIP, "row compaction failed: %s", hipGetErrorString(e));
    }
    if (st == RLR_OK) {
        ix->n_rows = first_dead + keep.size();
        st = sync_image(ix, first_dead);
    }
    return st;
}

int32_t rlr_index_set_documents(rlr_index *ix, const uint32_t *doc_of_row, uint64_t n)
{
    RLR_TRY(docs_entry_check(ix));
    if (n != ix->n_rows)
        return set_error(RLR_E_INVALID, "%llu document ids for an index of %llu rows", static_cast<unsigned long long>(n),
                         static_cast<unsigned long long>(ix->n_rows));
    if (n == 0)
        return RLR_OK;
    if (!doc_of_row)
        return set_error(RLR_E_INVALID, "doc_of_row is null");
    RLR_TRY(ensure_docs(ix));
    RLR_HIP(hipMemcpy(ix->d_docs.get(), doc_of_row, n * sizeof(uint32_t), hipMemcpyHostToDevice));
    return RLR_OK;
}

int32_t rlr_index_tag_rows(rlr_index *ix, uint64_t first, uint64_t count, uint32_t doc)
{
    RLR_TRY(docs_entry_check(ix));
    if (first > ix->n_rows || count > ix->n_rows - first)
        return set_error(RLR_E_RANGE, "rows [%llu, +%llu) out of range (index holds %llu rows)", static_cast<unsigned long long>(first),
                         static_cast<unsigned long long>(count), static_cast<unsigned long long>(ix->n_rows));
    if (count == 0)
        return RLR_OK;
    RLR_TRY(ensure_docs(ix));
    RLR_HIP(launch_docs_fill(ix->d_docs.get() + first, count, doc, nullptr));
    RLR_HIP(hipStreamSynchronize(nullptr));
    return RLR_OK;
}

int32_t rlr_index_get_documents(rlr_index *ix, uint64_t first, uint64_t count, uint32_t *out)
{
    RLR_TRY(docs_entry_check(ix));
    if (first > ix->n_rows || count > ix->n_rows - first)
        return set_error(RLR_E_RANGE, "rows [%llu, +%llu) out of range (index holds %llu rows)", static_cast<unsigned long long>(first),
                         static_cast<unsigned long long>(count), static_cast<unsigned long long>(ix->n_rows));
    if (count == 0)
        return RLR_OK;
    if (!out)
        return set_error(RLR_E_INVALID, "out is null");
    if (!ix->d_docs) {
        std::fill(out, out + count, RLR_DOC_NONE);
        return RLR_OK;
    }
    RLR_HIP(hipMemcpy(out, ix->d_docs.get() + first, count * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return RLR_OK;
}

int32_t rlr_index_delete_documents(rlr_index *ix, const uint32_t *docs, uint32_t n_docs, uint64_t *rows_out, uint64_t cap,
                                   uint64_t *n_deleted)
{
    if (n_deleted)
        *n_deleted = 0;
    RLR_TRY(docs_entry_check(ix));
    if (!n_deleted)
        return set_error(RLR_E_INVALID, "n_deleted is null");
    std::vector<uint32_t> set;
    RLR_TRY(docs_set(docs, n_docs, &set));
    if (set.empty() || !ix->d_docs || ix->n_rows == 0)
        return RLR_OK;
    const uint64_t N = ix->n_rows;
    CtxLease lease(ix);
    RLR_TRY(ctx_acquire(ix, &lease.c));
    hipStream_t s = lease.c->stream;
    // phase 1: mark and count
    DocsPass pass;
    DevBuf<uint64_t> dead_mask;
    RLR_HIP(dead_mask.reserve((N + 63) / 64));
    uint32_t n_dead = 0;
    RLR_TRY(docs_mark(ix, s, set, dead_mask.get(), &pass, nullptr, &n_dead));
    *n_deleted = n_dead;
    if (n_dead == 0)
        return RLR_OK;
    if (n_dead > cap)
        return set_error(RLR_E_RANGE, "%u rows to delete but room for %llu row numbers (nothing was changed)", n_dead,
                         static_cast<unsigned long long>(cap));
    if (!rows_out)
        return set_error(RLR_E_INVALID, "rows_out is null");
    // phase 2: the dead list (the size of a document) comes back; the keep list stays on the device
    DevBuf<uint32_t> dead_list;
    RLR_HIP(dead_list.reserve(n_dead));
    RLR_HIP(launch_docs_scatter(dead_mask.get(), static_cast<uint32_t>(N), pass.counts(), pass.tile_sums(), 0, 0, dead_list.get(), s));
    std::vector<uint32_t> h_dead(n_dead);
    RLR_HIP(hipMemcpyAsync(h_dead.data(), dead_list.get(), n_dead * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    RLR_HIP(hipStreamSynchronize(s));
    const uint64_t first_dead = h_dead[0], n_keep = N - first_dead - n_dead;
    const uint64_t chunk = ix->compact_chunk_rows ? ix->compact_chunk_rows : std::max<uint64_t>(1, (256ull << 20) / row_bytes(ix));
    const uint64_t cr = std::min<uint64_t>(chunk, std::max<uint64_t>(n_keep, 1));
    DevBuf<uint32_t> keep, docs_bounce;
    DevBuf<uint8_t> bounce;
    hipError_t e = keep.reserve(std::max<uint64_t>(n_keep, 1));
    if (e == hipSuccess)
        e = bounce.reserve(cr * row_bytes(ix));
    if (e == hipSuccess)
        e = docs_bounce.reserve(cr);
    if (e != hipSuccess)
        return set_error(RLR_E_OOM, "compaction buffer allocation failed");
    for (uint32_t i = 0; i < n_dead; ++i)
        rows_out[i] = h_dead[i];
    ix->mutations.fetch_add(1, std::memory_order_acq_rel); // (deletion renumbers rows: a filter made before it names other rows now)
    if (n_keep)
        e = launch_docs_scatter(dead_mask.get(), static_cast<uint32_t>(N), pass.counts(), pass.tile_sums(), 1,
                                static_cast<uint32_t>(first_dead), keep.get(), s);
    // stable in-place compaction through a bounce buffer, as in rlr_index_delete_rows: destination rows
    // [first_dead + i0, first_dead + i1) only overwrite rows below every source still to move.  One stream orders the steps.
    for (uint64_t i0 = 0; i0 < n_keep && e == hipSuccess; i0 += cr) {
        const uint64_t m = std::min<uint64_t>(cr, n_keep - i0);
        e = launch_compact_rows(ix->d_rows.get(), bounce.get(), ix->pitch16, keep.get() + i0, static_cast<uint32_t>(m), s);
        if (e == hipSuccess)
            e = hipMemcpyAsync(static_cast<char *>(ix->d_rows.get()) + (first_dead + i0) * row_bytes(ix), bounce.get(),
                               m * row_bytes(ix), hipMemcpyDeviceToDevice, s);
        if (e == hipSuccess)
            e = compact_docs_step(ix, keep.get() + i0, m, first_dead + i0, docs_bounce.get(), s);
    }
    if (e == hipSuccess)
        e = hipStreamSynchronize(s);
    if (e != hipSuccess)
        return set_error(RLR_E_HIP, "row compaction failed: %s", hipGetErrorString(e));
    ix->n_rows = first_dead + n_keep;
    return sync_image(ix, first_dead);
}

int32_t rlr_index_enable_batch_image(rlr_index *ix, int32_t enable)
{
    RLR_TRY(check_handle(ix));
    RLR_TRY(use_device(ix));
    const bool want_image = (enable & 3) != 0, want_q8 = (enable & 4) != 0;
    if (!want_q8 && ix->q8_enabled) {
        ix->q8_enabled = false;
        ix->d_q8.reset();
        ix->d_q8_scale.reset();
    }
    if (!want_image) {
        ix->image_enabled = false;
        ix->image_scan = false;
        ix->d_image.reset();
    }
    if (want_q8 && !ix->q8_enabled) {
        if (ix->dim % 16 != 0 || ix->dim > 2048)
            return set_error(RLR_E_INVALID, "the 8-bit nomination copy needs dim %% 16 == 0, dim <= 2048 (dim = %u)", ix->dim);
        ix->q8_enabled = true;
        RLR_TRY(sync_q8(ix, 0));
    }
    if (want_image) {
        if (ix->dim % 64 != 0)
            return set_error(RLR_E_INVALID, "the nomination image needs dim %% 64 == 0 (dim = %u)", ix->dim);
        ix->image_scan = (enable & 2) != 0;
        if (!(ix->image_enabled && ix->d_image.get())) {
            ix->image_enabled = true;
            const bool q8 = ix->q8_enabled;
            ix->q8_enabled = false; // the 8-bit copy is current: rebuild the image only
            const int32_t st = sync_image(ix, 0);
            ix->q8_enabled = q8;
            RLR_TRY(st);
        }
    }
    return RLR_OK;
}

int32_t rlr_index_fill_synthetic(rlr_index *ix, uint64_t n_rows, uint64_t row0, uint64_t seed, uint32_t n_clusters)
{
    RLR_TRY(check_handle(ix));
    ix->mutations.fetch_add(1, std::memory_order_acq_rel); // (row filters made before this call are stale from here on)
    RLR_TRY(use_device(ix));
    ix->n_rows = 0;
    ix->d_docs.reset(); // (new rows: the document column goes with the old ones)
    RLR_TRY(ensure_rows(ix, n_rows));
    const uint64_t chunk = 1ull << 20;
    DevBuf<float> norm;
    RLR_HIP(norm.reserve(std::min(chunk, std::max<uint64_t>(n_rows, 1))));
    float *const d_norm = norm.get();
    int32_t st = RLR_OK;
    // bit 30: the last n_rows / 100 rows repeat the first n_rows / 100 (exact duplicates)
    const uint64_t n_dup = (n_clusters & 0x40000000u) ? n_rows / 100 : 0;
    const uint64_t seam = n_rows - n_dup; // rows [seam, n_rows) are generator rows [row0, row0 + n_dup) again
    n_clusters &= ~0x40000000u;
    for (uint64_t r0 = 0; r0 < n_rows && st == RLR_OK;) {
        uint64_t m = std::min(chunk, n_rows - r0);
        if (r0 < seam)
            m = std::min(m, seam - r0); // (a launch never straddles the seam)
        const uint64_t src = r0 < seam ? row0 + r0 : row0 + (r0 - seam);
        hipError_t e = launch_synth(static_cast<char *>(ix->d_rows.get()) + r0 * row_bytes(ix), ix->pitch16, ix->dim, ix->dtype,
                                    src, static_cast<uint32_t>(m), seed, n_clusters, d_norm, nullptr);
        if (e == hipSuccess)
            e = hipStreamSynchronize(nullptr);
        if (e != hipSuccess)
            st = set_error(RLR_E_HIP, "synthetic fill failed: %s", hipGetErrorString(e));
        r0 += m;
    }
    if (st == RLR_OK) {
        ix->n_rows = n_rows;
        st = sync_image(ix, 0);
    }
    return st;
}

int32_t rlr_search_topk(rlr_index *ix, const float *queries, uint32_t n_queries, uint32_t k, float guard_eps,
                        uint64_t *rows_out, float *cos_out, uint32_t *n_out)
{
    RLR_TRY(check_handle(ix));
    if (n_queries && (!queries || !n_out))
        return set_error(RLR_E_INVALID, "queries / n_out is null");
    if (n_queries && k && (!rows_out || !cos_out))
        return set_error(RLR_E_INVALID, "output buffers are null");
    RLR_TRY(use_device(ix));
    if (ix->n_rows == 0 || k == 0) {
        for (uint32_t q = 0; q < n_queries; ++q)
            n_out[q] = 0;
        return RLR_OK;
    }
    if (n_queries == 1 && ix->co_max.load(std::memory_order_relaxed) >= 2 && coalesce_eligible(ix, k))
        return coalesced_search(ix, queries, k, guard_eps, rows_out, cos_out, n_out);
    return search_topk_host(ix, queries, n_queries, k, guard_eps, rows_out, cos_out, n_out);
}

int32_t rlr_filter_create_rows(rlr_index *ix, const uint64_t *rows, uint64_t n, rlr_filter **out)
{
    RLR_TRY(filter_create_check(ix, out));
    if (n && !rows)
        return set_error(RLR_E_INVALID, "rows is null");
    std::vector<uint64_t> mask((ix->n_rows + 63) / 64, 0);
    for (uint64_t i = 0; i < n; ++i) {
        if (rows[i] >= ix->n_rows)
            return set_error(RLR_E_RANGE, "row %llu out of range (index holds %llu rows)", static_cast<unsigned long long>(rows[i]),
                             static_cast<unsigned long long>(ix->n_rows));
        mask[rows[i] >> 6] |= 1ull << (rows[i] & 63);
    }
    return filter_finish(ix, std::move(mask), out);
}

int32_t rlr_filter_create_ranges(rlr_index *ix, const uint64_t *first, const uint64_t *count, uint32_t n_ranges, rlr_filter **out)
{
    RLR_TRY(filter_create_check(ix, out));
    if (n_ranges && (!first || !count))
        return set_error(RLR_E_INVALID, "first / count is null");
    std::vector<uint64_t> mask((ix->n_rows + 63) / 64, 0);
    for (uint32_t i = 0; i < n_ranges; ++i) {
        if (count[i] == 0)
            continue;
        if (first[i] >= ix->n_rows || count[i] > ix->n_rows - first[i])
            return set_error(RLR_E_RANGE, "range [%llu, +%llu) out of range (index holds %llu rows)",
                             static_cast<unsigned long long>(first[i]), static_cast<unsigned long long>(count[i]),
                             static_cast<unsigned long long>(ix->n_rows));
        const uint64_t lo = first[i], hi = first[i] + count[i]; // [lo, hi)
        for (uint64_t w = lo >> 6; w <= (hi - 1) >> 6; ++w) {
            const uint64_t b0 = std::max<uint64_t>(lo, w * 64) - w * 64, b1 = std::min<uint64_t>(hi, w * 64 + 64) - w * 64; // bits [b0, b1)
            const uint64_t upto = b1 == 64 ? ~0ull : (1ull << b1) - 1ull;
            mask[w] |= upto & ~((1ull << b0) - 1ull);
        }
    }
    return filter_finish(ix, std::move(mask), out);
}

int32_t rlr_filter_create_documents(rlr_index *ix, const uint32_t *docs, uint32_t n_docs, rlr_filter **out)
{
    RLR_TRY(filter_create_check(ix, out));
    std::vector<uint32_t> set;
    RLR_TRY(docs_set(docs, n_docs, &set));
    const size_t words = (ix->n_rows + 63) / 64;
    if (set.empty() || !ix->d_docs || ix->n_rows == 0) // no document names a row: the empty filter
        return filter_finish(ix, std::vector<uint64_t>(words, 0), out);
    std::unique_ptr<rlr_filter> f(new (std::nothrow) rlr_filter());
    if (!f)
        return set_error(RLR_E_OOM, "host allocation failed");
    f->ix = ix;
    f->index_rows = ix->n_rows;
    f->mutations = ix->mutations.load(std::memory_order_acquire);
    f->h_mask.resize(words);
    RLR_HIP(f->d_mask.reserve(words));
    CtxLease lease(ix);
    RLR_TRY(ctx_acquire(ix, &lease.c));
    hipStream_t s = lease.c->stream;
    // mask words and their count on the device, the mask copied to h_mask as well (the host-side checks read it); the
    // row list is scattered on the device and never built on the host
    DocsPass pass;
    uint32_t n_allowed = 0;
    RLR_TRY(docs_mark(ix, s, set, f->d_mask.get(), &pass, f->h_mask.data(), &n_allowed));
    f->n_allowed = n_allowed;
    f->path = f->n_allowed < kFilterListMax ? 0 : 1;
    RLR_HIP(f->d_list.reserve(std::max<size_t>(n_allowed, 1)));
    if (n_allowed) {
        RLR_HIP(launch_docs_scatter(f->d_mask.get(), static_cast<uint32_t>(ix->n_rows), pass.counts(), pass.tile_sums(), 0, 0,
                                    f->d_list.get(), s));
        RLR_HIP(hipStreamSynchronize(s)); // (the searches that read the list run on other, non-blocking streams)
    }
    *out = f.release();
    return RLR_OK;
}

int32_t rlr_filter_read(const rlr_filter *f, uint64_t *mask_words_out, uint32_t *list_out)
{
    if (rlr_device_count() <= 0)
        return set_error(RLR_E_NO_DEVICE, "no HIP device is visible (this library has no CPU path)");
    if (!f)
        return set_error(RLR_E_INVALID, "null filter handle");
    RLR_TRY(use_device(f->ix));
    const size_t words = (f->index_rows + 63) / 64;
    if (mask_words_out && words)
        RLR_HIP(hipMemcpy(mask_words_out, f->d_mask.get(), words * sizeof(uint64_t), hipMemcpyDeviceToHost));
    if (list_out && f->n_allowed)
        RLR_HIP(hipMemcpy(list_out, f->d_list.get(), f->n_allowed * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return RLR_OK;
}

int32_t rlr_filter_destroy(rlr_filter *f)
{
    if (!f)
        return RLR_OK;
    if (f->ix)
        (void)hipSetDevice(f->ix->device);
    delete f;
    return RLR_OK;
}

int32_t rlr_filter_info(const rlr_filter *f, uint64_t *index_rows, uint64_t *n_allowed, int32_t *path, int32_t *stale)
{
    if (!f)
        return set_error(RLR_E_INVALID, "null filter handle");
    if (index_rows) *index_rows = f->index_rows;
    if (n_allowed) *n_allowed = f->n_allowed;
    if (path) *path = f->path;
    if (stale) *stale = f->mutations != f->ix->mutations.load(std::memory_order_acquire) ? 1 : 0;
    return RLR_OK;
}

int32_t rlr_filter_set_path(rlr_filter *f, int32_t path)
{
    if (!f || (path != 0 && path != 1))
        return set_error(RLR_E_INVALID, "null filter handle, or a path other than 0 / 1");
    f->path = path;
    return RLR_OK;
}

int32_t rlr_search_topk_filtered(rlr_index *ix, const rlr_filter *f, const float *queries, uint32_t n_queries, uint32_t k,
                                 float guard_eps, uint64_t *rows_out, float *cos_out, uint32_t *n_out)
{
    RLR_TRY(check_handle(ix));
    RLR_TRY(check_filter(ix, f)); // (a stale filter is refused before any GPU work)
    if (n_queries && (!queries || !n_out))
        return set_error(RLR_E_INVALID, "queries / n_out is null");
    if (n_queries && k && (!rows_out || !cos_out))
        return set_error(RLR_E_INVALID, "output buffers are null");
    RLR_TRY(use_device(ix));
    for (uint32_t q = 0; q < n_queries; ++q)
        n_out[q] = 0;
    if (f->n_allowed == 0 || k == 0 || n_queries == 0)
        return RLR_OK;
    CtxLease lease(ix);
    RLR_TRY(ctx_acquire(ix, &lease.c));
    StreamDrain drain{lease.c->stream};
    // Chunks of up to 8 queries share one masked pass where the gate says so (filtered_batch_eligible); on the list path
    // runs of queries share one synchronisation; everything else -- binary16 rows, other widths and pitches, a last chunk
    // of one query -- goes query by query.  No matrix-core batch, no coalesced group.
    const uint32_t k_eff = static_cast<uint32_t>(std::min<uint64_t>(k, f->n_allowed));
    const uint32_t list_run = static_cast<uint32_t>(std::min<uint64_t>(
        kFilterListBatchQueries,
        std::max<uint64_t>(1, kFilterListBatchEntries / next_pow2(std::max<uint32_t>(static_cast<uint32_t>(f->n_allowed), k_eff)))));
    const rlr_filter *const fs[8] = {f, f, f, f, f, f, f, f}; // (a chunk's filter per query)
    for (uint32_t q0 = 0; q0 < n_queries;) {
        const float *qs = queries + static_cast<size_t>(q0) * ix->dim;
        uint64_t *ro = rows_out + static_cast<size_t>(q0) * k;
        float *co = cos_out + static_cast<size_t>(q0) * k;
        uint32_t m = std::min<uint32_t>(8, n_queries - q0);
        if (filtered_batch_eligible(ix, fs, m, k_eff, /*one_filter=*/true)) {
            RLR_TRY(masked_batch(ix, lease.c, fs, /*one_filter=*/true, qs, m, k, guard_eps, ro, co, n_out + q0));
        } else if (f->path == 0 && (m = std::min(list_run, n_queries - q0)) >= 2) {
            RLR_TRY(filtered_list_batch(ix, lease.c, f, qs, m, k, guard_eps, ro, co, n_out + q0));
        } else {
            m = 1;
            RLR_TRY(filtered_query(ix, lease.c, f, qs, k, guard_eps, ro, co, &n_out[q0]));
        }
        q0 += m;
    }
    drain.armed = false;
    return RLR_OK;
}

int32_t rlr_search_topk_scoped(rlr_index *ix, const rlr_filter *const *filters, const float *queries, uint32_t n_queries,
                               uint32_t k, float guard_eps, uint64_t *rows_out, float *cos_out, uint32_t *n_out)
{
    if (!filters)
        return set_error(RLR_E_INVALID, "null filter array");
    RLR_TRY(check_handle(ix));
    for (uint32_t q = 0; q < n_queries; ++q)
        RLR_TRY(check_filter(ix, filters[q])); // (null, foreign, stale: every entry, before any GPU work)
    if (n_queries && (!queries || !n_out))
        return set_error(RLR_E_INVALID, "queries / n_out is null");
    if (n_queries && k && (!rows_out || !cos_out))
        return set_error(RLR_E_INVALID, "output buffers are null");
    RLR_TRY(use_device(ix));
    for (uint32_t q = 0; q < n_queries; ++q)
        n_out[q] = 0;
    if (k == 0 || n_queries == 0)
        return RLR_OK;
    CtxLease lease(ix);
    RLR_TRY(ctx_acquire(ix, &lease.c));
    StreamDrain drain{lease.c->stream};
    // The queries that can join a shared pass (masked_query_joins), in call order, in chunks of up to 8: a chunk the gate
    // accepts is one pass over the union of its scopes (or, all filters being one object, the one-filter pass); every
    // other query -- a list-path filter, fewer allowed rows than k, binary16 rows, other widths, a chunk the gate
    // declines, a last chunk of one -- runs alone through filtered_query inside its own filter.
    std::vector<uint32_t> joins;
    for (uint32_t q = 0; q < n_queries; ++q)
        if (masked_query_joins(ix, filters[q], k))
            joins.push_back(q);
    std::vector<char> served(n_queries, 0);
    std::vector<float> qs;
    std::vector<uint64_t> ro;
    std::vector<float> co;
    for (size_t j0 = 0; j0 < joins.size(); j0 += 8) {
        const uint32_t m = static_cast<uint32_t>(std::min<size_t>(8, joins.size() - j0));
        const rlr_filter *fs[8] = {};
        bool same = true;
        for (uint32_t i = 0; i < m; ++i) {
            fs[i] = filters[joins[j0 + i]];
            same = same && fs[i] == fs[0];
        }
        const bool one_filter = same && filtered_batch_eligible(ix, fs, m, k, /*one_filter=*/true);
        if (!one_filter && !filtered_batch_eligible(ix, fs, m, k, /*one_filter=*/false))
            continue;
        qs.resize(static_cast<size_t>(m) * ix->dim);
        ro.resize(static_cast<size_t>(m) * k);
        co.resize(static_cast<size_t>(m) * k);
        uint32_t got[8] = {};
        for (uint32_t i = 0; i < m; ++i)
            std::memcpy(qs.data() + static_cast<size_t>(i) * ix->dim, queries + static_cast<size_t>(joins[j0 + i]) * ix->dim,
                        static_cast<size_t>(ix->dim) * sizeof(float));
        RLR_TRY(masked_batch(ix, lease.c, fs, one_filter, qs.data(), m, k, guard_eps, ro.data(), co.data(), got));
        for (uint32_t i = 0; i < m; ++i) {
            const uint32_t q = joins[j0 + i];
            n_out[q] = got[i];
            std::memcpy(rows_out + static_cast<size_t>(q) * k, ro.data() + static_cast<size_t>(i) * k, static_cast<size_t>(got[i]) * sizeof(uint64_t));
            std::memcpy(cos_out + static_cast<size_t>(q) * k, co.data() + static_cast<size_t>(i) * k, static_cast<size_t>(got[i]) * sizeof(float));
            served[q] = 1;
        }
    }
    for (uint32_t q = 0; q < n_queries; ++q) {
        if (served[q] || filters[q]->n_allowed == 0)
            continue;
        RLR_TRY(filtered_query(ix, lease.c, filters[q], queries + static_cast<size_t>(q) * ix->dim, k, guard_eps,
                               rows_out + static_cast<size_t>(q) * k, cos_out + static_cast<size_t>(q) * k, &n_out[q]));
    }
    drain.armed = false;
    return RLR_OK;
}

int32_t rlr_search_topk_device(rlr_index *ix, const float *queries, uint32_t n_queries, uint32_t k, float guard_eps,
                               void *d_packed_out, void *stream)
{
    RLR_TRY(check_handle(ix));
    if (n_queries && k && (!queries || !d_packed_out))
        return set_error(RLR_E_INVALID, "queries / d_packed_out is null");
    RLR_TRY(use_device(ix));
    if (n_queries == 0 || k == 0)
        return RLR_OK;
    hipStream_t user = static_cast<hipStream_t>(stream);
    if (ix->n_rows == 0) {
        RLR_HIP(hipMemsetAsync(d_packed_out, 0, static_cast<size_t>(n_queries) * k * sizeof(uint64_t), user));
        return RLR_OK;
    }
    CtxLease lease(ix);
    RLR_TRY(ctx_acquire(ix, &lease.c));
    Ctx *c = lease.c;
    SearchPlan p;
    if (k <= ix->n_rows) {
        RLR_TRY(run_search(ix, c, queries, n_queries, k, guard_eps, static_cast<uint64_t *>(d_packed_out), &p, nullptr));
    } else {
        // fewer rows than k: produce the n_rows results, then spread them into k-strided slots
        const uint64_t *h_res = nullptr;
        RLR_TRY(run_search(ix, c, queries, n_queries, k, guard_eps, nullptr, &p, &h_res));
        RLR_HIP(hipMemsetAsync(d_packed_out, 0, static_cast<size_t>(n_queries) * k * sizeof(uint64_t), c->stream));
        RLR_HIP(hipMemcpy2DAsync(d_packed_out, static_cast<size_t>(k) * 8, h_res, static_cast<size_t>(p.k) * 8,
                                 static_cast<size_t>(p.k) * 8, n_queries, hipMemcpyHostToDevice, c->stream));
        RLR_HIP(hipStreamSynchronize(c->stream));
    }
    // run_search has synchronised the context stream, so the results are complete; a later
    // enqueue on `user` is ordered after them.
    (void)user;
    return RLR_OK;
}

// Asynchronous flavour for the sharded step: begin() enqueues the pipelines and makes `stream` wait for
// them, so the caller can queue its collective and merge behind the scan without a host round trip; end()
// joins, reports queries whose guard band overflowed (their slots in d_packed_out are not valid: the caller
// re-runs the step through rlr_search_topk_device) and returns the context.
int32_t rlr_search_topk_device_begin(rlr_index *ix, const float *queries, uint32_t n_queries, uint32_t k, float guard_eps,
                                     void *d_packed_out, void *stream, void **ticket_out)
{
    RLR_TRY(check_handle(ix));
    if (!ticket_out)
        return set_error(RLR_E_INVALID, "ticket_out is null");
    *ticket_out = nullptr;
    if (n_queries && k && (!queries || !d_packed_out))
        return set_error(RLR_E_INVALID, "queries / d_packed_out is null");
    RLR_TRY(use_device(ix));
    // anything but the plain single-query pipelines runs synchronously (ticket stays null)
    const bool timed = ix->profiling; // one query: its four events are read in end()
    if (n_queries == 0 || k == 0 || ix->n_rows == 0 || k > ix->n_rows || (timed && n_queries > 1) ||
        batch_eligible(ix, n_queries, k))
        return rlr_search_topk_device(ix, queries, n_queries, k, guard_eps, d_packed_out, stream);
    Ctx *c = nullptr;
    RLR_TRY(ctx_acquire(ix, &c));
    CtxLease lease(ix);
    lease.c = c; // released on every error path below
    const SearchPlan p = make_plan(ix, queries, n_queries, k, guard_eps);
    RLR_TRY(ctx_prepare(ix, c, n_queries, p));
    count_f16_fallbacks(ix, p, n_queries, false);
    const size_t q_bytes = static_cast<size_t>(n_queries) * ix->q_pitch * sizeof(float);
    RLR_TRY(pin_reserve(c, q_bytes + (static_cast<size_t>(n_queries) * k + n_queries) * sizeof(uint64_t)));
    float *h_q = static_cast<float *>(c->h_pin.get());
    uint64_t *h_meta = reinterpret_cast<uint64_t *>(static_cast<char *>(c->h_pin.get()) + q_bytes) + static_cast<size_t>(n_queries) * k;
    stage_queries(ix, c, queries, n_queries, h_q);
    // The pipelines go on the CALLER's stream: whatever it queues next (all-gather, merge) is ordered behind
    // them by the stream itself.  (A cross-stream event wait was measured first: +20 us per step.)  The
    // context's own stream is idle -- every earlier use of this context ended with a synchronisation.
    hipStream_t own = c->stream;
    c->stream = static_cast<hipStream_t>(stream);
    hipStream_t s = c->stream;
    arm_meta(h_meta, n_queries); // (what _end polls instead of the stream's completion signal)
    hipError_t e = stage_queries_for_scans(ix, c, h_q, q_bytes, s);
    uint64_t *out = static_cast<uint64_t *>(d_packed_out);
    for (uint32_t q = 0; q < n_queries && e == hipSuccess; ++q)
        e = enqueue_query(ix, c, q, p, out + static_cast<size_t>(q) * k, h_meta + q, timed);
    c->stream = own;
    if (e != hipSuccess) {
        // pipelines already enqueued on the caller's stream still use this context's buffers: wait for them before
        // the lease hands the context back to the pool (ctx_acquire's recovery only knows the context's own stream)
        (void)hipStreamSynchronize(s);
        return set_error(RLR_E_HIP, "enqueue on the caller's stream failed: %s", hipGetErrorString(e));
    }
    c->pending_stream = s;
    c->pending_timed = timed;
    c->pending_q = n_queries;
    c->pending_meta = h_meta;
    c->pending_k = k;
    lease.c = nullptr; // the ticket owns the context until end()
    *ticket_out = c;
    return RLR_OK;
}

int32_t rlr_search_topk_device_end(rlr_index *ix, void *ticket, uint32_t *n_overflow_out)
{
    RLR_TRY(check_handle(ix));
    if (n_overflow_out)
        *n_overflow_out = 0;
    if (!ticket)
        return RLR_OK; // begin() ran synchronously
    Ctx *c = static_cast<Ctx *>(ticket);
    CtxLease lease(ix);
    lease.c = c;
    RLR_TRY(use_device(ix));
    if (c->pending_timed)
        RLR_HIP(hipStreamSynchronize(c->pending_stream)); // (the events are read below)
    else // usually already there: whatever the caller queued behind the pipelines and waited for ran after them
        RLR_TRY(wait_results(c->pending_meta, nullptr, c->pending_q, c->pending_k, kLdsSortCap, c->pending_stream, nullptr));
    RLR_TRY(check_hist_assert(c));
    uint32_t over = 0;
    uint64_t n_cand = 0;
    for (uint32_t q = 0; q < c->pending_q; ++q) {
        const uint32_t nc = static_cast<uint32_t>(c->pending_meta[q]);
        n_cand += nc;
        over += nc > kLdsSortCap;
    }
    c->hist_dirty = false;
    RLR_TRY(note_search(ix, c, c->pending_q, n_cand, over, c->pending_timed));
    c->pending_q = 0;
    c->pending_timed = false;
    if (n_overflow_out)
        *n_overflow_out = over;
    return RLR_OK;
}

int32_t rlr_merge_topk(int32_t device_id, const void *d_gathered, uint32_t world, uint32_t n_queries, uint32_t k,
                       const uint64_t *bases, uint64_t *rows_out, float *cos_out, uint32_t *n_out, void *stream)
{
    if (n_queries == 0 || k == 0)
        return RLR_OK;
    if (!d_gathered || !bases || !rows_out || !cos_out || !n_out)
        return set_error(RLR_E_INVALID, "null argument");
    if (world == 0 || world > 16)
        return set_error(RLR_E_INVALID, "world size %u not in [1, 16]", world);
    if (static_cast<uint64_t>(world) * k > 8192)
        return set_error(RLR_E_INVALID, "world * k = %llu exceeds the 8192-entry merge", static_cast<unsigned long long>(world) * k);
    for (uint32_t r = 0; r < world; ++r) // (the merge key holds the global row in 32 bits: corpora of < 2^32 rows)
        if (bases[r] >= 0xFFFFFFFFull)
            return set_error(RLR_E_INVALID, "shard base %llu is not below 2^32 - 1", static_cast<unsigned long long>(bases[r]));
    RLR_HIP(hipSetDevice(device_id));
    // results are written straight into pinned, device-mapped host memory: no D2H copy
    // Freed when the calling thread exits (it used to be leaked).  Intended: a thread's destructors run at its own exit,
    // the main thread's at the start of exit(), both before the HIP runtime's statics go; a thread still alive when the
    // process exits never runs them at all.
    thread_local PinBuf h_pin;
    const size_t nk = static_cast<size_t>(n_queries) * k;
    const size_t need = nk * (sizeof(uint64_t) + sizeof(float)) + n_queries * (sizeof(uint32_t) + sizeof(uint64_t)) + 64;
    RLR_HIP(h_pin.reserve(std::max<size_t>(need, 1 << 16)));
    uint64_t *h_rows = static_cast<uint64_t *>(h_pin.get());
    uint64_t *h_flag = h_rows + nk;
    float *h_cos = reinterpret_cast<float *>(h_flag + n_queries);
    uint32_t *h_n = reinterpret_cast<uint32_t *>(h_cos + nk);
    rlr::MergeBases mb;
    for (uint32_t r = 0; r < 16; ++r)
        mb.base[r] = r < world ? bases[r] : 0;
    hipStream_t s = static_cast<hipStream_t>(stream);
    for (uint32_t q = 0; q < n_queries; ++q)
        h_flag[q] = kMetaPending;
    hipLaunchKernelGGL(rlr::merge_topk_kernel, dim3(n_queries), dim3(1024), 0, s, static_cast<const uint64_t *>(d_gathered),
                       world, n_queries, k, mb, h_rows, h_cos, h_n, h_flag);
    RLR_HIP(hipGetLastError());
    // (this wait usually spans the scans queued in front of the merge on the same stream)
    thread_local WaitEma merge_wait;
    const volatile uint64_t *vf = h_flag;
    const volatile uint64_t *vr = h_rows;
    const volatile uint32_t *vc = reinterpret_cast<const volatile uint32_t *>(h_cos);
    uint32_t verified = n_queries;
    RLR_TRY(wait_polling(
        [&]() {
            while (verified > 0) {
                const uint32_t q = verified - 1;
                const uint64_t m = vf[q];
                if (m == kMetaPending)
                    return false;
                uint32_t chk = 0;
                for (uint32_t i = 0; i < k; ++i)
                    chk += result_chk_term(vr[static_cast<size_t>(q) * k + i], i) +
                           result_chk_term(vc[static_cast<size_t>(q) * k + i], i + k);
                if (chk != static_cast<uint32_t>(m >> 32))
                    return false;
                verified--;
            }
            return true;
        },
        s, &merge_wait, world * 65536u + n_queries));
    std::memcpy(rows_out, h_rows, nk * sizeof(uint64_t));
    std::memcpy(cos_out, h_cos, nk * sizeof(float));
    std::memcpy(n_out, h_n, n_queries * sizeof(uint32_t));
    return RLR_OK;
}

uint64_t rlr_pack_result(float score, uint32_t row)
{
    return pack_result(score, row);
}

void rlr_unpack_result(uint64_t packed, float *score, uint32_t *row)
{
    float s;
    uint32_t r;
    unpack_result(packed, &s, &r);
    if (score) *score = s;
    if (row) *row = r;
}

int32_t rlr_score_rows(rlr_index *ix, const float *query, const uint64_t *rows, uint32_t n, float *cos_out)
{
    RLR_TRY(check_handle(ix));
    if (n == 0)
        return RLR_OK;
    if (!query || !rows || !cos_out)
        return set_error(RLR_E_INVALID, "null argument");
    RLR_TRY(use_device(ix));
    CtxLease lease(ix);
    RLR_TRY(ctx_acquire(ix, &lease.c));
    Ctx *c = lease.c;
    RLR_TRY(upload_list(ix, c, rows, n));
    RLR_TRY(reserve_queries(ix, c, 1));
    RLR_HIP(hipMemcpyAsync(c->d_query.get(), query, ix->dim * sizeof(float), hipMemcpyHostToDevice, c->stream));
    RLR_HIP(launch_score_rows(ix->d_rows.get(), ix->pitch16, ix->dim, ix->dtype, c->d_query.get(), c->d_list.get(), n, c->d_vals.get(),
                              c->stream));
    RLR_HIP(hipMemcpyAsync(cos_out, c->d_vals.get(), static_cast<size_t>(n) * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    RLR_HIP(hipStreamSynchronize(c->stream));
    return RLR_OK;
}

int32_t rlr_fetch_rows(rlr_index *ix, const uint64_t *rows, uint32_t n, float *out)
{
    RLR_TRY(check_handle(ix));
    if (n == 0)
        return RLR_OK;
    if (!rows || !out)
        return set_error(RLR_E_INVALID, "null argument");
    RLR_TRY(use_device(ix));
    CtxLease lease(ix);
    RLR_TRY(ctx_acquire(ix, &lease.c));
    Ctx *c = lease.c;
    RLR_TRY(upload_list(ix, c, rows, n));
    RLR_HIP(c->d_pool.reserve(static_cast<uint64_t>(n) * ix->dim));
    RLR_HIP(launch_gather_f32(ix->d_rows.get(), ix->pitch16, ix->dim, ix->dtype, c->d_list.get(), n, c->d_pool.get(), c->stream));
    RLR_HIP(hipMemcpyAsync(out, c->d_pool.get(), static_cast<size_t>(n) * ix->dim * sizeof(float), hipMemcpyDeviceToHost,
                           c->stream));
    RLR_HIP(hipStreamSynchronize(c->stream));
    return RLR_OK;
}

int32_t rlr_index_row_bytes(const rlr_index *ix, uint32_t *bytes_out)
{
    RLR_TRY(check_handle(ix));
    if (!bytes_out)
        return set_error(RLR_E_INVALID, "bytes_out is null");
    *bytes_out = static_cast<uint32_t>(row_bytes(ix));
    return RLR_OK;
}

int32_t rlr_gather_rows_device(rlr_index *ix, const uint64_t *rows, uint32_t n, void *d_out)
{
    RLR_TRY(check_handle(ix));
    if (n == 0)
        return RLR_OK;
    if (!rows || !d_out)
        return set_error(RLR_E_INVALID, "null argument");
    RLR_TRY(use_device(ix));
    CtxLease lease(ix);
    RLR_TRY(ctx_acquire(ix, &lease.c));
    Ctx *c = lease.c;
    RLR_TRY(upload_list(ix, c, rows, n));
    RLR_HIP(launch_compact_rows(ix->d_rows.get(), d_out, ix->pitch16, c->d_list.get(), n, c->stream));
    RLR_HIP(hipStreamSynchronize(c->stream));
    return RLR_OK;
}

int32_t rlr_fetch_rows_device(rlr_index *ix, const uint64_t *rows, uint32_t n, void *d_out)
{
    RLR_TRY(check_handle(ix));
    if (n == 0)
        return RLR_OK;
    if (!rows || !d_out)
        return set_error(RLR_E_INVALID, "null argument");
    RLR_TRY(use_device(ix));
    CtxLease lease(ix);
    RLR_TRY(ctx_acquire(ix, &lease.c));
    Ctx *c = lease.c;
    RLR_TRY(upload_list(ix, c, rows, n));
    RLR_HIP(launch_gather_f32(ix->d_rows.get(), ix->pitch16, ix->dim, ix->dtype, c->d_list.get(), n, static_cast<float *>(d_out), c->stream));
    RLR_HIP(hipStreamSynchronize(c->stream));
    return RLR_OK;
}

int32_t rlr_index_probe_bandwidth(rlr_index *ix, int32_t mode, uint32_t reps, double *gbps_out, double *ms_out)
{
    RLR_TRY(check_handle(ix));
    if (!gbps_out || mode < 0 || mode > 3)
        return set_error(RLR_E_INVALID, "mode must be 0 (read), 1 (copy), 2 / 3 (the scan kernel without / with its histogram), gbps_out non-null");
    *gbps_out = 0.0;
    if (ms_out)
        *ms_out = 0.0;
    RLR_TRY(use_device(ix));
    const size_t bytes = static_cast<size_t>(ix->n_rows) * row_bytes(ix);
    if (bytes < (1u << 20))
        return set_error(RLR_E_INVALID, "the probe needs at least 1 MiB of rows");
    reps = std::max(reps, 1u);
    CtxLease lease(ix);
    RLR_TRY(ctx_acquire(ix, &lease.c));
    Ctx *c = lease.c;
    hipStream_t s = c->stream;
    DevBuf<uint8_t> scratch_buf;
    int32_t st = RLR_OK;
    double best_ms = 0.0;
    size_t moved = 0;
    auto timed = [&](auto &&launch) -> int32_t { // one warm-up, then `reps` launches between two events
        RLR_HIP(launch());
        RLR_HIP(hipEventRecord(c->ev[0], s));
        for (uint32_t i = 0; i < reps; ++i)
            RLR_HIP(launch());
        RLR_HIP(hipEventRecord(c->ev[1], s));
        RLR_HIP(hipStreamSynchronize(s));
        float ms = 0;
        RLR_HIP(hipEventElapsedTime(&ms, c->ev[0], c->ev[1]));
        const double per = static_cast<double>(ms) / reps;
        if (best_ms == 0.0 || per < best_ms)
            best_ms = per;
        return RLR_OK;
    };
    if (mode == 0) {
        RLR_HIP(scratch_buf.reserve(static_cast<size_t>(ix->n_cu) * 8 * 256 * sizeof(float)));
        void *const scratch = scratch_buf.get();
        moved = bytes / 1024 * 1024;
        for (int shape = 0; shape < 3 && st == RLR_OK; ++shape)
            st = timed([&] { return launch_probe_read(ix->d_rows.get(), bytes, static_cast<float *>(scratch), ix->n_cu, shape, s); });
    } else if (mode >= 2) {
        // diagnostic: the scan kernel itself over the rows with a zero query, scores into a scratch array, without (2) or
        // with (3) the digit-1 histogram it accumulates in LDS and flushes with global atomics
        const size_t sc_bytes = (static_cast<size_t>(ix->n_rows) + 2 * kHistBins + ix->q_pitch) * sizeof(float);
        RLR_HIP(scratch_buf.reserve(sc_bytes));
        void *const scratch = scratch_buf.get();
        RLR_HIP(hipMemsetAsync(scratch, 0, sc_bytes, s));
        float *sc = static_cast<float *>(scratch);
        const ScanArgs sa = scan_args(ix, sc + ix->n_rows + 2 * kHistBins, sc,
                                      mode == 3 ? reinterpret_cast<uint32_t *>(sc + ix->n_rows) : nullptr);
        moved = static_cast<size_t>(ix->n_rows) * ix->dim * (ix->dtype == RLR_F16 ? 2 : 4);
        st = timed([&] { return launch_scan(sa, s); });
    } else {
        const size_t half = std::min<size_t>(bytes / 2, 4ull << 30) & ~static_cast<size_t>(255);
        if (scratch_buf.reserve(half) != hipSuccess)
            return set_error(RLR_E_OOM, "scratch allocation of %zu bytes for the copy probe failed", half);
        void *const scratch = scratch_buf.get();
        moved = 2 * half;
        st = timed([&] { return hipMemcpyAsync(scratch, ix->d_rows.get(), half, hipMemcpyDeviceToDevice, s); });
    }
    (void)hipStreamSynchronize(s);
    if (st != RLR_OK)
        return st;
    *gbps_out = static_cast<double>(moved) / (best_ms * 1e-3) / 1e9;
    if (ms_out)
        *ms_out = best_ms;
    return RLR_OK;
}

int32_t rlr_index_set_coalescing(rlr_index *ix, uint32_t max_group, uint32_t linger_us)
{
    RLR_TRY(check_handle(ix));
    if (max_group > 8)
        return set_error(RLR_E_INVALID, "max_group %u: at most 8 queries share one pass", max_group);
    if (linger_us > 1000000)
        return set_error(RLR_E_INVALID, "linger_us %u: at most 1 s", linger_us);
    {
        std::lock_guard<std::mutex> lk(ix->co_mu);
        ix->co_linger_us = linger_us;
    }
    ix->co_max.store(max_group >= 2 ? max_group : 0, std::memory_order_relaxed);
    return RLR_OK;
}

int32_t rlr_index_coalesce_stats(rlr_index *ix, rlr_coalesce_stats *out, int32_t reset)
{
    RLR_TRY(check_handle(ix));
    if (!out)
        return set_error(RLR_E_INVALID, "out is null");
    std::lock_guard<std::mutex> lk(ix->co_mu);
    *out = ix->co_stats;
    if (reset)
        ix->co_stats = rlr_coalesce_stats{};
    return RLR_OK;
}

int32_t rlr_profile_enable(rlr_index *ix, int32_t enable)
{
    RLR_TRY(check_handle(ix));
    ix->profiling = enable != 0;
    return RLR_OK;
}

int32_t rlr_profile_read(rlr_index *ix, rlr_profile *out, int32_t reset)
{
    RLR_TRY(check_handle(ix));
    if (!out)
        return set_error(RLR_E_INVALID, "out is null");
    std::lock_guard<std::mutex> lk(ix->mu);
    *out = ix->prof;
    if (reset)
        ix->prof = rlr_profile{};
    return RLR_OK;
}

} // extern "C"

namespace rlr {
int32_t filter_view(const rlr_filter *f, FilterView *out)
{
    if (!f)
        return set_error(RLR_E_INVALID, "null filter handle");
    RLR_TRY(check_filter(f->ix, f));
    out->h_mask = f->h_mask.data();
    out->d_mask = f->d_mask.get();
    out->index_rows = f->index_rows;
    out->n_allowed = f->n_allowed;
    out->device = f->ix->device;
    return RLR_OK;
}

int32_t filter_check(const rlr_index *ix, const rlr_filter *f)
{
    return check_filter(ix, f);
}
} // namespace rlr
