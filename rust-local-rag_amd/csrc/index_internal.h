// index_internal.h -- the frame every search entry point of the index is built on, declared once for the translation units
// that implement the C ABI of include/rlr_gpu.h:
//   index.hip           state, ingest, contexts and the waits; the definitions of everything declared here; the plain,
//                       batched and coalesced pipelines; the searches inside a row set (filters, the document column)
//   index_fused.hip     search chains that end in a blend or MMR on the device: MMR, diversified and hybrid search
//   index_grouped.hip   grouped, range and capped search, one query at a time and in chunks behind a shared scan
// A new feature may rely on what this header declares and on nothing else of index.hip.
#pragma once

#include "../../include/rlr_gpu.h"
#include "common.h"
#include "device_buffer.h"
#include "kernels.h"

#include <atomic>
#include <condition_variable>
#include <memory>
#include <mutex>
#include <vector>

#define RLR_HIP(call)                                                                                    \
    do {                                                                                                 \
        hipError_t e_ = (call);                                                                          \
        if (e_ != hipSuccess)                                                                            \
            return set_error(e_ == hipErrorOutOfMemory ? RLR_E_OOM : RLR_E_HIP, "%s failed: %s (%s:%d)", \
                             #call, hipGetErrorString(e_), __FILE__, __LINE__);                          \
    } while (0)

#define RLR_TRY(call)                                                                              \
    do {                                                                                           \
        int32_t s_ = (call);                                                                       \
        if (s_ != RLR_OK)                                                                          \
            return s_;                                                                             \
    } while (0)

namespace rlr {

constexpr uint32_t kLdsSortCap = 4096; // candidates the single-workgroup sort can take
constexpr uint32_t kMaxDim = 8192;
constexpr uint32_t kBatchMaxQueries = 1024; // queries per batched pipeline run (bounds the workspace)

inline uint32_t next_pow2(uint32_t v)
{
    uint32_t p = 1;
    while (p < v)
        p <<= 1;
    return p;
}

// how long the recent waits of one kind took (the hybrid wait sleeps through most of that before it polls)
struct WaitEma {
    double us = 0.0;
    uint32_t key = 0; // what "one kind" means to the caller (number of queries, ...): a change resets the average
};

// -------- per-call context ---------------------------------------------------------
struct Ctx {
    hipStream_t stream = nullptr;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    // device
    // (buffers named together grow together: reserve_group, device_buffer.h)
    DevBuf<float> d_query;         // q x q_pitch floats, with d_state
    DevBuf<float> d_scores;
    DevBuf<uint32_t> d_hist;       // 2 * kHistBins
    DevBuf<SelectState> d_state;   // q states
    DevBuf<uint32_t> d_cand;       // with d_packed
    DevBuf<uint64_t> d_packed;     // (a power of two)
    DevBuf<uint64_t> d_out;        // packed results
    DevBuf<uint32_t> d_list;       // row lists (score_rows / fetch / mmr), with d_vals
    DevBuf<float> d_vals;          // float outputs for lists / mmr
    DevBuf<float> d_pool;          // mmr pool P x dim, then gram P x P
    // batched (MFMA) path workspace
    DevBuf<uint8_t> d_qfrag;        // binary16 fragment-major queries
    DevBuf<float> d_tau;            // per-query nomination threshold; with d_bstate, d_bhist, d_bstatus and h_batch
    DevBuf<SelectState> d_bstate;
    DevBuf<uint32_t> d_bhist;       // q x 2 x kHistBins
    DevBuf<uint32_t> d_bstatus;
    DevBuf<uint32_t> d_gsync;      // 256 words: sibling-group arrival counters of the persistent batched GEMM (gemm.hip)
    PinBuf h_batch;                // SelectState[q] | status[q] (pageable staging makes the async copies synchronous)
    bool no_f16 = false;            // this call's queries or the rows leave binary16 range: no binary16 nomination
    DevBuf<uint64_t> d_bcand;       // q x fin_cap packed candidates
    DevBuf<float> d_sample;         // q x S nominated scores of the sample rows
    hipEvent_t bev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    PinBuf h_pin;                   // staging of a call's queries and results
    std::vector<float> q_norm; // ||q||_2 of the staged queries (band of the 8-bit nomination scan)
    WaitEma wait_ema;          // how long the last waits for a call's completion words took (wait_flags)
    const float *h_q_kq = nullptr; // set for the duration of a call whose scans take their query in the kernel arguments
                                   // (ScanArgs::query_host): the staged queries in pinned host memory, q_pitch floats each
    bool hist_dirty = false; // a pipeline was enqueued and did not complete: d_hist may hold counts
    PinBuf h_assert;         // RLR_POISON_ALLOC=1 only: pinned word the zero-histogram assertion kernel counts into
    // grouped search (group.hip), grown lazily: the document table, t_g per row, the heads' histograms, the candidates
    DevBuf<uint32_t> d_gkeys;      // 1 << bits slots, with d_gvals
    DevBuf<uint64_t> d_gvals;      // slots x per_doc
    DevBuf<uint64_t> d_gtg;        // rows
    DevBuf<uint32_t> d_ghist;      // 2 * kHistBins, with d_gstate, d_gcand and d_gcdoc
    DevBuf<GroupState> d_gstate;
    DevBuf<uint64_t> d_gcand;      // kGroupCap
    DevBuf<uint32_t> d_gcdoc;      // kGroupCap
    DevBuf<uint64_t> d_gout;       // batched grouped search (grouped_batch_chunk): the chunk's result words; the buffers above hold a slice per query
    // range search (range.hip), grown lazily: the two counters and the unordered exact keys of the hits
    DevBuf<RangeState> d_rstate;   // with d_rhits
    DevBuf<uint64_t> d_rhits;      // min(cap, RLR_RANGE_DEVICE_MAX) of the largest call so far
    // batched range search (range_batch_chunk): tau | lo | hi per query, and the chunk's result words
    DevBuf<float> d_rbounds;
    DevBuf<uint64_t> d_rout;
    // rlr_search_topk_device_begin / _end
    hipStream_t pending_stream = nullptr;
    uint32_t pending_q = 0, pending_k = 0;
    bool pending_timed = false;
    const uint64_t *pending_meta = nullptr;
};

// One caller's part in a coalesced group: its query and where its results go (the caller's own buffers; the caller
// blocks until the group is done, so they outlive the group's use of them).
struct CoalesceMember {
    const float *query;
    uint32_t k;
    uint64_t *rows_out;
    float *cos_out;
    uint32_t *n_out;
};

struct CoalesceGroup {
    uint32_t key = 0;      // bits of the members' guard_eps
    uint32_t cap = 0;      // members it takes
    std::vector<CoalesceMember *> members; // [0] is the leader
    bool sealed = false;   // takes no more members
    bool go = false;       // holds a pipeline slot
    bool done = false;     // results written (or status set)
    int32_t status = 0;
    char msg[512] = "";
};

} // namespace rlr

struct rlr_index {
    uint32_t dim = 0;
    int32_t dtype = RLR_F32;
    int32_t device = 0;
    uint32_t pitch16 = 0;   // row pitch in 16-byte units
    uint32_t q_pitch = 0;   // floats per staged query (row pitch in elements)
    uint64_t n_rows = 0;
    uint64_t cap_rows = 0;
    rlr::DevBuf<char> d_rows;    // cap_rows x row_bytes
    rlr::DevBuf<uint32_t> d_docs; // optional document column: one id per row (capacity >= cap_rows), RLR_DOC_NONE = no document;
                             // absent until rlr_index_set_documents / rlr_index_tag_rows
    uint64_t compact_chunk_rows = 0; // RLR_COMPACT_CHUNK_ROWS: rows per bounce-buffer step of rlr_index_delete_documents
                                     // (0: as many as fit in 256 MiB); a test forces several steps on a small index with it
    int n_cu = 256;
    int scan_variant = 0;
    int fused_tail = -1;         // select -> re-score -> sort behind the scan in two launches (tail.hip): RLR_TAIL=1 always, 0 never
                                 // (the five-launch form), unset: while the corpus is small enough for the one-pass mode to be the rule
    uint32_t tail_direct_max = 3584; // RLR_TAIL_DIRECT_MAX: most scores in/above the k-th score's digit-1 bin for the one-pass mode (0: always
                                     // refine).  Re-scoring a few thousand candidates costs less than the two extra passes of the refine
                                     // mode (they spread over the workgroups that found them); 512 slots of the 4096 stay for the guard band.
                                     // A call that builds an MMR pool from the candidates caps it at 1024 (what the pool kernel takes).
    // Hybrid (text) searches: how many rows by cosine the blend asks the tail for beyond the `need` it keeps.  A lexical term
    // only ever ADDS to a row's blended score (weights and BM25 scores are non-negative as a rule), so the need + 8 best
    // cosines already hold every non-lexical row that can reach the pool, whatever the lexical rows among them do; the
    // blend kernel checks that on what it got -- its need-th blended score must beat anything an unfetched row can reach,
    // status 2 and the host's widening path else (a negative lexical weight, a tie across the boundary).  Rounds 2-3
    // fetched need + n_lexical + 8 (every lexical row counted as if it displaced one): 1808 rows instead of 332 for a
    // top-100 text search, a crowded digit-1 bin and ~25 us more tail.  RLR_HYBRID_FETCH=full at creation restores that.
    bool hybrid_fetch_full = false;
    uint32_t batch_min = 0;   // smallest batch that takes the matrix-core path; 0 = decide by the cost model,
                              // RLR_BATCH_MIN=n forces a threshold (a huge n disables the path)
    float max_row_sumsq = 1.0f; // largest sum of squares of a row stored with normalize_on_device = 0 (>= 1): the guard
                                // bands are derived for unit-norm operands and scale with |row| * |query|
    bool f16_overflow = false;  // an f32 row stored as given holds an element outside binary16 range (|x| > 65504):
                                // binary16 nomination would see it as +-Inf (and Inf - Inf = NaN); such rows stay
                                // on the f32 paths until the next upload
    bool image_enabled = false; // keep a binary16 nomination image of the rows for the batched GEMM
    bool image_scan = false;    // single queries nominate over the image too (half the bytes of f32 rows)
    // optional 8-bit nomination copy for single queries (q8.hip): a quarter of the f32 bytes
    bool q8_enabled = false;
    rlr::DevBuf<uint8_t> d_q8;        // cap_rows x dim bytes, with d_q8_scale
    rlr::DevBuf<float> d_q8_scale;    // cap_rows
    rlr::DevBuf<uint32_t> d_q8_stats; // [0] max row error norm (float bits), [1] max scale (float bits), [2] an Inf row exists
    float q8_delta = 0.0f, q8_scale_max = 0.0f;
    bool q8_has_inf = false;
    rlr::DevBuf<uint8_t> d_image;
    std::mutex mu;
    std::condition_variable ctx_cv; // callers beyond ctx_cap wait here for a context to come back
    std::vector<rlr::Ctx *> free_ctx;
    int ctx_made = 0;               // contexts alive (in free_ctx or leased)
    int ctx_cap = 16;               // RLR_MAX_CONTEXTS (1..64)
    bool profiling = false;
    rlr_profile prof{};
    // coalescing of concurrent single-query searches (rlr_index_set_coalescing; the coalescer section of index.hip)
    std::atomic<uint32_t> co_max{0};  // 0: off -- the only thing a single-query call reads when it is
    uint32_t co_linger_us = 0;        // (co_mu)
    std::mutex co_mu;
    std::condition_variable co_cv;    // leaders wait for a pipeline slot / their group to fill, members for their results
    int co_running = 0;               // coalescer pipelines in flight (co_mu)
    std::vector<std::shared_ptr<rlr::CoalesceGroup>> co_pending; // groups waiting for a slot, oldest first (co_mu)
    rlr_coalesce_stats co_stats{};    // (co_mu)
    // bumped by every call that changes which rows the index holds (upload, append, delete_rows, fill_synthetic; load_json
    // goes through upload): a row filter records it at creation and is refused as stale once it has moved on
    std::atomic<uint64_t> mutations{0};
    uint64_t grouped_forms[4] = {0, 0, 0, 0}; // rlr_index_grouped_forms: queries served by each form (mu)
    uint64_t capped_forms[4] = {0, 0, 0, 0};  // rlr_index_capped_forms: the same for rlr_search_capped (mu)
    uint64_t range_forms[4] = {0, 0, 0, 0};   // rlr_index_range_forms: the same for rlr_search_range (mu)
    uint64_t range_batch_forms[4] = {0, 0, 0, 0}; // rlr_index_range_batch_forms: the same for rlr_search_range_batch (mu)
    std::atomic<int32_t> range_sharing{0};    // rlr_index_set_range_sharing: 0 auto (the cost model), 1 never, 2 wherever the shape allows
    uint64_t grouped_batch_forms[4] = {0, 0, 0, 0}; // rlr_index_grouped_batch_forms: queries of rlr_search_topk_grouped_batch by form (mu)
    std::atomic<int32_t> grouped_sharing{0};  // rlr_index_set_grouped_sharing: 0 the gate (grouped_share_wins), 1 never, 2 wherever the shape allows
    uint64_t capped_batch_forms[4] = {0, 0, 0, 0}; // rlr_index_capped_batch_forms: queries of rlr_search_capped_batch by form (mu)
    std::atomic<int32_t> capped_sharing{0};   // rlr_index_set_capped_sharing: 0 the gate (capped_share_wins), 1 never, 2 wherever the shape allows
};

// A set of rows of one index, fixed at creation (rlr_filter_create_*): one bit per index row on the device (tail bits of
// the last word zero) and on the host (the check that no returned row is masked, the engine's row enumeration), the
// allowed rows as an ascending list on the device (the list path, and the exact fall-back of the masked scan), the count.
struct rlr_filter {
    rlr_index *ix = nullptr;
    uint64_t index_rows = 0, n_allowed = 0, mutations = 0;
    int32_t path = 0; // 0: list path, 1: masked scan
    rlr::DevBuf<uint64_t> d_mask;
    rlr::DevBuf<uint32_t> d_list;
    std::vector<uint64_t> h_mask;
};

namespace rlr {

inline size_t row_bytes(const rlr_index *ix)
{
    return static_cast<size_t>(ix->pitch16) * 16;
}

// ---- contexts -----------------------------------------------------------------------------------------------------
int32_t check_handle(const rlr_index *ix);
int32_t use_device(const rlr_index *ix);

// A free context, a new one while fewer than ctx_cap exist, else wait until a call hands one back.  The reference serves
// searches from one tokio worker per core under a read lock (src/main.rs:140, src/mcp_server.rs:89, :377): callers may be
// many, but every context costs a stream, pinned memory and n_rows x 4 B of scores, and more streams than hardware
// queues buy no overlap -- so the pool is bounded like the lexical index' workspaces and the surplus callers queue.
int32_t ctx_acquire(rlr_index *ix, Ctx **out);
void ctx_release(rlr_index *ix, Ctx *c);

struct CtxLease {
    rlr_index *ix;
    Ctx *c = nullptr;
    explicit CtxLease(rlr_index *i) : ix(i) {}
    ~CtxLease()
    {
        if (c)
            ctx_release(ix, c);
    }
};

int32_t pin_reserve(Ctx *c, size_t bytes);
// c->d_query / c->d_state for nq queries
int32_t reserve_queries(const rlr_index *ix, Ctx *c, uint32_t nq);
// c->d_list / c->d_vals for n rows (a power of two, at least 1024)
int32_t reserve_list(Ctx *c, uint32_t n);
int32_t upload_list(rlr_index *ix, Ctx *c, const uint64_t *rows, uint32_t n, uint64_t bound = ~0ull);

// ---- the waits ----------------------------------------------------------------------------------------------------
// The result block of a fused search -> MMR call (sort_emit.h).
int32_t wait_block(const volatile uint32_t *h_out, uint32_t k_cap, hipStream_t s, WaitEma *c);
// The completion words of nq single-query pipelines (sort_emit.h: count | checksum << 32, written last).  res != null:
// the k result words of each query are in host memory too and must match the checksum -- the word alone can overtake
// the results on their way through PCIe.
int32_t wait_results(const volatile uint64_t *meta, const volatile uint64_t *res, uint32_t nq, uint32_t k, uint32_t limit,
                     hipStream_t s, WaitEma *c);
// the completion words a polling wait watches (sort_emit.h): pre-set before the first enqueue, replaced by each
// pipeline's last store
void arm_meta(uint64_t *h_meta, uint32_t nq);
// The host reader of a complete block: its n picks into the caller's arrays (lex_out may be null), its status returned.
uint32_t read_block(const uint32_t *h_out, uint32_t k_cap, uint64_t *rows_out, float *cos_out, float *score_out, float *lex_out,
                    uint32_t *n_out);
// after a synchronisation: did the zero-histogram assertion of a poisoned run fire?
int32_t check_hist_assert(Ctx *c);

// ---- the plan and the staged queries of a call ----------------------------------------------------------------------
struct SearchPlan {
    uint32_t k;        // per query, already clamped to n_rows
    uint32_t cap;      // candidate capacity
    float two_eps;
    float two_eps_img; // band when the nomination scan ran over the binary16 image
    float scale = 1.0f; // |row|_max * |query|_max when that exceeds 1 (the bands above already carry it)
    float norm_sum = 2.0f; // |row|_max + |query|_max, rounded up: the binary16 subnormal term of nomination_eps
    bool f16_ok = true;    // every operand fits binary16 (see plan_bands)
    bool unordered = false; // the consumer wants the best k as a SET (the hybrid blend re-orders everything anyway)
};

// The plan of a call: k clamped to the rows, the band factors of its queries, the guard bands (the one place that knows
// the rule: the caller's guard_eps, or the default for this dim, times the operands' scale) and the candidate capacity.
SearchPlan make_plan(const rlr_index *ix, const float *queries, uint32_t nq, uint32_t k, float guard_eps, bool unordered = false);
int32_t ctx_prepare(rlr_index *ix, Ctx *c, uint32_t nq, const SearchPlan &p);
// A call whose operands leave binary16 range (plan_bands) nominates over the f32 rows: count the queries a binary16
// nomination would have served otherwise -- the batched GEMM (`batch_f16`) or the scan over the image.
void count_f16_fallbacks(rlr_index *ix, const SearchPlan &p, uint32_t nq, bool batch_f16);

// nq dim-long queries -> h_q, q_pitch floats each, zero padded
void pad_queries(const rlr_index *ix, const float *queries, uint32_t nq, float *h_q);
// The queries of a call that enqueues single-query pipelines, staged in pinned memory (h_q), their norms for the 8-bit
// band; from here on the context's histograms count as in use until the call has seen every pipeline finish.
void stage_queries(const rlr_index *ix, Ctx *c, const float *queries, uint32_t nq, float *h_q);
// The queries of a call whose pipelines start with enqueue_query_scan: by the scans themselves where they can, else uploaded.
hipError_t stage_queries_for_scans(const rlr_index *ix, Ctx *c, const float *h_q, size_t q_bytes, hipStream_t s);
// The staged queries (pinned host memory, zero padded to the row pitch) -> the context's device buffer.  A few KB: one
// small kernel on the search's own stream reads them over PCIe itself.  hipMemcpyAsync does the same with the runtime's
// copy kernel, but the scan behind it then starts 4-5 us after that copy has finished (every other boundary of the
// pipeline: < 1 us; scratch/step_timeline.py) -- a stream's copies and kernels are ordered through a signal, kernels
// among themselves by the queue.
hipError_t upload_queries(Ctx *c, const float *h_q, size_t q_bytes, hipStream_t s);
// The pinned memory of a call (c->h_pin): nq staged queries, res_words result words behind them.
struct Staged {
    float *h_q;
    uint64_t *h_res;
};
// Reserve and carve that memory, stage the queries (stage_queries) and send them on their way -- for_scans: left to the
// scans where they can take them (stage_queries_for_scans), else uploaded, with c->h_q_kq null.
int32_t stage_call(rlr_index *ix, Ctx *c, const float *queries, uint32_t nq, size_t res_words, bool for_scans, Staged *out);
// a scan over the index' rows (query_host stays null: the caller sets it where the query may travel in the arguments)
ScanArgs scan_args(const rlr_index *ix, const float *query, float *scores, uint32_t *hist);

// ---- profile bookkeeping ----------------------------------------------------------------------------------------------
// c->ev[0] .. c->ev[3] of a timed single-query pipeline: scan | select | re-score + sort, added to *t
struct StageMs {
    double scan = 0, select = 0, rescore = 0, total = 0;
};

// profile bookkeeping of an MMR call: c->ev[0] .. c->ev[1] bracket gather + Gram + greedy on the context's stream
void note_mmr(rlr_index *ix, Ctx *c, uint32_t n_queries);
// Profile bookkeeping of a search call that has synchronised: nq queries, their candidates and large-candidate retries.
// timed: the pipelines recorded their events -- read here once, or already summed per query by the caller (*summed);
// mmr_chain: c->bev[0] .. c->bev[1] bracket the blend / Gram / greedy chain of a fused search -> MMR call.
// A failed event read leaves its times zero; the counters are kept either way and the failure is the return value (the
// fused paths, whose results are complete by then, ignore it as they always have).
int32_t note_search(rlr_index *ix, Ctx *c, uint32_t nq, uint64_t n_candidates, uint64_t n_retries, bool timed,
                    bool mmr_chain = false, const StageMs *summed = nullptr);

// From the first enqueue on, work may be running on `s` (and, for a batched text search, on the stream that records
// `also`): an exit that has not seen it finish drains it before the lease hands the context back.
struct StreamDrain {
    hipStream_t s;
    hipEvent_t also = nullptr;
    bool armed = true;
    ~StreamDrain()
    {
        if (also)
            (void)hipEventSynchronize(also);
        if (armed)
            (void)hipStreamSynchronize(s);
    }
};

// ---- workspace layouts ---------------------------------------------------------------------------------------------
// A cursor over a base pointer that hands out regions in declaration order.  Each layout built on it is ONE list of
// regions, a member per region initialised by its take(): built over null bases it only measures (what reserve() /
// pin_reserve() are asked for), built again over the buffers it yields every pointer -- the size and the pointers cannot
// disagree.  Region order and sizes are what the kernels and copies have always used; what a layout relies on is said next
// to it.
struct Carver {
    char *base;
    size_t bytes = 0;
    explicit Carver(void *b) : base(static_cast<char *>(b)) {}
    template <typename T>
    T *take(uint64_t count)
    {
        T *p = base ? reinterpret_cast<T *>(base + bytes) : nullptr;
        bytes += static_cast<size_t>(count) * sizeof(T);
        return p;
    }
    uint64_t floats() const { return bytes / sizeof(float); } // c->d_pool is grown in floats; every region is whole words
};

// ---- the pipelines ----------------------------------------------------------------------------------------------------
// Enqueue the whole pipeline for query `qi` on the context's stream:
//   scan (+digit-1 histogram) -> the tail in two launches (tail.hip), or in its split form: digit-2 histogram (bin search
//   folded in) -> collect (bin search folded in) -> LDS-staged reference-order re-score -> sort + emit; either way the
//   candidate count (| checksum) goes into *d_meta_q last.
// The context's histograms are zero on entry: cleared at creation and by every pipeline (tail stage 2 / the re-score kernel).
// (in two halves, so that a caller with work for ANOTHER stream -- the BM25 kernels of a text search -- can launch it right
// behind the scan instead of behind every launch of the pipeline: enqueue_query_scan, then enqueue_query_rest)
// f != nullptr: a document-scoped search -- the masked scan over the master rows, whatever copies the index keeps.
// master_rows: the scan reads the master rows even where the index keeps a nomination copy (a grouped search: its band is the plan's).
hipError_t enqueue_query_scan(rlr_index *ix, Ctx *c, uint32_t qi, bool timed, const rlr_filter *f = nullptr, bool master_rows = false);
// pool != nullptr (with emit == false): a diversified search -- when the fused tail runs, its finish builds the MMR pool in
// the same launch and *pool_done = true; otherwise the caller launches pool_prepare_kernel itself.
hipError_t enqueue_query_rest(rlr_index *ix, Ctx *c, uint32_t qi, const SearchPlan &p, uint64_t *d_out_q, uint64_t *d_meta_q,
                              bool timed, bool emit = true, const PoolArgs *pool = nullptr, bool *pool_done = nullptr,
                              bool master_scan = false);
hipError_t enqueue_query(rlr_index *ix, Ctx *c, uint32_t qi, const SearchPlan &p, uint64_t *d_out_q, uint64_t *d_meta_q,
                         bool timed, bool emit = true, const PoolArgs *pool = nullptr, bool *pool_done = nullptr);

// Runs nq queries.  Packed results (k per query) end up in d_out_user when given (device-resident
// variant), else in the context buffer AND in pinned host memory (*h_results, nq x k u64) -- one
// H2D (queries), one D2H (results + per-query candidate counts) and one stream synchronisation
// per call on the common path.
// coalesced: the queries are a group of concurrent single-query calls (batch_multi_shape); *n_handed_back (optional):
// how many of them the batched pipeline handed back to the single-query pipeline.
int32_t run_search(rlr_index *ix, Ctx *c, const float *queries, uint32_t nq, uint32_t k_req, float guard_eps,
                   uint64_t *d_out_user, SearchPlan *plan_out, const uint64_t **h_results, bool coalesced = false,
                   uint32_t *n_handed_back = nullptr);

// 2..8 queries over f32 rows of these shapes share one VALU scan (scan_multi_kernel) in run_batched.  `coalesced`: the
// queries are a group of concurrent single-query calls (rlr_index_set_coalescing) -- those also share one pass over
// binary16 rows of 256 / 512 / 768 / 1024 elements (scan_multi_h_kernel); explicit multi-query calls over binary16
// rows keep the matrix-core pipeline.
bool batch_multi_shape(const rlr_index *ix, uint32_t nq, bool coalesced = false);
// The per-query workspace of a batched run of nq queries (select states, histograms, status words, fin_cap candidates and
// s_stride sample scores each), the states armed for rank `rank` of n scored rows, histograms and status words cleared on
// the context's stream.  Shared by run_batched and the filtered shared pass.
int32_t batch_arm(Ctx *c, uint32_t nq, uint32_t fin_cap, uint64_t s_stride, uint32_t rank, uint64_t n);
// unpack_result of `take` packed results into a caller's rows / cosines, written without branches so that the loop
// vectorises (a batch of 1024 x 308 results is 315 k of them)
void unpack_results(const uint64_t *__restrict__ src, uint32_t take, uint64_t *__restrict__ ro, float *cos_out);

// ---- searches inside a row set ----------------------------------------------------------------------------------------
int32_t check_filter(const rlr_index *ix, const rlr_filter *f);
// is `row` an allowed row of `f`?  (the host copy of the mask: what every returned row is tested against)
bool filter_holds(const rlr_filter *f, uint32_t row);
// A masked row must never be returned.  Its sentinel keeps it out of every collect whose threshold key is above 0; a
// threshold of 0 (k reaches allowed rows whose own nomination score is NaN) lets it in, and re-scored from its real values
// it can rank anywhere.  So every returned row is tested against the host copy of the mask -- if none is masked the result
// is the right one -- and a caller that finds one takes its exact path.  keys: n packed results; f == nullptr: no filter.
bool masked_row_among(const rlr_filter *f, const uint64_t *keys, uint32_t n);
// One query over the rows of `f` (n_allowed > 0, k > 0).  Filtered calls scan the master rows and never use the
// nomination copies, the matrix-core batch or the coalescer.
int32_t filtered_query(rlr_index *ix, Ctx *c, const rlr_filter *f, const float *query, uint32_t k, float guard_eps,
                       uint64_t *rows_out, float *cos_out, uint32_t *n_out);
// One form read-out (rlr_index_*_forms): the queries each form served since the last reset.
int32_t read_forms(rlr_index *ix, uint64_t (rlr_index::*forms)[4], uint64_t counts[4], int32_t reset);

// The fused one-enqueue calls (rlr_search_diverse / rlr_search_hybrid / search_hybrid_begin) cannot share their scan:
// while coalescing is on and a group of two with this k would qualify, they hand the query back (*fallback = 1) so that
// the caller's two-call path reaches the coalescer through rlr_search_topk.
bool coalesce_hands_back(rlr_index *ix, uint32_t k);

// ---- defined in index_fused.hip, called by rlr_search_capped / capped_query of index_grouped.hip -------------------------
// one pool of up to 4096 candidates; d_matrix != null: pool_rows are slots of that staged matrix (see mmr_batch_impl)
int32_t mmr_single_impl(rlr_index *ix, const uint64_t *pool_rows, const float *pool_scores, uint32_t P, uint32_t k,
                        float lambda, uint32_t *order_out, float *mmr_out, uint32_t *n_out, const void *d_matrix,
                        uint64_t n_matrix);
// the greedy kernel writes the picks of a fused search into the pinned block itself
MmrEmit mmr_emit(const uint32_t *list, const float *comb, const float *cosv, const float *lexv, const uint32_t *info,
                 uint32_t k_cap, uint32_t *h_out);

} // namespace rlr
