// kernels.h -- launch wrappers of the gfx950 kernels (definitions in *.hip).
// Host-callable; every wrapper only enqueues work on `stream`.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rlr {

// Every device allocation of the library goes through here.  RLR_POISON_ALLOC=1 (a test switch) fills each new
// buffer with 0xFF bytes -- NaN as f32 / binary16, huge as a counter -- so that a kernel reading memory nobody
// has written shows up as a wrong answer in the parity tests instead of hiding behind the zero pages a fresh
// process usually gets (tests/test_gpu_fuzz.py::test_poisoned_allocations).
hipError_t dev_malloc(void **p, size_t bytes);
bool poison_mode(); // RLR_POISON_ALLOC=1

// index.hip: sets the thread-local rlr_last_error() message, returns `code`
int32_t set_error(int32_t code, const char *fmt, ...);

// ---- scan.hip : wavefront-order candidate scan (HBM-bound) ----------------
struct ScanArgs {
    const void *rows;     // n_rows x pitch16 x 16 B, row-major
    const float *query;   // device, q_pitch floats (zero padded to the row pitch)
    float *scores;        // n_rows
    uint32_t *hist;       // kHistBins bins of score_key >> 21, pre-zeroed; may be null
    uint32_t n_rows;
    uint32_t dim;         // logical elements per row
    uint32_t pitch16;     // row pitch in 16-byte units
    int dtype;            // RLR_F32 / RLR_F16
    int n_cu;
    int variant;          // tuning knob, 0 = default
    // Optional: the same (zero padded) query in HOST memory.  When set and the shape allows it (f32 rows of <= 768
    // elements on the fixed kernel), the query travels in the kernel's ARGUMENTS and workgroup 0 writes it to `query`
    // for the kernels behind the scan: no upload in front of the scan (a 2.5 us kernel plus the ~4 us the host needs to
    // submit the next launch, during which the device idles).  launch_scan_takes_host_query() says whether it will.
    const float *query_host = nullptr;
};
hipError_t launch_scan(const ScanArgs &a, hipStream_t stream);
bool launch_scan_takes_host_query(const ScanArgs &a);
// the same scan over the rows a filter allows: `mask` holds one bit per row (ceil(n_rows / 64) words, tail bits zero),
// n_allowed of them set (it only picks the launch shape); masked rows are not read, score NaN (score_key 0) and are not
// counted in `hist`.  The query comes from a.query.
hipError_t launch_scan_masked(const ScanArgs &a, const uint64_t *mask, uint64_t n_allowed, hipStream_t stream);
// one pass over the rows for 2..8 queries (a.query = n_queries x q_pitch floats, a.scores = n_queries x score_stride);
// false when the shape is not served (then nothing was launched)
bool launch_scan_multi(const ScanArgs &a, uint32_t q_pitch, uint32_t n_queries, size_t score_stride, hipStream_t s,
                       hipError_t *err);
// one MASKED pass for 2..8 queries (a document-scoped batch): launch_scan_multi's arguments and score layout,
// launch_scan_masked's mask; masked rows leave as NaN in every query's array, no histogram.  f32 rows of 1..4 KiB
// only -- binary16 rows, other widths and other pitches return false and keep the one-by-one masked scans.
bool launch_scan_masked_multi(const ScanArgs &a, const uint64_t *mask, uint64_t n_allowed, uint32_t q_pitch, uint32_t n_queries,
                              size_t score_stride, hipStream_t s, hipError_t *err);
// one masked pass for 2..8 queries with a mask EACH (queries scoped to different documents): masks[q] is query q's mask as
// launch_scan_masked takes it (slots at or beyond n_queries are ignored; two slots may hold the same pointer), the pass
// reads every row of the UNION of the masks once and query q's score array is the one launch_scan_masked_multi writes
// with masks[q].  union_estimate (an upper bound of the rows in the union is enough) only picks the launch shape, the
// way n_allowed does there.  Same shapes, same return value.
struct ScopeMasks {
    const uint64_t *m[8];
};
bool launch_scan_masked_scopes(const ScanArgs &a, const uint64_t *const masks[8], uint64_t union_estimate, uint32_t q_pitch,
                               uint32_t n_queries, size_t score_stride, hipStream_t s, hipError_t *err);
// launch_scan_multi over binary16 rows of C x 512 B (C = 1..4), f32 arithmetic on the exactly widened elements (coalesced
// single-query calls only; see run_batched)
bool launch_scan_multi_f16(const ScanArgs &a, uint32_t q_pitch, uint32_t n_queries, size_t score_stride, hipStream_t s,
                           hipError_t *err);

// read-only streaming probe over `bytes` of device memory (sink: blocks * 256 floats, blocks <= n_cu * 8); shape 0..2
hipError_t launch_probe_read(const void *p, size_t bytes, float *sink, int n_cu, int shape, hipStream_t s);

// ---- select.hip : radix select / collect / sort -------------------------
// Selection state kept on the device between the stages of one query.
struct SelectState {
    uint32_t k;          // in : rank wanted (1-based), <= n
    uint32_t bin1;       // out of find1: digit of the k-th key, bits 31..21
    uint32_t k2;         // rank inside bin1
    uint32_t bin2;       // out of find2: bits 20..10
    uint32_t key_lo;     // collect threshold (guard band applied)
    uint32_t n_cand;     // collect counter (may exceed cap)
    uint32_t cap;        // in : candidate buffer capacity
    uint32_t pad;
    // fused tail (tail.hip); all four are zero between two queries of a context
    uint32_t n_work;     // candidate slots handed out so far (becomes n_cand when the tail finishes)
    uint32_t done;       // workgroups of the refine-mode stage 2 that have finished their slice
    uint32_t flags;      // bit 0: a workgroup found more candidates in its slice than its local list holds
    uint32_t mode;       // written by stage 1: 1 = direct (candidates collected and re-scored there), 2 = refine
};
hipError_t launch_collect(const float *scores, uint32_t n, SelectState *st, uint32_t *cand,
                          int n_cu, hipStream_t s);
// single-query pipeline: bin searches folded into the kernels that need them
hipError_t launch_hist2_find1(const float *scores, uint32_t n, const uint32_t *hist1, uint32_t *hist2,
                              SelectState *st, uint32_t k, uint32_t cap, int n_cu, hipStream_t s);
hipError_t launch_collect_find2(const float *scores, uint32_t n, const uint32_t *hist2, SelectState *st,
                                float two_eps, uint32_t *cand, int n_cu, hipStream_t s);
// sort `n_pad` (power of two) packed u64 descending in place; entries >= n are 0.
hipError_t launch_sort_desc(uint64_t *packed, uint32_t n_pad, hipStream_t s);

hipError_t launch_batch_select(const float *scores, uint32_t n, size_t score_stride, uint32_t q_count,
                               uint32_t *hist, SelectState *st, float two_eps, float *tau_out, uint64_t *cand,
                               uint32_t cand_stride, int n_cu, hipStream_t s);

// ---- tail.hip : everything behind the scan of a single-query search in two launches ----------------
// stage 1: bin search over hist1 (folded in), then either DIRECT -- at most `direct_max` scores sit in or above the
//          k-th score's digit-1 bin: every workgroup appends the rows of its slice at or above (bin floor - band) and
//          re-scores them in reference order on the spot (packed[slot] = (exact score, row)) -- or REFINE: the digit-2
//          histogram of that bin (what launch_hist2_find1 does);
// stage 2: DIRECT: workgroup 0 sorts and emits; REFINE: digit-2 bin search, collect + re-score per workgroup, the
//          workgroup that finishes last sorts and emits.  Both clear the two histograms for the next query.
// out == nullptr: no sort / emit (the caller orders packed[0, st->n_cand) itself); *meta receives the candidate count.
// false: the row shape does not fit the staged re-score (the caller takes the split five-launch pipeline).
// The MMR pool of a diversified search built by the workgroup that finishes the tail (pool_prepare.h) instead of the
// sort / emit: the `fetch` best candidates -> combined scores, order, cut to `need`.
struct PoolArgs {
    uint32_t fetch, need, n_rows;
    float w_e, w_l;
    uint32_t *list; // pool slot -> row
    float *comb;    // combined score per slot
    float *cosv;    // cosine per slot
    uint32_t *info; // [0] pool size, [1] status
};
struct TailArgs {
    const float *scores;
    uint32_t n;
    uint32_t *hist; // 2 * kHistBins (digit 1, digit 2), zero on entry, zero again when stage 2 has run
    SelectState *st;
    uint32_t k, cap;
    float two_eps;
    const void *rows;
    uint32_t pitch16, dim;
    int dtype;
    const float *query;
    uint64_t *packed; // cap entries
    uint64_t *out;
    uint64_t *meta;
    bool unordered;
    uint32_t direct_max;
    int n_cu;
    const PoolArgs *pool = nullptr; // non-null (with out == nullptr): the finish builds the MMR pool from the candidates
};
bool tail_fits(uint32_t pitch16, uint32_t dim, int dtype);
hipError_t launch_tail_stage1(const TailArgs &a, hipStream_t s);
hipError_t launch_tail_stage2(const TailArgs &a, hipStream_t s);

// ---- gemm.hip : batched queries, MFMA nomination + per-query exact finish ----------------
float nomination_eps(uint32_t dim, int dtype, float prod = 1.0f, float norm_sum = 2.0f);
uint32_t batch_finish_capacity();
hipError_t launch_prep_queries(const float *q, uint32_t n_queries, uint32_t q_pitch, uint32_t dim, int dtype,
                               void *qfrag, hipStream_t s);
// scores != null: materialise nominated scores of rows [row_begin,row_end) (column = row - row_begin);
// scores == null: filter mode, append (score,row) >= tau[q] to cand[q].
hipError_t launch_gemm_nominate(const void *rows, uint32_t pitch16, uint32_t dim, int dtype, uint32_t row_begin,
                                uint32_t row_end, const void *qfrag, uint32_t n_queries, const float *tau,
                                uint64_t *cand, uint32_t cand_stride, SelectState *st, float *scores,
                                size_t score_stride, const void *image, hipStream_t s, uint32_t *sync_ws = nullptr);
// optional binary16 nomination image of the corpus in GEMM-fragment order (see gemm.hip)
size_t image_bytes(uint32_t dim, uint64_t n_rows);
// whether launch_gemm_nominate serves rows of this width from the image (else it reads the row-major matrix)
bool gemm_image_usable(uint32_t dim);
// single-query nomination scan over the image (binary16, half the bytes of the f32 rows); dim % 64 == 0,
// query = dim floats on the device; same outputs as launch_scan; error bound nomination_eps(dim, dtype)
hipError_t launch_scan_image(const void *image, uint32_t n_rows, uint32_t dim, const float *query, float *scores,
                             uint32_t *hist, int n_cu, hipStream_t s);
hipError_t launch_build_image(const void *rows, uint32_t pitch16, uint32_t dim, int dtype, uint32_t n_rows,
                              uint32_t tile_begin, uint32_t tile_end, void *image, hipStream_t s);
// batched finish = band cut (sort the nominated candidates, keep the guard band) -> staged reference-order
// re-score of every band (exact.hip) -> final order + emit.  `cand` is overwritten; st[q].pad receives the
// band length.
hipError_t launch_batch_finish(const void *rows, uint32_t pitch16, uint32_t dim, int dtype, const float *queries,
                               uint32_t q_pitch, uint32_t n_queries, uint64_t *cand, uint32_t cand_stride,
                               SelectState *st, uint32_t k, float two_eps, uint64_t *out, uint32_t *status,
                               hipStream_t s);
bool batch_rescore_fits(uint32_t pitch16, uint32_t dim, int dtype);
bool launch_batch_rescore(const void *rows, uint32_t pitch16, uint32_t dim, int dtype, const float *queries,
                          uint32_t q_pitch, uint32_t n_queries, uint64_t *band, uint32_t band_stride,
                          const SelectState *st, hipStream_t s, hipError_t *err);

// ---- exact.hip : reference-order arithmetic --------------------------------
// packed_out[i] = pack(dot_ref(query, row[cand[i]]), cand[i]) for i < min(n_cand, cap);
// entries up to n_pad are zero-filled.  n_cand is read from the device (st->n_cand).
hipError_t launch_rescore(const void *rows, uint32_t pitch16, uint32_t dim, int dtype,
                          const float *query, const uint32_t *cand, const SelectState *st,
                          uint64_t *packed_out, uint32_t n_pad, hipStream_t s);
// LDS-staged variant for the fast path (no zero fill; also clears 2*kHistBins words at hist_clear).
bool launch_rescore_staged(const void *rows, uint32_t pitch16, uint32_t dim, int dtype, const float *query,
                           const uint32_t *cand, const SelectState *st, uint64_t *packed_out, uint32_t n_max,
                           uint32_t *hist_clear, hipStream_t s, hipError_t *err);
// cos_out[i] = dot_ref(query, row[list[i]]) for an explicit row list.
// n_dev != null: the list length is min(*n_dev, n) (known only on the device); rows >= n_rows_clamp (markers) score row 0
hipError_t launch_score_rows(const void *rows, uint32_t pitch16, uint32_t dim, int dtype, const float *query,
                             const uint32_t *list, uint32_t n, float *cos_out, hipStream_t s,
                             const uint32_t *n_dev = nullptr, uint32_t n_rows_clamp = 0xFFFFFFFFu);
// the same for n_queries queries at once: query q (queries + q * q_pitch) against list + q * stride, length
// min(stride, n_dev[q * n_dev_stride]), into cos_out + q * stride
hipError_t launch_score_rows_batch(const void *rows, uint32_t pitch16, uint32_t dim, int dtype, const float *queries,
                                   uint32_t q_pitch, uint32_t n_queries, const uint32_t *list, uint32_t stride, float *cos_out,
                                   const uint32_t *n_dev, uint32_t n_dev_stride, uint32_t n_rows_clamp, hipStream_t s);
// Reference normalize() of n rows of f32 staging data (in place), then store as dtype.
hipError_t launch_normalize_store(float *staging, uint32_t n, uint32_t dim, int do_normalize,
                                  void *rows_out, uint32_t pitch16, int dtype, float *norm_tmp,
                                  hipStream_t s);
hipError_t launch_synth(void *rows_out, uint32_t pitch16, uint32_t dim, int dtype, uint64_t row0,
                        uint32_t n, uint64_t seed, uint32_t n_clusters, float *norm_tmp,
                        hipStream_t s);
// out[i][0..dim) = widen(row[list[i]]), dense f32 with pitch `dim`.
hipError_t launch_gather_f32(const void *rows, uint32_t pitch16, uint32_t dim, int dtype,
                             const uint32_t *list, uint32_t n, float *out, hipStream_t s);
// stable compaction: dst row i = src row keep[i]
hipError_t launch_compact_rows(const void *src, void *dst, uint32_t pitch16, const uint32_t *keep,
                               uint32_t n_keep, hipStream_t s);
// gram[i*P + j] = dot_ref(pool[i], pool[j]) over a dense f32 P x dim pool.
hipError_t launch_gram(const float *pool, uint32_t P, uint32_t dim, float *gram, uint32_t n_queries, hipStream_t s);
// the same with the pool rows read straight from the index through list[q * P + i] (no gathered f32 copy)
hipError_t launch_gram_rows(const void *rows, uint32_t pitch16, uint32_t dim, int dtype, const uint32_t *list, uint32_t P,
                            float *gram, uint32_t n_queries, hipStream_t s);
// Optional tail of the greedy kernel for a single pool (the fused search paths): the picks go straight to (pinned)
// memory as [row | cos | combined | lexical] x k_cap, then n, status -- no separate emit launch.
struct MmrEmit {
    const uint32_t *list = nullptr; // pool slot -> row
    const float *comb = nullptr, *cosv = nullptr, *lexv = nullptr; // per pool slot (lexv may be null: zeros)
    const uint32_t *info = nullptr; // info[1] != 0: the pool is not usable, n = 0
    uint32_t k_cap = 0;
    uint32_t *h_out = nullptr;      // null: no emit
};
// greedy MMR over the gram matrix; out_order/out_mmr/out_n on the device.
hipError_t launch_mmr_greedy(const float *gram, const float *scores, uint32_t P, uint32_t k,
                             float lambda, uint32_t *out_order, float *out_mmr, uint32_t *out_n,
                             const uint32_t *sizes, uint32_t n_queries, hipStream_t s, const MmrEmit *emit = nullptr);

// ---- q8.hip : optional 8-bit nomination copy of f32 rows (single-query scans at a quarter of the bytes) ----
hipError_t launch_q8_build(const void *rows, uint32_t pitch16, uint32_t dim, int dtype, uint32_t row_begin, uint32_t n_rows,
                           void *q8, float *scale, uint32_t *stats, hipStream_t s);
hipError_t launch_q8_scan(const void *q8, const float *scale, uint32_t n_rows, uint32_t dim, const float *query,
                          float *scores, uint32_t *hist, int n_cu, hipStream_t s);
float q8_arith_eps(uint32_t dim, float scale_max, float q_norm);

// ---- docs.hip : the per-row document column -> filter mask / row list / keep list, on the device ----
constexpr uint32_t kDocsRowsPerGroup = 4096; // rows (64 mask words) one workgroup of the mask / scatter launches covers
constexpr uint32_t kDocsSumsPerGroup = 1024; // per-workgroup counts one workgroup of the scan launches covers
// The membership switch: up to this many distinct document ids are staged in LDS (8 KiB: a workgroup's 4096 rows then
// cost 12 LDS probes each and the set is read from global memory once per workgroup); a larger set is binary-searched
// where it lies (global memory, L2-resident).
constexpr uint32_t kDocsLdsMax = 2048;
uint32_t docs_groups(uint32_t n_rows);  // workgroups (= counts) of the mask launch
uint32_t docs_tiles(uint32_t n_groups); // workgroups (= tile sums) of the first scan launch
// mask[w] bit b = (col[64 w + b] is one of the n_docs sorted, distinct ids at `docs`), tail bits zero; counts[g] = set
// bits of workgroup g's words.  n_rows, n_docs >= 1; RLR_DOC_NONE is never a member.
hipError_t launch_docs_mask(const uint32_t *col, uint32_t n_rows, const uint32_t *docs, uint32_t n_docs, uint64_t *mask,
                            uint32_t *counts, hipStream_t s);
// counts[0 .. n_groups) -> exclusive scan within tiles of kDocsSumsPerGroup, tile_sums[0 .. docs_tiles) -> exclusive
// scan of the tiles' sums (untouched for one tile), *total = the sum of all counts
hipError_t launch_docs_scan(uint32_t *counts, uint32_t n_groups, uint32_t *tile_sums, uint32_t *total, hipStream_t s);
// the rows of the set bits in ascending order -> list; invert != 0: the rows >= first_row (= the first set bit's row)
// with a CLEAR bit instead, i.e. the keep list of a deletion from its first dead row on
hipError_t launch_docs_scatter(const uint64_t *mask, uint32_t n_rows, const uint32_t *offsets, const uint32_t *tile_offsets,
                               int invert, uint32_t first_row, uint32_t *list, hipStream_t s);
hipError_t launch_docs_fill(uint32_t *col, uint64_t n, uint32_t doc, hipStream_t s);                               // col[i] = doc
hipError_t launch_docs_gather(const uint32_t *col, const uint32_t *keep, uint64_t n, uint32_t *out, hipStream_t s); // out[i] = col[keep[i]]

// ---- group.hip : the tail of a grouped search (at most per_doc results per document), behind the scan ----
constexpr uint32_t kGroupCap = 2048;  // candidates the one-workgroup finish holds
constexpr uint32_t kGroupKMax = 1024; // largest k the finish emits
struct GroupState {
    uint32_t n_cand;  // candidate slots handed out (may exceed kGroupCap)
    uint32_t n_valid; // rows whose nominated score is a number (masked rows and NaN nominations are not)
    uint32_t flags;   // bit 0: a workgroup's local candidate list overflowed, bit 1: the document table ran out of slots
    uint32_t u_bits;  // collect: the bits of U, the floor of the k-th head's bin (-inf with fewer than k heads)
};
// A capped hybrid search (rlr_search_capped): capped_finish_kernel in place of group_finish_kernel.  The finish unites the
// re-scored grouped candidates with the lexical rows, blends, caps per document in combined order and leaves the first
// `k` (= need) accepted entries as the pool a PoolArgs consumer expects.
constexpr uint32_t kCappedLexMax = 2048;                        // lexical rows the finish holds
constexpr uint32_t kCappedSlots = kGroupCap + kCappedLexMax;    // entries of the union: its LDS is sized from this
// pinned side block of a capped call: [n | checksum | rows x need | document ids x need]
inline uint32_t capped_side_words(uint32_t need) { return 2 + 2 * need; }
struct CappedArgs {
    float w_e, w_l, eps;      // the resolved weights (w_e > 0, w_l >= 0) and the plan's half band
    uint32_t n_allowed;       // |A|
    const uint32_t *lrow;     // n_lex lexical rows: ascending, unique, inside A
    const float *lscore;      // their BM25 scores (>= 0)
    const float *lcos;        // their reference-order cosines
    uint32_t n_lex;           // <= kCappedLexMax
    float max_lex;
    float *scratch;           // 3 x kCappedSlots floats: combined | cos | lexn per entry
    uint32_t *list;           // the pool: slot -> row ...
    float *comb, *cosv, *lexv; // ... combined, cosine, normalised lexical score
    uint32_t *info;           // [0] pool size, [1] status (0 decided, 1 capacity, 2 undecidable here)
    uint32_t *h_side;         // capped_side_words(need) pinned words: the pool's rows and document ids
    uint32_t k_cap;
    uint32_t *h_out;          // non-null: no diversification -- the pool is the result, emitted as a result block (sort_emit.h)
};
struct GroupArgs {
    const float *scores;  // n nominated scores (NaN: masked, or a NaN nomination)
    const uint32_t *docs; // n document ids, or null: no column (every row a group of its own)
    uint32_t n, k, per_doc;
    float two_eps;        // 2 x the plan's half band
    uint32_t *tab_keys;   // 1 << tab_bits document ids (open addressing)
    uint64_t *tab_vals;   // per_doc packed keys per slot: the group's largest, second largest, ... nominated key
    uint32_t tab_bits;
    uint64_t *tg;         // n: the per_doc-th largest nominated key of the row's group (0: the group is smaller)
    uint32_t *hist;       // 2 * kHistBins: digit 1 and digit 2 of the heads
    GroupState *st;
    const void *rows;
    uint32_t pitch16, dim;
    int dtype;
    const float *query;
    uint64_t *cand;       // kGroupCap exact packed keys
    uint32_t *cand_doc;   // ... and their document ids
    uint64_t *out;        // group_out_words(k) words: k results | ceil(k / 2) words of document ids | n_valid + (n_out << 32)
    uint64_t *meta;       // candidate count | checksum of `out` << 32, written last
    uint32_t *ctx_hist;   // the context's digit-1 histogram (the scan counted into it): cleared for the next query
    int n_cu;
    const CappedArgs *capped = nullptr; // non-null: out / meta unused, the capped finish runs
};
inline uint32_t group_out_words(uint32_t k) { return k + (k + 1) / 2 + 1; }
bool group_fits(uint32_t pitch16, uint32_t dim, int dtype);
hipError_t launch_group_tail(const GroupArgs &a, hipStream_t s, hipEvent_t after_rounds = nullptr);
hipError_t launch_group_iota(uint32_t *list, uint32_t n, hipStream_t s); // list[i] = i
// the LDS staging of a workgroup's re-score (at most 56 KB): candidates per pass and the dynamic LDS bytes; false: too wide
bool group_shape(uint32_t pitch16, uint32_t dim, int dtype, uint32_t *cpb_out, size_t *staging_out);

// The tail of a BATCHED grouped search (rlr_search_topk_grouped_batch): a chunk of n_queries (2..8) queries whose nominated
// scores came from ONE shared scan, one score array per query, score_stride apart.  One set of launches serves the chunk.
// The allowed rows and the document column are the same for every query, so the chunk has ONE key table; everything else
// is per query: value plane q at tab_vals + q * slots * per_doc, t_g at tg + q * n, the two histograms at
// hist + q * 2 * kHistBins, st[q], kGroupCap candidate slots at cand + q * kGroupCap, and group_batch_words(k) words of `out`
// (device memory; one copy brings the whole chunk back):
//   group_out_words(k) words as GroupArgs::out has them | status: the candidate count, or kGroupBatchBack when the finish
//   could not decide (more than kGroupCap candidates, a local list or the table overflowed)
constexpr uint64_t kGroupBatchBack = 0xFFFFFFFFull;
// The capped part of a batched tail (rlr_search_capped_batch): capped_finish_multi_kernel in place of the grouped finish,
// one workgroup per query of the chunk.  What CappedArgs holds once is held per query here.  The lexical pairs lie
// lex_stride apart (query q's rows, scores and cosines at lrow / lscore / lcos + q * lex_stride, n_lex[q] of them:
// ascending, unique, inside A -- the fixed-stride layout launch_score_rows_batch scores); scratch, the pool planes and
// the document ids are `need` (= GroupBatchArgs::k) respectively 3 * kCappedSlots apart.
struct CappedBatchArgs {
    float w_e, w_l, eps;       // per call: the resolved weights and the chunk plan's half band
    uint32_t n_allowed;        // |A|
    const uint32_t *lrow;
    const float *lscore, *lcos;
    uint32_t lex_stride;
    uint32_t n_lex[8];         // <= kCappedLexMax each
    float max_lex[8];
    float *scratch;            // n_queries x 3 x kCappedSlots floats
    uint32_t *list;            // n_queries x need: the pools, slot -> row ...
    float *comb, *cosv, *lexv; // ... combined, cosine, normalised lexical score
    uint32_t *docs;            // ... document id
    uint32_t *info;            // n_queries x {pool size, status (0 decided, 1 capacity, 2 undecidable here)}
    uint32_t *sizes;           // n_queries pool sizes (0 with a non-zero status): what the batched greedy launch reads
};
struct GroupBatchArgs {
    uint32_t n_queries;
    const float *scores;  // n_queries x score_stride nominated scores (NaN: masked, or a NaN nomination)
    size_t score_stride;
    const uint32_t *docs; // n document ids, or null: no column
    uint32_t n, k, per_doc;
    float two_eps;
    uint32_t *tab_keys;   // 1 << tab_bits document ids, shared by the chunk
    uint64_t *tab_vals;   // n_queries planes of (1 << tab_bits) x per_doc packed keys
    uint32_t tab_bits;
    uint64_t *tg;         // n_queries x n
    uint32_t *hist;       // n_queries x 2 * kHistBins
    GroupState *st;       // n_queries
    const void *rows;
    uint32_t pitch16, dim;
    int dtype;
    const float *queries; // device, q_pitch floats each
    uint32_t q_pitch;
    uint64_t *cand;       // n_queries x kGroupCap
    uint32_t *cand_doc;
    uint64_t *out;        // n_queries x group_batch_words(k)
    int n_cu;
    const CappedBatchArgs *capped = nullptr; // non-null: out unused, the capped multi finish runs (k = need)
};
inline uint32_t group_batch_words(uint32_t k) { return group_out_words(k) + 1; }
hipError_t launch_group_batch_tail(const GroupBatchArgs &a, hipStream_t s);

// ---- range.hip : the tail of a range search (every row scoring at or above a threshold), behind the scan ----
constexpr uint32_t kRangeFinishMax = 2048; // hits the one-workgroup finish orders and emits
struct RangeState {
    uint32_t n_hits;  // exact hits counted (may exceed the key capacity)
    uint32_t n_valid; // rows whose nominated score is a number (masked rows and NaN nominations are not)
};
// One ulp outward; NaN and the infinity on that side stay.  (Host and device decide against the SAME two floats: the host
// computes them once and the kernels only compare.)
inline float range_step(float x, bool up)
{
    const float inf = __builtin_inff();
    if (!(x == x) || x == (up ? inf : -inf))
        return x;
    if (x == 0.0f)
        return __builtin_bit_cast(float, up ? 0x00000001u : 0x80000001u);
    const uint32_t b = __builtin_bit_cast(uint32_t, x);
    const bool neg = (b & 0x80000000u) != 0;
    return __builtin_bit_cast(float, neg == up ? b - 1u : b + 1u);
}
// lo <= tau - 2 eps and hi >= tau + 2 eps in real arithmetic: the f32 difference / sum is rounded to nearest, so one step
// outward covers the rounding.  A NaN bound (tau and the band both infinite) makes every row a candidate and none sure.
inline void range_bounds(float tau, float two_eps, float *lo, float *hi)
{
    *lo = range_step(tau - two_eps, false);
    *hi = range_step(tau + two_eps, true);
}
struct RangeArgs {
    const float *scores; // n nominated scores (NaN: masked, or a NaN nomination)
    uint32_t n;
    float tau, two_eps;
    uint32_t hit_cap;    // keys `hits` holds; 0: count only
    uint32_t out_keys;   // keys the pinned block holds: min(hit_cap, kRangeFinishMax)
    RangeState *st;
    const void *rows;
    uint32_t pitch16, dim;
    int dtype;
    const float *query;
    uint64_t *hits;      // hit_cap exact packed keys, in no order
    uint64_t *out;       // range_out_words(out_keys) pinned words: the keys in result order, zeros behind | n_hits + (n_valid << 32)
    uint64_t *meta;      // keys emitted (0 / 1) | checksum of `out` << 32, written last
    uint32_t *ctx_hist;  // the context's digit-1 histogram (the scan counted into it): cleared for the next query
    int n_cu;
};
inline uint32_t range_out_words(uint32_t out_keys) { return out_keys + 1; }
hipError_t launch_range_tail(const RangeArgs &a, hipStream_t s);

// The tail of a BATCHED range search (rlr_search_range_batch): n_queries queries whose nominated scores came from ONE
// pass over the rows -- either `scores` (a shared VALU scan: one score array per query, score_stride apart; the multi-query
// collect, then the finish orders and emits) or `cand` (the nomination GEMM in filter mode with d_tau[q] = lo[q]: query q's
// (nominated key, row) words at cand + q * cand_stride, their count in bst[q].n_cand; the finish does the whole tail).
// Every query keeps up to kRangeFinishMax exact keys when rows are wanted (cap != 0), whatever cap is -- lower than the
// single path's min(cap, RLR_RANGE_DEVICE_MAX): a query with more hits is handed back and the single path owns that case.
// Per query, range_batch_words(out_keys) words in `out` (device memory; one copy brings the whole chunk back):
//   out_keys = min(cap, kRangeFinishMax) keys in result order, zeros behind | n_hits + (n_valid << 32) | status
enum RangeBatchStatus : uint32_t {
    kRangeBatchDecided = 0,
    kRangeBatchCandidates = 1, // behind the GEMM: the candidate list overflowed (or the image kernel's bit 31 mark is set)
    kRangeBatchHits = 2,       // rows wanted and more than kRangeFinishMax hits
};
struct RangeBatchArgs {
    uint32_t n_queries;
    uint32_t n;              // rows of the index
    const float *scores;     // shared scan: n_queries x score_stride nominated scores (NaN: masked, or a NaN nomination); else null
    size_t score_stride;
    const uint64_t *cand;    // GEMM: n_queries x cand_stride nominated (key, row) words; else null
    uint32_t cand_stride;    // = the capacity the lists were armed with
    const SelectState *bst;  // GEMM: n_cand per query (bit 31: the image kernel's workgroup list overflowed)
    const uint64_t *mask;    // GEMM with a mask-path filter: one bit per row, candidates with a clear bit are dropped; else null
    const float *bounds;     // device, n_queries x 3: tau | lo | hi (range_bounds, computed once on the host)
    uint32_t cap;            // the caller's cap; 0: count only
    RangeState *st;          // shared scan: n_queries states
    const void *rows;
    uint32_t pitch16, dim;
    int dtype;
    const float *queries;    // device, q_pitch floats each
    uint32_t q_pitch;
    uint64_t *hits;          // n_queries x kRangeFinishMax exact packed keys, in no order (untouched when cap == 0)
    uint64_t *out;           // n_queries x range_batch_words(min(cap, kRangeFinishMax)) words
    int n_cu;
};
inline uint32_t range_batch_words(uint32_t out_keys) { return out_keys + 2; }
hipError_t launch_range_batch_tail(const RangeBatchArgs &a, hipStream_t s);

} // namespace rlr
