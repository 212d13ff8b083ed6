// filter_internal.h -- what the other translation units of the library see of a row filter (include/rlr_gpu.h,
// rlr_filter_create_*; the object itself is declared in index_internal.h and made in index.hip).
#pragma once

#include "../../include/rlr_gpu.h"

namespace rlr {

struct FilterView {
    const uint64_t *h_mask = nullptr; // host: one bit per index row, ceil(index_rows / 64) words, tail bits zero
    const uint64_t *d_mask = nullptr; // the same words on the filter's device
    uint64_t index_rows = 0;          // rows of the index when the filter was made
    uint64_t n_allowed = 0;
    int32_t device = 0;
};

// RLR_E_INVALID (message in rlr_last_error) for a null filter or one whose index has been mutated since it was made
int32_t filter_view(const rlr_filter *f, FilterView *out);
// the same, and RLR_E_INVALID for a filter that was made for another index than `ix`; no GPU work
int32_t filter_check(const rlr_index *ix, const rlr_filter *f);

// (index_fused.hip) rlr_score_rows for nq prepared (dim-long) queries with a row list each, for the batched text search inside a filter:
// query q against rows[q * stride .. q * stride + counts[q]) -> cos_out at the same places, bit for bit what
// rlr_score_rows returns per pair.  One upload, one launch, one copy back, one synchronisation.
int32_t score_rows_batch(rlr_index *ix, const float *queries, uint32_t nq, const uint64_t *rows, const uint32_t *counts,
                         uint32_t stride, float *cos_out);

} // namespace rlr
