// filter_internal.h -- what the other translation units of the library see of a row filter (include/rlr_gpu.h,
// rlr_filter_create_*; the object itself lives in index.hip).
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

} // namespace rlr
