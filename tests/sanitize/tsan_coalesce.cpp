// TEST INFRASTRUCTURE -- the coalescer of concurrent single-query searches (rlr_index_set_coalescing) under
// ThreadSanitizer: the whole of csrc/ compiled with -fsanitize=thread and linked against tests/sanitize/stub_hip.cpp (see
// tests/test_coalesce_cpu.py).  4..16 caller threads run rlr_search_topk with one query each, mixed k and two guard
// bands, plus the fused diversified call (which hands its query back while coalescing is on); the stub's simulated
// device latency (STUB_SYNC_US) keeps a pass running long enough that later callers join pending groups.
// Between rounds the main thread appends and deletes rows and switches coalescing off and on again, alone.  Kernels do
// nothing on the stub, so answers are not checked here (tests/test_gpu_coalesce.py does that): the pass criterion is
// no ThreadSanitizer report, no deadlock, every call returns RLR_OK, and the statistics add up.
#include "../../include/rlr_gpu.h"

#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

namespace {
uint64_t next(uint64_t *s)
{
    uint64_t z = (*s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
std::atomic<int> g_fail{0};
#define CHECK(call)                                                                                                    \
    do {                                                                                                               \
        const int32_t st_ = (call);                                                                                    \
        if (st_ != RLR_OK) {                                                                                           \
            fprintf(stderr, "%s -> %d (%s)\n", #call, st_, rlr_last_error());                                           \
            g_fail++;                                                                                                  \
        }                                                                                                              \
    } while (0)
} // namespace

int main(int argc, char **argv)
{
    const int rounds = argc > 1 ? atoi(argv[1]) : 2;
    const int iters = argc > 2 ? atoi(argv[2]) : 20;
    const uint32_t dim = 256; // (the shared pass takes rows of 1 KiB multiples and >= 4096 of them)
    uint64_t n_rows = 6000, seed = 77;
    rlr_index *ix = nullptr;
    CHECK(rlr_index_create(dim, RLR_F32, 0, &ix));
    std::vector<float> rows(n_rows * dim);
    for (auto &v : rows)
        v = static_cast<float>(static_cast<int64_t>(next(&seed) % 2001) - 1000) / 1000.0f;
    CHECK(rlr_index_upload(ix, rows.data(), n_rows, 1));
    CHECK(rlr_index_set_coalescing(ix, 8, 200));
    uint64_t total_calls = 0;
    const int thread_counts[] = {4, 8, 12, 16};
    for (int rd = 0; rd < rounds; ++rd) {
        for (int nt : thread_counts) {
            std::vector<std::thread> ts;
            std::atomic<uint64_t> calls{0};
            for (int t = 0; t < nt; ++t)
                ts.emplace_back([&, t] {
                    uint64_t s = 1234567 + 977 * t + 31 * rd;
                    std::vector<float> q(dim);
                    std::vector<uint64_t> r(100);
                    std::vector<float> c(100);
                    std::vector<float> sc(100);
                    for (int it = 0; it < iters; ++it) {
                        // Query elements are binary32 subnormals (bit patterns 1..4000).  On the stub nothing writes a
                        // query's candidate count, so a call reads a stale word of its context's pinned staging buffer
                        // as one -- possibly an earlier, larger group's query; small bit patterns keep that "count"
                        // under the sort's capacity instead of sending the call down the large-candidate path with a
                        // multi-GB workspace.
                        for (auto &v : q) {
                            const uint32_t b = static_cast<uint32_t>(next(&s) % 4000) + 1;
                            memcpy(&v, &b, sizeof(v));
                        }
                        if ((t + it) % 4 == 3) { // the fused call hands the query back without touching a context
                            uint32_t n = 0;
                            int32_t fb = 0;
                            CHECK(rlr_search_diverse(ix, q.data(), 15, 5, 0.3f, 0.7f, 0.3f, -1.0f, r.data(), c.data(), sc.data(),
                                                     &n, &fb));
                            if (fb != 1) {
                                fprintf(stderr, "caller %d: rlr_search_diverse did not hand the query back\n", t);
                                g_fail++;
                            }
                            continue;
                        }
                        const uint32_t k = (t + it) % 3 == 0 ? 10 : (t + it) % 3 == 1 ? 50 : 100;
                        const float eps = t % 2 ? -1.0f : 1e-4f;
                        uint32_t n = 0;
                        CHECK(rlr_search_topk(ix, q.data(), 1, k, eps, r.data(), c.data(), &n));
                        if (n != k) {
                            fprintf(stderr, "caller %d: %u results for k = %u\n", t, n, k);
                            g_fail++;
                        }
                        calls++;
                    }
                });
            for (auto &t : ts)
                t.join();
            total_calls += calls.load();
            printf("round %d, %2d threads done\n", rd, nt);
            fflush(stdout);
        }
        // mutations, alone (external exclusion): append, delete, coalescing off and on again
        const uint64_t add = 1000;
        std::vector<float> more(add * dim, 0.25f);
        uint64_t first = 0;
        CHECK(rlr_index_append(ix, more.data(), add, 1, &first));
        n_rows += add;
        std::vector<uint64_t> drop = {5, 17, n_rows - 1};
        CHECK(rlr_index_delete_rows(ix, drop.data(), static_cast<uint64_t>(drop.size())));
        n_rows -= drop.size();
        CHECK(rlr_index_set_coalescing(ix, 0, 0));
        CHECK(rlr_index_set_coalescing(ix, 8, rd % 2 ? 0 : 200));
    }
    rlr_coalesce_stats st{};
    CHECK(rlr_index_coalesce_stats(ix, &st, 0));
    uint64_t grouped = 0, groups = 0;
    for (int s = 0; s <= 8; ++s) {
        grouped += static_cast<uint64_t>(s) * st.group_size[s];
        groups += st.group_size[s];
    }
    printf("calls %llu (topk %llu), solo %llu, groups %llu, grouped %llu, engine hand-backs %llu\n",
           static_cast<unsigned long long>(st.n_calls), static_cast<unsigned long long>(total_calls),
           static_cast<unsigned long long>(st.n_solo), static_cast<unsigned long long>(st.n_groups),
           static_cast<unsigned long long>(st.n_grouped_queries), static_cast<unsigned long long>(st.n_engine_handbacks));
    if (grouped != st.n_grouped_queries || groups != st.n_groups || st.n_solo + st.n_grouped_queries != st.n_calls ||
        st.n_calls < total_calls) {
        fprintf(stderr, "tsan_coalesce: the statistics do not add up\n");
        g_fail++;
    }
    if (st.n_groups == 0 || st.n_engine_handbacks == 0) {
        fprintf(stderr, "tsan_coalesce: no group formed / no engine hand-back\n");
        g_fail++;
    }
    CHECK(rlr_index_destroy(ix));
    if (g_fail.load()) {
        fprintf(stderr, "tsan_coalesce: %d failures\n", g_fail.load());
        return 1;
    }
    printf("tsan_coalesce ok\n");
    return 0;
}
