// TEST INFRASTRUCTURE -- csrc/device_buffer.h under AddressSanitizer + UBSan on the CPU.  "Device" and pinned memory are
// malloc'ed here, so a double free, a use after a move or a leak of the owners is the sanitizer's to find; the stand-ins
// count live allocations and fail the N-th allocation on request, which is how the all-or-none rule of reserve_group is
// driven through every position.  Nothing here ships (see tests/test_host_sanitize_cpu.py).
#include "../../rust-local-rag_amd/csrc/device_buffer.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>

namespace {
int g_live_dev = 0, g_live_pin = 0;
int g_allocs = 0;   // allocations asked for since the last arm()
int g_fail_at = -1; // the g_fail_at-th of them (from 0) fails

void arm(int fail_at)
{
    g_allocs = 0;
    g_fail_at = fail_at;
}

bool refuse() { return g_allocs++ == g_fail_at; }

#define CHECK(cond)                                                         \
    do {                                                                    \
        if (!(cond)) {                                                      \
            std::printf("devbuf_san: %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                   \
        }                                                                   \
    } while (0)
} // namespace

namespace rlr {
hipError_t dev_malloc(void **p, size_t bytes)
{
    if (refuse())
        return hipErrorOutOfMemory;
    *p = std::malloc(bytes ? bytes : 1);
    std::memset(*p, 0xFF, bytes);
    g_live_dev++;
    return hipSuccess;
}
} // namespace rlr

extern "C" {
hipError_t hipFree(void *p)
{
    if (p) {
        g_live_dev--;
        std::free(p);
    }
    return hipSuccess;
}
hipError_t hipHostMalloc(void **p, size_t bytes, unsigned int flags)
{
    CHECK(flags == hipHostMallocDefault);
    if (refuse())
        return hipErrorOutOfMemory;
    *p = std::malloc(bytes ? bytes : 1);
    g_live_pin++;
    return hipSuccess;
}
hipError_t hipHostFree(void *p)
{
    if (p) {
        g_live_pin--;
        std::free(p);
    }
    return hipSuccess;
}
}

using rlr::DevBuf;
using rlr::PinBuf;
using rlr::Want;

static void test_reserve()
{
    arm(-1);
    DevBuf<float> b;
    CHECK(!b && b.get() == nullptr && b.capacity() == 0);
    CHECK(b.reserve(0) == hipSuccess && !b && g_allocs == 0); // nothing asked for, nothing allocated
    CHECK(b.reserve(100) == hipSuccess && b && b.capacity() == 100 && g_live_dev == 1);
    b.get()[99] = 1.0f; // (the sanitizer checks the extent)
    float *const first = b.get();
    CHECK(b.reserve(100) == hipSuccess && b.get() == first && g_allocs == 1); // equal: untouched
    CHECK(b.reserve(7) == hipSuccess && b.get() == first && b.capacity() == 100 && g_allocs == 1); // smaller: untouched
    CHECK(b.reserve(101) == hipSuccess && b.capacity() == 101 && g_allocs == 2 && g_live_dev == 1); // exactly what was asked
    b.get()[100] = 2.0f;
    // a failed regrow leaves the buffer empty, not stale
    arm(0);
    CHECK(b.reserve(1000) == hipErrorOutOfMemory && !b && b.capacity() == 0 && g_live_dev == 0);
    arm(-1);
    CHECK(b.reserve(5) == hipSuccess && b.capacity() == 5 && g_live_dev == 1);
    b.reset();
    CHECK(!b && b.capacity() == 0 && g_live_dev == 0);
    b.reset(); // twice is once
    CHECK(g_live_dev == 0);

    PinBuf h;
    CHECK(h.reserve(64) == hipSuccess && h && h.capacity() == 64 && g_live_pin == 1);
    static_cast<char *>(h.get())[63] = 1;
    void *const hp = h.get();
    CHECK(h.reserve(64) == hipSuccess && h.reserve(1) == hipSuccess && h.get() == hp);
    CHECK(h.reserve(65) == hipSuccess && h.capacity() == 65 && g_live_pin == 1);
    arm(0);
    CHECK(h.reserve(4096) == hipErrorOutOfMemory && !h && h.capacity() == 0 && g_live_pin == 0);
    arm(-1);
    CHECK(h.reserve(8) == hipSuccess && g_live_pin == 1);
} // (h is freed by its destructor)

static void test_moves()
{
    arm(-1);
    DevBuf<int> a;
    CHECK(a.reserve(10) == hipSuccess);
    a.get()[3] = 42;
    int *const p = a.get();
    DevBuf<int> b(std::move(a));
    CHECK(!a && a.capacity() == 0 && b.get() == p && b.capacity() == 10 && b.get()[3] == 42 && g_live_dev == 1);
    DevBuf<int> c;
    CHECK(c.reserve(3) == hipSuccess && g_live_dev == 2);
    c = std::move(b); // frees what c held
    CHECK(!b && c.get() == p && c.capacity() == 10 && g_live_dev == 1);
    DevBuf<int> &self = c;
    c = std::move(self);
    CHECK(c.get() == p && c.capacity() == 10 && g_live_dev == 1);
    CHECK(a.reserve(2) == hipSuccess && g_live_dev == 2); // a moved-from buffer is an empty one

    PinBuf h, g;
    CHECK(h.reserve(16) == hipSuccess && g.reserve(32) == hipSuccess && g_live_pin == 2);
    void *const hp = h.get();
    g = std::move(h);
    CHECK(!h && g.get() == hp && g.capacity() == 16 && g_live_pin == 1);
    PinBuf k(std::move(g));
    CHECK(!g && k.get() == hp && g_live_pin == 1);
}

// a group of four (three device buffers of different element types and one pinned): a failure at every position
static void test_group()
{
    for (int fail_at = -1; fail_at < 4; ++fail_at) {
        DevBuf<float> a;
        DevBuf<double> b;
        DevBuf<char> c;
        PinBuf h;
        DevBuf<int> bystander; // not of the group: survives whatever happens to it
        arm(-1);
        CHECK(bystander.reserve(1) == hipSuccess);
        CHECK(rlr::reserve_group(Want{a, 4}, Want{b, 4}, Want{c, 8}, Want{h, 16}) == hipSuccess);
        CHECK(a.capacity() == 4 && b.capacity() == 4 && c.capacity() == 8 && h.capacity() == 16);
        CHECK(g_live_dev == 4 && g_live_pin == 1 && g_allocs == 5);
        float *const pa = a.get();
        CHECK(rlr::reserve_group(Want{a, 4}, Want{b, 2}, Want{c, 8}, Want{h, 1}) == hipSuccess); // fits: untouched
        CHECK(a.get() == pa && g_allocs == 5);
        arm(fail_at);
        // one member too small: all four are rebuilt
        const hipError_t e = rlr::reserve_group(Want{a, 4}, Want{b, 9}, Want{c, 8}, Want{h, 16});
        if (fail_at < 0) {
            CHECK(e == hipSuccess && a.capacity() == 4 && b.capacity() == 9 && c.capacity() == 8 && h.capacity() == 16);
            CHECK(g_allocs == 4 && g_live_dev == 4 && g_live_pin == 1);
            b.get()[8] = 1.0;
        } else {
            CHECK(e == hipErrorOutOfMemory && g_allocs == fail_at + 1); // (nothing is tried behind the failure)
            CHECK(!a && !b && !c && !h);
            CHECK(a.capacity() == 0 && b.capacity() == 0 && c.capacity() == 0 && h.capacity() == 0);
            CHECK(g_live_dev == 1 && g_live_pin == 0); // the bystander alone
            arm(-1);
            CHECK(rlr::reserve_group(Want{a, 1}, Want{b, 1}, Want{c, 1}, Want{h, 1}) == hipSuccess); // and the next call rebuilds it
            CHECK(g_live_dev == 4 && g_live_pin == 1);
        }
        CHECK(bystander && bystander.capacity() == 1);
    }
}

int main()
{
    test_reserve();
    CHECK(g_live_dev == 0 && g_live_pin == 0);
    test_moves();
    CHECK(g_live_dev == 0 && g_live_pin == 0);
    test_group();
    CHECK(g_live_dev == 0 && g_live_pin == 0);
    std::printf("devbuf_san ok\n");
    return 0;
}
