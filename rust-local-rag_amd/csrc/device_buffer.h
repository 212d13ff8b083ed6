// device_buffer.h -- the owners of the library's device and pinned host memory.  A buffer is a member or a local of one
// of these types and is freed by its destructor; how much to ask for (floors, headroom, zero fill) is the call site's
// business.  reserve() frees before it allocates, so a failed regrow leaves the buffer EMPTY (null, capacity 0), never
// stale: the call that needed it fails, and the next one reserves again.
#pragma once

#include <hip/hip_runtime_api.h>
#include <stddef.h>

namespace rlr {

hipError_t dev_malloc(void **p, size_t bytes); // index.hip: the library's only hipMalloc (RLR_POISON_ALLOC=1 fills it)

// One device allocation of `capacity()` elements of T.
template <typename T>
class DevBuf {
public:
    DevBuf() = default;
    DevBuf(DevBuf &&o) noexcept : p_(o.p_), cap_(o.cap_) { o.p_ = nullptr, o.cap_ = 0; }
    DevBuf &operator=(DevBuf &&o) noexcept
    {
        if (this != &o) {
            reset();
            p_ = o.p_, cap_ = o.cap_;
            o.p_ = nullptr, o.cap_ = 0;
        }
        return *this;
    }
    ~DevBuf() { reset(); }

    // at least n elements; the contents do not survive a regrow
    hipError_t reserve(size_t n)
    {
        if (cap_ >= n)
            return hipSuccess;
        reset();
        void *p = nullptr;
        const hipError_t e = dev_malloc(&p, n * sizeof(T));
        if (e == hipSuccess)
            p_ = static_cast<T *>(p), cap_ = n;
        return e;
    }
    void reset()
    {
        if (p_)
            (void)hipFree(p_);
        p_ = nullptr, cap_ = 0;
    }
    T *get() const { return p_; }
    size_t capacity() const { return cap_; }
    explicit operator bool() const { return p_ != nullptr; }

private:
    T *p_ = nullptr;
    size_t cap_ = 0;
};

// One pinned host allocation (hipHostMallocDefault) of `capacity()` bytes.
class PinBuf {
public:
    PinBuf() = default;
    PinBuf(PinBuf &&o) noexcept : p_(o.p_), cap_(o.cap_) { o.p_ = nullptr, o.cap_ = 0; }
    PinBuf &operator=(PinBuf &&o) noexcept
    {
        if (this != &o) {
            reset();
            p_ = o.p_, cap_ = o.cap_;
            o.p_ = nullptr, o.cap_ = 0;
        }
        return *this;
    }
    ~PinBuf() { reset(); }

    hipError_t reserve(size_t bytes)
    {
        if (cap_ >= bytes)
            return hipSuccess;
        reset();
        const hipError_t e = hipHostMalloc(&p_, bytes, hipHostMallocDefault);
        if (e == hipSuccess)
            cap_ = bytes;
        else
            p_ = nullptr;
        return e;
    }
    void reset()
    {
        if (p_)
            (void)hipHostFree(p_);
        p_ = nullptr, cap_ = 0;
    }
    void *get() const { return p_; }
    size_t capacity() const { return cap_; }
    explicit operator bool() const { return p_ != nullptr; }

private:
    void *p_ = nullptr;
    size_t cap_ = 0;
};

// Buffers that are sized by one shared count grow together: reserve_group(Want{a, n_a}, Want{b, n_b}, ...).  If any of
// them is too small all are freed first and then allocated in the order given; on a failure the whole group is left
// empty, so no member can be null beside a sibling whose capacity says the group is ready.
template <typename B>
struct Want {
    B &buf;
    size_t n;
};
template <typename B>
Want(B &, size_t) -> Want<B>;

template <typename... B>
hipError_t reserve_group(Want<B>... w)
{
    if ((... && (w.buf.capacity() >= w.n)))
        return hipSuccess;
    (w.buf.reset(), ...);
    hipError_t e = hipSuccess;
    ((e = e == hipSuccess ? w.buf.reserve(w.n) : e), ...);
    if (e != hipSuccess)
        (w.buf.reset(), ...);
    return e;
}

} // namespace rlr
