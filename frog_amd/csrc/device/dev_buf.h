// dev_buf.h -- the owning device allocation of libfrog_hip.so (the solver context in ctx.h, the transform chains in chain.hip).
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <utility>
#include <vector>

namespace frog {

// Owning device allocation.
// alloc() keeps the old block when it is large enough (lattices are re-created many
// times per run; hipFree/hipMalloc synchronise the device and cost milliseconds).
template <class T> struct DevBuf {
    T *p = nullptr;
    size_t n = 0;
    size_t cap = 0;
    bool borrowed = false;      // p points into another DevBuf's block (borrow()): nothing to free
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { release(); }
    void release()
    {
        if (p && !borrowed) (void)hipFree(p);
        p = nullptr; n = 0; cap = 0; borrowed = false;
    }
    void borrow(T *from, size_t count) { release(); p = from; n = count; cap = count; borrowed = true; }
    // (the solver's lattices change roles this way; they are only ever alloc()'d -- GridRecord::kept* alone borrow -- but ownership travels with the block)
    void swap(DevBuf &o) { std::swap(p, o.p); std::swap(n, o.n); std::swap(cap, o.cap); std::swap(borrowed, o.borrowed); }
    // `reserve` (>= count): capacity to allocate when a new block is needed at all
    hipError_t alloc(size_t count, size_t reserve = 0)
    {
        if (count <= cap && p) { n = count; return hipSuccess; }
        release();
        if (!count) return hipSuccess;
        const size_t want = reserve > count ? reserve : count;
        hipError_t e = hipMalloc((void **)&p, want * sizeof(T));
        if (e != hipSuccess && want > count) {              // no room for the head-room: take what is needed
            (void)hipGetLastError();
            e = hipMalloc((void **)&p, count * sizeof(T));
            if (e == hipSuccess) { n = count; cap = count; }
            return e;
        }
        if (e == hipSuccess) { n = count; cap = want; }
        return e;
    }
    // stream-ordered allocation from the device's pool: no device synchronisation (used on the regrid path)
    hipError_t alloc_async(size_t count, hipStream_t s)
    {
        release();
        if (!count) return hipSuccess;
        hipError_t e = hipMallocAsync((void **)&p, count * sizeof(T), s);
        if (e != hipSuccess) { (void)hipGetLastError(); return alloc(count); }
        n = count; cap = count;
        return e;
    }
    template <class A> hipError_t upload(const std::vector<T, A> &v, hipStream_t s)
    {
        hipError_t e = alloc(v.size());
        if (e != hipSuccess || v.empty()) return e;
        return hipMemcpyAsync(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, s);
    }
    size_t bytes() const { return n * sizeof(T); }
};

} // namespace frog
