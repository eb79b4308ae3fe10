// pt_devmem.hpp — who owns memory: every device and pinned host allocation of a context, a multi-stream group or a single call is one of these.
// Host code only.  The kernels' argument structs (State, DevScene, Batch, the *Job structs) keep raw pointers, copied from the owners beside them.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

// Move-only owner of one allocation, readable wherever a T* is.  ON_DEVICE: hipMalloc / hipFree; else pinned host memory, hipHostMalloc with
// HOST_FLAGS / hipHostFree.  Freed by release() or when the owner goes: the owner of the owner sees to it that the device is idle and, for
// another device's memory, current by then.  Used under its two names below.
template <typename T, bool ON_DEVICE, unsigned HOST_FLAGS>
struct Owned {
    T* p = nullptr;
    size_t bytes = 0;
    Owned() = default;
    Owned(const Owned&) = delete;
    Owned& operator=(const Owned&) = delete;
    Owned(Owned&& o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr; o.bytes = 0; }
    Owned& operator=(Owned&& o) noexcept {
        if (this != &o) { release(); p = o.p; bytes = o.bytes; o.p = nullptr; o.bytes = 0; }
        return *this;
    }
    ~Owned() { release(); }
    operator T*() const { return p; }
    T* operator->() const { return p; }
    hipError_t release() {
        if (!p) return hipSuccess;
        void* q = (void*)p;
        p = nullptr; bytes = 0;
        if constexpr (ON_DEVICE) return hipFree(q); else return hipHostFree(q);
    }
    // a fresh allocation of n bytes, whatever was there (contents undefined)
    hipError_t reset(size_t n) {
        hipError_t e = release();
        if (e != hipSuccess) return e;
        void* q = nullptr;
        if constexpr (ON_DEVICE) e = hipMalloc(&q, n); else e = hipHostMalloc(&q, n, HOST_FLAGS);
        if (e == hipSuccess) { p = (T*)q; bytes = n; }
        return e;
    }
    // at least n bytes: allocates when there is nothing or too little, else keeps the allocation and the pointers handed out
    hipError_t ensure(size_t n) { return p && bytes >= n ? hipSuccess : reset(n); }
    // a fresh allocation of n bytes (16 for none) with src, when given, copied in on stream s
    hipError_t upload(const void* src, size_t n, hipStream_t s) {
        const hipError_t e = reset(n ? n : 16);
        return e == hipSuccess && src && n ? hipMemcpyAsync(p, src, n, hipMemcpyHostToDevice, s) : e;
    }
};
template <typename T>
using Dev = Owned<T, true, 0>;
template <typename T, unsigned HOST_FLAGS = hipHostMallocDefault>
using Pinned = Owned<T, false, HOST_FLAGS>;
