// dev_mem.h -- the two owners of the C ABI glue's memory (host code only; needs nothing but the HIP runtime API header).
//   DevBuf<T>: hipMalloc / hipFree          PinBuf<T>: hipHostMalloc(hipHostMallocDefault) / hipHostFree
// An owner holds the pointer and the byte count, frees in its destructor, and can be moved and swapped but not copied -- "build the new
// block beside the old one, then replace it" is a move assignment or a swap.  A buffer of the library is a member or a local of one of
// these types and is never freed by hand.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <utility>

namespace dpmm {

#ifdef DPMM_POISON
// Diagnostic build (scripts/build_variant.sh poison -DDPMM_POISON=0xFF): every device allocation of the library is filled with the poison
// byte before anybody uses it -- a kernel that reads memory nobody wrote then reads NaNs / -1 on EVERY box, not only on one whose memory
// holds another process's leftovers.  (Built while a one-in-twenty chain divergence on fresh boxes was tracked down: it ruled device MEMORY
// out; the cause was a never-written LDS word, found with tests/tools/poison.py -- DESIGN section 5.)
inline hipError_t dev_malloc(void **p, size_t n) {
    hipError_t e = hipMalloc(p, n);
    if (e == hipSuccess && n > 0) { e = hipMemset(*p, DPMM_POISON, n); if (e == hipSuccess) e = hipDeviceSynchronize(); }
    return e;
}
#else
inline hipError_t dev_malloc(void **p, size_t n) { return hipMalloc(p, n); }
#endif

// Pinned = false: device memory; true: pinned host memory.  Use the two names below.
template <typename T, bool Pinned>
struct Owned {
    T *ptr = nullptr;
    size_t bytes = 0;

    Owned() = default;
    Owned(const Owned &) = delete;
    Owned &operator=(const Owned &) = delete;
    Owned(Owned &&o) noexcept : ptr(o.ptr), bytes(o.bytes) { o.ptr = nullptr; o.bytes = 0; }
    Owned &operator=(Owned &&o) noexcept { if (this != &o) { reset(); swap(o); } return *this; }
    ~Owned() { reset(); }

    void reset() {
        if (ptr) (void)(Pinned ? hipHostFree(ptr) : hipFree(ptr));
        ptr = nullptr; bytes = 0;
    }
    void swap(Owned &o) noexcept { std::swap(ptr, o.ptr); std::swap(bytes, o.bytes); }
    // The old block goes first, as in every routine this replaces.  On failure the owner is empty and the HIP error is cleared and returned.
    hipError_t alloc(size_t n) {
        reset();
        void *p = nullptr;
        const hipError_t e = Pinned ? hipHostMalloc(&p, n, hipHostMallocDefault) : dev_malloc(&p, n);
        if (e != hipSuccess) { (void)hipGetLastError(); return e; }
        ptr = static_cast<T *>(p); bytes = n;
        return hipSuccess;
    }
    T *get() const { return ptr; }
    operator T *() const { return ptr; }
};
template <typename T, bool P>
void swap(Owned<T, P> &a, Owned<T, P> &b) noexcept { a.swap(b); }

template <typename T> using DevBuf = Owned<T, false>;
template <typename T> using PinBuf = Owned<T, true>;

// capacity of a buffer grown on demand: exactly `need`, or with a floor the smallest floor * 2^k that holds it
inline size_t grow_capacity(size_t need, size_t floor) {
    if (floor == 0) return need;
    size_t cap = floor;
    while (cap < need) cap *= 2;
    return cap;
}

}  // namespace dpmm
