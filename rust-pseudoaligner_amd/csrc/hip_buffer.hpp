// Owning HIP allocations of the host runtime and its one check of a HIP call's status.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

#include "pa_common.hpp"

// a HIP call that fails returns PA_ERR_HIP from the enclosing function (the call's text and HIP's message in pa_last_error())
#define PA_HIP_TRY(call)                                                                                        \
    do {                                                                                                        \
        const hipError_t e_ = (call);                                                                           \
        if (e_ != hipSuccess) return ::pa::fail(PA_ERR_HIP, "%s: %s", #call, hipGetErrorString(e_));            \
    } while (0)

namespace pa {

enum class Mem { device, pinned };

// Exactly n elements of T in HBM (hipMalloc) or in pinned host memory (hipHostMalloc, default flags), freed with the matching call
// on release(), on the next alloc() and on destruction. Move-only. Sizes are the caller's: nothing is rounded up here.
template <class T, Mem M>
class HipBuffer {
public:
    HipBuffer() = default;
    HipBuffer(HipBuffer&& o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr; o.n_ = 0; }
    HipBuffer& operator=(HipBuffer&& o) noexcept {
        if (this != &o) {
            release();
            p_ = o.p_; n_ = o.n_;
            o.p_ = nullptr; o.n_ = 0;
        }
        return *this;
    }
    ~HipBuffer() { release(); }

    // frees what is held, then allocates n elements; on failure the buffer is empty and PA_ERR_OOM is returned
    int alloc(size_t n) {
        release();
        void* p = nullptr;
        const size_t bytes = n * sizeof(T);
        const hipError_t e = M == Mem::device ? hipMalloc(&p, bytes) : hipHostMalloc(&p, bytes, hipHostMallocDefault);
        if (e != hipSuccess) return fail(PA_ERR_OOM, "%s(%zu): %s", M == Mem::device ? "hipMalloc" : "hipHostMalloc", bytes, hipGetErrorString(e));
        p_ = static_cast<T*>(p);
        n_ = n;
        return PA_OK;
    }
    // nothing while at least `need` elements are held, else alloc(want)
    int reserve(size_t need, size_t want) { return n_ >= need ? PA_OK : alloc(want); }
    void release() {
        if (p_) (void)(M == Mem::device ? hipFree(p_) : hipHostFree(p_));
        p_ = nullptr;
        n_ = 0;
    }

    T* get() const { return p_; }
    template <class U> U* as() const { return reinterpret_cast<U*>(p_); }
    size_t size() const { return n_; }

private:
    T* p_ = nullptr;
    size_t n_ = 0;
};

template <class T> using DeviceBuffer = HipBuffer<T, Mem::device>;
template <class T> using PinnedBuffer = HipBuffer<T, Mem::pinned>;

}  // namespace pa
