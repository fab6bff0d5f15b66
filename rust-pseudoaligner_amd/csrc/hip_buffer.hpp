// Owning HIP allocations of the host runtime, its one check of a HIP call's status, and what every driver that launches on a stream of its own
// needs around pa_map_batch_device: the owner of that stream and the one rule for a mapping whose arena turned out too small.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <vector>

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
    size_t size() const { return n_; }

private:
    T* p_ = nullptr;
    size_t n_ = 0;
};

template <class T> using DeviceBuffer = HipBuffer<T, Mem::device>;
template <class T> using PinnedBuffer = HipBuffer<T, Mem::pinned>;

// grow-only device scratch of `need` elements: a quarter more than asked for (and 256 bytes' worth) when it has to grow
template <class T> int grow(DeviceBuffer<T>& b, size_t need) { return b.reserve(need, need + (need + 3) / 4 + 256 / sizeof(T)); }

// n elements to a new device buffer (16 bytes when there are none)
template <class T> int upload(DeviceBuffer<T>& dst, const T* src, size_t n) {
    const int e = dst.alloc(n ? n : 16 / sizeof(T));
    if (e != PA_OK) return e;
    if (n) PA_HIP_TRY(hipMemcpy(dst.get(), src, n * sizeof(T), hipMemcpyHostToDevice));
    return PA_OK;
}
template <class T> int upload(DeviceBuffer<T>& dst, const std::vector<T>& src) { return upload(dst, src.data(), src.size()); }

// makes `device` current; PA_ERR_NO_DEVICE without a usable GPU, PA_ERR_INVALID_ARG for a device that does not exist (device_plumbing.hip)
int use_device(int device);
// PA_ERR_NO_DEVICE without a usable GPU; the current device stays as it is (device_plumbing.hip)
int have_device();

// A non-blocking stream that launches on `idx`. The index keeps a launch context per stream (2 GB of list-mode rows): a stream that is
// destroyed without pa_index_release_stream strands it there. release() and destruction: synchronise, release the context, destroy.
// Move-only.
class IndexStream {
public:
    IndexStream() = default;
    IndexStream(IndexStream&& o) noexcept : idx_(o.idx_), s_(o.s_) { o.s_ = nullptr; }
    IndexStream& operator=(IndexStream&& o) noexcept { if (this != &o) { release(); idx_ = o.idx_; s_ = o.s_; o.s_ = nullptr; } return *this; }
    ~IndexStream() { release(); }
    int create(pa_index* idx) { release(); PA_HIP_TRY(hipStreamCreateWithFlags(&s_, hipStreamNonBlocking)); idx_ = idx; return PA_OK; }
    void release() {
        if (!s_) return;
        (void)hipStreamSynchronize(s_); (void)pa_index_release_stream(idx_, s_); (void)hipStreamDestroy(s_);
        s_ = nullptr;
    }
    hipStream_t get() const { return s_; }

private:
    pa_index* idx_ = nullptr;
    hipStream_t s_ = nullptr;
};

// finish(&need) — pa_map_finish of a mapping, or its equal for a caller that holds the launch context's lock; while it answers PA_ERR_ARENA_FULL,
// at most three times, the arena is reallocated to an eighth more than was needed plus 4096 entries and relaunch() (a pa_status: everything the
// caller enqueued that wrote into the arena, the mapping first) runs again. Any other status is returned as it is.
template <class Finish, class Relaunch>
int map_finish_regrow(DeviceBuffer<uint32_t>& arena, Finish&& finish, Relaunch&& relaunch) {
    uint64_t need = 0;
    int e = finish(&need);
    for (int attempt = 0; e == PA_ERR_ARENA_FULL && attempt < 3; ++attempt) {
        if ((e = arena.alloc(need + need / 8 + 4096)) != PA_OK) return e;
        e = relaunch();
        if (e == PA_OK) e = finish(&need);
    }
    return e;
}
// ... with pa_map_finish on `stream`; *used = the arena entries of the mapping that was finished last
template <class Relaunch>
int map_finish_regrow(pa_index* idx, hipStream_t stream, DeviceBuffer<uint32_t>& arena, uint64_t* used, Relaunch&& relaunch) {
    return map_finish_regrow(arena, [&](uint64_t* need) { return pa_map_finish(idx, stream, used, need); }, relaunch);
}

}  // namespace pa
