// Device-wide primitives of the host runtime's setup paths (sorts, scans, run-length encodes, reductions by key, compactions):
// the one place rocPRIM is called from, and the one place its two-phase protocol ("ask for the scratch bytes, allocate, call
// again") is written; and the "collapse" of sorted items into their runs (collapse_runs and its two kernels), which index_build.hip's
// own pa_ib_heads_kernel (64-bit counts, other outputs) does not use. Host side; included by .hip sources only: barcode_counts.hip,
// bus.hip, bus_correct.hip, bus_knee.hip, bus_umi.hip, compact.hip, fastq_scan.hip, genes.hip (both through molecule_stage.hpp too), index_build.hip,
// pair_scan.hip, pairs.hip and strands.hip (through pair_stage.hpp), quant.hip, quant_boot.hip, render.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <cstring>   // (before rocPRIM: its texture iterator calls memset without including it)

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_reduce_by_key.hpp>
#include <rocprim/device/device_run_length_encode.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/device/device_select.hpp>
#include <rocprim/iterator/counting_iterator.hpp>

#include <type_traits>

#include "hip_buffer.hpp"

namespace pa {

// blocks of `block` threads that cover n items; 0 when that count does not fit 32 bits (a launch of no blocks fails, where a count cut
// to its low 32 bits would run a small grid over the first few items and say nothing)
inline uint32_t grid_for(uint64_t n, uint32_t block = 256) {
    const uint64_t blocks = n / block + (n % block != 0);
    return blocks > 0xFFFFFFFFull ? 0u : (uint32_t)blocks;
}

// bits that hold 0..max_value: 0 for 0, 64 at most (a radix sort wants at least one: std::max(1u, bits_for(v)))
inline uint32_t bits_for(uint64_t max_value) {
    uint32_t b = 0;
    while (b < 64 && (max_value >> b) != 0) ++b;
    return b;
}

// the element at d once everything before it on the stream is done
template <class T>
int fetch(const T* d, hipStream_t s, T& out) {
    PA_HIP_TRY(hipMemcpyAsync(&out, d, sizeof(T), hipMemcpyDeviceToHost, s));
    PA_HIP_TRY(hipStreamSynchronize(s));
    return PA_OK;
}
inline int fetch_u32(const uint32_t* d, hipStream_t s, uint32_t& out) { return fetch(d, s, out); }

// kernel<<<blocks, block, 0, s>>>(args...) and the status of the launch
template <class... P, class... A>
int launch(void (*kernel)(P...), uint32_t blocks, uint32_t block, hipStream_t s, A... args) {
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(block), 0, s, args...);
    PA_HIP_TRY(hipGetLastError());
    return PA_OK;
}

// fn(void* scratch, size_t& bytes) -> hipError_t is one rocPRIM call: with a null scratch it only reports the bytes it needs.
// prim_bytes is that query alone, for callers that carve the scratch out of a block they were given.
template <class F>
size_t prim_bytes(F&& fn) {
    size_t bytes = 0;
    (void)fn(nullptr, bytes);
    return bytes;
}

// The query, then the call on `tmp`, which grows to the largest request of its chain of operations and never shrinks (rocPRIM asks
// for at least 4 bytes, so the second call never sees a null scratch). Growing it while earlier work of the stream may still read
// the old block is safe: alloc() frees that block with hipFree, which waits for the device.
template <class F>
int prim_call(DeviceBuffer<uint8_t>& tmp, F&& fn) {
    size_t bytes = 0;
    PA_HIP_TRY(fn(nullptr, bytes));
    if (bytes > tmp.size()) {
        const int e = tmp.alloc(bytes);
        if (e != PA_OK) return e;
    }
    PA_HIP_TRY(fn(tmp.get(), bytes));
    return PA_OK;
}

// ---- the operations the project uses, each on stream s with its scratch in tmp ----

// Stable radix sorts over the key bits [begin_bit, end_bit). rocPRIM indexes with 32 bits when the count's type has 32 and with
// 64 bits otherwise, and these are different kernels: the count goes on in the type the caller gives it.
template <class K, class N>
int sort_keys(hipStream_t s, DeviceBuffer<uint8_t>& tmp, const K* in, K* out, N n, uint32_t begin_bit, uint32_t end_bit) {
    static_assert(std::is_integral<N>::value, "the count of a sort is an integer");
    return prim_call(tmp, [&](void* t, size_t& b) { return rocprim::radix_sort_keys(t, b, in, out, n, begin_bit, end_bit, s); });
}
template <class K, class V, class N>
int sort_pairs(hipStream_t s, DeviceBuffer<uint8_t>& tmp, const K* kin, K* kout, const V* vin, V* vout, N n, uint32_t begin_bit, uint32_t end_bit) {
    static_assert(std::is_integral<N>::value, "the count of a sort is an integer");
    return prim_call(tmp, [&](void* t, size_t& b) { return rocprim::radix_sort_pairs(t, b, kin, kout, vin, vout, n, begin_bit, end_bit, s); });
}
template <class K, class V, class N>
int sort_pairs_desc(hipStream_t s, DeviceBuffer<uint8_t>& tmp, const K* kin, K* kout, const V* vin, V* vout, N n, uint32_t begin_bit, uint32_t end_bit) {
    static_assert(std::is_integral<N>::value, "the count of a sort is an integer");
    return prim_call(tmp, [&](void* t, size_t& b) { return rocprim::radix_sort_pairs_desc(t, b, kin, kout, vin, vout, n, begin_bit, end_bit, s); });
}

// out[i] = in[0] + .. + in[i], summed as Out
template <class In, class Out>
int scan_inclusive(hipStream_t s, DeviceBuffer<uint8_t>& tmp, const In* in, Out* out, size_t n) {
    return prim_call(tmp, [&](void* t, size_t& b) { return rocprim::inclusive_scan(t, b, in, out, n, rocprim::plus<Out>(), s); });
}

// ... and total = out[n - 1] on the host (n >= 1; synchronises s)
template <class In, class Out>
int scan_inclusive_total(hipStream_t s, DeviceBuffer<uint8_t>& tmp, const In* in, Out* out, size_t n, Out& total) {
    const int e = scan_inclusive(s, tmp, in, out, n);
    return e != PA_OK ? e : fetch((const Out*)out + (n - 1), s, total);
}

// out[i] = in[0] + .. + in[i - 1], summed as Out (out[0] = 0). This is the rocPRIM call itself, for prim_bytes and for callers with
// a scratch block of their own; scan_exclusive below is the same on `tmp`.
template <class In, class Out>
hipError_t scan_exclusive_on(void* scratch, size_t& bytes, const In* in, Out* out, size_t n, hipStream_t s) {
    return rocprim::exclusive_scan(scratch, bytes, in, out, Out(0), n, rocprim::plus<Out>(), s);
}
template <class In, class Out>
int scan_exclusive(hipStream_t s, DeviceBuffer<uint8_t>& tmp, const In* in, Out* out, size_t n) {
    return prim_call(tmp, [&](void* t, size_t& b) { return scan_exclusive_on(t, b, in, out, n, s); });
}

// runs of equal consecutive keys -> unique[r], counts[r]; *d_runs = their number (n below 2^32)
template <class K>
int run_length_encode(hipStream_t s, DeviceBuffer<uint8_t>& tmp, const K* in, size_t n, K* unique, uint32_t* counts, uint32_t* d_runs) {
    return prim_call(tmp, [&](void* t, size_t& b) { return rocprim::run_length_encode(t, b, in, (unsigned int)n, unique, counts, d_runs, s); });
}

// runs of equal consecutive keys -> unique[r], sums[r] = the sum of the run's values; *d_runs = their number
template <class K, class V>
int reduce_by_key_sum(hipStream_t s, DeviceBuffer<uint8_t>& tmp, const K* kin, const V* vin, size_t n, K* unique, V* sums, uint32_t* d_runs) {
    return prim_call(tmp, [&](void* t, size_t& b) {
        return rocprim::reduce_by_key(t, b, kin, vin, n, unique, sums, d_runs, rocprim::plus<V>(), rocprim::equal_to<K>(), s);
    });
}

// the indices i in [0, n) with flags[i] != 0, ascending; *d_count = their number
template <class I>
int select_flagged_indices(hipStream_t s, DeviceBuffer<uint8_t>& tmp, const uint32_t* flags, size_t n, I* out, uint32_t* d_count) {
    return prim_call(tmp, [&](void* t, size_t& b) { return rocprim::select(t, b, rocprim::counting_iterator<I>(0), flags, out, d_count, n, s); });
}

// ---- the collapse of sorted items: flag the first of every run, scan, scatter ----
constexpr uint32_t RUN_BLOCK = 256;   // 4 waves

// key_at(i), the key of item i as a kernel reads it: an array of keys, or the barcode field of BUS records
template <class K>
struct KeyArray {
    typedef K key_type;
    const K* keys;
    __device__ K operator()(uint32_t i) const { return keys[i]; }
};
struct RecordBarcode {
    typedef unsigned long long key_type;
    const pa_bus_record* rec;
    __device__ key_type operator()(uint32_t i) const { return rec[i].barcode; }
};

template <class KeyAt>
__global__ __launch_bounds__(RUN_BLOCK) void pa_run_heads_kernel(const KeyAt key_at, uint32_t n, uint32_t* __restrict__ heads) {
    const uint32_t i = blockIdx.x * RUN_BLOCK + threadIdx.x;
    if (i < n) heads[i] = (i == 0 || key_at(i) != key_at(i - 1)) ? 1u : 0u;
}
// pos = inclusive scan of heads: run r = pos[i] - 1 begins at its head i; with a start: start[r] = i, start[runs] = n
template <class KeyAt>
__global__ __launch_bounds__(RUN_BLOCK) void pa_run_scatter_kernel(const KeyAt key_at, const uint32_t* __restrict__ heads, const uint32_t* __restrict__ pos, uint32_t n,
                                                                    uint32_t runs, typename KeyAt::key_type* __restrict__ unique, uint32_t* __restrict__ start) {
    const uint32_t i = blockIdx.x * RUN_BLOCK + threadIdx.x;
    if (i >= n) return;
    if (heads[i] && pos[i] - 1 < runs) {   // (the bound is the caller's: unique and start have that many entries)
        unique[pos[i] - 1] = key_at(i);
        if (start) start[pos[i] - 1] = i;
    }
    if (start && i == n - 1) start[runs] = n;
}
// The two halves of the collapse, for a caller that sizes `unique` by the run count or flags the heads in a pass of its own.
// n >= 1 sorted items -> heads[n] (1 at the first of every run), pos[n] (their inclusive scan), runs = pos[n - 1]; synchronises s
template <class KeyAt>
int flag_runs(hipStream_t s, DeviceBuffer<uint8_t>& tmp, KeyAt key_at, uint32_t n, uint32_t* heads, uint32_t* pos, uint32_t& runs) {
    const int e = launch(pa_run_heads_kernel<KeyAt>, grid_for(n, RUN_BLOCK), RUN_BLOCK, s, key_at, n, heads);
    return e != PA_OK ? e : scan_inclusive_total(s, tmp, (const uint32_t*)heads, pos, (size_t)n, runs);
}
// heads, pos and runs as flag_runs leaves them -> unique[runs] and, unless start is null, start[runs + 1]
template <class KeyAt>
int scatter_runs(hipStream_t s, KeyAt key_at, const uint32_t* heads, const uint32_t* pos, uint32_t n, uint32_t runs, typename KeyAt::key_type* unique, uint32_t* start) {
    return launch(pa_run_scatter_kernel<KeyAt>, grid_for(n, RUN_BLOCK), RUN_BLOCK, s, key_at, heads, pos, n, runs, unique, start);
}
// n >= 1 sorted items -> unique[runs], start[runs + 1] (start may be null); heads[n] and pos[n] hold the flags and their scan afterwards
template <class KeyAt>
int collapse_runs(hipStream_t s, DeviceBuffer<uint8_t>& tmp, KeyAt key_at, uint32_t n, uint32_t* heads, uint32_t* pos, typename KeyAt::key_type* unique, uint32_t* start,
                  uint32_t& runs) {
    const int e = flag_runs(s, tmp, key_at, n, heads, pos, runs);
    return e != PA_OK ? e : scatter_runs(s, key_at, (const uint32_t*)heads, (const uint32_t*)pos, n, runs, unique, start);
}

}  // namespace pa
