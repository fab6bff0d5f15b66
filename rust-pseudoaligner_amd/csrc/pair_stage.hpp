// What the two stages behind the map launch share (pairs.hip: two mates -> a pair; strands.hip: two strands -> an item): the control block at
// the start of the caller's scratch and its finish, the scratch layout, the kernels' parameter block, and the device helpers on id lists.
// Private to those two sources.
#pragma once
#include <hip/hip_runtime.h>

#include "device_prims.hpp"
#include "hip_buffer.hpp"
#include "kernel_utils.hpp"
#include "kernels.hpp"
#include "pa_common.hpp"

namespace pa {

constexpr uint32_t PAIR_UNFIT = (uint32_t)PA_MAX_ARENA_ENTRIES;       // class_off of a record whose ids did not fit the arena
constexpr uint32_t PAIR_CTL_BYTES = 256;
constexpr uint64_t PAIR_MAX_PAIRS = 0x7FFFFFF0ull;   // pair and item indices, and 2 n + 1 flags, are 32-bit
static_assert(PA_STRAND_STATS == PA_PAIR_STATS, "both stages keep their stats in one control block");

struct PairCtl {   // the first PAIR_CTL_BYTES of the scratch, zeroed by every launch
    unsigned long long arena_top;                // ids asked for so far (exact: no chunks, no padding)
    unsigned long long stats[PA_PAIR_STATS];
    unsigned long long novel_ctr;                // results on the novel list
    unsigned long long arena_cap;                // of the launch (what the finish clamps arena_used to)
    uint32_t status, pad;
};
static_assert(sizeof(PairCtl) <= PAIR_CTL_BYTES, "the control block fits its slot");

struct PairParams {
    DevIndexView ix;
    const uint32_t* class_table;
    uint64_t class_table_size;
    const pa_read_result *res1, *res2;   // (strands.hip: the sense and the antisense candidate)
    const uint32_t *arena1, *arena2;
    uint32_t n;                  // pairs (below 2^31)
    pa_read_result* results;
    uint32_t* arena;
    uint64_t arena_cap;
    unsigned long long* counts;  // or nullptr
    PairCtl* ctl;
    uint32_t* flags;             // [2n + 1]: lane bin [0, n), wave bin [n, 2n), one zero
    uint32_t* off;               // [2n + 1]: their exclusive scan; off[n] = lane items, off[2n] = all items
    uint32_t* items;             // [n]: pair of every item, lane items first
    uint32_t* novel;             // [2n] {arena offset, length} of the results for the overflow table, or nullptr
};

__device__ __forceinline__ const uint32_t* ids_of(const pa_read_result& r, const uint32_t* arena, const DevIndexView& ix) {
    return (r.class_off & PA_CLASS_REF) ? class_ids(ix, ix.class_ref[r.class_off & ~PA_CLASS_REF]) : arena + r.class_off;
}

// first position in v[lo, hi) whose id is not below a
__device__ __forceinline__ uint32_t lower_bound_ids(const uint32_t* __restrict__ v, uint32_t lo, uint32_t hi, uint32_t a) {
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (v[mid] < a) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// class_of_list (kernel_utils.hpp) for the list {v[t] : bit t of keep}, n = its length: the same hash, the same table
__device__ __forceinline__ uint32_t class_of_masked(const uint32_t* __restrict__ v, uint32_t keep, uint32_t n, const DevIndexView& ix, const uint32_t* class_table,
                                                    uint64_t class_table_size) {
    uint64_t h = 0x243f6a8885a308d3ull ^ n;
    for (uint32_t k = keep; k != 0; k &= k - 1) h = pa_mix64(h ^ v[__ffs((int)k) - 1]) + 0x9e3779b97f4a7c15ull;
    uint64_t j = h % class_table_size;
    for (;;) {
        const uint32_t cand = class_table[j];
        if (cand == NO_CLASS) return cand;
        if (ix.class_len[cand] == n) {
            const uint32_t* ids = class_ids(ix, ix.class_ref[cand]);
            bool eq = true;
            uint32_t o = 0;
            for (uint32_t k = keep; k != 0 && eq; k &= k - 1) eq = ids[o++] == v[__ffs((int)k) - 1];
            if (eq) return cand;
        }
        if (++j == class_table_size) j = 0;
    }
}

// adds the number of lanes whose flag is set to *ctr, one atomic per wave (every lane of the wave calls it)
__device__ __forceinline__ void wave_count(bool flag, unsigned long long* ctr) {
    const unsigned long long m = __ballot(flag);
    if (m != 0 && lane_id() == (uint32_t)__ffsll((long long)m) - 1) atomicAdd(ctr, (unsigned long long)__popcll(m));
}

// the class fields of an item's record (coverage and mismatches are the classify kernel's)
__device__ __forceinline__ void put_class(const PairParams& p, uint32_t pair, uint32_t off, uint32_t len) {
    uint32_t* rec = reinterpret_cast<uint32_t*>(p.results + pair);
    rec[2] = off;
    rec[3] = len;
}

// ---------------------------------------------------------------------------------------------- scratch
inline size_t round256(size_t b) { return (b + 255) & ~(size_t)255; }

struct PairScratch {
    size_t flags, off, items, novel, tmp, tmp_bytes, total;
};
inline PairScratch scratch_layout(uint64_t n) {
    PairScratch s{};
    size_t at = PAIR_CTL_BYTES;
    s.flags = at; at += round256((2 * n + 1) * 4);
    s.off = at;   at += round256((2 * n + 1) * 4);
    s.items = at; at += round256((n + 1) * 4);
    s.novel = at; at += round256((n + 1) * 8);
    s.tmp = at;
    s.tmp_bytes = round256(prim_bytes([&](void* t, size_t& b) { return scan_exclusive_on(t, b, (const uint32_t*)nullptr, (uint32_t*)nullptr, (size_t)(2 * n + 1), nullptr); }));
    s.total = at + s.tmp_bytes;
    return s;
}

// the parameter block of a launch over `lay`, everything but the inputs (res1 / res2 / arena1 / arena2)
inline PairParams stage_params(const PairIndexView& v, uint64_t n, pa_read_result* d_results, uint32_t* d_arena, uint64_t arena_cap, uint64_t* d_counts, void* d_scratch,
                               const PairScratch& lay) {
    uint8_t* base = static_cast<uint8_t*>(d_scratch);
    PairParams p{};
    p.ix = v.dv;
    p.class_table = v.class_table;
    p.class_table_size = v.class_table_size;
    p.n = (uint32_t)n;
    p.results = d_results;
    p.arena = d_arena;
    p.arena_cap = arena_cap > PA_MAX_ARENA_ENTRIES ? PA_MAX_ARENA_ENTRIES : arena_cap;   // offsets leave bit 31 of class_off free
    p.counts = reinterpret_cast<unsigned long long*>(d_counts);
    p.ctl = reinterpret_cast<PairCtl*>(base);
    p.flags = reinterpret_cast<uint32_t*>(base + lay.flags);
    p.off = reinterpret_cast<uint32_t*>(base + lay.off);
    p.items = reinterpret_cast<uint32_t*>(base + lay.items);
    p.novel = (d_counts && v.ovf) ? reinterpret_cast<uint32_t*>(base + lay.novel) : nullptr;
    return p;
}

// the arena bound of both stages: `kernel` sums what the n records of a and b can need into the first 8 bytes of d_scratch; synchronises `stream`.
// too_many: the text for a batch beyond one launch
using BoundKernel = void (*)(const pa_read_result*, const pa_read_result*, uint64_t, unsigned long long*);
inline int stage_arena_bound(pa_index* idx, BoundKernel kernel, const pa_read_result* d_a, const pa_read_result* d_b, uint64_t n, void* d_scratch, void* stream, uint64_t* bound,
                             const char* too_many) {
    if (!idx || !d_scratch || !bound || (n && (!d_a || !d_b))) return fail(PA_ERR_INVALID_ARG, "null argument");
    PairIndexView v;
    index_pair_view(idx, &v);
    PA_HIP_TRY(hipSetDevice(v.device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    PA_HIP_TRY(hipMemsetAsync(d_scratch, 0, 8, s));
    if (n) {
        const uint32_t blocks = grid_for(n);
        if (blocks == 0) return fail(PA_ERR_UNSUPPORTED, "%s", too_many);
        hipLaunchKernelGGL(kernel, dim3(blocks), dim3(256), 0, s, d_a, d_b, n, static_cast<unsigned long long*>(d_scratch));
        PA_HIP_TRY(hipGetLastError());
    }
    unsigned long long h = 0;
    PA_HIP_TRY(hipMemcpyAsync(&h, d_scratch, 8, hipMemcpyDeviceToHost, s));
    PA_HIP_TRY(hipStreamSynchronize(s));
    *bound = h;
    return PA_OK;
}

// the finish of both stages: the control block to the host behind the launch; `what` names the arena in the message
inline int stage_finish(pa_index* idx, void* d_scratch, void* stream, uint64_t* stats, uint64_t* arena_used, uint64_t* arena_needed, const char* what) {
    if (!idx || !d_scratch) return fail(PA_ERR_INVALID_ARG, "null argument");
    PairIndexView v;
    index_pair_view(idx, &v);
    PA_HIP_TRY(hipSetDevice(v.device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    PairCtl h{};
    PA_HIP_TRY(hipMemcpyAsync(&h, d_scratch, sizeof h, hipMemcpyDeviceToHost, s));
    PA_HIP_TRY(hipStreamSynchronize(s));
    if (stats) for (int j = 0; j < PA_PAIR_STATS; ++j) stats[j] = h.stats[j];
    if (arena_used) *arena_used = h.arena_top < h.arena_cap ? h.arena_top : h.arena_cap;
    if (arena_needed) *arena_needed = h.arena_top;
    if (h.status & PA_STATUS_ARENA_FULL) return fail(PA_ERR_ARENA_FULL, "%s arena too small: %llu entries needed", what, h.arena_top);
    return PA_OK;
}

}  // namespace pa
