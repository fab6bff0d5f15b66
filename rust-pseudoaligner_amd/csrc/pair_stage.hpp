// The stage behind the map launch, written once: two finished record sets in (ordinary pa_read_result records plus arena ids), one record per
// item out, its ids in the stage's own arena. pairs.hip (two mates -> a pair, the classes intersected) and strands.hip (two strands -> an item,
// the winner's list or the union of a tie) each give it a RULE and instantiate the kernels; the control flow is here and nowhere else:
//
//   stage_classify_kernel  a thread per item: the rule's verdict from the two records alone. A record that needs no id traffic is final here
//                          and counted; the others get coverage and mismatches and a WORK KEY. Keys up to Rule::LANE_MAX go to the lane bin,
//                          longer ones to the wave bin
//   exclusive scan         (device_prims.hpp) over the two bins' flags laid end to end: where every item goes in the item list, and the two
//                          bins' sizes, which stay on the device
//   stage_scatter_kernel   the item list: lane items, then wave items, both in item order
//   stage_lane_kernel      a lane per short item: the rule combines the two lists into m and an enumerator of the result's ids (ascending);
//                          the result is looked up by content in the index's class-list hash table BEFORE it takes arena space, which the
//                          wave takes with one atomic for all its lanes
//   stage_wave_kernel      a wave per long item: the rule's counting pass gives m, the wave takes exactly that much arena with one atomic,
//                          the rule's writing pass fills it and lane 0 looks the list up by content where it lies
//   stage_bound_kernel     the arena bound: the rule's `need` of every item, summed
// and around them stage_launch, stage_finish and stage_arena_bound, the control block at the start of the caller's scratch (arena top, status,
// stats, novel counter), the scratch layout and the kernels' parameter block.
//
// A rule is a type with
//   LANE_MAX, NOUN ("pairs" / "items", for messages)
//   CLASSIFY_STAT        the stat slot of `Classified::own`
//   EMPTY_STAT           the stat slot of a combined result with no ids (counted in slot num_classes + 1), or NO_STAT: there is no such result
//   classify(r1, r2, nc) -> Classified
//   need(r1, r2)         the arena entries the item can take at most
//   lists_of(p, item)    -> IdLists, for an item with a work key
//   lane_combine(l, m)   -> Each, an enumerator: each(f) calls f(id) for every id of the result, ascending; m = their number
//   wave_count(l, lane)  -> m, the same in every lane;  wave_write(l, lane, out, m): the result's ids to out[0, m)
// Private to those two sources.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>

#include "device_prims.hpp"
#include "hip_buffer.hpp"
#include "kernel_utils.hpp"
#include "kernels.hpp"
#include "pa_common.hpp"

namespace pa {

constexpr uint32_t PAIR_UNFIT = (uint32_t)PA_MAX_ARENA_ENTRIES;       // class_off of a record whose ids did not fit the arena
constexpr uint32_t PAIR_CTL_BYTES = 256;
static_assert(PA_STRAND_STATS == PA_PAIR_STATS, "both stages keep their stats in one control block");
// the stat slots both stages give one meaning (items; both / only the first / only the second / neither input mapped; the result is an index
// class; its ids are in the arena). Slot 5 is the rule's
constexpr uint32_t ST_ITEMS = 0, ST_BOTH = 1, ST_ONLY1 = 2, ST_ONLY2 = 3, ST_NEITHER = 4, ST_REF = 6, ST_ARENA = 7, NO_STAT = ~0u;

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

// what a rule says of an item from its two records alone
struct Classified {
    pa_read_result rec;   // the output record (an item with work: coverage and mismatches; its class follows from the lane / wave kernel)
    uint32_t key;         // the work key (0: the record is final)
    uint32_t slot;        // the count slot of a final record
    bool m1, m2;          // the inputs are mapped
    bool own, by_ref;     // stats: the rule's own slot (Rule::CLASSIFY_STAT); final, by reference
};

// the two lists of an item that has work to do
struct IdLists {
    const uint32_t *a, *b;
    uint32_t na, nb, a_class, b_class;   // *_class: the index class the list is given by, or NO_CLASS
};

__device__ __forceinline__ const uint32_t* ids_of(const pa_read_result& r, const uint32_t* arena, const DevIndexView& ix) {
    return (r.class_off & PA_CLASS_REF) ? class_ids(ix, ix.class_ref[r.class_off & ~PA_CLASS_REF]) : arena + r.class_off;
}
__device__ __forceinline__ uint32_t ref_class_of(const pa_read_result& r) { return (r.class_off & PA_CLASS_REF) ? (r.class_off & ~PA_CLASS_REF) : NO_CLASS; }

// first position in v[lo, hi) whose id is not below a
__device__ __forceinline__ uint32_t lower_bound_ids(const uint32_t* __restrict__ v, uint32_t lo, uint32_t hi, uint32_t a) {
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (v[mid] < a) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// class_of_list (kernel_utils.hpp) for the m ids that `each` enumerates: the same hash, the same table
template <class Each>
__device__ __forceinline__ uint32_t class_of_each(uint32_t m, const Each& each, const DevIndexView& ix, const uint32_t* class_table, uint64_t class_table_size) {
    uint64_t h = 0x243f6a8885a308d3ull ^ m;
    each([&](uint32_t id) { h = pa_mix64(h ^ id) + 0x9e3779b97f4a7c15ull; });
    uint64_t j = h % class_table_size;
    for (;;) {
        const uint32_t cand = class_table[j];
        if (cand == NO_CLASS) return cand;
        if (ix.class_len[cand] == m) {
            const uint32_t* ids = class_ids(ix, ix.class_ref[cand]);
            bool eq = true;
            uint32_t o = 0;
            each([&](uint32_t id) { eq = eq && ids[o] == id; ++o; });   // (o stays below m: `each` has m ids)
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

// ---------------------------------------------------------------------------------------------- classify, bound, scatter
template <class Rule>
__global__ __launch_bounds__(256) void stage_classify_kernel(const PairParams p) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = i < p.n;
    bool both = false, only1 = false, only2 = false, own = false, by_ref = false;
    if (live) {
        const pa_read_result r1 = p.res1[i], r2 = p.res2[i];   // (copies: one 16-byte load each)
        const Classified c = Rule::classify(r1, r2, p.ix.num_classes);
        both = c.m1 && c.m2; only1 = c.m1 && !c.m2; only2 = c.m2 && !c.m1;
        own = c.own; by_ref = c.by_ref;
        p.results[i] = c.rec;
        p.flags[i] = c.key != 0 && c.key <= Rule::LANE_MAX;
        p.flags[(uint64_t)p.n + i] = c.key > Rule::LANE_MAX;
        if (i == 0) { p.flags[2ull * p.n] = 0; p.ctl->arena_cap = p.arena_cap; }
        if (p.counts && c.key == 0) atomicAdd(p.counts + c.slot, 1ull);
    }
    wave_count(live, p.ctl->stats + ST_ITEMS);
    wave_count(both, p.ctl->stats + ST_BOTH);
    wave_count(only1, p.ctl->stats + ST_ONLY1);
    wave_count(only2, p.ctl->stats + ST_ONLY2);
    wave_count(live && !both && !only1 && !only2, p.ctl->stats + ST_NEITHER);
    wave_count(own, p.ctl->stats + Rule::CLASSIFY_STAT);
    wave_count(by_ref, p.ctl->stats + ST_REF);
}

template <class Rule>
__global__ __launch_bounds__(256) void stage_bound_kernel(const pa_read_result* __restrict__ res1, const pa_read_result* __restrict__ res2, uint64_t n,
                                                          unsigned long long* __restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t need = 0;
    if (i < n) {
        const pa_read_result r1 = res1[i], r2 = res2[i];
        need = Rule::need(r1, r2);
    }
    const uint32_t total = (uint32_t)__shfl((int)wave_incl_scan(need), 63);   // (a list has fewer than 2^24 ids: 128 of them fit 32 bits)
    if (lane_id() == 0 && total != 0) atomicAdd(out, (unsigned long long)total);
}

template <class Rule>
__global__ __launch_bounds__(256) void stage_scatter_kernel(const PairParams p) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= p.n) return;
    if (p.flags[i]) p.items[p.off[i]] = (uint32_t)i;
    if (p.flags[(uint64_t)p.n + i]) p.items[p.off[(uint64_t)p.n + i]] = (uint32_t)i;
}

// ---------------------------------------------------------------------------------------------- a lane per short item
template <class Rule>
__global__ __launch_bounds__(256) void stage_lane_kernel(const PairParams p) {
    constexpr bool may_be_empty = Rule::EMPTY_STAT != NO_STAT;
    const uint32_t n_items = p.off[p.n];
    const uint32_t nc = p.ix.num_classes;
    const uint32_t lane = lane_id();
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t j0 = (uint64_t)blockIdx.x * blockDim.x + (threadIdx.x & ~63u); j0 < n_items; j0 += stride) {   // (whole waves go round together)
        const uint64_t j = j0 + lane;
        const bool live = j < n_items;
        uint32_t m = 0, cls = NO_CLASS, item = 0;
        typename Rule::Each each{};
        if (live) {
            item = p.items[j];
            const IdLists l = Rule::lists_of(p, item);
            each = Rule::lane_combine(l, m);
            if (!may_be_empty || m != 0) {
                if (m == l.na && l.a_class != NO_CLASS) cls = l.a_class;
                else if (m == l.nb && l.b_class != NO_CLASS) cls = l.b_class;
                else cls = class_of_each(m, each, p.ix, p.class_table, p.class_table_size);
            }
        }
        const bool empty = may_be_empty && live && m == 0;
        // arena space for the results that are no index class: one atomic for the wave
        const uint32_t need = (live && !empty && cls == NO_CLASS) ? m : 0;
        const uint32_t incl = wave_incl_scan(need);
        const uint32_t total = (uint32_t)__shfl((int)incl, 63);
        unsigned long long base = 0;
        if (total != 0) {
            if (lane == 63) base = atomicAdd(&p.ctl->arena_top, (unsigned long long)total);
            base = __shfl(base, 63);
        }
        const unsigned long long at = base + incl - need;
        const bool fits = need != 0 && at + need <= p.arena_cap;
        if (need != 0) {
            if (fits) { uint32_t* out = p.arena + at; uint32_t o = 0; each([&](uint32_t id) { out[o++] = id; }); }
            else atomicOr(&p.ctl->status, PA_STATUS_ARENA_FULL);
        }
        if (live) {
            if (!empty) put_class(p, item, cls != NO_CLASS ? (cls | PA_CLASS_REF) : fits ? (uint32_t)at : PAIR_UNFIT, m);
            if (p.counts) atomicAdd(p.counts + (empty ? nc + 1 : cls != NO_CLASS ? cls : nc), 1ull);
        }
        if (p.novel) {
            const unsigned long long mask = __ballot(fits);
            if (mask != 0) {
                unsigned long long nb = 0;
                const uint32_t leader = (uint32_t)__ffsll((long long)mask) - 1;
                if (lane == leader) nb = atomicAdd(&p.ctl->novel_ctr, (unsigned long long)__popcll(mask));
                nb = __shfl(nb, (int)leader);
                if (fits) {
                    const unsigned long long e = nb + __popcll(mask & ((1ull << lane) - 1));
                    p.novel[2 * e] = (uint32_t)at;
                    p.novel[2 * e + 1] = m;
                }
            }
        }
        if constexpr (may_be_empty) wave_count(empty, p.ctl->stats + Rule::EMPTY_STAT);
        wave_count(live && !empty && cls != NO_CLASS, p.ctl->stats + ST_REF);
        wave_count(need != 0, p.ctl->stats + ST_ARENA);
    }
}

// ---------------------------------------------------------------------------------------------- a wave per long item
template <class Rule>
__global__ __launch_bounds__(256) void stage_wave_kernel(const PairParams p) {
    constexpr bool may_be_empty = Rule::EMPTY_STAT != NO_STAT;
    const uint32_t n_lane_items = p.off[p.n], n_items = p.off[2ull * p.n] - n_lane_items;
    const uint32_t nc = p.ix.num_classes;
    const uint32_t lane = lane_id();
    const uint32_t waves = gridDim.x * (blockDim.x >> 6);
    for (uint32_t w = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); w < n_items; w += waves) {
        const uint32_t item = p.items[n_lane_items + w];
        const IdLists l = Rule::lists_of(p, item);
        const uint32_t m = Rule::wave_count(l, lane);
        const bool empty = may_be_empty && m == 0;
        uint32_t cls = NO_CLASS;
        unsigned long long at = 0;
        bool fits = false;
        if (!empty) {
            if (m == l.na && l.a_class != NO_CLASS) cls = l.a_class;
            else if (m == l.nb && l.b_class != NO_CLASS) cls = l.b_class;
            else {
                if (lane == 0) at = atomicAdd(&p.ctl->arena_top, (unsigned long long)m);
                at = __shfl(at, 0);
                fits = at + m <= p.arena_cap;
                if (fits) {
                    Rule::wave_write(l, lane, p.arena + at, m);
                    __threadfence();   // lane 0 reads what the other lanes wrote
                    if (lane == 0) cls = class_of_list(p.arena + at, m, p.ix, p.class_table, p.class_table_size);
                    cls = (uint32_t)__shfl((int)cls, 0);
                }
            }
        }
        if (lane == 0) {
            const bool in_arena = !empty && cls == NO_CLASS;
            if (!empty) put_class(p, item, cls != NO_CLASS ? (cls | PA_CLASS_REF) : fits ? (uint32_t)at : PAIR_UNFIT, m);
            if (in_arena && !fits) atomicOr(&p.ctl->status, PA_STATUS_ARENA_FULL);
            if (p.counts) atomicAdd(p.counts + (empty ? nc + 1 : cls != NO_CLASS ? cls : nc), 1ull);
            if (p.novel && in_arena && fits) {
                const unsigned long long e = atomicAdd(&p.ctl->novel_ctr, 1ull);
                p.novel[2 * e] = (uint32_t)at;
                p.novel[2 * e + 1] = m;
            }
            atomicAdd(p.ctl->stats + (empty ? Rule::EMPTY_STAT : in_arena ? ST_ARENA : ST_REF), 1ull);
        }
    }
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
inline size_t stage_scratch_bytes(uint64_t n) { return n > PAIR_MAX_PAIRS ? 0 : scratch_layout(n).total; }

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

// the launch of both stages, asynchronous on `stream`: records and arenas 1 and 2 as two finished launches left them
template <class Rule>
int stage_launch(pa_index* idx, const pa_read_result* d_res1, const uint32_t* d_arena1, const pa_read_result* d_res2, const uint32_t* d_arena2, uint64_t n,
                 pa_read_result* d_results, uint32_t* d_arena, uint64_t arena_cap, uint64_t* d_counts, void* d_scratch, size_t scratch_bytes, void* stream) {
    if (!idx || !d_scratch || (n && (!d_res1 || !d_res2 || !d_results)) || (arena_cap && !d_arena)) return fail(PA_ERR_INVALID_ARG, "null argument");
    if (n > PAIR_MAX_PAIRS) return fail(PA_ERR_UNSUPPORTED, "at most %llu %s in one launch", (unsigned long long)PAIR_MAX_PAIRS, Rule::NOUN);
    if ((uintptr_t)d_scratch & 255) return fail(PA_ERR_INVALID_ARG, "the scratch must be 256-byte aligned");
    const PairScratch lay = scratch_layout(n);
    if (scratch_bytes < lay.total) return fail(PA_ERR_INVALID_ARG, "scratch of %zu bytes, %zu needed", scratch_bytes, lay.total);
    PairIndexView v;
    index_pair_view(idx, &v);
    PA_HIP_TRY(hipSetDevice(v.device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    uint8_t* base = static_cast<uint8_t*>(d_scratch);
    PairParams p = stage_params(v, n, d_results, d_arena, arena_cap, d_counts, d_scratch, lay);
    p.res1 = d_res1; p.res2 = d_res2; p.arena1 = d_arena1; p.arena2 = d_arena2;
    PA_HIP_TRY(hipMemsetAsync(base, 0, PAIR_CTL_BYTES, s));
    if (n == 0) return PA_OK;
    const uint32_t blocks = grid_for(n);
    const uint32_t cus = (uint32_t)std::max(1, v.num_cus);
    int rc;
    if ((rc = launch(stage_classify_kernel<Rule>, blocks, 256, s, p)) != PA_OK) return rc;
    size_t tmp_bytes = lay.tmp_bytes;
    PA_HIP_TRY(scan_exclusive_on(base + lay.tmp, tmp_bytes, (const uint32_t*)p.flags, p.off, (size_t)(2 * n + 1), s));
    if ((rc = launch(stage_scatter_kernel<Rule>, blocks, 256, s, p)) != PA_OK) return rc;
    // the bins' sizes stay on the device: both kernels are launched for the worst case and their waves go round over the items there are
    if ((rc = launch(stage_lane_kernel<Rule>, std::min(blocks, cus * 8), 256, s, p)) != PA_OK) return rc;
    if ((rc = launch(stage_wave_kernel<Rule>, std::min(grid_for(n, 4), cus * 4), 256, s, p)) != PA_OK) return rc;
    if (p.novel) return overflow_after_map(v.ovf, p.novel, &p.ctl->novel_ctr, n, d_arena, s);
    return PA_OK;
}

// the arena bound of both stages: what the n records of a and b can need, summed into the first 8 bytes of d_scratch; synchronises `stream`
template <class Rule>
int stage_arena_bound(pa_index* idx, const pa_read_result* d_a, const pa_read_result* d_b, uint64_t n, void* d_scratch, void* stream, uint64_t* bound) {
    if (!idx || !d_scratch || !bound || (n && (!d_a || !d_b))) return fail(PA_ERR_INVALID_ARG, "null argument");
    PairIndexView v;
    index_pair_view(idx, &v);
    PA_HIP_TRY(hipSetDevice(v.device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    PA_HIP_TRY(hipMemsetAsync(d_scratch, 0, 8, s));
    if (n) {
        const uint32_t blocks = grid_for(n);
        if (blocks == 0) return fail(PA_ERR_UNSUPPORTED, "too many %s for one launch", Rule::NOUN);
        hipLaunchKernelGGL(stage_bound_kernel<Rule>, dim3(blocks), dim3(256), 0, s, d_a, d_b, n, static_cast<unsigned long long*>(d_scratch));
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
