// Unstranded libraries behind the map launch (include/pseudoaligner_amd.h, "unstranded libraries"). An item (a read or a pair)
// arrives with two candidate results, S (as given) and R (the other strand), each ordinary pa_read_result records plus arena ids; this
// stage merges them per item by the rule of the header into ordinary records plus ids in its own arena. The skeleton is pairs.hip's
// (pair_stage.hpp holds what the two share):
//
//   pa_strands_classify_kernel  a thread per item: the record of every item that needs no id traffic is final here (neither candidate mapped;
//                               a winner whose class is empty or given by reference; a tie of the same reference twice; a tie of two
//                               empties); the others get coverage and mismatches and a WORK KEY: the length of the winner's list, or
//                               na + nb for the union of a tie. Keys up to STRAND_LANE_MAX go to the lane bin, longer ones to the wave bin
//   exclusive scan, scatter     as in pairs.hip: the item list, lane items first, both bins in item order
//   pa_strands_lane_kernel      a lane per short item: a two-pointer merge over the two lists, three times at most and with no private
//                               array: the union's size; its hash and the content lookup in the index's class-list table BEFORE arena is
//                               taken (one atomic per wave for all its lanes); the ids written
//   pa_strands_wave_kernel      a wave per long item, no sort and no LDS: lanes take 64 ids of one list at a time and binary-search the other.
//                               a[i] lands at i + lower_bound_b(a[i]) - (common ids before i), b[j] at j + lower_bound_a(b[j]) - (common ids
//                               before j) unless it is in a; "common ids before" is a ballot prefix popcount plus a running count over the
//                               chunks. A counting pass over a gives the exact size, one atomic takes that much arena, the writing pass
//                               scatters, lane 0 looks the list up by content where it lies
// A winner whose ids lie in a candidate's arena is that list merged with the EMPTY list (nb = 0): the same kernels copy it, the searches in
// the other list cost nothing and there is no pass over b.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "pair_stage.hpp"

namespace pa {
namespace {

constexpr uint32_t STRAND_LANE_MAX = 32;   // work key (ids to walk over) up to this: a lane; more: a wave
constexpr uint32_t ST_ITEMS = 0, ST_BOTH = 1, ST_ONLY_S = 2, ST_ONLY_R = 3, ST_NEITHER = 4, ST_TIES = 5, ST_REF = 6, ST_ARENA = 7;

// what the rule says of an item without looking at its ids
struct Verdict {
    bool ms, mr;     // the candidates are mapped
    bool tie;        // both mapped, equal keys
    bool r_wins;     // (no tie) the result is R
};
__device__ __forceinline__ Verdict verdict_of(const pa_read_result& s, const pa_read_result& r) {
    Verdict v;
    v.ms = s.mismatches & PA_MAPPED_BIT;
    v.mr = r.mismatches & PA_MAPPED_BIT;
    v.tie = false;
    v.r_wins = !v.ms;
    if (v.ms && v.mr) {   // keys (class non-empty, coverage, -mismatches), compared lexicographically
        const bool es = s.class_len != 0, er = r.class_len != 0;
        if (es != er) v.r_wins = er;
        else if (s.coverage != r.coverage) v.r_wins = r.coverage > s.coverage;
        else if (s.mismatches != r.mismatches) v.r_wins = r.mismatches < s.mismatches;
        else v.tie = true;
    }
    return v;
}

// the two lists of an item that has work to do: a tie's two lists, or the winner's list and an empty one
struct StrandLists {
    const uint32_t *a, *b;
    uint32_t na, nb, a_class, b_class;   // *_class: the index class the list is given by, or NO_CLASS
};
__device__ __forceinline__ StrandLists lists_of(const PairParams& p, uint32_t item) {
    const pa_read_result s = p.res1[item], r = p.res2[item];
    const Verdict v = verdict_of(s, r);
    StrandLists l;
    const pa_read_result x = (v.tie || !v.r_wins) ? s : r;
    l.a = ids_of(x, (v.tie || !v.r_wins) ? p.arena1 : p.arena2, p.ix);
    l.na = x.class_len;
    l.a_class = (x.class_off & PA_CLASS_REF) ? (x.class_off & ~PA_CLASS_REF) : NO_CLASS;
    l.b = l.a;
    l.nb = 0;
    l.b_class = NO_CLASS;
    if (v.tie) {
        l.b = ids_of(r, p.arena2, p.ix);
        l.nb = r.class_len;
        l.b_class = (r.class_off & PA_CLASS_REF) ? (r.class_off & ~PA_CLASS_REF) : NO_CLASS;
    }
    return l;
}

// ---------------------------------------------------------------------------------------------- classify
__global__ __launch_bounds__(256) void pa_strands_classify_kernel(const PairParams p) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = i < p.n;
    const uint32_t nc = p.ix.num_classes;
    bool both = false, only_s = false, only_r = false, tie = false, by_ref = false;
    if (live) {
        const pa_read_result s = p.res1[i], r = p.res2[i];
        const Verdict v = verdict_of(s, r);
        pa_read_result o{0, 0, 0, 0};
        uint32_t slot = nc + 2, key = 0;   // key: the work key (0: the record is final)
        both = v.ms && v.mr; only_s = v.ms && !v.mr; only_r = v.mr && !v.ms;
        tie = v.tie;
        if (v.ms || v.mr) {
            const pa_read_result w = (v.tie || !v.r_wins) ? s : r;   // the winner; on a tie coverage and mismatches are common
            o.coverage = w.coverage;
            o.mismatches = w.mismatches;
            if (w.class_len == 0) slot = nc + 1;   // (a tie with an empty S has an empty R: the key's first entry)
            else if ((w.class_off & PA_CLASS_REF) && (!v.tie || r.class_off == w.class_off)) { o.class_off = w.class_off; o.class_len = w.class_len; slot = w.class_off & ~PA_CLASS_REF; by_ref = true; }
            else key = v.tie ? s.class_len + r.class_len : w.class_len;
        }
        p.results[i] = o;   // (an item with work: coverage and mismatches; its class follows from the lane / wave kernel)
        p.flags[i] = key != 0 && key <= STRAND_LANE_MAX;
        p.flags[(uint64_t)p.n + i] = key > STRAND_LANE_MAX;
        if (i == 0) { p.flags[2ull * p.n] = 0; p.ctl->arena_cap = p.arena_cap; }
        if (p.counts && key == 0) atomicAdd(p.counts + slot, 1ull);
    }
    wave_count(live, p.ctl->stats + ST_ITEMS);
    wave_count(both, p.ctl->stats + ST_BOTH);
    wave_count(only_s, p.ctl->stats + ST_ONLY_S);
    wave_count(only_r, p.ctl->stats + ST_ONLY_R);
    wave_count(live && !both && !only_s && !only_r, p.ctl->stats + ST_NEITHER);
    wave_count(tie, p.ctl->stats + ST_TIES);
    wave_count(by_ref, p.ctl->stats + ST_REF);
}

__global__ __launch_bounds__(256) void pa_strands_bound_kernel(const pa_read_result* __restrict__ resS, const pa_read_result* __restrict__ resR, uint64_t n,
                                                               unsigned long long* __restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t need = 0;
    if (i < n) {
        const pa_read_result s = resS[i], r = resR[i];
        const bool ms = s.mismatches & PA_MAPPED_BIT, mr = r.mismatches & PA_MAPPED_BIT;
        need = (ms ? s.class_len : 0) + (mr ? r.class_len : 0);
    }
    const uint32_t total = (uint32_t)__shfl((int)wave_incl_scan(need), 63);   // (a list has fewer than 2^24 ids: 128 of them fit 32 bits)
    if (lane_id() == 0 && total != 0) atomicAdd(out, (unsigned long long)total);
}

__global__ __launch_bounds__(256) void pa_strands_scatter_kernel(const PairParams p) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= p.n) return;
    if (p.flags[i]) p.items[p.off[i]] = (uint32_t)i;
    if (p.flags[(uint64_t)p.n + i]) p.items[p.off[(uint64_t)p.n + i]] = (uint32_t)i;
}

// ---------------------------------------------------------------------------------------------- a lane per short item
// f(id) for every id of the union of a[0, na) and b[0, nb), ascending, once
template <class F>
__device__ __forceinline__ void for_union(const uint32_t* __restrict__ a, uint32_t na, const uint32_t* __restrict__ b, uint32_t nb, F&& f) {
    uint32_t i = 0, j = 0;
    while (i < na || j < nb) {
        const uint32_t x = i < na ? a[i] : 0, y = j < nb ? b[j] : 0;
        const bool ta = j >= nb || (i < na && x <= y), tb = i >= na || (j < nb && y <= x);   // (both: an id of both lists)
        f(ta ? x : y);
        i += ta;
        j += tb;
    }
}

// class_of_list (kernel_utils.hpp) for the union of the two lists, m = its size: the same hash, the same table
__device__ __forceinline__ uint32_t class_of_union(const StrandLists& l, uint32_t m, const DevIndexView& ix, const uint32_t* class_table, uint64_t class_table_size) {
    uint64_t h = 0x243f6a8885a308d3ull ^ m;
    for_union(l.a, l.na, l.b, l.nb, [&](uint32_t id) { h = pa_mix64(h ^ id) + 0x9e3779b97f4a7c15ull; });
    uint64_t j = h % class_table_size;
    for (;;) {
        const uint32_t cand = class_table[j];
        if (cand == NO_CLASS) return cand;
        if (ix.class_len[cand] == m) {
            const uint32_t* ids = class_ids(ix, ix.class_ref[cand]);
            bool eq = true;
            uint32_t o = 0;
            for_union(l.a, l.na, l.b, l.nb, [&](uint32_t id) { eq = eq && ids[o] == id; ++o; });   // (o stays below m: the union has m ids)
            if (eq) return cand;
        }
        if (++j == class_table_size) j = 0;
    }
}

__global__ __launch_bounds__(256) void pa_strands_lane_kernel(const PairParams p) {
    const uint32_t n_items = p.off[p.n];
    const uint32_t nc = p.ix.num_classes;
    const uint32_t lane = lane_id();
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t j0 = (uint64_t)blockIdx.x * blockDim.x + (threadIdx.x & ~63u); j0 < n_items; j0 += stride) {   // (whole waves go round together)
        const uint64_t j = j0 + lane;
        const bool live = j < n_items;
        uint32_t m = 0, cls = NO_CLASS, item = 0;
        StrandLists l{};
        if (live) {
            item = p.items[j];
            l = lists_of(p, item);
            for_union(l.a, l.na, l.b, l.nb, [&](uint32_t) { ++m; });
            if (m == l.na && l.a_class != NO_CLASS) cls = l.a_class;         // (b adds nothing to a)
            else if (m == l.nb && l.b_class != NO_CLASS) cls = l.b_class;
            else cls = class_of_union(l, m, p.ix, p.class_table, p.class_table_size);
        }
        // arena space for the results that are no index class: one atomic for the wave
        const uint32_t need = (live && cls == NO_CLASS) ? m : 0;
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
            if (fits) { uint32_t* out = p.arena + at; uint32_t o = 0; for_union(l.a, l.na, l.b, l.nb, [&](uint32_t id) { out[o++] = id; }); }
            else atomicOr(&p.ctl->status, PA_STATUS_ARENA_FULL);
        }
        if (live) {
            put_class(p, item, cls != NO_CLASS ? (cls | PA_CLASS_REF) : fits ? (uint32_t)at : PAIR_UNFIT, m);
            if (p.counts) atomicAdd(p.counts + (cls != NO_CLASS ? cls : nc), 1ull);
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
        wave_count(live && cls != NO_CLASS, p.ctl->stats + ST_REF);
        wave_count(need != 0, p.ctl->stats + ST_ARENA);
    }
}

// ---------------------------------------------------------------------------------------------- a wave per long item
__global__ __launch_bounds__(256) void pa_strands_wave_kernel(const PairParams p) {
    const uint32_t n_lane_items = p.off[p.n], n_items = p.off[2ull * p.n] - n_lane_items;
    const uint32_t nc = p.ix.num_classes;
    const uint32_t lane = lane_id();
    const unsigned long long below = (1ull << lane) - 1;
    const uint32_t waves = gridDim.x * (blockDim.x >> 6);
    for (uint32_t w = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); w < n_items; w += waves) {
        const uint32_t item = p.items[n_lane_items + w];
        const StrandLists l = lists_of(p, item);
        uint32_t common = 0;
        for (uint32_t t0 = 0; t0 < l.na && l.nb != 0; t0 += 64) {   // first pass: how many ids of a are in b too
            const uint32_t t = t0 + lane;
            bool hit = false;
            if (t < l.na) {
                const uint32_t a = l.a[t];
                const uint32_t q = lower_bound_ids(l.b, 0, l.nb, a);
                hit = q < l.nb && l.b[q] == a;
            }
            common += (uint32_t)__popcll(__ballot(hit));
        }
        const uint32_t m = l.na + l.nb - common;   // (at least na, which is at least 1)
        uint32_t cls = NO_CLASS;
        unsigned long long at = 0;
        bool fits = false;
        if (m == l.na && l.a_class != NO_CLASS) cls = l.a_class;
        else if (m == l.nb && l.b_class != NO_CLASS) cls = l.b_class;
        else {
            if (lane == 0) at = atomicAdd(&p.ctl->arena_top, (unsigned long long)m);
            at = __shfl(at, 0);
            fits = at + m <= p.arena_cap;
            if (fits) {
                uint32_t* out = p.arena + at;
                uint32_t before = 0;   // ids of both lists in the chunks done
                for (uint32_t t0 = 0; t0 < l.na; t0 += 64) {   // every id of a to its place in the union
                    const uint32_t t = t0 + lane;
                    bool hit = false;
                    uint32_t a = 0, q = 0;
                    if (t < l.na) {
                        a = l.a[t];
                        q = lower_bound_ids(l.b, 0, l.nb, a);
                        hit = q < l.nb && l.b[q] == a;
                    }
                    const unsigned long long mask = __ballot(hit);
                    const uint32_t at_a = t + q - (before + (uint32_t)__popcll(mask & below));
                    if (t < l.na && at_a < m) out[at_a] = a;   // (at_a < m holds for ascending lists; lists that are not must not write outside)
                    before += (uint32_t)__popcll(mask);
                }
                before = 0;
                for (uint32_t t0 = 0; t0 < l.nb; t0 += 64) {   // every id of b that is not in a to its place
                    const uint32_t t = t0 + lane;
                    bool hit = false;
                    uint32_t b = 0, q = 0;
                    if (t < l.nb) {
                        b = l.b[t];
                        q = lower_bound_ids(l.a, 0, l.na, b);
                        hit = q < l.na && l.a[q] == b;
                    }
                    const unsigned long long mask = __ballot(hit);
                    const uint32_t at_b = t + q - (before + (uint32_t)__popcll(mask & below));
                    if (t < l.nb && !hit && at_b < m) out[at_b] = b;
                    before += (uint32_t)__popcll(mask);
                }
                __threadfence();   // lane 0 reads what the other lanes wrote
                if (lane == 0) cls = class_of_list(p.arena + at, m, p.ix, p.class_table, p.class_table_size);
                cls = (uint32_t)__shfl((int)cls, 0);
            }
        }
        if (lane == 0) {
            const bool in_arena = cls == NO_CLASS;
            put_class(p, item, cls != NO_CLASS ? (cls | PA_CLASS_REF) : fits ? (uint32_t)at : PAIR_UNFIT, m);
            if (in_arena && !fits) atomicOr(&p.ctl->status, PA_STATUS_ARENA_FULL);
            if (p.counts) atomicAdd(p.counts + (cls != NO_CLASS ? cls : nc), 1ull);
            if (p.novel && in_arena && fits) {
                const unsigned long long e = atomicAdd(&p.ctl->novel_ctr, 1ull);
                p.novel[2 * e] = (uint32_t)at;
                p.novel[2 * e + 1] = m;
            }
            atomicAdd(p.ctl->stats + (in_arena ? ST_ARENA : ST_REF), 1ull);
        }
    }
}

}  // namespace
}  // namespace pa

using namespace pa;

extern "C" size_t pa_strands_scratch_bytes(uint64_t n) { return n > PAIR_MAX_PAIRS ? 0 : scratch_layout(n).total; }

extern "C" int pa_strands_merge_device(pa_index* idx, const pa_read_result* d_resS, const uint32_t* d_arenaS, const pa_read_result* d_resR, const uint32_t* d_arenaR,
                                       uint64_t n, pa_read_result* d_results, uint32_t* d_arena, uint64_t arena_cap, uint64_t* d_counts, void* d_scratch, size_t scratch_bytes,
                                       void* stream) {
    if (!idx || !d_scratch || (n && (!d_resS || !d_resR || !d_results)) || (arena_cap && !d_arena)) return fail(PA_ERR_INVALID_ARG, "null argument");
    if (n > PAIR_MAX_PAIRS) return fail(PA_ERR_UNSUPPORTED, "at most %llu items in one launch", (unsigned long long)PAIR_MAX_PAIRS);
    if ((uintptr_t)d_scratch & 255) return fail(PA_ERR_INVALID_ARG, "the scratch must be 256-byte aligned");
    const PairScratch lay = scratch_layout(n);
    if (scratch_bytes < lay.total) return fail(PA_ERR_INVALID_ARG, "scratch of %zu bytes, %zu needed", scratch_bytes, lay.total);
    PairIndexView v;
    index_pair_view(idx, &v);
    PA_HIP_TRY(hipSetDevice(v.device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    uint8_t* base = static_cast<uint8_t*>(d_scratch);
    PairParams p = stage_params(v, n, d_results, d_arena, arena_cap, d_counts, d_scratch, lay);
    p.res1 = d_resS; p.res2 = d_resR; p.arena1 = d_arenaS; p.arena2 = d_arenaR;
    PA_HIP_TRY(hipMemsetAsync(base, 0, PAIR_CTL_BYTES, s));
    if (n == 0) return PA_OK;
    const uint32_t blocks = grid_for(n);
    const uint32_t cus = (uint32_t)std::max(1, v.num_cus);
    hipLaunchKernelGGL(pa_strands_classify_kernel, dim3(blocks), dim3(256), 0, s, p);
    PA_HIP_TRY(hipGetLastError());
    size_t tmp_bytes = lay.tmp_bytes;
    PA_HIP_TRY(scan_exclusive_on(base + lay.tmp, tmp_bytes, (const uint32_t*)p.flags, p.off, (size_t)(2 * n + 1), s));
    hipLaunchKernelGGL(pa_strands_scatter_kernel, dim3(blocks), dim3(256), 0, s, p);
    PA_HIP_TRY(hipGetLastError());
    // the bins' sizes stay on the device: both kernels are launched for the worst case and their waves go round over the items there are
    hipLaunchKernelGGL(pa_strands_lane_kernel, dim3(std::min(blocks, cus * 8)), dim3(256), 0, s, p);
    PA_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(pa_strands_wave_kernel, dim3(std::min(grid_for(n, 4), cus * 4)), dim3(256), 0, s, p);
    PA_HIP_TRY(hipGetLastError());
    if (p.novel) return overflow_after_map(v.ovf, p.novel, &p.ctl->novel_ctr, n, d_arena, s);
    return PA_OK;
}

int pa::strands_arena_bound(pa_index* idx, const pa_read_result* d_resS, const pa_read_result* d_resR, uint64_t n, void* d_scratch, void* stream, uint64_t* bound) {
    return stage_arena_bound(idx, pa_strands_bound_kernel, d_resS, d_resR, n, d_scratch, stream, bound, "too many items for one launch");
}

extern "C" int pa_strands_finish(pa_index* idx, void* d_scratch, void* stream, uint64_t stats[PA_STRAND_STATS], uint64_t* arena_used, uint64_t* arena_needed) {
    return stage_finish(idx, d_scratch, stream, stats, arena_used, arena_needed, "strand");
}
