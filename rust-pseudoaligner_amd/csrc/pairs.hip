// Paired-end reads behind the map launch (include/pseudoaligner_amd.h, "paired-end reads"). Nothing here touches the map,
// resolve, count or ingest sources: the mates are mapped by two ordinary pa_map_batch_device launches and this stage combines their
// records per pair into ordinary pa_read_result records plus arena ids.
//
//   pa_revcomp_kernel         reverse complement of packed reads in the tile layout: a thread per (read, output word); the output word is
//                             cut out of the one or two input words it straddles, its 32 two-bit groups reversed (__brevll + swap of the
//                             two bits of a group) and complemented. No per-base loop; lanes of a wave are the 64 reads of a tile, so
//                             loads and stores are coalesced whenever the tile's reads have one length
//   pa_pairs_classify_kernel  a thread per pair: the record of every pair that needs no id traffic (neither mate mapped, a mate with an
//                             empty class, one mate mapped by reference, the same reference twice) is final here; the others get
//                             coverage and mismatches and a WORK KEY: the length of the shorter list. Keys up to PAIR_LANE_MAX go to the
//                             lane bin, longer ones to the wave bin
//   exclusive scan            (device_prims.hpp) over the two bins' flags laid end to end: where every pair goes in the item list, and the
//                             two bins' sizes, which stay on the device
//   pa_pairs_scatter_kernel   the item list: lane items, then wave items, both in pair order
//   pa_pairs_lane_kernel      a lane per short pair: the ids of the shorter list looked up one after the other in the rest of the longer
//                             one (a merge whose steps in the longer list are binary searches); the result, a mask of the shorter list's positions, is
//                             looked up by content in the index's class-list hash table BEFORE it takes arena space, which the wave
//                             takes with one atomic for all its lanes
//   pa_pairs_wave_kernel      a wave per long pair: lanes take 64 ids of the shorter list at a time and binary-search the longer one; a
//                             ballot and a prefix popcount give every survivor its ordered position. First pass counts, then the wave
//                             takes exactly that much arena with one atomic, the second pass writes (a block of 64 ids: one burst) and
//                             lane 0 looks the list up by content where it lies
// A mate mapped alone whose ids lie in its mate arena is the pair "list with itself": the same two kernels copy it into the pair arena.
// The control block (arena top, status, stats, novel counter) lives at the start of the caller's scratch. What this stage shares with the
// unstranded stage (strands.hip) — control block, scratch layout, parameter block, the helpers on id lists — is pair_stage.hpp. The
// host-buffer paths at the end (pa_map_pairs, pa_map_pairs_unstranded, pa_map_batch_strand) share map_mate and the stage runners.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <memory>
#include <vector>

#include "device_prims.hpp"
#include "hip_buffer.hpp"
#include "kernel_utils.hpp"
#include "kernels.hpp"
#include "pa_common.hpp"
#include "pair_stage.hpp"

namespace pa {
namespace {

constexpr uint32_t PAIR_LANE_MAX = 16;                                // the shorter list has at most this many ids: a lane; more: a wave
constexpr uint32_t ST_PAIRS = 0, ST_BOTH = 1, ST_ONLY1 = 2, ST_ONLY2 = 3, ST_NEITHER = 4, ST_EMPTY = 5, ST_REF = 6, ST_ARENA = 7;

// the two lists of a pair that has work to do: a = the shorter one (mate 1 on a tie); a mate mapped alone is paired with itself
struct PairLists {
    const uint32_t *a, *b;
    uint32_t na, nb, a_class, b_class;   // *_class: the index class the list is given by, or NO_CLASS
};
__device__ __forceinline__ PairLists lists_of(const PairParams& p, uint32_t pair) {
    const pa_read_result r1 = p.res1[pair], r2 = p.res2[pair];
    const bool m1 = r1.mismatches & PA_MAPPED_BIT, m2 = r2.mismatches & PA_MAPPED_BIT;
    const pa_read_result x = m1 ? r1 : r2, y = m2 ? r2 : r1;        // (one mate alone: x == y)
    const uint32_t *ax = m1 ? p.arena1 : p.arena2, *ay = m2 ? p.arena2 : p.arena1;
    PairLists l;
    const bool swap = y.class_len < x.class_len;
    const pa_read_result s = swap ? y : x, g = swap ? x : y;
    l.a = ids_of(s, swap ? ay : ax, p.ix);
    l.b = ids_of(g, swap ? ax : ay, p.ix);
    l.na = s.class_len;
    l.nb = g.class_len;
    l.a_class = (s.class_off & PA_CLASS_REF) ? (s.class_off & ~PA_CLASS_REF) : NO_CLASS;
    l.b_class = (g.class_off & PA_CLASS_REF) ? (g.class_off & ~PA_CLASS_REF) : NO_CLASS;
    return l;
}

// ---------------------------------------------------------------------------------------------- reverse complement
__global__ __launch_bounds__(256) void pa_revcomp_kernel(const uint64_t* __restrict__ in, const uint32_t* __restrict__ lens, uint64_t n_reads, uint32_t wpr,
                                                         uint64_t* __restrict__ out) {
    const uint64_t gid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t ntiles = (n_reads + 63) >> 6;
    if (gid >= ntiles * wpr * 64) return;
    const uint32_t r = (uint32_t)(gid & 63);
    const uint64_t tw = gid >> 6, tile = tw / wpr;
    const uint32_t w = (uint32_t)(tw % wpr);
    const uint64_t rid = tile * 64 + r;
    uint64_t v = 0;
    if (rid < n_reads) {
        uint64_t len = lens[rid];
        if (len > 32ull * wpr) len = 32ull * wpr;
        if (len > 32ull * w) {
            // output bases 32 w + t (t = 0..31) are input bases hi - t: the window of 32 input bases that ENDS at hi, reversed
            const uint64_t hi = len - 1 - 32ull * w;
            const uint64_t* src = in + tile * wpr * 64 + r;
            uint64_t win;
            if (hi >= 31) {
                const uint64_t s = hi - 31, i = s >> 5;
                const uint32_t sh = (uint32_t)(s & 31) * 2;
                win = src[i * 64] >> sh;
                if (sh) win |= src[(i + 1) * 64] << (64 - sh);   // (word i + 1 holds base hi: it is below the read's last word or that word)
            } else {
                win = src[0] << (2 * (31 - (uint32_t)hi));        // the read's first hi + 1 bases, at the top of the window
            }
            uint64_t x = __brevll(win);                           // groups reversed, and the two bits inside every group too:
            x = ((x >> 1) & 0x5555555555555555ull) | ((x & 0x5555555555555555ull) << 1);   // put those back
            x = ~x;                                               // 3 - code
            const uint64_t nb = len - 32ull * w;                  // bases of this output word
            v = nb >= 32 ? x : x & ((1ull << (2 * nb)) - 1);
        }
    }
    out[gid] = v;
}

// ---------------------------------------------------------------------------------------------- classify
__global__ __launch_bounds__(256) void pa_pairs_classify_kernel(const PairParams p) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = i < p.n;
    const uint32_t nc = p.ix.num_classes;
    bool both = false, only1 = false, only2 = false, empty_both = false, by_ref = false;
    if (live) {
        const pa_read_result r1 = p.res1[i], r2 = p.res2[i];
        const bool m1 = r1.mismatches & PA_MAPPED_BIT, m2 = r2.mismatches & PA_MAPPED_BIT;
        pa_read_result o{0, 0, 0, 0};
        uint32_t slot = nc + 2, key = 0;   // key: the work key (0: the record is final)
        both = m1 && m2; only1 = m1 && !m2; only2 = m2 && !m1;
        if (both) {
            o.coverage = r1.coverage + r2.coverage;
            o.mismatches = ((r1.mismatches & ~PA_MAPPED_BIT) + (r2.mismatches & ~PA_MAPPED_BIT)) | PA_MAPPED_BIT;
            if (r1.class_len == 0 || r2.class_len == 0) { slot = nc + 1; empty_both = true; }
            else if ((r1.class_off & PA_CLASS_REF) && r1.class_off == r2.class_off) { o.class_off = r1.class_off; o.class_len = r1.class_len; slot = r1.class_off & ~PA_CLASS_REF; by_ref = true; }
            else key = r1.class_len < r2.class_len ? r1.class_len : r2.class_len;
        } else if (m1 || m2) {
            const pa_read_result r = m1 ? r1 : r2;
            o.coverage = r.coverage;
            o.mismatches = r.mismatches;
            if (r.class_len == 0) slot = nc + 1;
            else if (r.class_off & PA_CLASS_REF) { o.class_off = r.class_off; o.class_len = r.class_len; slot = r.class_off & ~PA_CLASS_REF; by_ref = true; }
            else key = r.class_len;
        }
        p.results[i] = o;   // (a pair with work: coverage and mismatches; its class follows from the lane / wave kernel)
        p.flags[i] = key != 0 && key <= PAIR_LANE_MAX;
        p.flags[(uint64_t)p.n + i] = key > PAIR_LANE_MAX;
        if (i == 0) { p.flags[2ull * p.n] = 0; p.ctl->arena_cap = p.arena_cap; }
        if (p.counts && key == 0) atomicAdd(p.counts + slot, 1ull);
    }
    wave_count(live, p.ctl->stats + ST_PAIRS);
    wave_count(both, p.ctl->stats + ST_BOTH);
    wave_count(only1, p.ctl->stats + ST_ONLY1);
    wave_count(only2, p.ctl->stats + ST_ONLY2);
    wave_count(live && !both && !only1 && !only2, p.ctl->stats + ST_NEITHER);
    wave_count(empty_both, p.ctl->stats + ST_EMPTY);
    wave_count(by_ref, p.ctl->stats + ST_REF);
}

__global__ __launch_bounds__(256) void pa_pairs_bound_kernel(const pa_read_result* __restrict__ res1, const pa_read_result* __restrict__ res2, uint64_t n,
                                                             unsigned long long* __restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t need = 0;
    if (i < n) {
        const pa_read_result r1 = res1[i], r2 = res2[i];
        const bool m1 = r1.mismatches & PA_MAPPED_BIT, m2 = r2.mismatches & PA_MAPPED_BIT;
        need = m1 && m2 ? (r1.class_len < r2.class_len ? r1.class_len : r2.class_len) : m1 ? r1.class_len : m2 ? r2.class_len : 0;
    }
    const uint32_t total = (uint32_t)__shfl((int)wave_incl_scan(need), 63);   // (a list has fewer than 2^24 ids: 64 of them fit 32 bits)
    if (lane_id() == 0 && total != 0) atomicAdd(out, (unsigned long long)total);
}

__global__ __launch_bounds__(256) void pa_pairs_scatter_kernel(const PairParams p) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= p.n) return;
    if (p.flags[i]) p.items[p.off[i]] = (uint32_t)i;
    if (p.flags[(uint64_t)p.n + i]) p.items[p.off[(uint64_t)p.n + i]] = (uint32_t)i;
}

// ---------------------------------------------------------------------------------------------- a lane per short pair
__global__ __launch_bounds__(256) void pa_pairs_lane_kernel(const PairParams p) {
    const uint32_t n_items = p.off[p.n];
    const uint32_t nc = p.ix.num_classes;
    const uint32_t lane = lane_id();
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t j0 = (uint64_t)blockIdx.x * blockDim.x + (threadIdx.x & ~63u); j0 < n_items; j0 += stride) {   // (whole waves go round together)
        const uint64_t j = j0 + lane;
        const bool live = j < n_items;
        uint32_t keep = 0, m = 0, cls = NO_CLASS, pair = 0;   // keep: bit t = id t of the shorter list survives
        const uint32_t* a_ids = nullptr;
        if (live) {
            pair = p.items[j];
            const PairLists l = lists_of(p, pair);
            a_ids = l.a;
            uint32_t pb = 0;
            for (uint32_t t = 0; t < l.na && t < PAIR_LANE_MAX && pb < l.nb; ++t) {
                const uint32_t a = l.a[t];
                pb = lower_bound_ids(l.b, pb, l.nb, a);
                if (pb < l.nb && l.b[pb] == a) { keep |= 1u << t; ++pb; }
            }
            m = (uint32_t)__popc(keep);
            if (m != 0) {
                if (m == l.na && l.a_class != NO_CLASS) cls = l.a_class;
                else if (m == l.nb && l.b_class != NO_CLASS) cls = l.b_class;
                else cls = class_of_masked(l.a, keep, m, p.ix, p.class_table, p.class_table_size);
            }
        }
        // arena space for the results that are no index class: one atomic for the wave
        const uint32_t need = (m != 0 && cls == NO_CLASS) ? m : 0;
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
            if (fits) { uint32_t o = 0; for (uint32_t k = keep; k != 0; k &= k - 1) p.arena[at + o++] = a_ids[__ffs((int)k) - 1]; }
            else atomicOr(&p.ctl->status, PA_STATUS_ARENA_FULL);
        }
        if (live) {
            if (m != 0) put_class(p, pair, cls != NO_CLASS ? (cls | PA_CLASS_REF) : fits ? (uint32_t)at : PAIR_UNFIT, m);
            if (p.counts) atomicAdd(p.counts + (m == 0 ? nc + 1 : cls != NO_CLASS ? cls : nc), 1ull);
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
        wave_count(live && m == 0, p.ctl->stats + ST_EMPTY);
        wave_count(live && m != 0 && cls != NO_CLASS, p.ctl->stats + ST_REF);
        wave_count(need != 0, p.ctl->stats + ST_ARENA);
    }
}

// ---------------------------------------------------------------------------------------------- a wave per long pair
__global__ __launch_bounds__(256) void pa_pairs_wave_kernel(const PairParams p) {
    const uint32_t n_lane_items = p.off[p.n], n_items = p.off[2ull * p.n] - n_lane_items;
    const uint32_t nc = p.ix.num_classes;
    const uint32_t lane = lane_id();
    const unsigned long long below = (1ull << lane) - 1;
    const uint32_t waves = gridDim.x * (blockDim.x >> 6);
    for (uint32_t w = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); w < n_items; w += waves) {
        const uint32_t pair = p.items[n_lane_items + w];
        const PairLists l = lists_of(p, pair);
        uint32_t m = 0;
        for (uint32_t t0 = 0; t0 < l.na; t0 += 64) {   // first pass: how many ids survive
            const uint32_t t = t0 + lane;
            bool hit = false;
            if (t < l.na) {
                const uint32_t a = l.a[t];
                const uint32_t q = lower_bound_ids(l.b, 0, l.nb, a);
                hit = q < l.nb && l.b[q] == a;
            }
            m += (uint32_t)__popcll(__ballot(hit));
        }
        uint32_t cls = NO_CLASS;
        unsigned long long at = 0;
        bool fits = false;
        if (m != 0) {
            if (m == l.na && l.a_class != NO_CLASS) cls = l.a_class;
            else if (m == l.nb && l.b_class != NO_CLASS) cls = l.b_class;
            else {
                if (lane == 0) at = atomicAdd(&p.ctl->arena_top, (unsigned long long)m);
                at = __shfl(at, 0);
                fits = at + m <= p.arena_cap;
                if (fits) {
                    uint32_t done = 0;
                    for (uint32_t t0 = 0; t0 < l.na; t0 += 64) {   // second pass: every survivor to its ordered place
                        const uint32_t t = t0 + lane;
                        bool hit = false;
                        uint32_t a = 0;
                        if (t < l.na) {
                            a = l.a[t];
                            const uint32_t q = lower_bound_ids(l.b, 0, l.nb, a);
                            hit = q < l.nb && l.b[q] == a;
                        }
                        const unsigned long long mask = __ballot(hit);
                        if (hit) p.arena[at + done + __popcll(mask & below)] = a;
                        done += (uint32_t)__popcll(mask);
                    }
                    __threadfence();   // lane 0 reads what the other lanes wrote
                    if (lane == 0) cls = class_of_list(p.arena + at, m, p.ix, p.class_table, p.class_table_size);
                    cls = (uint32_t)__shfl((int)cls, 0);
                }
            }
        }
        if (lane == 0) {
            const bool in_arena = m != 0 && cls == NO_CLASS;
            if (m != 0) put_class(p, pair, cls != NO_CLASS ? (cls | PA_CLASS_REF) : fits ? (uint32_t)at : PAIR_UNFIT, m);
            if (in_arena && !fits) atomicOr(&p.ctl->status, PA_STATUS_ARENA_FULL);
            if (p.counts) atomicAdd(p.counts + (m == 0 ? nc + 1 : cls != NO_CLASS ? cls : nc), 1ull);
            if (p.novel && in_arena && fits) {
                const unsigned long long e = atomicAdd(&p.ctl->novel_ctr, 1ull);
                p.novel[2 * e] = (uint32_t)at;
                p.novel[2 * e + 1] = m;
            }
            atomicAdd(p.ctl->stats + (m == 0 ? ST_EMPTY : in_arena ? ST_ARENA : ST_REF), 1ull);
        }
    }
}

}  // namespace
}  // namespace pa

using namespace pa;

extern "C" int pa_revcomp_tiles_device(const pa_index* idx, const uint64_t* d_tiles_in, const uint32_t* d_lens, uint64_t n_reads, uint32_t words_per_read,
                                       uint64_t* d_tiles_out, void* stream) {
    if (!idx || words_per_read == 0 || (n_reads && (!d_tiles_in || !d_lens || !d_tiles_out))) return fail(PA_ERR_INVALID_ARG, "null argument");
    if (d_tiles_in == d_tiles_out && n_reads) return fail(PA_ERR_INVALID_ARG, "the reverse complement is not taken in place");
    if (n_reads == 0) return PA_OK;
    int device = 0;
    const uint32_t *h_ec = nullptr, *h_ref = nullptr;
    index_host_classes(idx, &h_ec, &h_ref, &device);
    PA_HIP_TRY(hipSetDevice(device));
    const uint32_t blocks = grid_for((uint64_t)pa_tiles_words(n_reads, words_per_read));
    if (blocks == 0) return fail(PA_ERR_UNSUPPORTED, "a batch of %llu reads of %u words is too large for one launch", (unsigned long long)n_reads, words_per_read);
    hipLaunchKernelGGL(pa_revcomp_kernel, dim3(blocks), dim3(256), 0, static_cast<hipStream_t>(stream), d_tiles_in, d_lens, n_reads, words_per_read, d_tiles_out);
    PA_HIP_TRY(hipGetLastError());
    return PA_OK;
}

extern "C" size_t pa_pairs_scratch_bytes(uint64_t n_pairs) { return n_pairs > PAIR_MAX_PAIRS ? 0 : scratch_layout(n_pairs).total; }

extern "C" int pa_pairs_combine_device(pa_index* idx, const pa_read_result* d_res1, const uint32_t* d_arena1, const pa_read_result* d_res2,
                                       const uint32_t* d_arena2, uint64_t n_pairs, pa_read_result* d_results, uint32_t* d_arena, uint64_t arena_cap,
                                       uint64_t* d_counts, void* d_scratch, size_t scratch_bytes, void* stream) {
    if (!idx || !d_scratch || (n_pairs && (!d_res1 || !d_res2 || !d_results)) || (arena_cap && !d_arena)) return fail(PA_ERR_INVALID_ARG, "null argument");
    if (n_pairs > PAIR_MAX_PAIRS) return fail(PA_ERR_UNSUPPORTED, "at most %llu pairs in one launch", (unsigned long long)PAIR_MAX_PAIRS);
    if ((uintptr_t)d_scratch & 255) return fail(PA_ERR_INVALID_ARG, "the scratch must be 256-byte aligned");
    const PairScratch lay = scratch_layout(n_pairs);
    if (scratch_bytes < lay.total) return fail(PA_ERR_INVALID_ARG, "scratch of %zu bytes, %zu needed", scratch_bytes, lay.total);
    PairIndexView v;
    index_pair_view(idx, &v);
    PA_HIP_TRY(hipSetDevice(v.device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    uint8_t* base = static_cast<uint8_t*>(d_scratch);
    PairParams p = stage_params(v, n_pairs, d_results, d_arena, arena_cap, d_counts, d_scratch, lay);
    p.res1 = d_res1; p.res2 = d_res2; p.arena1 = d_arena1; p.arena2 = d_arena2;
    PA_HIP_TRY(hipMemsetAsync(base, 0, PAIR_CTL_BYTES, s));
    if (n_pairs == 0) return PA_OK;
    const uint32_t blocks = grid_for(n_pairs);
    const uint32_t cus = (uint32_t)std::max(1, v.num_cus);
    hipLaunchKernelGGL(pa_pairs_classify_kernel, dim3(blocks), dim3(256), 0, s, p);
    PA_HIP_TRY(hipGetLastError());
    size_t tmp_bytes = lay.tmp_bytes;
    PA_HIP_TRY(scan_exclusive_on(base + lay.tmp, tmp_bytes, (const uint32_t*)p.flags, p.off, (size_t)(2 * n_pairs + 1), s));
    hipLaunchKernelGGL(pa_pairs_scatter_kernel, dim3(blocks), dim3(256), 0, s, p);
    PA_HIP_TRY(hipGetLastError());
    // the bins' sizes stay on the device: both kernels are launched for the worst case and their waves go round over the items there are
    hipLaunchKernelGGL(pa_pairs_lane_kernel, dim3(std::min(blocks, cus * 8)), dim3(256), 0, s, p);
    PA_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(pa_pairs_wave_kernel, dim3(std::min(grid_for(n_pairs, 4), cus * 4)), dim3(256), 0, s, p);
    PA_HIP_TRY(hipGetLastError());
    if (p.novel) return overflow_after_map(v.ovf, p.novel, &p.ctl->novel_ctr, n_pairs, d_arena, s);
    return PA_OK;
}

int pa::pairs_arena_bound(pa_index* idx, const pa_read_result* d_res1, const pa_read_result* d_res2, uint64_t n_pairs, void* d_scratch, void* stream, uint64_t* bound) {
    return stage_arena_bound(idx, pa_pairs_bound_kernel, d_res1, d_res2, n_pairs, d_scratch, stream, bound, "too many pairs for one launch");
}

extern "C" int pa_pairs_finish(pa_index* idx, void* d_scratch, void* stream, uint64_t stats[PA_PAIR_STATS], uint64_t* arena_used, uint64_t* arena_needed) {
    return stage_finish(idx, d_scratch, stream, stats, arena_used, arena_needed, "pair");
}

// ---- host-buffer convenience: encode, orient, two launches, combine, D2H, CSR in pair order ----
namespace {

struct MateBuffers {
    DeviceBuffer<uint8_t> ascii;
    DeviceBuffer<uint64_t> offsets, tiles, rc_tiles;
    DeviceBuffer<uint32_t> lens, arena;
    DeviceBuffer<pa_read_result> results;
};

// one mate of every pair: H2D, encode, reverse complement if asked, map (the arena regrown as pa_map_finish asks)
int map_mate(pa_index* idx, const uint8_t* ascii, const uint64_t* offsets, uint64_t n, uint32_t maxlen, bool revcomp, uint32_t allowed, MateBuffers& b, hipStream_t s,
             uint64_t* arena_used = nullptr) {
    const uint32_t wpr = pa_words_per_read(std::max(1u, maxlen));
    const uint64_t total = offsets[n] - offsets[0];
    int rc;
    if ((rc = b.ascii.alloc(total + 64)) || (rc = b.offsets.alloc(n + 1)) || (rc = b.tiles.alloc(pa_tiles_words(n, wpr) + 1)) || (rc = b.lens.alloc(n + 64)) ||
        (rc = b.results.alloc(n + 1)))
        return rc;
    std::vector<uint64_t> rel(n + 1);
    for (uint64_t i = 0; i <= n; ++i) rel[i] = offsets[i] - offsets[0];
    if (total) PA_HIP_TRY(hipMemcpyAsync(b.ascii.get(), ascii + offsets[0], total, hipMemcpyHostToDevice, s));
    PA_HIP_TRY(hipMemcpyAsync(b.offsets.get(), rel.data(), (n + 1) * 8, hipMemcpyHostToDevice, s));
    if ((rc = pa_encode_reads_device(idx, b.ascii.get(), b.offsets.get(), n, wpr, b.tiles.get(), b.lens.get(), s)) != PA_OK) return rc;
    PA_HIP_TRY(hipStreamSynchronize(s));   // (`rel` is pageable and dies with this call)
    const uint64_t* tiles = b.tiles.get();
    if (revcomp) {
        if ((rc = b.rc_tiles.alloc(pa_tiles_words(n, wpr) + 1)) != PA_OK) return rc;
        if ((rc = pa_revcomp_tiles_device(idx, b.tiles.get(), b.lens.get(), n, wpr, b.rc_tiles.get(), s)) != PA_OK) return rc;
        tiles = b.rc_tiles.get();
    }
    if ((rc = b.arena.alloc(pa_map_arena_hint(idx, n))) != PA_OK) return rc;
    auto launch = [&] { return pa_map_batch_device(idx, tiles, b.lens.get(), n, wpr, allowed, b.results.get(), b.arena.get(), b.arena.size(), nullptr, s); };
    if ((rc = launch()) != PA_OK) return rc;
    uint64_t used = 0;
    rc = map_finish_regrow(idx, s, b.arena, &used, launch);
    if (arena_used) *arena_used = used;
    return rc;
}

// the argument checks of the host-buffer paths for one read set ("mate 1", "mate 2", "read"); *maxlen = its longest read (at least 1)
int check_reads(const char* what, const uint8_t* ascii, const uint64_t* offsets, uint64_t n, uint64_t* maxlen) {
    *maxlen = 1;
    for (uint64_t i = 0; i < n; ++i) {
        if (offsets[i + 1] < offsets[i]) return fail(PA_ERR_INVALID_ARG, "%s: offsets not monotone at %llu", what, (unsigned long long)i);
        *maxlen = std::max(*maxlen, offsets[i + 1] - offsets[i]);
    }
    if (n && offsets[n] != offsets[0] && !ascii) return fail(PA_ERR_INVALID_ARG, "null argument");
    if (*maxlen > PA_MAX_READ_LEN) return fail(PA_ERR_UNSUPPORTED, "read longer than %u bases", PA_MAX_READ_LEN);
    return PA_OK;
}

std::vector<uint32_t>& csr_ids() {   // the CSR's ids of the host-buffer paths below: library-owned until this thread's next call of one of them
    static thread_local std::vector<uint32_t> ids;
    return ids;
}

// records and the used part of their arena to the host, the classes as a CSR in item order
int results_to_host(pa_index* idx, const pa_read_result* d_results, const uint32_t* d_arena, uint64_t used, uint64_t n, pa_read_result* results, uint64_t* class_offsets,
                    const uint32_t** class_ids, hipStream_t s) {
    PA_HIP_TRY(hipMemcpyAsync(results, d_results, n * sizeof(pa_read_result), hipMemcpyDeviceToHost, s));
    std::vector<uint32_t> h_arena(used + 1);
    if (used) PA_HIP_TRY(hipMemcpyAsync(h_arena.data(), d_arena, used * 4, hipMemcpyDeviceToHost, s));
    PA_HIP_TRY(hipStreamSynchronize(s));
    if (class_offsets || class_ids) classes_to_csr(idx, results, n, h_arena.data(), csr_ids(), class_offsets, class_ids);
    return PA_OK;
}

// One stage (pair combine or strand merge) over two finished record sets, uncounted, its arena grown until the ids fit
struct StageOut {
    DeviceBuffer<uint8_t> scratch;
    DeviceBuffer<pa_read_result> results;
    DeviceBuffer<uint32_t> arena;
    uint64_t used = 0;
};
template <class Launch, class Finish>
int run_stage(uint64_t n, size_t scratch_bytes, StageOut& o, Launch&& launch, Finish&& finish) {
    int rc;
    if ((rc = o.scratch.alloc(scratch_bytes)) || (rc = o.results.alloc(n + 1))) return rc;
    uint64_t cap = 4 * n + 4096, need = 0;
    for (int attempt = 0;; ++attempt) {
        if ((rc = o.arena.alloc(cap)) != PA_OK) return rc;
        if ((rc = launch(o, cap, scratch_bytes)) != PA_OK) return rc;
        rc = finish(o, &need);
        if (rc == PA_ERR_ARENA_FULL && attempt < 2) { cap = need + 64; continue; }
        return rc;
    }
}
int combine_mates(pa_index* idx, const MateBuffers& m1, const MateBuffers& m2, uint64_t n, StageOut& o, hipStream_t s) {
    return run_stage(n, pa_pairs_scratch_bytes(n), o,
                     [&](StageOut& x, uint64_t cap, size_t sb) {
                         return pa_pairs_combine_device(idx, m1.results.get(), m1.arena.get(), m2.results.get(), m2.arena.get(), n, x.results.get(), x.arena.get(), cap, nullptr,
                                                        x.scratch.get(), sb, s);
                     },
                     [&](StageOut& x, uint64_t* need) { return pa_pairs_finish(idx, x.scratch.get(), s, nullptr, &x.used, need); });
}
int merge_strands(pa_index* idx, const pa_read_result* resS, const uint32_t* arenaS, const pa_read_result* resR, const uint32_t* arenaR, uint64_t n, StageOut& o, hipStream_t s) {
    return run_stage(n, pa_strands_scratch_bytes(n), o,
                     [&](StageOut& x, uint64_t cap, size_t sb) {
                         return pa_strands_merge_device(idx, resS, arenaS, resR, arenaR, n, x.results.get(), x.arena.get(), cap, nullptr, x.scratch.get(), sb, s);
                     },
                     [&](StageOut& x, uint64_t* need) { return pa_strands_finish(idx, x.scratch.get(), s, nullptr, &x.used, need); });
}


// pa_map_pairs (orient) and pa_map_pairs_unstranded (unstranded: orient is not looked at)
int map_pairs_impl(pa_index* idx, const uint8_t* ascii1, const uint64_t* offsets1, const uint8_t* ascii2, const uint64_t* offsets2, uint64_t n, int orient, bool unstranded,
                   uint32_t allowed, pa_read_result* results, uint64_t* class_offsets, const uint32_t** class_ids) {
    if (!idx || !offsets1 || !offsets2 || (n && !results)) return fail(PA_ERR_INVALID_ARG, "null argument");
    if (!unstranded && orient != PA_PAIR_FR && orient != PA_PAIR_RF && orient != PA_PAIR_FF)
        return fail(PA_ERR_INVALID_ARG, "orientation %d (PA_PAIR_FR, PA_PAIR_RF or PA_PAIR_FF)", orient);
    if (n > PAIR_MAX_PAIRS) return fail(PA_ERR_UNSUPPORTED, "at most %llu pairs in one call", (unsigned long long)PAIR_MAX_PAIRS);
    uint64_t maxlen[2] = {1, 1};
    int rc;
    if ((rc = check_reads("mate 1", ascii1, offsets1, n, &maxlen[0])) != PA_OK || (rc = check_reads("mate 2", ascii2, offsets2, n, &maxlen[1])) != PA_OK) return rc;
    if (n == 0) { if (class_offsets) class_offsets[0] = 0; if (class_ids) *class_ids = nullptr; return PA_OK; }
    PairIndexView v;
    index_pair_view(idx, &v);
    PA_HIP_TRY(hipSetDevice(v.device));
    IndexStream stream;   // a stream of this call's own: its launch context on idx is shared with nobody and released at the end
    if ((rc = stream.create(idx)) != PA_OK) return rc;
    const hipStream_t s = stream.get();
    if (!unstranded) {
        MateBuffers mb[2];
        StageOut pair;
        if ((rc = map_mate(idx, ascii1, offsets1, n, (uint32_t)maxlen[0], orient == PA_PAIR_RF, allowed, mb[0], s)) != PA_OK) return rc;
        if ((rc = map_mate(idx, ascii2, offsets2, n, (uint32_t)maxlen[1], orient == PA_PAIR_FR, allowed, mb[1], s)) != PA_OK) return rc;
        if ((rc = combine_mates(idx, mb[0], mb[1], n, pair, s)) != PA_OK) return rc;
        return results_to_host(idx, pair.results.get(), pair.arena.get(), pair.used, n, results, class_offsets, class_ids, s);
    }
    // four mappings one after the other on the one stream (map_mate finishes each before the next is launched), the two candidates, the merge
    MateBuffers fw[2], rv[2];
    StageOut cand[2], item;
    if ((rc = map_mate(idx, ascii1, offsets1, n, (uint32_t)maxlen[0], false, allowed, fw[0], s)) != PA_OK) return rc;
    if ((rc = map_mate(idx, ascii2, offsets2, n, (uint32_t)maxlen[1], false, allowed, fw[1], s)) != PA_OK) return rc;
    if ((rc = map_mate(idx, ascii1, offsets1, n, (uint32_t)maxlen[0], true, allowed, rv[0], s)) != PA_OK) return rc;
    if ((rc = map_mate(idx, ascii2, offsets2, n, (uint32_t)maxlen[1], true, allowed, rv[1], s)) != PA_OK) return rc;
    if ((rc = combine_mates(idx, fw[0], rv[1], n, cand[0], s)) != PA_OK) return rc;   // S: PA_PAIR_FR
    if ((rc = combine_mates(idx, rv[0], fw[1], n, cand[1], s)) != PA_OK) return rc;   // R: PA_PAIR_RF
    if ((rc = merge_strands(idx, cand[0].results.get(), cand[0].arena.get(), cand[1].results.get(), cand[1].arena.get(), n, item, s)) != PA_OK) return rc;
    return results_to_host(idx, item.results.get(), item.arena.get(), item.used, n, results, class_offsets, class_ids, s);
}

int map_batch_strand_impl(pa_index* idx, const uint8_t* ascii, const uint64_t* offsets, uint64_t n, int strand, uint32_t allowed, pa_read_result* results,
                          uint64_t* class_offsets, const uint32_t** class_ids) {
    if (!idx || !offsets || (n && !results)) return fail(PA_ERR_INVALID_ARG, "null argument");
    if (strand != PA_STRAND_FWD && strand != PA_STRAND_REV && strand != PA_STRAND_BOTH)
        return fail(PA_ERR_INVALID_ARG, "strand %d (PA_STRAND_FWD, PA_STRAND_REV or PA_STRAND_BOTH)", strand);
    if (n > PAIR_MAX_PAIRS) return fail(PA_ERR_UNSUPPORTED, "at most %llu reads in one call", (unsigned long long)PAIR_MAX_PAIRS);
    uint64_t maxlen = 1;
    int rc = check_reads("read", ascii, offsets, n, &maxlen);
    if (rc != PA_OK) return rc;
    if (n == 0) { if (class_offsets) class_offsets[0] = 0; if (class_ids) *class_ids = nullptr; return PA_OK; }
    PairIndexView v;
    index_pair_view(idx, &v);
    PA_HIP_TRY(hipSetDevice(v.device));
    IndexStream stream;
    if ((rc = stream.create(idx)) != PA_OK) return rc;
    const hipStream_t s = stream.get();
    MateBuffers fw, rv;
    uint64_t used = 0;
    if (strand != PA_STRAND_BOTH) {
        MateBuffers& b = strand == PA_STRAND_REV ? rv : fw;
        if ((rc = map_mate(idx, ascii, offsets, n, (uint32_t)maxlen, strand == PA_STRAND_REV, allowed, b, s, &used)) != PA_OK) return rc;
        return results_to_host(idx, b.results.get(), b.arena.get(), used, n, results, class_offsets, class_ids, s);
    }
    StageOut item;
    if ((rc = map_mate(idx, ascii, offsets, n, (uint32_t)maxlen, false, allowed, fw, s)) != PA_OK) return rc;
    if ((rc = map_mate(idx, ascii, offsets, n, (uint32_t)maxlen, true, allowed, rv, s)) != PA_OK) return rc;
    if ((rc = merge_strands(idx, fw.results.get(), fw.arena.get(), rv.results.get(), rv.arena.get(), n, item, s)) != PA_OK) return rc;
    return results_to_host(idx, item.results.get(), item.arena.get(), item.used, n, results, class_offsets, class_ids, s);
}

template <class F>
int no_bad_alloc(const char* what, F&& f) {
    try {
        return f();
    } catch (const std::bad_alloc&) {
        return fail(PA_ERR_OOM, "out of host memory in %s", what);
    }
}

}  // namespace

extern "C" int pa_map_pairs(pa_index* idx, const uint8_t* ascii1, const uint64_t* offsets1, const uint8_t* ascii2, const uint64_t* offsets2, uint64_t n_pairs,
                            int orient, uint32_t allowed_mismatches, pa_read_result* results, uint64_t* class_offsets, const uint32_t** class_ids) {
    return no_bad_alloc("pa_map_pairs", [&] { return map_pairs_impl(idx, ascii1, offsets1, ascii2, offsets2, n_pairs, orient, false, allowed_mismatches, results, class_offsets, class_ids); });
}

extern "C" int pa_map_pairs_unstranded(pa_index* idx, const uint8_t* ascii1, const uint64_t* offsets1, const uint8_t* ascii2, const uint64_t* offsets2, uint64_t n_pairs,
                                       uint32_t allowed_mismatches, pa_read_result* results, uint64_t* class_offsets, const uint32_t** class_ids) {
    return no_bad_alloc("pa_map_pairs_unstranded", [&] { return map_pairs_impl(idx, ascii1, offsets1, ascii2, offsets2, n_pairs, 0, true, allowed_mismatches, results, class_offsets, class_ids); });
}

extern "C" int pa_map_batch_strand(pa_index* idx, const uint8_t* ascii, const uint64_t* offsets, uint64_t n_reads, int strand, uint32_t allowed_mismatches,
                                   pa_read_result* results, uint64_t* class_offsets, const uint32_t** class_ids) {
    return no_bad_alloc("pa_map_batch_strand", [&] { return map_batch_strand_impl(idx, ascii, offsets, n_reads, strand, allowed_mismatches, results, class_offsets, class_ids); });
}
