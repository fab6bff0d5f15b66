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
// The control block (arena top, status, stats, novel counter) lives at the start of the caller's scratch.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <memory>
#include <vector>

#include "device_prims.hpp"
#include "hip_buffer.hpp"
#include "kernel_utils.hpp"
#include "kernels.hpp"
#include "pa_common.hpp"

namespace pa {
namespace {

constexpr uint32_t PAIR_LANE_MAX = 16;                                // the shorter list has at most this many ids: a lane; more: a wave
constexpr uint32_t PAIR_UNFIT = (uint32_t)PA_MAX_ARENA_ENTRIES;       // class_off of a record whose ids did not fit the arena
constexpr uint32_t NO_CLASS = 0xFFFFFFFFu;
constexpr uint32_t PAIR_CTL_BYTES = 256;
constexpr uint32_t ST_PAIRS = 0, ST_BOTH = 1, ST_ONLY1 = 2, ST_ONLY2 = 3, ST_NEITHER = 4, ST_EMPTY = 5, ST_REF = 6, ST_ARENA = 7;

struct PairCtl {   // the first PAIR_CTL_BYTES of the scratch, zeroed by every launch
    unsigned long long arena_top;                // ids asked for so far (exact: no chunks, no padding)
    unsigned long long stats[PA_PAIR_STATS];
    unsigned long long novel_ctr;                // results on the novel list
    unsigned long long arena_cap;                // of the launch (what pa_pairs_finish clamps arena_used to)
    uint32_t status, pad;
};
static_assert(sizeof(PairCtl) <= PAIR_CTL_BYTES, "the control block fits its slot");

struct PairParams {
    DevIndexView ix;
    const uint32_t* class_table;
    uint64_t class_table_size;
    const pa_read_result *res1, *res2;
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

// the class fields of a pair's record (coverage and mismatches are the classify kernel's)
__device__ __forceinline__ void put_class(const PairParams& p, uint32_t pair, uint32_t off, uint32_t len) {
    uint32_t* rec = reinterpret_cast<uint32_t*>(p.results + pair);
    rec[2] = off;
    rec[3] = len;
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

// ---------------------------------------------------------------------------------------------- scratch
size_t round256(size_t b) { return (b + 255) & ~(size_t)255; }

struct PairScratch {
    size_t flags, off, items, novel, tmp, tmp_bytes, total;
};
PairScratch scratch_layout(uint64_t n) {
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

constexpr uint64_t PAIR_MAX_PAIRS = 0x7FFFFFF0ull;   // pair and item indices, and 2 n + 1 flags, are 32-bit

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
    PairParams p{};
    p.ix = v.dv;
    p.class_table = v.class_table;
    p.class_table_size = v.class_table_size;
    p.res1 = d_res1; p.res2 = d_res2; p.arena1 = d_arena1; p.arena2 = d_arena2;
    p.n = (uint32_t)n_pairs;
    p.results = d_results;
    p.arena = d_arena;
    p.arena_cap = arena_cap > PA_MAX_ARENA_ENTRIES ? PA_MAX_ARENA_ENTRIES : arena_cap;   // offsets leave bit 31 of class_off free
    p.counts = reinterpret_cast<unsigned long long*>(d_counts);
    p.ctl = reinterpret_cast<PairCtl*>(base);
    p.flags = reinterpret_cast<uint32_t*>(base + lay.flags);
    p.off = reinterpret_cast<uint32_t*>(base + lay.off);
    p.items = reinterpret_cast<uint32_t*>(base + lay.items);
    p.novel = (d_counts && v.ovf) ? reinterpret_cast<uint32_t*>(base + lay.novel) : nullptr;
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
    if (!idx || !d_scratch || !bound || (n_pairs && (!d_res1 || !d_res2))) return fail(PA_ERR_INVALID_ARG, "null argument");
    PairIndexView v;
    index_pair_view(idx, &v);
    PA_HIP_TRY(hipSetDevice(v.device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    PA_HIP_TRY(hipMemsetAsync(d_scratch, 0, 8, s));
    if (n_pairs) {
        const uint32_t blocks = grid_for(n_pairs);
        if (blocks == 0) return fail(PA_ERR_UNSUPPORTED, "too many pairs for one launch");
        hipLaunchKernelGGL(pa_pairs_bound_kernel, dim3(blocks), dim3(256), 0, s, d_res1, d_res2, n_pairs, static_cast<unsigned long long*>(d_scratch));
        PA_HIP_TRY(hipGetLastError());
    }
    unsigned long long h = 0;
    PA_HIP_TRY(hipMemcpyAsync(&h, d_scratch, 8, hipMemcpyDeviceToHost, s));
    PA_HIP_TRY(hipStreamSynchronize(s));
    *bound = h;
    return PA_OK;
}

extern "C" int pa_pairs_finish(pa_index* idx, void* d_scratch, void* stream, uint64_t stats[PA_PAIR_STATS], uint64_t* arena_used, uint64_t* arena_needed) {
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
    if (h.status & PA_STATUS_ARENA_FULL) return fail(PA_ERR_ARENA_FULL, "pair arena too small: %llu entries needed", h.arena_top);
    return PA_OK;
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
int map_mate(pa_index* idx, const uint8_t* ascii, const uint64_t* offsets, uint64_t n, uint32_t maxlen, bool revcomp, uint32_t allowed, MateBuffers& b, hipStream_t s) {
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
    return map_finish_regrow(idx, s, b.arena, &used, launch);
}

int map_pairs_impl(pa_index* idx, const uint8_t* ascii1, const uint64_t* offsets1, const uint8_t* ascii2, const uint64_t* offsets2, uint64_t n, int orient,
                   uint32_t allowed, pa_read_result* results, uint64_t* class_offsets, const uint32_t** class_ids) {
    if (!idx || !offsets1 || !offsets2 || (n && !results)) return fail(PA_ERR_INVALID_ARG, "null argument");
    if (orient != PA_PAIR_FR && orient != PA_PAIR_RF && orient != PA_PAIR_FF) return fail(PA_ERR_INVALID_ARG, "orientation %d (PA_PAIR_FR, PA_PAIR_RF or PA_PAIR_FF)", orient);
    if (n > PAIR_MAX_PAIRS) return fail(PA_ERR_UNSUPPORTED, "at most %llu pairs in one call", (unsigned long long)PAIR_MAX_PAIRS);
    uint64_t maxlen[2] = {1, 1};
    const uint64_t* offs[2] = {offsets1, offsets2};
    const uint8_t* asc[2] = {ascii1, ascii2};
    for (int mt = 0; mt < 2; ++mt) {
        for (uint64_t i = 0; i < n; ++i) {
            if (offs[mt][i + 1] < offs[mt][i]) return fail(PA_ERR_INVALID_ARG, "mate %d: offsets not monotone at pair %llu", mt + 1, (unsigned long long)i);
            maxlen[mt] = std::max(maxlen[mt], offs[mt][i + 1] - offs[mt][i]);
        }
        if (n && offs[mt][n] != offs[mt][0] && !asc[mt]) return fail(PA_ERR_INVALID_ARG, "null argument");
        if (maxlen[mt] > PA_MAX_READ_LEN) return fail(PA_ERR_UNSUPPORTED, "read longer than %u bases", PA_MAX_READ_LEN);
    }
    static thread_local std::vector<uint32_t> t_class_ids;   // the CSR's ids: library-owned until this thread's next call
    if (n == 0) { if (class_offsets) class_offsets[0] = 0; if (class_ids) *class_ids = nullptr; return PA_OK; }
    PairIndexView v;
    index_pair_view(idx, &v);
    PA_HIP_TRY(hipSetDevice(v.device));
    IndexStream stream;   // a stream of this call's own: its launch context on idx is shared with nobody and released at the end
    int rc = stream.create(idx);
    if (rc != PA_OK) return rc;
    const hipStream_t s = stream.get();
    MateBuffers mb[2];
    if ((rc = map_mate(idx, ascii1, offsets1, n, (uint32_t)maxlen[0], orient == PA_PAIR_RF, allowed, mb[0], s)) != PA_OK) return rc;
    if ((rc = map_mate(idx, ascii2, offsets2, n, (uint32_t)maxlen[1], orient == PA_PAIR_FR, allowed, mb[1], s)) != PA_OK) return rc;
    DeviceBuffer<uint8_t> scratch;
    DeviceBuffer<pa_read_result> d_results;
    DeviceBuffer<uint32_t> d_arena;
    const size_t scratch_bytes = pa_pairs_scratch_bytes(n);
    if ((rc = scratch.alloc(scratch_bytes)) || (rc = d_results.alloc(n + 1))) return rc;
    uint64_t cap = 4 * n + 4096, used = 0, need = 0;
    for (int attempt = 0;; ++attempt) {
        if ((rc = d_arena.alloc(cap)) != PA_OK) return rc;
        if ((rc = pa_pairs_combine_device(idx, mb[0].results.get(), mb[0].arena.get(), mb[1].results.get(), mb[1].arena.get(), n, d_results.get(), d_arena.get(), cap,
                                          nullptr, scratch.get(), scratch_bytes, s)) != PA_OK)
            return rc;
        rc = pa_pairs_finish(idx, scratch.get(), s, nullptr, &used, &need);
        if (rc == PA_ERR_ARENA_FULL && attempt < 2) { cap = need + 64; continue; }
        if (rc != PA_OK) return rc;
        break;
    }
    PA_HIP_TRY(hipMemcpyAsync(results, d_results.get(), n * sizeof(pa_read_result), hipMemcpyDeviceToHost, s));
    std::vector<uint32_t> h_arena(used + 1);
    if (used) PA_HIP_TRY(hipMemcpyAsync(h_arena.data(), d_arena.get(), used * 4, hipMemcpyDeviceToHost, s));
    PA_HIP_TRY(hipStreamSynchronize(s));
    if (class_offsets || class_ids) classes_to_csr(idx, results, n, h_arena.data(), t_class_ids, class_offsets, class_ids);
    return PA_OK;
}

}  // namespace

extern "C" int pa_map_pairs(pa_index* idx, const uint8_t* ascii1, const uint64_t* offsets1, const uint8_t* ascii2, const uint64_t* offsets2, uint64_t n_pairs,
                            int orient, uint32_t allowed_mismatches, pa_read_result* results, uint64_t* class_offsets, const uint32_t** class_ids) {
    try {
        return map_pairs_impl(idx, ascii1, offsets1, ascii2, offsets2, n_pairs, orient, allowed_mismatches, results, class_offsets, class_ids);
    } catch (const std::bad_alloc&) {
        return fail(PA_ERR_OOM, "out of host memory in pa_map_pairs");
    }
}
