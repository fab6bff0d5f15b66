// Paired-end reads behind the map launch (include/pseudoaligner_amd.h, "paired-end reads"). Nothing here touches the map,
// resolve, count or ingest sources: the mates are mapped by two ordinary pa_map_batch_device launches and the stage of pair_stage.hpp combines
// their records per pair into ordinary pa_read_result records plus arena ids, by the rule below.
//
//   pa_revcomp_kernel  reverse complement of packed reads in the tile layout: a thread per (read, output word); the output word is cut out of
//                      the one or two input words it straddles, its 32 two-bit groups reversed (__brevll + swap of the two bits of a group)
//                      and complemented. No per-base loop; lanes of a wave are the 64 reads of a tile, so loads and stores are coalesced
//                      whenever the tile's reads have one length
//   PairRule           classify: the record of every pair that needs no id traffic (neither mate mapped, a mate with an empty class, one
//                      mate mapped by reference, the same reference twice) is final; the others get the WORK KEY "length of the shorter list"
//                      lane: the ids of the shorter list looked up one after the other in the rest of the longer one (a merge whose steps in
//                      the longer list are binary searches); the result is a mask of the shorter list's positions
//                      wave: lanes take 64 ids of the shorter list at a time and binary-search the longer one; a ballot and a prefix popcount
//                      give every survivor its ordered position (a block of 64 ids: one burst)
// A mate mapped alone whose ids lie in its mate arena is the pair "list with itself": the same two kernels copy it into the pair arena.
#include <hip/hip_runtime.h>

#include "pair_stage.hpp"

namespace pa {
namespace {

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

}  // namespace

// ---------------------------------------------------------------------------------------------- the pair rule
// stats: slot 5 = the pair's class is empty (a mate's class is, or the intersection)
struct PairRule {
    static constexpr uint32_t LANE_MAX = 16;                              // the shorter list has at most this many ids: a lane; more: a wave
    static constexpr const char* NOUN = "pairs";
    static constexpr uint32_t ST_EMPTY = 5, CLASSIFY_STAT = ST_EMPTY, EMPTY_STAT = ST_EMPTY;

    static __device__ __forceinline__ Classified classify(const pa_read_result& r1, const pa_read_result& r2, uint32_t nc) {
        Classified c{{0, 0, 0, 0}, 0, nc + 2, (r1.mismatches & PA_MAPPED_BIT) != 0, (r2.mismatches & PA_MAPPED_BIT) != 0, false, false};
        pa_read_result& o = c.rec;
        if (c.m1 && c.m2) {
            o.coverage = r1.coverage + r2.coverage;
            o.mismatches = ((r1.mismatches & ~PA_MAPPED_BIT) + (r2.mismatches & ~PA_MAPPED_BIT)) | PA_MAPPED_BIT;
            if (r1.class_len == 0 || r2.class_len == 0) { c.slot = nc + 1; c.own = true; }
            else if ((r1.class_off & PA_CLASS_REF) && r1.class_off == r2.class_off) { o.class_off = r1.class_off; o.class_len = r1.class_len; c.slot = r1.class_off & ~PA_CLASS_REF; c.by_ref = true; }
            else c.key = r1.class_len < r2.class_len ? r1.class_len : r2.class_len;
        } else if (c.m1 || c.m2) {
            const pa_read_result r = c.m1 ? r1 : r2;
            o.coverage = r.coverage;
            o.mismatches = r.mismatches;
            if (r.class_len == 0) c.slot = nc + 1;
            else if (r.class_off & PA_CLASS_REF) { o.class_off = r.class_off; o.class_len = r.class_len; c.slot = r.class_off & ~PA_CLASS_REF; c.by_ref = true; }
            else c.key = r.class_len;
        }
        return c;
    }

    static __device__ __forceinline__ uint32_t need(const pa_read_result& r1, const pa_read_result& r2) {
        const bool m1 = r1.mismatches & PA_MAPPED_BIT, m2 = r2.mismatches & PA_MAPPED_BIT;
        return m1 && m2 ? (r1.class_len < r2.class_len ? r1.class_len : r2.class_len) : m1 ? r1.class_len : m2 ? r2.class_len : 0;
    }

    // a = the shorter list (mate 1 on a tie); a mate mapped alone is paired with itself
    static __device__ __forceinline__ IdLists lists_of(const PairParams& p, uint32_t pair) {
        const pa_read_result r1 = p.res1[pair], r2 = p.res2[pair];
        const bool m1 = r1.mismatches & PA_MAPPED_BIT, m2 = r2.mismatches & PA_MAPPED_BIT;
        const pa_read_result x = m1 ? r1 : r2, y = m2 ? r2 : r1;        // (one mate alone: x == y)
        const uint32_t *ax = m1 ? p.arena1 : p.arena2, *ay = m2 ? p.arena2 : p.arena1;
        const bool swap = y.class_len < x.class_len;
        const pa_read_result s = swap ? y : x, g = swap ? x : y;
        return IdLists{ids_of(s, swap ? ay : ax, p.ix), ids_of(g, swap ? ax : ay, p.ix), s.class_len, g.class_len, ref_class_of(s), ref_class_of(g)};
    }

    struct Each {   // {a[t] : bit t of keep}
        const uint32_t* a;
        uint32_t keep;
        template <class F>
        __device__ __forceinline__ void operator()(F&& f) const {
            for (uint32_t k = keep; k != 0; k &= k - 1) f(a[__ffs((int)k) - 1]);
        }
    };
    static __device__ __forceinline__ Each lane_combine(const IdLists& l, uint32_t& m) {
        uint32_t keep = 0, pb = 0;   // keep: bit t = id t of the shorter list survives
        for (uint32_t t = 0; t < l.na && t < LANE_MAX && pb < l.nb; ++t) {
            const uint32_t a = l.a[t];
            pb = lower_bound_ids(l.b, pb, l.nb, a);
            if (pb < l.nb && l.b[pb] == a) { keep |= 1u << t; ++pb; }
        }
        m = (uint32_t)__popc(keep);
        return Each{l.a, keep};
    }

    static __device__ __forceinline__ uint32_t wave_count(const IdLists& l, uint32_t lane) {
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
        return m;
    }
    static __device__ __forceinline__ void wave_write(const IdLists& l, uint32_t lane, uint32_t* out, uint32_t) {
        const unsigned long long below = (1ull << lane) - 1;
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
            if (hit) out[done + __popcll(mask & below)] = a;
            done += (uint32_t)__popcll(mask);
        }
    }
};

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

extern "C" size_t pa_pairs_scratch_bytes(uint64_t n_pairs) { return stage_scratch_bytes(n_pairs); }

extern "C" int pa_pairs_combine_device(pa_index* idx, const pa_read_result* d_res1, const uint32_t* d_arena1, const pa_read_result* d_res2,
                                       const uint32_t* d_arena2, uint64_t n_pairs, pa_read_result* d_results, uint32_t* d_arena, uint64_t arena_cap,
                                       uint64_t* d_counts, void* d_scratch, size_t scratch_bytes, void* stream) {
    return stage_launch<PairRule>(idx, d_res1, d_arena1, d_res2, d_arena2, n_pairs, d_results, d_arena, arena_cap, d_counts, d_scratch, scratch_bytes, stream);
}

int pa::pairs_arena_bound(pa_index* idx, const pa_read_result* d_res1, const pa_read_result* d_res2, uint64_t n_pairs, void* d_scratch, void* stream, uint64_t* bound) {
    return stage_arena_bound<PairRule>(idx, d_res1, d_res2, n_pairs, d_scratch, stream, bound);
}

extern "C" int pa_pairs_finish(pa_index* idx, void* d_scratch, void* stream, uint64_t stats[PA_PAIR_STATS], uint64_t* arena_used, uint64_t* arena_needed) {
    return stage_finish(idx, d_scratch, stream, stats, arena_used, arena_needed, "pair");
}
