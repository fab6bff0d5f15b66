// The host-buffer paths behind pa_map_pairs, pa_map_pairs_unstranded and pa_map_batch_strand (include/pseudoaligner_amd.h):
// encode, orient, the map launches, the pair combine and / or the strand merge, D2H, the classes as a CSR in item order. Everything here goes
// through the C ABI and the HIP runtime: no kernel of its own, and the stages' device side (pair_stage.hpp) is not seen.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <new>
#include <vector>

#include "hip_buffer.hpp"
#include "kernels.hpp"
#include "pa_common.hpp"

using namespace pa;

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
