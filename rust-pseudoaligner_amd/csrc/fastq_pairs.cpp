// The drivers that map BOTH mates of PAIRED FASTQ files: pa_count_pairs (the mates oriented, their classes intersected -> the class-count table) and
// pa_count_pairs_unstranded (both orientations mapped, the candidates merged: DESIGN.md §4h), and what a call reports of its input. Reader, batches, loop,
// call frame and stage sizing are pair_reader.hpp's; a mapping that ran out of arena goes through map_finish_regrow (hip_buffer.hpp).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "pair_reader.hpp"

using namespace pa;
using namespace pa::ingest;

namespace {

// ---- pa_count_pairs ----
struct PairBatch : MateBatch {   // + the reverse-complemented tiles of one mate, the pair stage's outputs
    static constexpr int STREAMS = 2, STATS = PA_PAIR_STATS;
    DeviceBuffer<uint64_t> d_rc;
    DeviceBuffer<uint32_t> d_parena;
    DeviceBuffer<pa_read_result> d_presults;
    DeviceBuffer<uint8_t> d_scratch;
};

// the mate whose reverse complement is mapped (-1: neither)
int revcomp_mate(int orient) { return orient == PA_PAIR_RF ? 0 : orient == PA_PAIR_FR ? 1 : -1; }

// the batch's GPU leg up to the two mappings: mate m on s[m] (each stream has its own launch context on idx), all asynchronous
int batch_map(pa_index* idx, PairBatch& b, int orient, uint32_t allowed, const hipStream_t s[2]) {
    int e = PA_OK;
    for (int m = 0; m < 2; ++m)
        if ((e = b.mate[m].encode(idx, b.n, 64, s[m])) != PA_OK) return e;
    if ((e = b.d_presults.reserve(b.n + 64, b.mate[0].off_size() + 64)) != PA_OK) return e;
    for (int m = 0; m < 2; ++m) {
        Mate& x = b.mate[m];
        const uint64_t* tiles = x.d_tiles.get();
        if (m == revcomp_mate(orient)) {
            const size_t tw = std::max(pa_tiles_words(b.n, b.mate[0].wpr()), pa_tiles_words(b.n, b.mate[1].wpr())) + 1;
            if ((e = b.d_rc.reserve(tw, tw)) != PA_OK) return e;
            if ((e = pa_revcomp_tiles_device(idx, x.d_tiles.get(), x.d_lens.get(), b.n, x.wpr(), b.d_rc.get(), s[m])) != PA_OK) return e;
            tiles = b.d_rc.get();
        }
        if ((e = x.map(idx, tiles, b.n, allowed, s[m])) != PA_OK) return e;
    }
    return PA_OK;
}

// waits for the two mappings (regrowing an arena as pa_map_finish asks), then combines and counts the batch on s[0]
int batch_count(pa_index* idx, PairBatch& b, int orient, uint32_t allowed, uint64_t* d_counts, const hipStream_t s[2], uint64_t* stats, double* st) {
    double t0 = now();
    Mate &m1 = b.mate[0], &m2 = b.mate[1];
    for (int m = 0; m < 2; ++m) {
        Mate& x = b.mate[m];
        const uint64_t* tiles = m == revcomp_mate(orient) ? b.d_rc.get() : x.d_tiles.get();
        uint64_t used = 0;
        const int e = map_finish_regrow(idx, s[m], x.d_arena, &used, [&] { return x.map(idx, tiles, b.n, allowed, s[m]); });
        if (e != PA_OK) return e;
    }
    st[ST_WAIT] += now() - t0;
    t0 = now();
    const size_t scratch_bytes = pa_pairs_scratch_bytes(b.n);
    int e = size_stage(idx, pairs_arena_bound, m1.d_results.get(), m2.d_results.get(), b.n, scratch_bytes, b.d_scratch, b.d_parena, s[0]);
    if (e != PA_OK) return e;
    if ((e = pa_pairs_combine_device(idx, m1.d_results.get(), m1.d_arena.get(), m2.d_results.get(), m2.d_arena.get(), b.n, b.d_presults.get(), b.d_parena.get(), b.d_parena.size(),
                                     d_counts, b.d_scratch.get(), scratch_bytes, s[0])) != PA_OK)
        return e;
    uint64_t bst[PA_PAIR_STATS], used = 0, need = 0;
    if ((e = pa_pairs_finish(idx, b.d_scratch.get(), s[0], bst, &used, &need)) != PA_OK) return e;
    for (int j = 0; j < PA_PAIR_STATS; ++j) stats[j] += bst[j];
    st[ST_TALLY] += now() - t0;
    return PA_OK;
}

// ---- pa_count_pairs_unstranded ----
// Streams: s[m] maps mate m as given, s[2 + m] its reverse complement: four launch contexts on idx, so that all four mappings of a batch are in
// flight while the next batch is gathered. The tiles and lengths s[2 + m] reads are made on s[m]: it waits for `encoded[m]`.
struct StrandBatch : MateBatch {
    static constexpr int STREAMS = 4, STATS = PA_STRAND_STATS;
    DeviceBuffer<uint64_t> d_rc[2];                   // per mate: the reverse-complemented tiles and what their mapping leaves
    DeviceBuffer<uint32_t> d_rc_arena[2];
    DeviceBuffer<pa_read_result> d_rc_results[2];
    GpuEvent encoded[2];
    DeviceBuffer<uint32_t> d_carena[2], d_marena;     // the candidates' (S, R) and the merge's outputs
    DeviceBuffer<pa_read_result> d_cresults[2], d_mresults;
    DeviceBuffer<uint8_t> d_cscratch[2], d_mscratch;
};

int strand_map_rc(pa_index* idx, StrandBatch& b, int m, uint32_t allowed, hipStream_t s) {
    Mate& x = b.mate[m];
    return pa_map_batch_device(idx, b.d_rc[m].get(), x.d_lens.get(), b.n, x.wpr(), allowed, b.d_rc_results[m].get(), b.d_rc_arena[m].get(), b.d_rc_arena[m].size(), nullptr, s);
}

// the batch's GPU leg up to the four mappings, all asynchronous
int batch_map(pa_index* idx, StrandBatch& b, int, uint32_t allowed, const hipStream_t s[4]) {
    int e = PA_OK;
    const size_t reads = b.mate[0].off_size() + 64;
    const uint64_t hint = pa_map_arena_hint(idx, b.n);
    for (int m = 0; m < 2; ++m) {
        Mate& x = b.mate[m];
        if ((e = x.encode(idx, b.n, 64, s[m])) != PA_OK) return e;
        const size_t tw = pa_tiles_words(b.n, x.wpr()) + 1;
        if ((e = b.d_rc[m].reserve(tw, tw)) || (e = b.d_rc_results[m].reserve(b.n + 64, reads)) || (e = b.d_rc_arena[m].reserve(hint, hint)) ||
            (e = b.d_cresults[m].reserve(b.n + 64, reads)))
            return e;
        if ((e = b.encoded[m].record(s[m])) != PA_OK) return e;
        PA_HIP_TRY(hipStreamWaitEvent(s[2 + m], b.encoded[m].e, 0));
        if ((e = pa_revcomp_tiles_device(idx, x.d_tiles.get(), x.d_lens.get(), b.n, x.wpr(), b.d_rc[m].get(), s[2 + m])) != PA_OK) return e;
        if ((e = x.map(idx, x.d_tiles.get(), b.n, allowed, s[m])) != PA_OK || (e = strand_map_rc(idx, b, m, allowed, s[2 + m])) != PA_OK) return e;
    }
    return b.d_mresults.reserve(b.n + 64, reads);
}

// waits for the four mappings (regrowing an arena as pa_map_finish asks), combines S on s[0] and R on s[1], both uncounted, then merges and counts on s[0]
int batch_count(pa_index* idx, StrandBatch& b, int, uint32_t allowed, uint64_t* d_counts, const hipStream_t s[4], uint64_t* stats, double* st) {
    double t0 = now();
    int e = PA_OK;
    for (int m = 0; m < 2; ++m) {
        Mate& x = b.mate[m];
        uint64_t used = 0;
        if ((e = map_finish_regrow(idx, s[m], x.d_arena, &used, [&] { return x.map(idx, x.d_tiles.get(), b.n, allowed, s[m]); })) != PA_OK) return e;
        if ((e = map_finish_regrow(idx, s[2 + m], b.d_rc_arena[m], &used, [&] { return strand_map_rc(idx, b, m, allowed, s[2 + m]); })) != PA_OK) return e;
    }
    st[ST_WAIT] += now() - t0;
    t0 = now();
    // every arena is sized by a bound on what its launch can need: the combines are not re-run, and the counted merge cannot be (it would count twice)
    Mate &m1 = b.mate[0], &m2 = b.mate[1];
    const pa_read_result* res1[2] = {m1.d_results.get(), b.d_rc_results[0].get()};   // candidate c: mate 1's records, its arena, mate 2's
    const uint32_t* ar1[2] = {m1.d_arena.get(), b.d_rc_arena[0].get()};
    const pa_read_result* res2[2] = {b.d_rc_results[1].get(), m2.d_results.get()};
    const uint32_t* ar2[2] = {b.d_rc_arena[1].get(), m2.d_arena.get()};
    const size_t cbytes = pa_pairs_scratch_bytes(b.n), mbytes = pa_strands_scratch_bytes(b.n);
    for (int c = 0; c < 2; ++c) {
        if ((e = size_stage(idx, pairs_arena_bound, res1[c], res2[c], b.n, cbytes, b.d_cscratch[c], b.d_carena[c], s[c])) != PA_OK) return e;
        if ((e = pa_pairs_combine_device(idx, res1[c], ar1[c], res2[c], ar2[c], b.n, b.d_cresults[c].get(), b.d_carena[c].get(), b.d_carena[c].size(), nullptr,
                                         b.d_cscratch[c].get(), cbytes, s[c])) != PA_OK)
            return e;
    }
    for (int c = 0; c < 2; ++c)
        if ((e = pa_pairs_finish(idx, b.d_cscratch[c].get(), s[c], nullptr, nullptr, nullptr)) != PA_OK) return e;
    if ((e = size_stage(idx, strands_arena_bound, b.d_cresults[0].get(), b.d_cresults[1].get(), b.n, mbytes, b.d_mscratch, b.d_marena, s[0])) != PA_OK) return e;
    if ((e = pa_strands_merge_device(idx, b.d_cresults[0].get(), b.d_carena[0].get(), b.d_cresults[1].get(), b.d_carena[1].get(), b.n, b.d_mresults.get(), b.d_marena.get(),
                                     b.d_marena.size(), d_counts, b.d_mscratch.get(), mbytes, s[0])) != PA_OK)
        return e;
    uint64_t bst[PA_STRAND_STATS], used = 0, need = 0;
    if ((e = pa_strands_finish(idx, b.d_mscratch.get(), s[0], bst, &used, &need)) != PA_OK) return e;
    for (int j = 0; j < PA_STRAND_STATS; ++j) stats[j] += bst[j];
    st[ST_TALLY] += now() - t0;
    return PA_OK;
}

// The driver of both entry points: Batch's pairs mapped on Batch::STREAMS streams (the gathered bytes are read on the first two) by batch_map, counted into
// one table on s[0] by batch_count. orient: what pa_count_pairs was given (the unstranded stage maps both orientations and does not look at it)
template <class Batch>
int count_table(pa_index* idx, const char* r1_path, const char* r2_path, int orient, uint32_t allowed, int num_threads, uint64_t* h_counts, uint64_t* n_pairs, uint64_t* stats_out) {
    DeviceBuffer<uint64_t> d_counts;   // (in front of the frame: freed behind its streams)
    PairedCall call(num_threads);
    if (!idx || !r1_path || !r2_path || !h_counts) return fail(PA_ERR_INVALID_ARG, "null argument");
    if (orient != PA_PAIR_FR && orient != PA_PAIR_RF && orient != PA_PAIR_FF) return fail(PA_ERR_INVALID_ARG, "orientation %d (PA_PAIR_FR, PA_PAIR_RF or PA_PAIR_FF)", orient);
    int rc = call.open(idx, r1_path, r2_path, 0xFFFFFFFFu, Batch::STREAMS, 2);
    if (rc != PA_OK) return rc;
    const hipStream_t* const s = call.s;
    const uint64_t counts_len = pa_counts_len(idx);
    if ((rc = d_counts.alloc(counts_len)) != PA_OK) return rc;
    PA_HIP_TRY(hipMemsetAsync(d_counts.get(), 0, counts_len * 8, s[0]));
    Batch batches[2];
    uint64_t stats[Batch::STATS] = {0};
    rc = run_batches(*call.rd, batches, [&](Batch& b) { return batch_map(idx, b, orient, allowed, s); },
                     [&](Batch& b) { return batch_count(idx, b, orient, allowed, d_counts.get(), s, stats, call.st); });
    if (rc != PA_OK) return rc;
    PA_HIP_TRY(hipMemcpyAsync(h_counts, d_counts.get(), counts_len * 8, hipMemcpyDeviceToHost, s[0]));
    PA_HIP_TRY(hipStreamSynchronize(s[0]));
    if (n_pairs) *n_pairs = call.rd->pairs;
    if (stats_out) for (int j = 0; j < Batch::STATS; ++j) stats_out[j] = stats[j];
    call.done();
    return PA_OK;
}

}  // namespace

extern "C" int pa_count_pairs(pa_index* idx, const char* r1_path, const char* r2_path, int orient, uint32_t allowed_mismatches, int num_threads, uint64_t* h_counts,
                              uint64_t* n_pairs, uint64_t stats[PA_PAIR_STATS]) {
    return no_throw("pa_count_pairs", [&] { return count_table<PairBatch>(idx, r1_path, r2_path, orient, allowed_mismatches, num_threads, h_counts, n_pairs, stats); });
}

extern "C" int pa_count_pairs_unstranded(pa_index* idx, const char* r1_path, const char* r2_path, uint32_t allowed_mismatches, int num_threads, uint64_t* h_counts,
                                         uint64_t* n_pairs, uint64_t stats[PA_STRAND_STATS]) {
    return no_throw("pa_count_pairs_unstranded", [&] { return count_table<StrandBatch>(idx, r1_path, r2_path, PA_PAIR_FF, allowed_mismatches, num_threads, h_counts, n_pairs, stats); });
}

extern "C" int pa_pairs_input_stats(uint64_t out[2 * PA_INGEST_INPUT_STATS]) {
    if (!out) return fail(PA_ERR_INVALID_ARG, "null argument");
    memcpy(out, last_pairs_input(), sizeof(uint64_t) * 2 * PA_INGEST_INPUT_STATS);
    return PA_OK;
}

extern "C" int pa_pairs_input_path(void) { return (int)last_pairs_input()[2 * PA_INGEST_INPUT_STATS]; }
