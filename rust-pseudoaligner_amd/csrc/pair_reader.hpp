// What the drivers that read PAIRED FASTQ files share (fastq_cells.cpp: R1 is a barcode + UMI prefix that is never mapped; fastq_pairs.cpp: both mates are
// mapped): a batch of pairs as two Mates, the reader that fills it, the two-batch loop (run_batches: batch b is gathered while batch b - 1 is on the GPU), the
// frame of a call (PairedCall) and the sizing of a stage behind the mappings (size_stage).
// The reader has two types. DevicePairReader: the host does not look at the text — each file is a WindowFeed (window_feed.hpp), ids are compared and R2 / the R1
// prefix gathered on the GPU (pair_scan.hip) straight into the buffers that encode, counter and BUS stage read. HostPairReader: the host's WindowScan, ids
// compared and bytes gathered into pinned memory by the pool. open_pair_reader decides which one a call gets.
#pragma once
#include <memory>
#include <optional>

#include "window_feed.hpp"

namespace pa {
namespace ingest {

// One mate of a batch of pairs: its bytes back to back and their offsets, pinned (the host gather writes them) and on the device, and what the
// mapping of that mate needs and leaves.
struct Mate {
    PinnedBuffer<uint8_t> h_bytes;
    PinnedBuffer<uint64_t> h_off;
    DeviceBuffer<uint8_t> d_bytes;
    DeviceBuffer<uint64_t> d_off, d_tiles;
    DeviceBuffer<uint32_t> d_lens, d_arena;
    DeviceBuffer<pa_read_result> d_results;
    uint64_t bytes = 0;
    uint32_t max_len = 0;   // longest gathered piece
    bool on_device = false; // the call's reader gathers on the GPU: d_bytes and d_off hold the batch already (set once per call by run_batches)
    uint32_t wpr() const { return pa_words_per_read(std::max(1u, max_len)); }
    size_t off_size() const { return on_device ? d_off.size() : h_off.size(); }   // pairs the offsets have room for
    // bytes and offsets of the batch's n pairs to the device, asynchronous on s
    int to_device(uint64_t n, hipStream_t s) {
        int e = PA_OK;
        if (on_device) return PA_OK;
        if ((e = d_bytes.reserve(bytes + 64, h_bytes.size())) || (e = d_off.reserve(n + 1, h_off.size()))) return e;
        PA_HIP_TRY(hipMemcpyAsync(d_bytes.get(), h_bytes.get(), bytes, hipMemcpyHostToDevice, s));
        PA_HIP_TRY(hipMemcpyAsync(d_off.get(), h_off.get(), (n + 1) * 8, hipMemcpyHostToDevice, s));
        return PA_OK;
    }
    // ... and packed into tiles there, with room for the mapping's outputs (spare: reads beyond the offsets' size that the per-read buffers are grown
    // to — each driver's own amount)
    int encode(pa_index* idx, uint64_t n, size_t spare, hipStream_t s) {
        const size_t tw = pa_tiles_words(n, wpr()) + 1, reads = off_size() + spare;
        const uint64_t hint = pa_map_arena_hint(idx, n);
        int e = to_device(n, s);
        if (e || (e = d_tiles.reserve(tw, tw)) || (e = d_lens.reserve(n + 64, reads)) || (e = d_results.reserve(n + 64, reads)) || (e = d_arena.reserve(hint, hint)))
            return e;
        return pa_encode_reads_device(idx, d_bytes.get(), d_off.get(), n, wpr(), d_tiles.get(), d_lens.get(), s);
    }
    // the mapping of `tiles` (the mate's own, or their reverse complement), asynchronous on s
    int map(pa_index* idx, const uint64_t* tiles, uint64_t n, uint32_t allowed, hipStream_t s) {
        return pa_map_batch_device(idx, tiles, d_lens.get(), n, wpr(), allowed, d_results.get(), d_arena.get(), d_arena.size(), nullptr, s);
    }
};

struct GpuEvent {   // an event that is created on first use and may be pending
    hipEvent_t e = nullptr;
    bool pending = false;
    GpuEvent() = default;
    GpuEvent(const GpuEvent&) = delete;
    GpuEvent& operator=(const GpuEvent&) = delete;
    ~GpuEvent() { if (e) (void)hipEventDestroy(e); }
    int record(hipStream_t s) {
        if (!e) PA_HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        PA_HIP_TRY(hipEventRecord(e, s));
        return PA_OK;
    }
};

struct MateBatch {   // one batch of pairs: R1 (all of it, or the prefix a barcoded driver asks for) and R2
    Mate mate[2];
    uint64_t n = 0;
    GpuEvent consumed[2];   // device reader: behind the last work of the batch's consumers on their streams (the next gather into these buffers waits for it)
};

// pa_pairs_input_stats / pa_pairs_input_path: of this thread's last paired call — R1's six entries, R2's, the path
uint64_t* last_pairs_input();

// The pair scan and gather: the two files a window of records at a time, record counts and the ids (pair_id_len) compared on the way, whole windows'
// worth of pairs gathered into a batch — all of R2 and the first `prefix` bytes of every R1 (0xFFFFFFFF: all of it) — each piece copied before its
// window is given up. What run_batches needs of either type.
struct PairReader {
    const char *const r1_path, *const r2_path;
    Pool& pool;
    const uint32_t prefix;
    double* const st;              // the call's stage seconds
    const uint64_t batch_pairs;
    const bool on_device;          // what Mate::on_device of the call's batches is
    uint64_t pairs = 0;            // pairs of the batches launched so far (run_batches adds a batch when it launches it)
    bool ended = false;
    PairReader(const char* r1, const char* r2, Pool& pl, uint32_t prefix_, double* st_, uint64_t batch, bool dev)
        : r1_path(r1), r2_path(r2), pool(pl), prefix(prefix_), st(st_), batch_pairs(batch), on_device(dev) {}
    virtual ~PairReader() = default;
    virtual int gather(MateBatch& b) = 0;                   // the next batch into b: R1 (its prefix) into mate[0], R2 into mate[1]
    virtual void consume_on(const hipStream_t*, int) {}     // the streams the batches are consumed on (before the first batch; the host type has no use for them)
    virtual int consumed(MateBatch&) { return PA_OK; }      // the batch's consumers have been given their last work
    virtual void release() = 0;                             // the files are given up (more than once is harmless)
    int no_mate(uint64_t left1, uint64_t at) const {        // one file has ended, the other holds `left` more records
        return fail(PA_ERR_FORMAT, "%s has more records than %s: record %llu has no mate", left1 ? r1_path : r2_path, left1 ? r2_path : r1_path, (unsigned long long)at);
    }
    int ids_differ(uint64_t at) const { return fail(PA_ERR_FORMAT, "record %llu: the ids of %s and %s differ", (unsigned long long)at, r1_path, r2_path); }
};

// Both files opened and the call's reader made: the device type when both are BGZF — or, with PA_PAIRS_DEVICE_PLAIN=1, plain mapped text or BGZF in any
// mix — and PA_PAIRS_HOST_SCAN is not set (PA_INGEST_BGZF=0: no file counts as BGZF). PA_INGEST_BATCH: pairs of a batch, any value >= 1
int open_pair_reader(const char* r1_path, const char* r2_path, Pool& pool, uint32_t prefix, double* st, std::unique_ptr<PairReader>& out);

// The two-batch loop of all drivers: batch b is gathered while batch b - 1 is on the GPU, then b - 1 is finished (and counted), then b is
// launched. launch(batch) and finish(batch) return a pa_status; the reader's files are given up at the end, on every path.
template <class Batch, class Launch, class Finish>
int run_batches(PairReader& rd, Batch (&batches)[2], Launch&& launch, Finish&& finish) {
    int rc = PA_OK, cur = 0;
    bool in_flight = false;
    for (Batch& b : batches) b.mate[0].on_device = b.mate[1].on_device = rd.on_device;
    for (;;) {
        Batch& b = batches[cur];
        b.n = 0;
        rc = rd.ended ? PA_OK : rd.gather(b);   // (while the batch before is on the GPU)
        if (rc != PA_OK) break;
        if (in_flight) {
            if ((rc = finish(batches[cur ^ 1])) != PA_OK || (rc = rd.consumed(batches[cur ^ 1])) != PA_OK) break;
            in_flight = false;
        }
        if (b.n == 0) break;
        const double t0 = now();
        if ((rc = launch(b)) != PA_OK) break;
        rd.st[ST_LAUNCH] += now() - t0;
        rd.pairs += b.n;
        in_flight = true;
        cur ^= 1;
    }
    rd.release();
    return rc;
}

// The frame of a paired call. Its members are declared in the order they are made; a driver declares its two batches BEHIND its PairedCall. Teardown is
// then: run_batches has released the reader on every path (the gather stream synchronised, the input stats stored, the feeds dropped); the batches' buffers
// and events go first, then the IndexStreams (each synchronised), then what is left of the reader, then the pool. What a batch's kernels write into besides
// the batch (a count table, the cell counter, the BUS object) is declared IN FRONT of the frame, so that it goes behind the streams.
struct PairedCall {
    double* const st = last_stage_seconds();
    const double t_call = now();
    const int num_threads;
    std::optional<Pool> pool;   // (made by open(): a call refused for its arguments starts no thread)
    std::unique_ptr<PairReader> rd;
    IndexStream streams[4];
    hipStream_t s[4] = {nullptr, nullptr, nullptr, nullptr};
    explicit PairedCall(int threads) : num_threads(threads) { for (int j = 0; j < PA_INGEST_STAGES; ++j) st[j] = 0.0; }
    // the pool, the reader over both files, n_streams streams with a launch context on idx each; batches are consumed on the first n_consumers of them
    int open(pa_index* idx, const char* r1_path, const char* r2_path, uint32_t prefix, int n_streams, int n_consumers);
    void done() {   // the call has succeeded
        st[ST_CALL] = now() - t_call;
        st[ST_RECORDS] = (double)rd->pairs;
    }
};

// A stage behind the mappings (pair combine, strand merge) is sized before its launch, which cannot be run again (a counted one would count twice): the
// scratch, then `bound_of` (pairs_arena_bound / strands_arena_bound over the records a and b, on s, which it synchronises), then the arena — or the batch is refused
using ArenaBound = int (*)(pa_index*, const pa_read_result*, const pa_read_result*, uint64_t, void*, void*, uint64_t*);
int size_stage(pa_index* idx, ArenaBound bound_of, const pa_read_result* d_a, const pa_read_result* d_b, uint64_t n, size_t scratch_bytes, DeviceBuffer<uint8_t>& scratch,
               DeviceBuffer<uint32_t>& arena, hipStream_t s);

}  // namespace ingest
}  // namespace pa
