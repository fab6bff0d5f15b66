// The stages of the host ingest pipeline that pa_process_reads (fastq_reads.cpp: records inside a FASTQ file) and the record stream
// (record_stream.cpp: records pushed by the caller) share: worker pool, 2-bit packing into pinned tiles, the GPU leg of one
// batch (H2D -> pa_map_batch_device -> D2H, arena regrown on demand) and the rendering of the reference's Debug tuples
// (src/pseudoaligner.rs:455-461, :490). Pure host code around the C ABI's device entry points; header-only, internal.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <mutex>
#include <new>
#include <thread>
#include <vector>

#include "hip_buffer.hpp"
#include "kernels.hpp"
#include "pa_common.hpp"

namespace pa {
namespace ingest {

// persistent worker threads; run(n, fn) executes fn(0..n-1) on them (and on the caller) and returns when all are done
class Pool {
public:
    explicit Pool(int threads) : nthreads_(threads < 1 ? 1 : threads) {
        for (int t = 1; t < nthreads_; ++t) workers_.emplace_back([this] { loop(); });
    }
    ~Pool() {
        { std::lock_guard<std::mutex> g(mu_); stop_ = true; }
        cv_.notify_all();
        for (auto& w : workers_) w.join();
    }
    int size() const { return nthreads_; }
    void run(int ntasks, const std::function<void(int)>& fn) {
        if (ntasks <= 0) return;
        { std::lock_guard<std::mutex> g(mu_); fn_ = &fn; ntasks_ = ntasks; next_ = 0; pending_ = ntasks; ++epoch_; }
        cv_.notify_all();
        work();
        std::unique_lock<std::mutex> g(mu_);
        done_.wait(g, [this] { return pending_ == 0; });
        fn_ = nullptr;
    }

    // the same without the caller: begin() hands the tasks to the workers and returns, end() waits for them (pa_process_reads reads the next window of the
    // text while the caller launches the kernels of the one before). One job at a time: run() / begin() only after end(). Without workers begin() runs the tasks.
    void begin(int ntasks, std::function<void(int)> fn) {
        if (ntasks <= 0) return;
        if (workers_.empty()) { for (int t = 0; t < ntasks; ++t) fn(t); return; }
        { std::lock_guard<std::mutex> g(mu_); async_fn_ = std::move(fn); fn_ = &async_fn_; ntasks_ = ntasks; next_ = 0; pending_ = ntasks; ++epoch_; }
        cv_.notify_all();
    }
    void end() {
        std::unique_lock<std::mutex> g(mu_);
        done_.wait(g, [this] { return pending_ == 0; });
        fn_ = nullptr;
    }

private:
    void work() {
        for (;;) {
            int t;
            const std::function<void(int)>* fn;
            { std::lock_guard<std::mutex> g(mu_); if (!fn_ || next_ >= ntasks_) return; t = next_++; fn = fn_; }
            (*fn)(t);
            { std::lock_guard<std::mutex> g(mu_); if (--pending_ == 0) done_.notify_all(); }
        }
    }
    void loop() {
        uint64_t seen = 0;
        for (;;) {
            { std::unique_lock<std::mutex> g(mu_); cv_.wait(g, [&] { return stop_ || epoch_ != seen; }); if (stop_) return; seen = epoch_; }
            work();
        }
    }
    int nthreads_;
    std::vector<std::thread> workers_;
    std::mutex mu_;
    std::condition_variable cv_, done_;
    const std::function<void(int)>* fn_ = nullptr;
    std::function<void(int)> async_fn_;
    int ntasks_ = 0, next_ = 0, pending_ = 0;
    uint64_t epoch_ = 0;
    bool stop_ = false;
};

// text of one batch: one growable byte buffer per formatting thread, reused from batch to batch (fresh memory would be
// page-faulted in again every time)
struct RawBytes {   // growable bytes that are NOT zero-filled when they grow (a std::vector would write every new byte once before the copy writes it again)
    char* p = nullptr;
    size_t cap = 0;
    RawBytes() = default;
    RawBytes(RawBytes&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    RawBytes& operator=(RawBytes&& o) noexcept { if (this != &o) { free(p); p = o.p; cap = o.cap; o.p = nullptr; o.cap = 0; } return *this; }
    RawBytes(const RawBytes&) = delete;
    RawBytes& operator=(const RawBytes&) = delete;
    ~RawBytes() { free(p); }
    char* data() { return p; }
    const char* data() const { return p; }
    size_t size() const { return cap; }
    void grow(size_t want, size_t keep) {
        char* q = (char*)malloc(want);
        if (!q) throw std::bad_alloc();
        if (keep) memcpy(q, p, keep);
        free(p);
        p = q;
        cap = want;
    }
};
struct TextBuf {
    RawBytes mem;
    size_t len = 0;
    char* room(size_t need) {   // at least `need` more bytes
        if (len + need > mem.size()) mem.grow(std::max(mem.size() * 2, len + need + (1 << 16)), len);
        return mem.data() + len;
    }
};

struct Record {   // one record inside a text (the mapped FASTQ file, or the bytes a caller pushed): offsets into that text
    uint64_t id_off;
    uint32_t id_len, seq_len;
    uint64_t seq_off;
};


struct BatchCtx {   // pinned host buffers + device buffers of one batch in flight
    DeviceBuffer<uint64_t> d_tiles;
    DeviceBuffer<uint32_t> d_lens, d_arena;
    DeviceBuffer<pa_read_result> d_results;
    // (a) record stream: the batch's sequences as the records hold them (ASCII, back to back) and their offsets: the 2-bit packing into
    // tiles runs on the GPU (pa_encode_reads_device), the host only gathers the bytes into pinned memory
    PinnedBuffer<uint8_t> h_ascii;
    PinnedBuffer<uint64_t> h_soff;
    DeviceBuffer<uint8_t> d_ascii;
    DeviceBuffer<uint64_t> d_soff;
    size_t ascii_bytes = 0, soff_cap = 0;
    // ... and the ids (record.id(), :456) for the render kernels (render.hip), which write the batch's output tuples: lengths, offsets
    // (d_off[n] = bytes of the whole text), the text itself, and its copy in pinned memory
    PinnedBuffer<uint8_t> h_ids;
    PinnedBuffer<uint64_t> h_idoff;
    DeviceBuffer<uint8_t> d_ids, d_scan, d_text;
    DeviceBuffer<uint64_t> d_idoff, d_off;
    DeviceBuffer<uint32_t> d_len;
    DeviceBuffer<unsigned long long> d_flag;
    PinnedBuffer<unsigned long long> h_tot;   // {text bytes, flagged reads by bucket [PA_RENDER_FLAG_BUCKETS]}: bucket 0 = the reads before flag_mark, bucket j = the j-th million behind it
    PinnedBuffer<char> h_text;
    size_t ids_bytes = 0, scan_bytes = 0, text_bytes = 0;
    size_t text_guess = 0, spec_bytes = 0;   // the text's expected length (from the batch before) and what was rendered + fetched ahead of knowing it
    uint64_t flagged = 0, flag_mark = 0;
    hipEvent_t ev_text = nullptr;
    size_t reads_cap = 0;
    std::vector<Record> recs;
    uint64_t first = 0, n = 0;
    uint32_t wpr = 1;
    // (b) pa_process_reads: a WINDOW of the FASTQ text as the file holds it — pinned copy, copy in HBM — whose records are found where they
    // lie: by the GPU (fastq_scan.hip: d_chunk / d_first / d_ls scratch, d_rec the records, d_info -> h_info what the host needs to go on) or,
    // for text the GPU scan does not take (the end of the file, wrapped records), by the host's scan (h_rec). Sequences and ids are
    // then read in place: no gather, no second copy
    bool in_place = false;
    PinnedBuffer<uint8_t> h_raw;
    DeviceBuffer<uint8_t> d_raw;
    uint64_t raw_begin = 0, raw_end = 0;   // the window's bytes are [raw_begin, raw_end) of h_raw / d_raw
    DeviceBuffer<uint32_t> d_chunk, d_first, d_ls;
    DeviceBuffer<uint8_t> d_fq_tmp;
    DeviceBuffer<uint4> d_rec;
    DeviceBuffer<FqInfo> d_info;
    size_t chunk_cap = 0, fq_tmp_bytes = 0;
    PinnedBuffer<uint4> h_rec;
    PinnedBuffer<FqInfo> h_info;
    hipEvent_t ev_h2d = nullptr, ev_info = nullptr;
    // (c) a window of a BGZF file: its members' compressed bytes as they lie in the file (pinned copy, copy in HBM), their rows of the member table (in_off
    // counted from the window's first compressed byte) and their statuses; pa::bgzf_inflate_launch writes the text to d_raw + WINDOW_HEAD_ROOM on the copy stream
    PinnedBuffer<uint8_t> h_comp;
    DeviceBuffer<uint8_t> d_comp;
    PinnedBuffer<pa_bgzf_member> h_mrows;
    DeviceBuffer<pa_bgzf_member> d_mrows;
    PinnedBuffer<uint32_t> h_mstat;
    DeviceBuffer<uint32_t> d_mstat;
    uint64_t n_members = 0;   // of the window in the slot (0: not a BGZF window)
    // the tuples' way back on a stream of its own (the lane's; not owned here): the next window's kernels do not queue behind 14 MB of text going to the host
    hipStream_t back = nullptr;
    hipEvent_t ev_render = nullptr;
    bool text_on_back = false;
    // the text buffers' size (d_text is allocated after h_text: it is empty unless both are there)
    size_t text_cap() const { return d_text.size(); }
    void release() {
        for (hipEvent_t e : {ev_text, ev_h2d, ev_info, ev_render})
            if (e) (void)hipEventDestroy(e);
        *this = BatchCtx();
    }
};

// pinned host + device buffers of a batch of n reads of wpr words (grow-only; cap_reads: the size to allocate when growing)
inline int batch_ensure(pa_index* idx, BatchCtx& c, uint64_t n, uint32_t wpr, uint64_t cap_reads) {
    cap_reads = std::max<uint64_t>(n, cap_reads);
    int e = c.d_tiles.reserve(pa_tiles_words(n, wpr) + 1, pa_tiles_words(cap_reads, wpr) + 1);   // (the tiles only exist on the device: pa_encode_reads_device writes them)
    if (e != PA_OK) return e;
    if (n + 64 > c.reads_cap) {
        const size_t cap = cap_reads + 64;
        c.reads_cap = 0;
        c.d_lens.release(); c.d_results.release(); c.d_len.release(); c.d_off.release(); c.d_scan.release();
        c.scan_bytes = render_scan_bytes(cap);
        if ((e = c.d_lens.alloc(cap)) || (e = c.d_results.alloc(cap)) || (e = c.d_len.alloc(cap + 1)) || (e = c.d_off.alloc(cap + 1)) ||
            (e = c.d_scan.alloc(c.scan_bytes ? c.scan_bytes : 16)))
            return e;
        c.reads_cap = cap;
    }
    if (!c.h_tot.get()) {
        if ((e = c.h_tot.alloc(1 + PA_RENDER_FLAG_BUCKETS)) || (e = c.d_flag.alloc(PA_RENDER_FLAG_BUCKETS))) return e;
        PA_HIP_TRY(hipEventCreateWithFlags(&c.ev_text, hipEventDisableTiming | hipEventBlockingSync));
    }
    if (!c.in_place) {   // gathered ids and sequences (record stream)
        if (n + 64 > c.soff_cap) {
            const size_t cap = cap_reads + 64;
            c.soff_cap = 0;
            c.h_soff.release(); c.h_idoff.release(); c.d_soff.release(); c.d_idoff.release();
            if ((e = c.h_soff.alloc(cap + 1)) || (e = c.h_idoff.alloc(cap + 1)) || (e = c.d_soff.alloc(cap + 1)) || (e = c.d_idoff.alloc(cap + 1))) return e;
            c.soff_cap = cap;
        }
        // (h_* then d_*: the device buffer is empty unless both are there)
        if (c.ids_bytes + 64 > c.d_ids.size()) {
            const size_t want = std::max<size_t>(c.ids_bytes + c.ids_bytes / 8 + 4096, (size_t)cap_reads * 16);
            c.d_ids.release();
            if ((e = c.h_ids.alloc(want)) || (e = c.d_ids.alloc(want))) return e;
        }
        if (c.ascii_bytes + 64 > c.d_ascii.size()) {   // (ascii_bytes: set by the caller before this call — the sum of the batch's sequence lengths)
            const size_t want = std::max<size_t>(c.ascii_bytes + c.ascii_bytes / 8 + 4096, (size_t)cap_reads * 32ull * wpr / 2);
            c.d_ascii.release();
            if ((e = c.h_ascii.alloc(want)) || (e = c.d_ascii.alloc(want))) return e;
        }
    }
    const uint64_t hint = pa_map_arena_hint(idx, n);
    return c.d_arena.reserve(hint, hint);
}

// The batch's sequences (at text + rec.seq_off) gathered back to back into pinned memory, with their offsets: what the GPU packs
// (DnaString::from_dna_string, :450 -> pa_encode_reads_device). batch_offsets first (the caller sizes the buffers by ascii_bytes).
inline void batch_offsets(Pool& pool, BatchCtx& c, std::vector<uint64_t>& part) {   // part: [sequence bytes | id bytes] before every task's records
    const int ntask = pool.size() * 4;
    part.assign(2 * ((size_t)ntask + 1), 0);
    uint64_t* ps = part.data();
    uint64_t* pi = part.data() + ntask + 1;
    pool.run(ntask, [&](int t) {
        uint64_t sum = 0, isum = 0;
        for (uint64_t i = c.n * (uint64_t)t / ntask; i < c.n * (uint64_t)(t + 1) / ntask; ++i) { sum += c.recs[i].seq_len; isum += c.recs[i].id_len; }
        ps[(size_t)t + 1] = sum;
        pi[(size_t)t + 1] = isum;
    });
    for (int t = 0; t < ntask; ++t) { ps[(size_t)t + 1] += ps[(size_t)t]; pi[(size_t)t + 1] += pi[(size_t)t]; }
    c.ascii_bytes = ps[(size_t)ntask];
    c.ids_bytes = pi[(size_t)ntask];
}
inline void batch_gather_ascii(Pool& pool, BatchCtx& c, const char* text, const std::vector<uint64_t>& part) {
    const int ntask = pool.size() * 4;
    const uint64_t* ps = part.data();
    const uint64_t* pi = part.data() + ntask + 1;
    pool.run(ntask, [&](int t) {
        uint64_t o = ps[(size_t)t], io = pi[(size_t)t];
        for (uint64_t i = c.n * (uint64_t)t / ntask; i < c.n * (uint64_t)(t + 1) / ntask; ++i) {
            const Record& rec = c.recs[i];
            c.h_soff.get()[i] = o;
            memcpy(c.h_ascii.get() + o, text + rec.seq_off, rec.seq_len);
            o += rec.seq_len;
            c.h_idoff.get()[i] = io;
            memcpy(c.h_ids.get() + io, text + rec.id_off, rec.id_len);
            io += rec.id_len;
        }
    });
    c.h_soff.get()[c.n] = c.ascii_bytes;
    c.h_idoff.get()[c.n] = c.ids_bytes;
}

// the GPU leg of a batch, asynchronous on `stream`: tiles H2D -> index.map_read for every read (:451) -> records D2H
struct RecPos {   // where a record lies in the text and what of it counts: found by the scan (the only stage that looks at every byte), read by the gather stage
    uint64_t start;      // of the '@'
    uint32_t hdr, seq;   // bytes of the header line and of the sequence line (without their line breaks; a CR before the break still counted)
    uint32_t id_len;     // record.id() (:456): header[1..] up to its first space, trailing white space trimmed first (bio 1.5)
    uint32_t seq_len;    // record.seq() (:449): the sequence line without a CR before its line break
};


struct IngestCache {   // the two batches in flight of a pa_process_reads call or a record stream; parked on the index in between (pa_common.hpp)
    BatchCtx ctx[4];   // (a record stream uses the first two; pa_process_reads keeps four windows per lane in flight: read | scan | map + render | write)
    std::vector<RecPos> rec_pos;   // 24 bytes per record of a host-scanned window: kept, or every call would page them in again
    std::vector<std::vector<uint32_t>> brk;   // the host scan's line-break lists (4 bytes per line), kept for the same reason
    hipStream_t copy_stream = nullptr;   // pa_process_reads: the windows' text goes to the GPU on a stream of its own, beside the kernels of the window before
    hipStream_t scan_stream = nullptr;   // ... their records are found on another (a window's scan waits for its text and the scan before, not for the kernels of the window before)
    hipStream_t back_stream = nullptr;   // ... and the tuples go to the host on a third
    // the stream the batches run on travels with the buffers: its launch context inside the index (2 GB of list-mode rows)
    // is then reused by the next call instead of being stranded behind a destroyed stream
    pa_index* idx = nullptr;
    hipStream_t stream = nullptr;
    static void destroy(void* p) {
        IngestCache* c = static_cast<IngestCache*>(p);
        for (BatchCtx& b : c->ctx) b.release();
        for (hipStream_t s : {c->copy_stream, c->scan_stream, c->back_stream})
            if (s) { (void)hipStreamSynchronize(s); (void)hipStreamDestroy(s); }
        if (c->stream) {
            if (c->idx) (void)pa_index_release_stream(c->idx, c->stream);
            (void)hipStreamDestroy(c->stream);
        }
        delete c;
    }
};

// wall seconds of the host stages of this thread's last pa_process_reads call (pa_process_reads_stage_seconds)
inline double* last_stage_seconds() {
    static thread_local double st[PA_INGEST_STAGES] = {0, 0, 0, 0, 0, 0, 0, 0};
    return st;
}

// ---- windows of raw text (pa_process_reads) ----
constexpr uint64_t WINDOW_HEAD_ROOM = 1ull << 20;   // bytes in front of a window's own text for the unfinished last record of the window before

// pinned + device copy of a window of up to `bytes` bytes (grow-only; 64 spare bytes: the scan kernels load whole 16-byte groups)
inline int window_ensure_raw(BatchCtx& c, uint64_t bytes) {
    const size_t want = (size_t)bytes + 64;
    if (want <= c.d_raw.size()) return PA_OK;   // (h_raw then d_raw: d_raw is empty unless both are there)
    c.d_raw.release();
    int e = c.h_raw.alloc(want);
    return e != PA_OK ? e : c.d_raw.alloc(want);
}
// buffers of a BGZF window of `bytes` compressed bytes in `members` members (grow-only; h_* then d_*: the device buffer is empty unless both are there)
inline int window_ensure_comp(BatchCtx& c, uint64_t bytes, uint64_t members) {
    int e = PA_OK;
    if (bytes + 64 > c.d_comp.size()) {
        const size_t want = (size_t)(bytes + bytes / 8 + 4096);
        c.d_comp.release();
        if ((e = c.h_comp.alloc(want)) || (e = c.d_comp.alloc(want))) return e;
    }
    if (members > c.d_mstat.size()) {
        const size_t want = (size_t)(members + members / 4 + 64);
        c.d_mstat.release();
        if ((e = c.h_mrows.alloc(want)) || (e = c.d_mrows.alloc(want)) || (e = c.h_mstat.alloc(want)) || (e = c.d_mstat.alloc(want))) return e;
    }
    return PA_OK;
}
inline int window_ensure_events(BatchCtx& c) {
    if (!c.ev_h2d) PA_HIP_TRY(hipEventCreateWithFlags(&c.ev_h2d, hipEventDisableTiming));
    // (blocking: the thread that waits for a window's scan sleeps — the pool's workers are reading the next window on every CPU of the quota, and a spinning
    // waiter on top of them gets the whole process throttled)
    if (!c.ev_info) PA_HIP_TRY(hipEventCreateWithFlags(&c.ev_info, hipEventDisableTiming | hipEventBlockingSync));
    if (!c.ev_render) PA_HIP_TRY(hipEventCreateWithFlags(&c.ev_render, hipEventDisableTiming));
    if (!c.h_info.get()) {
        int e = c.h_info.alloc(1);
        if (e == PA_OK) e = c.d_info.alloc(1);
        if (e != PA_OK) return e;
    }
    return PA_OK;
}
// records of a window: room for `recs` of them on the device (and in pinned memory when the host fills them in)
inline int window_ensure_recs(BatchCtx& c, uint64_t recs, bool host_side) {
    const size_t want = (size_t)(recs + recs / 8 + 1024);
    int e = c.d_rec.reserve(recs + 1, want);
    if (e == PA_OK && host_side) e = c.h_rec.reserve(recs + 1, want);
    return e;
}
// scratch of the GPU scan of the window [raw_begin, raw_end): chunk counts and prefixes, line starts for `lines` lines (0: a guess from the
// window's size — FASTQ of 150-base reads has a line break per 79 bytes, of 60-base reads per 36)
inline int window_ensure_scan(BatchCtx& c, uint64_t lines) {
    int e = window_ensure_events(c);
    if (e != PA_OK) return e;
    const uint32_t chunks = fq_chunks(c.raw_begin, c.raw_end);
    if ((size_t)chunks + 1 > c.chunk_cap) {
        const size_t want = (size_t)chunks + chunks / 8 + 64;
        c.chunk_cap = 0;
        c.d_chunk.release(); c.d_first.release(); c.d_fq_tmp.release();
        c.fq_tmp_bytes = fq_scan_tmp_bytes((uint32_t)want);
        if ((e = c.d_chunk.alloc(want)) || (e = c.d_first.alloc(want)) || (e = c.d_fq_tmp.alloc(c.fq_tmp_bytes ? c.fq_tmp_bytes : 16))) return e;
        c.chunk_cap = want;
    }
    const uint64_t starts = lines ? lines + 8 : (c.raw_end - c.raw_begin) / 32 + 1024;
    if ((e = c.d_ls.reserve(starts, starts + starts / 8))) return e;
    return window_ensure_recs(c, c.d_ls.size() / 4, false);
}
// the window's records found on the GPU, asynchronous on `stream`: c.h_info is valid once c.ev_info has passed
inline int window_scan_enqueue(BatchCtx& c, bool rescan, hipStream_t stream) {
    const int k = launch_fq_scan(c.d_raw.get(), c.raw_begin, c.raw_end, c.d_chunk.get(), c.d_first.get(), c.d_fq_tmp.get(), c.fq_tmp_bytes, c.d_ls.get(), c.d_ls.size(),
                                 c.d_rec.get(), c.d_rec.size(), c.d_info.get(), rescan, stream);
    if (k) return fail(PA_ERR_HIP, "FASTQ scan: %s", hipGetErrorString((hipError_t)k));
    PA_HIP_TRY(hipMemcpyAsync(c.h_info.get(), c.d_info.get(), sizeof(FqInfo), hipMemcpyDeviceToHost, stream));
    PA_HIP_TRY(hipEventRecord(c.ev_info, stream));
    return PA_OK;
}

// The batch's output tuples (:455-461, :490) rendered where the records, the class table and the novel class ids are (render.hip):
// lengths + scan (d_off[n] = the text's bytes, copied to h_tot with the number of flagged reads), then — when buffers exist — the
// bytes and their copy to pinned memory, c.spec_bytes of them: a guess from the batch before (the host only learns the exact length
// when the batch is finished; a text that turns out longer is rendered again by batch_finish)
inline const uint8_t* batch_id_bytes(const BatchCtx& c) { return c.in_place ? c.d_raw.get() : c.d_ids.get(); }
inline const uint4* batch_rec(const BatchCtx& c) { return c.in_place ? c.d_rec.get() : nullptr; }
inline int batch_render_enqueue(pa_index* idx, BatchCtx& c, hipStream_t stream) {
    const uint64_t* d_cls_off = nullptr;
    const uint8_t* d_cls_txt = nullptr;
    int e = index_device_class_text(idx, &d_cls_off, &d_cls_txt);
    if (e != PA_OK) return e;
    PA_HIP_TRY(hipMemsetAsync(c.d_flag.get(), 0, PA_RENDER_FLAG_BUCKETS * 8, stream));
    int k = launch_render_len(c.d_results.get(), c.d_arena.get(), batch_id_bytes(c), c.d_idoff.get(), batch_rec(c), d_cls_off, d_cls_txt, c.n,
                              c.d_arena.size(), c.flag_mark, c.d_len.get(), c.d_off.get(), c.d_flag.get(), c.d_scan.get(), c.scan_bytes, stream);
    if (k) return fail(PA_ERR_HIP, "render (lengths): %s", hipGetErrorString((hipError_t)k));
    PA_HIP_TRY(hipMemcpyAsync(c.h_tot.get(), c.d_off.get() + c.n, 8, hipMemcpyDeviceToHost, stream));
    PA_HIP_TRY(hipMemcpyAsync(c.h_tot.get() + 1, c.d_flag.get(), PA_RENDER_FLAG_BUCKETS * 8, hipMemcpyDeviceToHost, stream));
    c.spec_bytes = 0;
    if (c.text_cap() && c.text_guess) {
        c.spec_bytes = std::min(c.text_cap(), c.text_guess);
        k = launch_render_write(c.d_results.get(), c.d_arena.get(), batch_id_bytes(c), c.d_idoff.get(), batch_rec(c), d_cls_off, d_cls_txt, c.n,
                                c.d_arena.size(), c.d_off.get(), c.d_text.get(), c.spec_bytes, stream);
        if (k) return fail(PA_ERR_HIP, "render (text): %s", hipGetErrorString((hipError_t)k));
        c.text_on_back = c.back && c.ev_render;
        if (c.text_on_back) {
            PA_HIP_TRY(hipEventRecord(c.ev_render, stream));
            PA_HIP_TRY(hipStreamWaitEvent(c.back, c.ev_render, 0));
        }
        PA_HIP_TRY(hipMemcpyAsync(c.h_text.get(), c.d_text.get(), c.spec_bytes, hipMemcpyDeviceToHost, c.text_on_back ? c.back : stream));
    }
    return PA_OK;
}

inline int batch_launch(pa_index* idx, BatchCtx& c, hipStream_t stream) {
    if (c.in_place) {   // sequences and ids are read where they lie in the window's text (already in HBM, records in d_rec)
        const int k = launch_encode_rec(c.d_raw.get(), c.d_rec.get(), c.n, c.wpr, c.d_tiles.get(), c.d_lens.get(), stream);   // :450
        if (k) return fail(PA_ERR_HIP, "encode launch: %s", hipGetErrorString((hipError_t)k));
    } else {
        PA_HIP_TRY(hipMemcpyAsync(c.d_ascii.get(), c.h_ascii.get(), c.ascii_bytes, hipMemcpyHostToDevice, stream));
        PA_HIP_TRY(hipMemcpyAsync(c.d_soff.get(), c.h_soff.get(), (c.n + 1) * 8, hipMemcpyHostToDevice, stream));
        PA_HIP_TRY(hipMemcpyAsync(c.d_ids.get(), c.h_ids.get(), c.ids_bytes, hipMemcpyHostToDevice, stream));
        PA_HIP_TRY(hipMemcpyAsync(c.d_idoff.get(), c.h_idoff.get(), (c.n + 1) * 8, hipMemcpyHostToDevice, stream));
        const int e0 = pa_encode_reads_device(idx, c.d_ascii.get(), c.d_soff.get(), c.n, c.wpr, c.d_tiles.get(), c.d_lens.get(), stream);   // :450
        if (e0 != PA_OK) return e0;
    }
    const int e = pa_map_batch_device(idx, c.d_tiles.get(), c.d_lens.get(), c.n, c.wpr, PA_DEFAULT_ALLOWED_MISMATCHES,
                                      c.d_results.get(), c.d_arena.get(), c.d_arena.size(), nullptr, stream);
    if (e != PA_OK) return e;
    return batch_render_enqueue(idx, c, stream);   // (the records stay on the device: the render kernels read them there)
}

// waits for the batch; an arena that turned out too small is regrown and the batch mapped (and rendered) again. Afterwards the batch's
// tuples are in c.h_text[0 .. c.text_bytes) — or on their way there (batch_text_wait)
inline int batch_finish(pa_index* idx, BatchCtx& c, hipStream_t stream) {
    uint64_t used = 0;
    int e = map_finish_regrow(idx, stream, c.d_arena, &used, [&] { return batch_launch(idx, c, stream); });
    if (e != PA_OK) return e;
    // (pa_map_finish synchronised the stream: the lengths — and the speculative text, if any — have arrived)
    c.text_bytes = (size_t)c.h_tot.get()[0];
    c.flagged = 0;
    for (uint32_t j = 0; j < PA_RENDER_FLAG_BUCKETS; ++j) c.flagged += c.h_tot.get()[1 + j];
    c.text_guess = c.text_bytes + c.text_bytes / 8 + (64 << 10);
    bool on_back = c.text_on_back && c.spec_bytes != 0;
    if (c.text_bytes > c.spec_bytes) {   // no guess yet (first batches) or a text longer than guessed: size the buffers, write it, fetch it
        if (on_back) { PA_HIP_TRY(hipStreamSynchronize(c.back)); on_back = false; }   // (the copy of the guessed part is not left in flight beside this one)
        if (c.text_bytes + 64 > c.text_cap()) {
            const size_t want = c.text_bytes + c.text_bytes / 4 + (1 << 20);
            c.d_text.release();
            if ((e = c.h_text.alloc(want)) || (e = c.d_text.alloc(want))) return e;
        }
        const uint64_t* d_cls_off = nullptr;
        const uint8_t* d_cls_txt = nullptr;
        if ((e = index_device_class_text(idx, &d_cls_off, &d_cls_txt)) != PA_OK) return e;
        const int k = launch_render_write(c.d_results.get(), c.d_arena.get(), batch_id_bytes(c), c.d_idoff.get(), batch_rec(c), d_cls_off, d_cls_txt, c.n,
                                          c.d_arena.size(), c.d_off.get(), c.d_text.get(), c.text_cap(), stream);
        if (k) return fail(PA_ERR_HIP, "render (text): %s", hipGetErrorString((hipError_t)k));
        if (c.text_bytes) PA_HIP_TRY(hipMemcpyAsync(c.h_text.get(), c.d_text.get(), c.text_bytes, hipMemcpyDeviceToHost, stream));
    }
    PA_HIP_TRY(hipEventRecord(c.ev_text, on_back ? c.back : stream));
    return PA_OK;
}
// the batch's tuples have arrived in c.h_text[0 .. c.text_bytes)
inline int batch_text_wait(BatchCtx& c) {
    PA_HIP_TRY(hipEventSynchronize(c.ev_text));
    return PA_OK;
}

}  // namespace ingest
}  // namespace pa
