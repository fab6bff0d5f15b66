// The drivers that read PAIRED FASTQ files: pa_count_cells (R1 = barcode + UMI, R2 mapped -> the cells x genes UMI matrix) and pa_count_pairs
// (both mates mapped, their classes intersected -> the class-count table; pa_count_pairs_unstranded: both orientations, merged), with the
// barcode whitelist's reader. All walk the two files with
// one PairReader, keep two batches of pairs — each two Mates — and run them through one loop (run_batches): batch b is gathered while batch
// b - 1 is on the GPU. The streams they launch on are IndexStreams, a mapping that ran out of arena goes through map_finish_regrow
// (hip_buffer.hpp).
// PairReader has two forms. In the DEVICE form the host does not look at the text: each file is a WindowFeed (window_feed.hpp: raw or compressed
// windows to HBM, records found by fastq_scan.hip — the window steps of text_window.hpp, which pa_process_reads runs too), and the ids are compared and R2 / the R1 prefix gathered on the GPU (pair_scan.hip), straight into
// the buffers that encode, counter and BUS stage read. It is the default when BOTH files are BGZF (the host form inflates them whole through one zlib
// stream each). With a plain text file on either side it is taken only on request, PA_PAIRS_DEVICE_PLAIN=1: its rate on plain text has not been
// measured against the host form's yet. An ordinary-gzip file on either side, or PA_PAIRS_HOST_SCAN=1, keeps the HOST form for the
// whole call in any case: the host's WindowScan, ids compared and bytes gathered into pinned memory by the pool.
#include <hip/hip_runtime.h>
#include <sys/stat.h>
#include <zlib.h>

#include <algorithm>
#include <atomic>
#include <cerrno>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>
#include <unordered_set>

#include "fastq_text.hpp"
#include "window_feed.hpp"

using namespace pa;
using namespace pa::ingest;

// ---- single-cell counting from files: the barcode whitelist and the paired-FASTQ driver of pa_cell_counter ----

extern "C" int pa_whitelist_load(const char* path, uint32_t bc_len, char* out, uint64_t cap, uint64_t* n) {
    if (!path || !n) return fail(PA_ERR_INVALID_ARG, "null argument");
    if (bc_len < 1 || bc_len > 16) return fail(PA_ERR_INVALID_ARG, "barcode length %u: must be 1..16", bc_len);
    *n = 0;
    gzFile g = gzopen(path, "rb");   // (plain text reads through as it is)
    if (!g) return fail(PA_ERR_IO, "cannot open %s: %s", path, strerror(errno));
    std::vector<char> text;
    {
        char buf[1 << 16];
        for (;;) {
            const int got = gzread(g, buf, sizeof buf);
            if (got < 0) { int e = 0; const char* why = gzerror(g, &e); const int rc = fail(PA_ERR_FORMAT, "%s: corrupt gzip stream: %s", path, why); gzclose(g); return rc; }
            if (got == 0) break;
            text.insert(text.end(), buf, buf + got);
        }
    }
    gzclose(g);
    std::vector<uint32_t> seen;   // packed barcodes (first base most significant) of the lines so far, for the duplicate check
    uint64_t count = 0, line = 0;
    for (size_t p = 0; p < text.size();) {
        const char* nl = (const char*)memchr(text.data() + p, '\n', text.size() - p);
        size_t e = nl ? (size_t)(nl - text.data()) : text.size();
        const size_t next = nl ? e + 1 : text.size();
        if (e > p && text[e - 1] == '\r') --e;
        ++line;
        if (e - p != bc_len) return fail(PA_ERR_FORMAT, "%s: line %llu has %zu bytes, a barcode has %u", path, (unsigned long long)line, e - p, bc_len);
        uint32_t bc = 0;
        for (size_t j = p; j < e; ++j) {
            const char c = text[j];
            const uint32_t b = c == 'A' ? 0u : c == 'C' ? 1u : c == 'G' ? 2u : c == 'T' ? 3u : 4u;
            if (b > 3) return fail(PA_ERR_FORMAT, "%s: line %llu: byte %zu is not A, C, G or T", path, (unsigned long long)line, j - p + 1);
            bc = (bc << 2) | b;
        }
        if (out && count < cap) memcpy(out + count * bc_len, text.data() + p, bc_len);
        seen.push_back(bc);
        ++count;
        p = next;
    }
    std::vector<uint64_t> order(seen.size());
    for (uint64_t i = 0; i < order.size(); ++i) order[i] = i;
    std::sort(order.begin(), order.end(), [&](uint64_t a, uint64_t b) { return seen[a] != seen[b] ? seen[a] < seen[b] : a < b; });
    for (uint64_t i = 1; i < order.size(); ++i)
        if (seen[order[i]] == seen[order[i - 1]])
            return fail(PA_ERR_FORMAT, "%s: line %llu repeats the barcode of line %llu", path, (unsigned long long)order[i] + 1, (unsigned long long)order[i - 1] + 1);
    *n = count;
    if (out && cap < count) return fail(PA_ERR_BUFFER_TOO_SMALL, "%s holds %llu barcodes, room for %llu", path, (unsigned long long)count, (unsigned long long)cap);
    return PA_OK;
}

namespace {

// one FASTQ file of the pair, a window of records at a time (host memory follows the window, not the file; gzip is inflated whole)
struct PairCursor {
    const char* path = nullptr;
    FastqText text;
    std::unique_ptr<WindowScan> ws;
    std::vector<RecPos> rec;
    std::vector<std::vector<uint32_t>> brk;
    uint64_t at = 0, before = 0;   // next record of the window, records of the windows before it
    void adopt(const char* p, FastqText&& opened) {   // a text that open_fastq has opened
        path = p;
        text = std::move(opened);
        opened = FastqText();
        ws.reset(new WindowScan(text));
    }
    // records left in the window (0: the file has ended); the window before is given up
    int ready(Pool& pool, uint64_t& left) {
        if (at >= ws->nrec) {
            before += ws->nrec;
            at = 0;
            const int rc = ws->next(path, before, pool, rec, brk);
            if (rc != PA_OK) return rc;
        }
        left = ws->nrec - at;
        return PA_OK;
    }
    const char* id(uint64_t i, uint32_t& len) const {   // record.id() with a trailing "/1" or "/2" cut
        const RecPos& r = rec[i];
        const char* s = ws->base + r.start + 1;
        len = r.id_len;
        if (len >= 2 && s[len - 2] == '/' && (s[len - 1] == '1' || s[len - 1] == '2')) len -= 2;
        return s;
    }
    const char* seq(uint64_t i) const { return ws->base + rec[i].start + rec[i].hdr + 1; }
};

// grow a pinned buffer to `want` elements, keeping the first `keep`
template <class T>
int grow_pinned(PinnedBuffer<T>& b, size_t want, size_t keep) {
    if (want <= b.size()) return PA_OK;
    PinnedBuffer<T> nb;
    const int e = nb.alloc(std::max(want, b.size() + b.size() / 2));
    if (e != PA_OK) return e;
    if (keep) memcpy(nb.get(), b.get(), keep * sizeof(T));
    b = std::move(nb);
    return PA_OK;
}

double secs_since(std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); }

// One mate of a batch of pairs: its bytes back to back and their offsets, pinned (the gather writes them) and on the device, and what the
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
    bool on_device = false; // the gather ran on the GPU: d_bytes and d_off hold the batch already
    uint32_t wpr() const { return pa_words_per_read(std::max(1u, max_len)); }
    // bytes and offsets of the batch's n pairs to the device, asynchronous on s
    int to_device(uint64_t n, hipStream_t s) {
        int e = PA_OK;
        if (on_device) return PA_OK;
        if ((e = d_bytes.reserve(bytes + 64, h_bytes.size())) || (e = d_off.reserve(n + 1, h_off.size()))) return e;
        PA_HIP_TRY(hipMemcpyAsync(d_bytes.get(), h_bytes.get(), bytes, hipMemcpyHostToDevice, s));
        PA_HIP_TRY(hipMemcpyAsync(d_off.get(), h_off.get(), (n + 1) * 8, hipMemcpyHostToDevice, s));
        return PA_OK;
    }
    // ... and packed into tiles there, with room for the mapping's outputs (spare: reads beyond the pinned offsets' size that the per-read
    // buffers are grown to — each driver's own amount)
    int encode(pa_index* idx, uint64_t n, size_t spare, hipStream_t s) {
        const size_t tw = pa_tiles_words(n, wpr()) + 1, reads = (on_device ? d_off.size() : h_off.size()) + spare;
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
};

struct CellBatch {   // one batch of pairs: R1 (pa_count_cells: its barcode + UMI prefix, which is never encoded or mapped) and R2
    Mate mate[2];
    uint64_t n = 0;
    GpuEvent consumed[2];   // device form: behind the last work of the batch's consumers on their streams (the next gather into these buffers waits for it)
};

uint64_t* last_pairs_input() {   // pa_pairs_input_stats / pa_pairs_input_path: of this thread's last paired call — R1's six entries, R2's, the path
    static thread_local uint64_t st[2 * PA_INGEST_INPUT_STATS + 1] = {0};
    return st;
}

// `want` bytes in b, the first `keep` of them kept (copied on s, which is waited for)
int grow_device_keep(DeviceBuffer<uint8_t>& b, size_t want, size_t keep, hipStream_t s) {
    if (want <= b.size()) return PA_OK;
    DeviceBuffer<uint8_t> nb;
    const int e = nb.alloc(std::max(want, b.size() + b.size() / 2));
    if (e != PA_OK) return e;
    if (keep) {
        PA_HIP_TRY(hipMemcpyAsync(nb.get(), b.get(), keep, hipMemcpyDeviceToDevice, s));
        PA_HIP_TRY(hipStreamSynchronize(s));
    }
    b = std::move(nb);
    return PA_OK;
}

// The pair scan and gather shared by pa_count_cells and pa_count_pairs: the two files a window of records at a time, record counts and
// record.id() (after a trailing "/1" or "/2" is cut) compared on the way, whole windows' worth of pairs gathered into a batch — all of
// R2 and the first `prefix` bytes of every R1 (0xFFFFFFFF: all of it) — each piece copied before its window is given up.
struct PairReader {
    const char *r1_path, *r2_path;
    Pool& pool;
    const uint32_t prefix;
    double* st;                    // stage seconds: [0] scan, [1] gather, [3] launch (run_batches)
    PairCursor f1, f2;
    uint64_t batch_pairs = DEFAULT_BATCH_READS;
    int ntask;
    std::vector<uint64_t> part, part1;
    std::vector<uint32_t> part_max, part_max1;
    uint64_t pairs = 0;            // pairs of the batches launched so far (run_batches adds a batch when it launches it)
    bool ended = false;
    // the device form: the two files as window feeds, one stream for match + gather, the batch's control block
    bool device = false;
    FastqText text[2];
    std::unique_ptr<WindowFeed> feed[2];
    FeedWindow win[2];
    uint64_t at[2] = {0, 0};       // next record of each file's window
    hipStream_t gs = nullptr;
    std::vector<hipStream_t> consumers;   // the streams the batches are consumed on (set by the driver before the first batch)
    DeviceBuffer<uint64_t> d_ctl;
    PinnedBuffer<uint64_t> h_ctl;
    DeviceBuffer<uint8_t> d_scratch;
    PairReader(const char* r1, const char* r2, Pool& pl, uint32_t prefix_, double* st_)
        : r1_path(r1), r2_path(r2), pool(pl), prefix(prefix_), st(st_), ntask(pl.size() * 4), part((size_t)ntask + 1), part1((size_t)ntask + 1), part_max((size_t)ntask),
          part_max1((size_t)ntask) {
        if (const char* v = getenv("PA_INGEST_BATCH")) { const long long x = atoll(v); if (x >= 1) batch_pairs = (uint64_t)x; }
    }
    ~PairReader() { release(); }
    // Both files are opened; the device form is taken when both are BGZF — or, with PA_PAIRS_DEVICE_PLAIN=1, plain mapped text or BGZF in any mix — and
    // PA_PAIRS_HOST_SCAN is not set
    int open() {
        const char* v = getenv("PA_PAIRS_HOST_SCAN");
        const bool host_only = v && *v && atoi(v) != 0;
        v = getenv("PA_INGEST_BGZF");
        const bool bgzf = !host_only && !(v && *v && atoi(v) == 0);
        v = getenv("PA_PAIRS_DEVICE_PLAIN");
        const bool plain_too = v && *v && atoi(v) != 0;
        const char* const paths[2] = {r1_path, r2_path};
        int rc = PA_OK;
        bool takes = !host_only;
        for (int i = 0; i < 2; ++i) {
            if (bgzf) open_bgzf(paths[i], text[i]);
            if (!text[i].bgzf && (rc = open_fastq(paths[i], text[i])) != PA_OK) return rc;
            takes = takes && WindowFeed::takes(text[i]) && (text[i].bgzf || plain_too);
        }
        uint64_t* const is = last_pairs_input();
        memset(is, 0, sizeof(uint64_t) * (2 * PA_INGEST_INPUT_STATS + 1));
        if (!takes) {   // today's host form for the whole call (a BGZF file is then inflated like any other .gz)
            for (int i = 0; i < 2; ++i)
                if (text[i].bgzf) { text[i].release(); text[i] = FastqText(); if ((rc = open_fastq(paths[i], text[i])) != PA_OK) return rc; }
            for (int i = 0; i < 2; ++i) is[i * PA_INGEST_INPUT_STATS] = text[i].inflated.empty() ? 0u : 1u;
            f1.adopt(r1_path, std::move(text[0]));
            f2.adopt(r2_path, std::move(text[1]));
            return PA_OK;
        }
        device = true;
        const uint64_t window = window_from_env(batch_pairs);   // (PA_INGEST_BATCH as the paired drivers read it: any value >= 1)
        PA_HIP_TRY(hipStreamCreateWithFlags(&gs, hipStreamNonBlocking));
        if ((rc = d_ctl.alloc(PA_PAIRS_CTL_WORDS)) != PA_OK || (rc = h_ctl.alloc(PA_PAIRS_CTL_WORDS)) != PA_OK) return rc;
        for (int i = 0; i < 2; ++i) {
            feed[i].reset(new WindowFeed(paths[i], text[i], pool, st, window, batch_pairs));
            if ((rc = feed[i]->start()) != PA_OK) return rc;
        }
        return PA_OK;
    }
    void release() {
        if (device) {
            if (gs) (void)hipStreamSynchronize(gs);
            uint64_t* const is = last_pairs_input();
            for (int i = 0; i < 2; ++i) {
                if (!feed[i]) continue;
                const InputStats fs = feed[i]->stats();
                memcpy(is + i * PA_INGEST_INPUT_STATS, &fs, sizeof fs);
                feed[i].reset();
            }
            is[2 * PA_INGEST_INPUT_STATS] = 1;
            if (gs) { (void)hipStreamDestroy(gs); gs = nullptr; }
            device = false;
        }
        for (int i = 0; i < 2; ++i) { text[i].release(); text[i] = FastqText(); }
        f1.text.release(); f2.text.release();
    }
    // the batch's consumers have been given their last work: the next gather into the batch's buffers waits for it (device form)
    int consumed(CellBatch& b) {
        if (!device) return PA_OK;
        for (size_t i = 0; i < consumers.size() && i < 2; ++i) {
            GpuEvent& ev = b.consumed[i];
            if (!ev.e) PA_HIP_TRY(hipEventCreateWithFlags(&ev.e, hipEventDisableTiming));
            PA_HIP_TRY(hipEventRecord(ev.e, consumers[i]));
            ev.pending = true;
        }
        return PA_OK;
    }
    // the batch's control block, once, behind its gathers: the first bad id, the longest pieces, the bytes
    int close_device_batch(CellBatch& b) {
        Mate &m1 = b.mate[0], &m2 = b.mate[1];
        if (b.n == 0) return PA_OK;
        const auto t0 = std::chrono::steady_clock::now();
        PA_HIP_TRY(hipMemcpyAsync(h_ctl.get(), d_ctl.get(), PA_PAIRS_CTL_WORDS * 8, hipMemcpyDeviceToHost, gs));
        PA_HIP_TRY(hipStreamSynchronize(gs));
        st[2] += secs_since(t0);
        const uint64_t* const c = h_ctl.get();
        if (c[5] != ~0ull) return fail(PA_ERR_INTERNAL, "pair scan: the record of pair %llu lies outside its window", (unsigned long long)(pairs + c[5]));
        if (c[0] != ~0ull) return fail(PA_ERR_FORMAT, "record %llu: the ids of %s and %s differ", (unsigned long long)(pairs + c[0]), r1_path, r2_path);
        if (c[3] > m1.d_bytes.size() || c[4] > m2.d_bytes.size()) return fail(PA_ERR_INTERNAL, "pair scan: a batch of %llu + %llu bytes did not fit its buffers", (unsigned long long)c[3], (unsigned long long)c[4]);
        m1.max_len = (uint32_t)c[1];
        m2.max_len = (uint32_t)c[2];
        m1.bytes = c[3];
        m2.bytes = c[4];
        return PA_OK;
    }
    // the device form of gather(): segments of m = min(records left in R1's window, in R2's window, room in the batch) pairs, matched and gathered on gs
    int gather_device(CellBatch& b) {
        Mate &m1 = b.mate[0], &m2 = b.mate[1];
        b.n = 0; m2.bytes = 0; m1.bytes = 0; m2.max_len = 0; m1.max_len = 0;
        m1.on_device = m2.on_device = true;
        int e = PA_OK;
        const size_t offs = (size_t)batch_pairs + 128;   // (the per-read buffers of the mapping are sized from it: a full batch + 64 fits)
        if ((e = m1.d_off.reserve(offs, offs)) || (e = m2.d_off.reserve(offs, offs))) return e;
        for (GpuEvent& ev : b.consumed)
            if (ev.pending) { PA_HIP_TRY(hipStreamWaitEvent(gs, ev.e, 0)); ev.pending = false; }
        uint64_t ub1 = 0, ub2 = 0;   // bounds of the bytes gathered so far: pairs x the longest sequence of their windows
        while (b.n < batch_pairs) {
            for (int i = 0; i < 2; ++i) {
                if (at[i] < win[i].n) continue;
                if (win[i].slot >= 0 && (e = feed[i]->release(win[i].slot, gs)) != PA_OK) return e;
                if ((e = feed[i]->next(win[i])) != PA_OK) {   // (an id that differs in the pairs gathered so far is the earlier error, as on the host path)
                    const std::string why = last_error_ref();
                    const int earlier = close_device_batch(b);
                    if (earlier != PA_OK) return earlier;
                    last_error_ref() = why;
                    return e;
                }
                at[i] = 0;
            }
            const uint64_t left1 = win[0].n - at[0], left2 = win[1].n - at[1];
            if (left1 == 0 || left2 == 0) {
                if ((e = close_device_batch(b)) != PA_OK) return e;   // (an id that differs in front of the missing mate is the earlier error)
                if (left1 != left2)
                    return fail(PA_ERR_FORMAT, "%s has more records than %s: record %llu has no mate", left1 ? r1_path : r2_path, left1 ? r2_path : r1_path,
                                (unsigned long long)(pairs + b.n));
                ended = true;
                return PA_OK;
            }
            const auto t0 = std::chrono::steady_clock::now();
            const uint64_t m = segment_pairs(left1, left2, batch_pairs, b.n);
            const uint64_t nb1 = ub1 + m * std::min<uint64_t>(win[0].max_seq, prefix), nb2 = ub2 + m * (uint64_t)win[1].max_seq;
            if ((e = grow_device_keep(m1.d_bytes, nb1 + 64, ub1, gs)) != PA_OK || (e = grow_device_keep(m2.d_bytes, nb2 + 64, ub2, gs)) != PA_OK) return e;
            const size_t sb = pa_pairs_gather_scratch_bytes(m);
            if ((e = d_scratch.reserve(sb, sb + sb / 4)) != PA_OK) return e;
            PA_HIP_TRY(hipStreamWaitEvent(gs, win[0].ready, 0));
            PA_HIP_TRY(hipStreamWaitEvent(gs, win[1].ready, 0));
            if ((e = pairs_gather_launch(win[0].d_raw, win[0].raw_bytes, reinterpret_cast<const uint32_t*>(win[0].d_rec + at[0]), win[1].d_raw, win[1].raw_bytes,
                                         reinterpret_cast<const uint32_t*>(win[1].d_rec + at[1]), m, prefix, b.n, m1.d_bytes.get(), m1.d_bytes.size(), m1.d_off.get(),
                                         m2.d_bytes.get(), m2.d_bytes.size(), m2.d_off.get(), d_ctl.get(), d_scratch.get(), d_scratch.size(), gs)) != PA_OK)
                return e;
            ub1 = nb1; ub2 = nb2;
            b.n += m;
            at[0] += m;
            at[1] += m;
            st[3] += secs_since(t0);
        }
        return close_device_batch(b);
    }
    // gather the next batch into b: R1 (its prefix) into mate[0], R2 into mate[1]
    int gather(CellBatch& b) {
        if (device) return gather_device(b);
        Mate &m1 = b.mate[0], &m2 = b.mate[1];
        b.n = 0; m2.bytes = 0; m1.bytes = 0; m2.max_len = 0; m1.max_len = 0;
        int e = PA_OK;
        if ((e = grow_pinned(m2.h_off, batch_pairs + 1, 0)) || (e = grow_pinned(m1.h_off, batch_pairs + 1, 0))) return e;
        if (prefix != 0xFFFFFFFFu && (e = grow_pinned(m1.h_bytes, (size_t)batch_pairs * prefix + 64, 0))) return e;
        while (b.n < batch_pairs) {
            uint64_t left1 = 0, left2 = 0;
            auto t0 = std::chrono::steady_clock::now();
            if ((e = f1.ready(pool, left1)) != PA_OK || (e = f2.ready(pool, left2)) != PA_OK) return e;
            st[0] += secs_since(t0);
            if (left1 == 0 || left2 == 0) {
                if (left1 != left2)
                    return fail(PA_ERR_FORMAT, "%s has more records than %s: record %llu has no mate", left1 ? r1_path : r2_path, left1 ? r2_path : r1_path,
                                (unsigned long long)(pairs + b.n));
                ended = true;
                break;
            }
            t0 = std::chrono::steady_clock::now();
            const uint64_t m = std::min(std::min(left1, left2), batch_pairs - b.n);
            const uint64_t a1 = f1.at, a2 = f2.at, base = b.n;
            std::atomic<uint64_t> bad{~0ull};
            pool.run(ntask, [&](int t) {   // R2 and R1-prefix bytes per task, ids compared on the way
                uint64_t sum2 = 0, sum1 = 0;
                uint32_t mx = 0, mx1 = 0;
                for (uint64_t i = m * (uint64_t)t / ntask; i < m * (uint64_t)(t + 1) / ntask; ++i) {
                    uint32_t l1, l2;
                    const char* id1 = f1.id(a1 + i, l1);
                    const char* id2 = f2.id(a2 + i, l2);
                    if (l1 != l2 || memcmp(id1, id2, l1) != 0) {
                        uint64_t first = bad.load();
                        while (i < first && !bad.compare_exchange_weak(first, i)) {}
                    }
                    const uint32_t len = f2.rec[a2 + i].seq_len, len1 = std::min(f1.rec[a1 + i].seq_len, prefix);
                    sum2 += len;
                    sum1 += len1;
                    mx = std::max(mx, len);
                    mx1 = std::max(mx1, len1);
                }
                part[(size_t)t + 1] = sum2;
                part1[(size_t)t + 1] = sum1;
                part_max[(size_t)t] = mx;
                part_max1[(size_t)t] = mx1;
            });
            if (bad.load() != ~0ull)
                return fail(PA_ERR_FORMAT, "record %llu: the ids of %s and %s differ", (unsigned long long)(pairs + base + bad.load()), r1_path, r2_path);
            part[0] = m2.bytes;
            part1[0] = m1.bytes;
            for (int t = 0; t < ntask; ++t) {
                part[(size_t)t + 1] += part[(size_t)t];
                part1[(size_t)t + 1] += part1[(size_t)t];
                m2.max_len = std::max(m2.max_len, part_max[(size_t)t]);
                m1.max_len = std::max(m1.max_len, part_max1[(size_t)t]);
            }
            if ((e = grow_pinned(m2.h_bytes, part[(size_t)ntask] + 64, m2.bytes)) != PA_OK) return e;
            if ((e = grow_pinned(m1.h_bytes, part1[(size_t)ntask] + 64, m1.bytes)) != PA_OK) return e;   // (a bounded prefix: sized above, nothing to do)
            pool.run(ntask, [&](int t) {   // all of R2, the first `prefix` bytes of R1
                uint64_t o2 = part[(size_t)t], o1 = part1[(size_t)t];
                for (uint64_t i = m * (uint64_t)t / ntask; i < m * (uint64_t)(t + 1) / ntask; ++i) {
                    const uint32_t len2 = f2.rec[a2 + i].seq_len;
                    m2.h_off.get()[base + i] = o2;
                    memcpy(m2.h_bytes.get() + o2, f2.seq(a2 + i), len2);
                    o2 += len2;
                    const uint32_t len1 = std::min(f1.rec[a1 + i].seq_len, prefix);
                    m1.h_off.get()[base + i] = o1;
                    memcpy(m1.h_bytes.get() + o1, f1.seq(a1 + i), len1);
                    o1 += len1;
                }
            });
            m1.bytes = part1[(size_t)ntask];
            m2.bytes = part[(size_t)ntask];
            b.n += m;
            f1.at += m;
            f2.at += m;
            st[1] += secs_since(t0);
        }
        m2.h_off.get()[b.n] = m2.bytes;
        m1.h_off.get()[b.n] = m1.bytes;
        return PA_OK;
    }
};

// The two-batch loop of both drivers: batch b is gathered while batch b - 1 is on the GPU, then b - 1 is finished (and counted), then b is
// launched. launch(batch) and finish(batch) return a pa_status; the reader's files are given up at the end.
template <class Batch, class Launch, class Finish>
int run_batches(PairReader& rd, Batch (&batches)[2], Launch&& launch, Finish&& finish) {
    int rc = PA_OK, cur = 0;
    bool in_flight = false;
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
        const auto t0 = std::chrono::steady_clock::now();
        if ((rc = launch(b)) != PA_OK) break;
        rd.st[3] += secs_since(t0);
        rd.pairs += b.n;
        in_flight = true;
        cur ^= 1;
    }
    rd.release();
    return rc;
}

// the batch's GPU leg up to the mapping: copies, encode, map (asynchronous on s)
int cell_batch_map(pa_index* idx, CellBatch& b, hipStream_t s) {
    Mate& r2 = b.mate[1];
    int e = PA_OK;
    if ((e = r2.encode(idx, b.n, 0, s)) != PA_OK || (e = b.mate[0].to_device(b.n, s)) != PA_OK) return e;
    return r2.map(idx, r2.d_tiles.get(), b.n, PA_DEFAULT_ALLOWED_MISMATCHES, s);
}

// waits for the mapping (regrowing the arena as pa_map_finish asks), then counts the batch
int cell_batch_count(pa_index* idx, pa_cell_counter* counter, CellBatch& b, hipStream_t s, double* st) {
    auto t0 = std::chrono::steady_clock::now();
    Mate &r1 = b.mate[0], &r2 = b.mate[1];
    uint64_t used = 0;
    int e = map_finish_regrow(idx, s, r2.d_arena, &used, [&] { return r2.map(idx, r2.d_tiles.get(), b.n, PA_DEFAULT_ALLOWED_MISMATCHES, s); });
    st[2] += secs_since(t0);
    if (e != PA_OK) return e;
    t0 = std::chrono::steady_clock::now();
    e = pa_cell_counter_add_device(counter, r2.d_results.get(), r2.d_arena.get(), r1.d_bytes.get(), r1.d_off.get(), b.n, s);
    st[4] += secs_since(t0);
    return e;
}

int write_text(const std::string& path, const std::string& text) {
    FILE* f = fopen(path.c_str(), "wb");
    if (!f) return fail(PA_ERR_IO, "cannot create %s: %s", path.c_str(), strerror(errno));
    const bool ok = fwrite(text.data(), 1, text.size(), f) == text.size();
    if (fclose(f) != 0 || !ok) return fail(PA_ERR_IO, "cannot write %s", path.c_str());
    return PA_OK;
}

int count_cells_impl(pa_index* idx, const pa_host_index* h, const char* r1_path, const char* r2_path, const char* whitelist_path, uint32_t bc_len,
                     uint32_t umi_len, const char* out_dir, int num_threads, uint64_t* stats) {
    const auto t_call = std::chrono::steady_clock::now();
    double* st = last_stage_seconds();
    for (int j = 0; j < PA_INGEST_STAGES; ++j) st[j] = 0.0;
    if (!idx || !h || !r1_path || !r2_path || !whitelist_path || !out_dir) return fail(PA_ERR_INVALID_ARG, "null argument");
    if (bc_len < 1 || bc_len > 16 || umi_len < 1 || umi_len > 16) return fail(PA_ERR_INVALID_ARG, "barcode length %u / UMI length %u: both must be 1..16", bc_len, umi_len);
    struct stat sd;
    if (stat(out_dir, &sd) != 0 || !S_ISDIR(sd.st_mode)) return fail(PA_ERR_IO, "%s is no directory", out_dir);
    uint64_t n_wl = 0;
    int rc = pa_whitelist_load(whitelist_path, bc_len, nullptr, 0, &n_wl);
    if (rc != PA_OK) return rc;
    std::vector<char> wl((size_t)n_wl * bc_len + 1);
    if ((rc = pa_whitelist_load(whitelist_path, bc_len, wl.data(), n_wl, &n_wl)) != PA_OK) return rc;
    const uint32_t ntx = pa_host_index_num_transcripts(h);
    std::vector<uint32_t> tx_gene(ntx ? ntx : 1);
    uint32_t num_genes = 0;
    if ((rc = pa_host_index_genes(h, tx_gene.data(), &num_genes)) != PA_OK) return rc;
    pa_cell_counter* counter = nullptr;
    if ((rc = pa_cell_counter_create(idx, h, tx_gene.data(), num_genes, wl.data(), n_wl, bc_len, umi_len, &counter)) != PA_OK) return rc;
    std::unique_ptr<pa_cell_counter, void (*)(pa_cell_counter*)> own(counter, pa_cell_counter_destroy);
    const uint32_t prefix = bc_len + umi_len;

    Pool pool(num_threads < 1 ? usable_threads() : num_threads);
    PairReader rd(r1_path, r2_path, pool, prefix, st);
    if ((rc = rd.open()) != PA_OK) return rc;
    IndexStream stream;
    if ((rc = stream.create(idx)) != PA_OK) return rc;
    hipStream_t s = stream.get();
    rd.consumers = {s};
    CellBatch batches[2];
    rc = run_batches(rd, batches, [&](CellBatch& b) { return cell_batch_map(idx, b, s); }, [&](CellBatch& b) { return cell_batch_count(idx, counter, b, s, st); });
    if (rc != PA_OK) return rc;
    auto t0 = std::chrono::steady_clock::now();
    uint64_t entries = 0;
    if ((rc = pa_cell_counter_finish(counter, &entries)) != PA_OK) return rc;
    st[4] += secs_since(t0);
    t0 = std::chrono::steady_clock::now();
    std::vector<uint32_t> cell(entries), gene(entries), umis(entries);
    if ((rc = pa_cell_counter_matrix(counter, cell.data(), gene.data(), umis.data(), entries)) != PA_OK) return rc;
    // columns: the cells with at least one UMI, in whitelist order (the matrix is sorted by cell)
    std::string bc_text, mtx;
    std::vector<uint32_t> column(entries);
    uint32_t cols = 0;
    for (uint64_t i = 0; i < entries; ++i) {
        if (i == 0 || cell[i] != cell[i - 1]) {
            bc_text.append(wl.data() + (size_t)cell[i] * bc_len, bc_len);
            bc_text.push_back('\n');
            ++cols;
        }
        column[i] = cols;
    }
    char head[96];
    snprintf(head, sizeof head, "%%%%MatrixMarket matrix coordinate integer general\n%u %u %llu\n", num_genes, cols, (unsigned long long)entries);
    // "gene cell umis" lines, rendered in pieces on the pool (a matrix has millions of entries; one formatted print per line cost
    // most of the call)
    auto put_u32 = [](char* p, uint32_t v) {   // decimal digits of v at p; returns the end
        char tmp[10];
        int n = 0;
        do { tmp[n++] = (char)('0' + v % 10); v /= 10; } while (v);
        while (n) *p++ = tmp[--n];
        return p;
    };
    const int pieces = std::max(1, std::min<int>(pool.size() * 4, (int)(entries / 4096) + 1));
    std::vector<std::string> piece((size_t)pieces);
    pool.run(pieces, [&](int t) {
        const uint64_t a = entries * (uint64_t)t / pieces, b = entries * (uint64_t)(t + 1) / pieces;
        std::string& o = piece[(size_t)t];
        o.resize((size_t)(b - a) * 33);
        char* p = &o[0];
        for (uint64_t i = a; i < b; ++i) {
            p = put_u32(p, gene[i] + 1); *p++ = ' ';
            p = put_u32(p, column[i]); *p++ = ' ';
            p = put_u32(p, umis[i]); *p++ = '\n';
        }
        o.resize((size_t)(p - o.data()));
    });
    mtx = head;
    size_t mtx_len = mtx.size();
    for (const std::string& x : piece) mtx_len += x.size();
    mtx.reserve(mtx_len);
    for (const std::string& x : piece) mtx += x;
    // gene names numbered as pa_host_index_genes numbers them (first appearance in transcript order), built once: the name lookup
    // of the C ABI rebuilds that table on every call
    std::string features;
    {
        std::unordered_set<std::string> seen;
        for (const std::string& g : h->h.tx_genes) {
            if (!seen.insert(g).second) continue;
            features += g;
            features += '\t';
            features += g;
            features += "\tGene Expression\n";
        }
        if (seen.size() != num_genes) return fail(PA_ERR_INTERNAL, "%zu gene names for %u genes", seen.size(), num_genes);
    }
    const std::string dir(out_dir);
    if ((rc = write_text(dir + "/matrix.mtx", mtx)) != PA_OK || (rc = write_text(dir + "/barcodes.tsv", bc_text)) != PA_OK ||
        (rc = write_text(dir + "/features.tsv", features)) != PA_OK)
        return rc;
    st[5] = secs_since(t0);
    if (stats) (void)pa_cell_counter_stats(counter, stats);
    st[6] = secs_since(t_call);
    st[7] = (double)rd.pairs;
    return PA_OK;
}

// ---- pa_write_bus: the same two files -> sorted (barcode, UMI, ec) records, output.bus + matrix.ec + transcripts.txt ----

// waits for the mapping (regrowing the arena as pa_map_finish asks), then adds the batch's records
int bus_batch_add(pa_index* idx, pa_bus* bus, CellBatch& b, hipStream_t s, double* st) {
    auto t0 = std::chrono::steady_clock::now();
    Mate &r1 = b.mate[0], &r2 = b.mate[1];
    uint64_t used = 0;
    int e = map_finish_regrow(idx, s, r2.d_arena, &used, [&] { return r2.map(idx, r2.d_tiles.get(), b.n, PA_DEFAULT_ALLOWED_MISMATCHES, s); });
    st[2] += secs_since(t0);
    if (e != PA_OK) return e;
    t0 = std::chrono::steady_clock::now();
    e = pa_bus_add_device(bus, r2.d_results.get(), r2.d_arena.get(), r2.d_arena.size(), r1.d_bytes.get(), r1.d_off.get(), b.n, s);
    st[4] += secs_since(t0);
    return e;
}

int write_bus_impl(pa_index* idx, const pa_host_index* h, const char* r1_path, const char* r2_path, uint32_t bc_len, uint32_t umi_len, const char* out_dir,
                   int num_threads, uint64_t* stats) {
    const auto t_call = std::chrono::steady_clock::now();
    double* st = last_stage_seconds();
    for (int j = 0; j < PA_INGEST_STAGES; ++j) st[j] = 0.0;
    if (!idx || !h || !r1_path || !r2_path || !out_dir) return fail(PA_ERR_INVALID_ARG, "null argument");
    struct stat sd;
    if (stat(out_dir, &sd) != 0 || !S_ISDIR(sd.st_mode)) return fail(PA_ERR_IO, "%s is no directory", out_dir);
    pa_bus* bus = nullptr;
    int rc = pa_bus_create(idx, h, bc_len, umi_len, &bus);
    if (rc != PA_OK) return rc;
    std::unique_ptr<pa_bus, void (*)(pa_bus*)> own(bus, pa_bus_destroy);

    Pool pool(num_threads < 1 ? usable_threads() : num_threads);
    PairReader rd(r1_path, r2_path, pool, bc_len + umi_len, st);
    if ((rc = rd.open()) != PA_OK) return rc;
    IndexStream stream;
    if ((rc = stream.create(idx)) != PA_OK) return rc;
    hipStream_t s = stream.get();
    rd.consumers = {s};
    CellBatch batches[2];
    rc = run_batches(rd, batches, [&](CellBatch& b) { return cell_batch_map(idx, b, s); }, [&](CellBatch& b) { return bus_batch_add(idx, bus, b, s, st); });
    if (rc != PA_OK) return rc;
    auto t0 = std::chrono::steady_clock::now();
    uint64_t n_records = 0;
    uint32_t n_ecs = 0;
    if ((rc = pa_bus_finish(bus, &n_records, &n_ecs)) != PA_OK) return rc;
    st[4] += secs_since(t0);
    t0 = std::chrono::steady_clock::now();
    if ((rc = pa_bus_write(bus, out_dir)) != PA_OK) return rc;
    st[5] = secs_since(t0);
    if (stats) (void)pa_bus_stats(bus, stats);
    st[6] = secs_since(t_call);
    st[7] = (double)rd.pairs;
    return PA_OK;
}

// ---- pa_count_pairs: two FASTQ files -> the class-count table of the pairs ----
struct PairBatch : CellBatch {   // + the reverse-complemented tiles of one mate, the pair stage's outputs
    DeviceBuffer<uint64_t> d_rc;
    DeviceBuffer<uint32_t> d_parena;
    DeviceBuffer<pa_read_result> d_presults;
    DeviceBuffer<uint8_t> d_scratch;
};

// the mate whose reverse complement is mapped (-1: neither)
int revcomp_mate(int orient) { return orient == PA_PAIR_RF ? 0 : orient == PA_PAIR_FR ? 1 : -1; }

// the batch's GPU leg up to the two mappings: mate m on s[m] (each stream has its own launch context on idx), all asynchronous
int pair_batch_map(pa_index* idx, PairBatch& b, int orient, uint32_t allowed, const hipStream_t s[2]) {
    int e = PA_OK;
    for (int m = 0; m < 2; ++m)
        if ((e = b.mate[m].encode(idx, b.n, 64, s[m])) != PA_OK) return e;
    if ((e = b.d_presults.reserve(b.n + 64, std::max(b.mate[0].h_off.size(), b.mate[0].d_off.size()) + 64)) != PA_OK) return e;
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
int pair_batch_count(pa_index* idx, PairBatch& b, int orient, uint32_t allowed, uint64_t* d_counts, const hipStream_t s[2], uint64_t* stats, double* st) {
    auto t0 = std::chrono::steady_clock::now();
    Mate &m1 = b.mate[0], &m2 = b.mate[1];
    for (int m = 0; m < 2; ++m) {
        Mate& x = b.mate[m];
        const uint64_t* tiles = m == revcomp_mate(orient) ? b.d_rc.get() : x.d_tiles.get();
        uint64_t used = 0;
        const int e = map_finish_regrow(idx, s[m], x.d_arena, &used, [&] { return x.map(idx, tiles, b.n, allowed, s[m]); });
        if (e != PA_OK) return e;
    }
    st[2] += secs_since(t0);
    t0 = std::chrono::steady_clock::now();
    // the pair arena is sized by a bound on what the batch can need, so that the counted launch cannot run out of it (a re-run would count twice)
    uint64_t bound = 0;
    const size_t scratch_bytes = pa_pairs_scratch_bytes(b.n);
    int e = b.d_scratch.reserve(scratch_bytes, scratch_bytes + scratch_bytes / 4);
    if (e != PA_OK) return e;
    if ((e = pairs_arena_bound(idx, m1.d_results.get(), m2.d_results.get(), b.n, b.d_scratch.get(), s[0], &bound)) != PA_OK) return e;
    if (bound > PA_MAX_ARENA_ENTRIES) return fail(PA_ERR_UNSUPPORTED, "a batch of %llu pairs may need %llu arena entries: lower PA_INGEST_BATCH", (unsigned long long)b.n, (unsigned long long)bound);
    if ((e = b.d_parena.reserve(bound + 64, bound + bound / 4 + 4096)) != PA_OK) return e;
    if ((e = pa_pairs_combine_device(idx, m1.d_results.get(), m1.d_arena.get(), m2.d_results.get(), m2.d_arena.get(), b.n, b.d_presults.get(), b.d_parena.get(), b.d_parena.size(),
                                     d_counts, b.d_scratch.get(), scratch_bytes, s[0])) != PA_OK)
        return e;
    uint64_t bst[PA_PAIR_STATS], used = 0, need = 0;
    if ((e = pa_pairs_finish(idx, b.d_scratch.get(), s[0], bst, &used, &need)) != PA_OK) return e;
    for (int j = 0; j < PA_PAIR_STATS; ++j) stats[j] += bst[j];
    st[4] += secs_since(t0);
    return PA_OK;
}

int count_pairs_impl(pa_index* idx, const char* r1_path, const char* r2_path, int orient, uint32_t allowed, int num_threads, uint64_t* h_counts, uint64_t* n_pairs,
                     uint64_t* stats_out) {
    const auto t_call = std::chrono::steady_clock::now();
    double* st = last_stage_seconds();
    for (int j = 0; j < PA_INGEST_STAGES; ++j) st[j] = 0.0;
    if (!idx || !r1_path || !r2_path || !h_counts) return fail(PA_ERR_INVALID_ARG, "null argument");
    if (orient != PA_PAIR_FR && orient != PA_PAIR_RF && orient != PA_PAIR_FF) return fail(PA_ERR_INVALID_ARG, "orientation %d (PA_PAIR_FR, PA_PAIR_RF or PA_PAIR_FF)", orient);
    Pool pool(num_threads < 1 ? usable_threads() : num_threads);
    PairReader rd(r1_path, r2_path, pool, 0xFFFFFFFFu, st);
    int rc = rd.open();
    if (rc != PA_OK) return rc;
    const uint64_t counts_len = pa_counts_len(idx);
    DeviceBuffer<uint64_t> d_counts;
    if ((rc = d_counts.alloc(counts_len)) != PA_OK) return rc;
    IndexStream streams[2];
    if ((rc = streams[0].create(idx)) != PA_OK || (rc = streams[1].create(idx)) != PA_OK) return rc;
    const hipStream_t s[2] = {streams[0].get(), streams[1].get()};
    PA_HIP_TRY(hipMemsetAsync(d_counts.get(), 0, counts_len * 8, s[0]));
    rd.consumers = {s[0], s[1]};
    PairBatch batches[2];
    uint64_t stats[PA_PAIR_STATS] = {0};
    rc = run_batches(rd, batches, [&](PairBatch& b) { return pair_batch_map(idx, b, orient, allowed, s); },
                     [&](PairBatch& b) { return pair_batch_count(idx, b, orient, allowed, d_counts.get(), s, stats, st); });
    if (rc != PA_OK) return rc;
    PA_HIP_TRY(hipMemcpyAsync(h_counts, d_counts.get(), counts_len * 8, hipMemcpyDeviceToHost, s[0]));
    PA_HIP_TRY(hipStreamSynchronize(s[0]));
    if (n_pairs) *n_pairs = rd.pairs;
    if (stats_out) for (int j = 0; j < PA_PAIR_STATS; ++j) stats_out[j] = stats[j];
    st[6] = secs_since(t_call);
    st[7] = (double)rd.pairs;
    return PA_OK;
}

// ---- pa_count_pairs_unstranded: the same two files -> the class-count table of the merged candidates ----
// Streams: s[m] maps mate m as given, s[2 + m] its reverse complement: four launch contexts on idx, so that all four mappings of a batch are in
// flight while the next batch is gathered. The tiles and lengths s[2 + m] reads are made on s[m]: it waits for `encoded[m]`.
struct StrandBatch : CellBatch {
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
int strand_batch_map(pa_index* idx, StrandBatch& b, uint32_t allowed, const hipStream_t s[4]) {
    int e = PA_OK;
    const size_t reads = std::max(b.mate[0].h_off.size(), b.mate[0].d_off.size()) + 64;
    const uint64_t hint = pa_map_arena_hint(idx, b.n);
    for (int m = 0; m < 2; ++m) {
        Mate& x = b.mate[m];
        if ((e = x.encode(idx, b.n, 64, s[m])) != PA_OK) return e;
        const size_t tw = pa_tiles_words(b.n, x.wpr()) + 1;
        if ((e = b.d_rc[m].reserve(tw, tw)) || (e = b.d_rc_results[m].reserve(b.n + 64, reads)) || (e = b.d_rc_arena[m].reserve(hint, hint)) ||
            (e = b.d_cresults[m].reserve(b.n + 64, reads)))
            return e;
        GpuEvent& ev = b.encoded[m];
        if (!ev.e) PA_HIP_TRY(hipEventCreateWithFlags(&ev.e, hipEventDisableTiming));
        PA_HIP_TRY(hipEventRecord(ev.e, s[m]));
        PA_HIP_TRY(hipStreamWaitEvent(s[2 + m], ev.e, 0));
        if ((e = pa_revcomp_tiles_device(idx, x.d_tiles.get(), x.d_lens.get(), b.n, x.wpr(), b.d_rc[m].get(), s[2 + m])) != PA_OK) return e;
        if ((e = x.map(idx, x.d_tiles.get(), b.n, allowed, s[m])) != PA_OK || (e = strand_map_rc(idx, b, m, allowed, s[2 + m])) != PA_OK) return e;
    }
    return b.d_mresults.reserve(b.n + 64, reads);
}

// waits for the four mappings (regrowing an arena as pa_map_finish asks), combines S on s[0] and R on s[1], both uncounted, then merges and counts on s[0]
int strand_batch_count(pa_index* idx, StrandBatch& b, uint32_t allowed, uint64_t* d_counts, const hipStream_t s[4], uint64_t* stats, double* st) {
    auto t0 = std::chrono::steady_clock::now();
    int e = PA_OK;
    for (int m = 0; m < 2; ++m) {
        Mate& x = b.mate[m];
        uint64_t used = 0;
        if ((e = map_finish_regrow(idx, s[m], x.d_arena, &used, [&] { return x.map(idx, x.d_tiles.get(), b.n, allowed, s[m]); })) != PA_OK) return e;
        if ((e = map_finish_regrow(idx, s[2 + m], b.d_rc_arena[m], &used, [&] { return strand_map_rc(idx, b, m, allowed, s[2 + m]); })) != PA_OK) return e;
    }
    st[2] += secs_since(t0);
    t0 = std::chrono::steady_clock::now();
    // every arena is sized by a bound on what its launch can need: the combines are not re-run, and the counted merge cannot be (it would count twice)
    Mate &m1 = b.mate[0], &m2 = b.mate[1];
    const pa_read_result* res1[2] = {m1.d_results.get(), b.d_rc_results[0].get()};   // candidate c: mate 1's records, its arena, mate 2's
    const uint32_t* ar1[2] = {m1.d_arena.get(), b.d_rc_arena[0].get()};
    const pa_read_result* res2[2] = {b.d_rc_results[1].get(), m2.d_results.get()};
    const uint32_t* ar2[2] = {b.d_rc_arena[1].get(), m2.d_arena.get()};
    const size_t cbytes = pa_pairs_scratch_bytes(b.n), mbytes = pa_strands_scratch_bytes(b.n);
    const char* const full = "a batch of %llu pairs may need %llu arena entries: lower PA_INGEST_BATCH";
    for (int c = 0; c < 2; ++c) {
        uint64_t bound = 0;
        if ((e = b.d_cscratch[c].reserve(cbytes, cbytes + cbytes / 4)) != PA_OK) return e;
        if ((e = pairs_arena_bound(idx, res1[c], res2[c], b.n, b.d_cscratch[c].get(), s[c], &bound)) != PA_OK) return e;
        if (bound > PA_MAX_ARENA_ENTRIES) return fail(PA_ERR_UNSUPPORTED, full, (unsigned long long)b.n, (unsigned long long)bound);
        if ((e = b.d_carena[c].reserve(bound + 64, bound + bound / 4 + 4096)) != PA_OK) return e;
        if ((e = pa_pairs_combine_device(idx, res1[c], ar1[c], res2[c], ar2[c], b.n, b.d_cresults[c].get(), b.d_carena[c].get(), b.d_carena[c].size(), nullptr,
                                         b.d_cscratch[c].get(), cbytes, s[c])) != PA_OK)
            return e;
    }
    for (int c = 0; c < 2; ++c)
        if ((e = pa_pairs_finish(idx, b.d_cscratch[c].get(), s[c], nullptr, nullptr, nullptr)) != PA_OK) return e;
    uint64_t bound = 0;
    if ((e = b.d_mscratch.reserve(mbytes, mbytes + mbytes / 4)) != PA_OK) return e;
    if ((e = strands_arena_bound(idx, b.d_cresults[0].get(), b.d_cresults[1].get(), b.n, b.d_mscratch.get(), s[0], &bound)) != PA_OK) return e;
    if (bound > PA_MAX_ARENA_ENTRIES) return fail(PA_ERR_UNSUPPORTED, full, (unsigned long long)b.n, (unsigned long long)bound);
    if ((e = b.d_marena.reserve(bound + 64, bound + bound / 4 + 4096)) != PA_OK) return e;
    if ((e = pa_strands_merge_device(idx, b.d_cresults[0].get(), b.d_carena[0].get(), b.d_cresults[1].get(), b.d_carena[1].get(), b.n, b.d_mresults.get(), b.d_marena.get(),
                                     b.d_marena.size(), d_counts, b.d_mscratch.get(), mbytes, s[0])) != PA_OK)
        return e;
    uint64_t bst[PA_STRAND_STATS], used = 0, need = 0;
    if ((e = pa_strands_finish(idx, b.d_mscratch.get(), s[0], bst, &used, &need)) != PA_OK) return e;
    for (int j = 0; j < PA_STRAND_STATS; ++j) stats[j] += bst[j];
    st[4] += secs_since(t0);
    return PA_OK;
}

int count_pairs_unstranded_impl(pa_index* idx, const char* r1_path, const char* r2_path, uint32_t allowed, int num_threads, uint64_t* h_counts, uint64_t* n_pairs,
                                uint64_t* stats_out) {
    const auto t_call = std::chrono::steady_clock::now();
    double* st = last_stage_seconds();
    for (int j = 0; j < PA_INGEST_STAGES; ++j) st[j] = 0.0;
    if (!idx || !r1_path || !r2_path || !h_counts) return fail(PA_ERR_INVALID_ARG, "null argument");
    Pool pool(num_threads < 1 ? usable_threads() : num_threads);
    PairReader rd(r1_path, r2_path, pool, 0xFFFFFFFFu, st);
    int rc = rd.open();
    if (rc != PA_OK) return rc;
    const uint64_t counts_len = pa_counts_len(idx);
    DeviceBuffer<uint64_t> d_counts;
    if ((rc = d_counts.alloc(counts_len)) != PA_OK) return rc;
    IndexStream streams[4];
    hipStream_t s[4];
    for (int j = 0; j < 4; ++j) {
        if ((rc = streams[j].create(idx)) != PA_OK) return rc;
        s[j] = streams[j].get();
    }
    PA_HIP_TRY(hipMemsetAsync(d_counts.get(), 0, counts_len * 8, s[0]));
    rd.consumers = {s[0], s[1]};   // (the gathered bytes and offsets are read by the encodes on s[0] and s[1] alone)
    StrandBatch batches[2];
    uint64_t stats[PA_STRAND_STATS] = {0};
    rc = run_batches(rd, batches, [&](StrandBatch& b) { return strand_batch_map(idx, b, allowed, s); },
                     [&](StrandBatch& b) { return strand_batch_count(idx, b, allowed, d_counts.get(), s, stats, st); });
    if (rc != PA_OK) return rc;
    PA_HIP_TRY(hipMemcpyAsync(h_counts, d_counts.get(), counts_len * 8, hipMemcpyDeviceToHost, s[0]));
    PA_HIP_TRY(hipStreamSynchronize(s[0]));
    if (n_pairs) *n_pairs = rd.pairs;
    if (stats_out) for (int j = 0; j < PA_STRAND_STATS; ++j) stats_out[j] = stats[j];
    st[6] = secs_since(t_call);
    st[7] = (double)rd.pairs;
    return PA_OK;
}

}  // namespace

extern "C" int pa_count_pairs_unstranded(pa_index* idx, const char* r1_path, const char* r2_path, uint32_t allowed_mismatches, int num_threads, uint64_t* h_counts,
                                         uint64_t* n_pairs, uint64_t stats[PA_STRAND_STATS]) {
    return no_throw("pa_count_pairs_unstranded", [&] { return count_pairs_unstranded_impl(idx, r1_path, r2_path, allowed_mismatches, num_threads, h_counts, n_pairs, stats); });
}

extern "C" int pa_count_cells(pa_index* idx, const pa_host_index* h, const char* r1_path, const char* r2_path, const char* whitelist_path, uint32_t bc_len,
                              uint32_t umi_len, const char* out_dir, int num_threads, uint64_t stats[PA_CELL_STATS]) {
    return no_throw("pa_count_cells", [&] { return count_cells_impl(idx, h, r1_path, r2_path, whitelist_path, bc_len, umi_len, out_dir, num_threads, stats); });
}

extern "C" int pa_count_pairs(pa_index* idx, const char* r1_path, const char* r2_path, int orient, uint32_t allowed_mismatches, int num_threads, uint64_t* h_counts,
                              uint64_t* n_pairs, uint64_t stats[PA_PAIR_STATS]) {
    return no_throw("pa_count_pairs", [&] { return count_pairs_impl(idx, r1_path, r2_path, orient, allowed_mismatches, num_threads, h_counts, n_pairs, stats); });
}

extern "C" int pa_write_bus(pa_index* idx, const pa_host_index* h, const char* r1_path, const char* r2_path, uint32_t bc_len, uint32_t umi_len, const char* out_dir,
                            int num_threads, uint64_t stats[PA_BUS_STATS]) {
    return no_throw("pa_write_bus", [&] { return write_bus_impl(idx, h, r1_path, r2_path, bc_len, umi_len, out_dir, num_threads, stats); });
}

extern "C" int pa_pairs_input_stats(uint64_t out[2 * PA_INGEST_INPUT_STATS]) {
    if (!out) return fail(PA_ERR_INVALID_ARG, "null argument");
    memcpy(out, last_pairs_input(), sizeof(uint64_t) * 2 * PA_INGEST_INPUT_STATS);
    return PA_OK;
}

extern "C" int pa_pairs_input_path(void) { return (int)last_pairs_input()[2 * PA_INGEST_INPUT_STATS]; }
