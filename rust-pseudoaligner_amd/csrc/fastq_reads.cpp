// pa_process_reads / pa_process_reads_multi, mirroring process_reads (src/pseudoaligner.rs:420-514): FASTQ in, one Rust-Debug-formatted tuple per
// read out, in INPUT order, with the flag rule of :455 as it is (true iff coverage >= 32 and the class is EMPTY). The pipeline over windows of
// raw text is described where it starts, below; the text itself is fastq_text.cpp's.
#include <hip/hip_runtime.h>
#include <emmintrin.h>
#include <sys/mman.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <string>
#include <cerrno>
#include <condition_variable>
#include <cstdio>
#include <chrono>
#include <cstdlib>
#include <deque>
#include <mutex>
#include <thread>

#include "fastq_text.hpp"

using namespace pa;
using namespace pa::ingest;

namespace {

// in-order writer: pieces of text (the batches' rendered tuples, in pinned memory) are written by a dedicated thread; the owner of a
// piece waits for its job before it overwrites the bytes
class Writer {
public:
    explicit Writer(FILE* f) : f_(f), th_([this] { loop(); }) {}
    uint64_t push(const char* p, size_t n) {   // returns the job's number (1, 2, ...)
        std::lock_guard<std::mutex> g(mu_);
        q_.push_back({p, n});
        cv_.notify_one();
        return ++pushed_;
    }
    void wait(uint64_t job) {                  // until job `job` has been written
        std::unique_lock<std::mutex> g(mu_);
        room_.wait(g, [&] { return written_ >= job; });
    }
    bool finish() {
        { std::lock_guard<std::mutex> g(mu_); done_ = true; }
        cv_.notify_one();
        th_.join();
        return ok_;
    }

private:
    void loop() {
        for (;;) {
            std::pair<const char*, size_t> job;
            {
                std::unique_lock<std::mutex> g(mu_);
                cv_.wait(g, [this] { return done_ || !q_.empty(); });
                if (q_.empty()) return;
                job = q_.front();
                q_.pop_front();
            }
            if (ok_ && job.second && fwrite(job.first, 1, job.second, f_) != job.second) ok_ = false;
            { std::lock_guard<std::mutex> g(mu_); ++written_; }
            room_.notify_all();
        }
    }
    FILE* f_;
    std::mutex mu_;
    std::condition_variable cv_, room_;
    std::deque<std::pair<const char*, size_t>> q_;
    uint64_t pushed_ = 0, written_ = 0;
    bool done_ = false, ok_ = true;
    std::thread th_;
};

// f32 as Rust's `{}` prints it (the progress line of :497-503): the shortest digits that read back as the same float, never an exponent
std::string rust_f32(float v) {
    if (v != v) return "NaN";
    if (v == 0.0f) return std::signbit(v) ? "-0" : "0";
    if (std::isinf(v)) return v < 0 ? "-inf" : "inf";
    char buf[64];
    int prec = 0;
    for (; prec < 9; ++prec) {
        snprintf(buf, sizeof buf, "%.*e", prec, (double)v);
        if (strtof(buf, nullptr) == v) break;
    }
    // buf = [-]d[.ddd]e[+-]xx  ->  digits and a decimal exponent
    std::string digits;
    const char* q = buf;
    const bool neg = *q == '-';
    if (neg) ++q;
    for (; *q && *q != 'e'; ++q)
        if (*q != '.') digits.push_back(*q);
    const int exp10 = atoi(q + 1);
    while (digits.size() > 1 && digits.back() == '0') digits.pop_back();
    std::string out = neg ? "-" : "";
    const int nd = (int)digits.size();
    if (exp10 < 0) {
        out += "0.";
        out.append((size_t)(-exp10 - 1), '0');
        out += digits;
    } else if (exp10 + 1 >= nd) {
        out += digits;
        out.append((size_t)(exp10 + 1 - nd), '0');
    } else {
        out += digits.substr(0, (size_t)exp10 + 1) + "." + digits.substr((size_t)exp10 + 1);
    }
    return out;
}

// ---- process_reads over WINDOWS of raw text ----
// The host does not look at the text: worker threads copy a window of the file into pinned memory (out of the file's mapping, page tables
// filled and dropped piece by piece: TextPipe::read_piece), the window goes to HBM as it is on a copy stream, the GPU finds its records (fastq_scan.hip) and the encode /
// map / render kernels read sequences and ids where they lie. A lane has FOUR streams: copy (text in), scan (a window's records: waits for its
// text and the scan before, not for the kernels of the window before), the kernels' stream, and back (the tuples' 14 MB per window to the host):
// on one stream the chain scan | encode | map | render | copy back + two host round trips was as long as a window's copy, and every hiccup a gap on the link. A window ends where the file offset says, not where a record does: the
// scan reports how many bytes its whole records take, and the unfinished record is read once more as the HEAD of the next window.
// Windows are dealt round-robin to LANES — one per index handle (pa_process_reads_multi: the GPUs of a node; the same handle twice
// gives two streams on one GPU) — and their tuples are written in input order. What the GPU scan does not take goes through the
// host's tolerant scan (scan_fastq) and the same in-place kernels: the last piece of the text (a missing final line break, trailing
// blank lines, an empty last record) and text that is not in four-line shape (wrapped records: rewritten first).
// process_reads_impl names the steps in order: open_lanes | gpu_windows (start_read, send_window, resolve, reread_from, enqueue_scan per window) | host_tail
// (host_batch per batch) | finish.
constexpr int LANE_SLOTS = 4;            // windows of a lane in flight: read | scan | map + render | write
constexpr uint32_t FLAG_BUCKETS = PA_RENDER_FLAG_BUCKETS;
constexpr uint64_t PIECE = 2ull << 20;   // bytes of a window that one task of the pool copies

struct Options {   // every switch the environment has for this driver, read once at the top of a call
    bool bgzf;              // PA_INGEST_BGZF=0 (diagnosis and A/B): a BGZF file is inflated on the host like any other .gz
    uint64_t batch_reads = DEFAULT_BATCH_READS;   // PA_INGEST_BATCH
    uint64_t window = 64ull << 20;   // bytes of a window the GPU scans (64 MiB: 128 MiB leaves more of the first read and the last kernels unoverlapped, 16 MiB costs launches) (PA_INGEST_WINDOW; never more than 256 bytes per read of a batch: the tests' small batches give small windows)
    bool verbose;           // PA_VERBOSE
    bool lane_serial;       // PA_LANE_SERIAL (knobs builds: A/B of the one-window-at-a-time rule for lanes that share a GPU)
    bool host_only;         // PA_INGEST_HOST_SCAN (diagnosis: every window through the host's scan)
    bool use_pread;         // PA_INGEST_PREAD (knobs builds: the windows through pread, as before; tools/microbench/host_read.cpp has both side by side)
    Options() {
        const char* v = getenv("PA_INGEST_BGZF");
        bgzf = !(v && *v && atoi(v) == 0);
        if ((v = getenv("PA_INGEST_BATCH"))) { const long long x = atoll(v); if (x >= 64) batch_reads = (uint64_t)x / 64 * 64; }
        if ((v = getenv("PA_INGEST_WINDOW"))) { const long long x = atoll(v); if (x >= 1) window = (uint64_t)x; }
        window = std::min<uint64_t>(std::min<uint64_t>(window, batch_reads * 256), 1ull << 31);
        verbose = getenv("PA_VERBOSE") != nullptr;
        lane_serial = knob_int("PA_LANE_SERIAL", 1) != 0;
        host_only = getenv("PA_INGEST_HOST_SCAN") != nullptr;
        use_pread = knob_int("PA_INGEST_PREAD", 0) != 0;
    }
    uint64_t window_of(const FastqText& t) const { return t.bgzf ? std::max<uint64_t>(window, PA_BGZF_MAX_ISIZE) : window; }   // a BGZF window's own text is a run of whole members
};

struct InputStats {   // pa_process_reads_input_stats, in the ABI's order: filled as the run goes, written once (TextPipe::finish)
    uint64_t text_kind = 0, members_total = 0, members_gpu = 0, members_host = 0, bytes_h2d = 0, text_bytes_gpu = 0;
};
static_assert(sizeof(InputStats) == sizeof(uint64_t) * PA_INGEST_INPUT_STATS, "one field per entry of the ABI's array");

uint64_t* last_input_stats() {   // pa_process_reads_input_stats: of this thread's last call
    static thread_local uint64_t st[PA_INGEST_INPUT_STATS] = {0};
    return st;
}

struct CopyTimer {   // PA_VERBOSE: how long the windows' copies to the GPU took (a window's events are read when the window eight later takes them over)
    bool on = false;
    hipEvent_t t0[8] = {nullptr}, t1[8] = {nullptr};
    uint64_t bytes[8] = {0};
    double ms = 0, total = 0;
    void begin(uint64_t id, hipStream_t s, uint64_t n) {
        if (!on) return;
        const int k = (int)(id % 8);
        if (!t0[k]) { (void)hipEventCreate(&t0[k]); (void)hipEventCreate(&t1[k]); }
        else { float w = 0; if (hipEventElapsedTime(&w, t0[k], t1[k]) == hipSuccess) { ms += w; total += (double)bytes[k]; } }
        (void)hipEventRecord(t0[k], s);
        bytes[k] = n;
    }
    void end(uint64_t id, hipStream_t s) { if (on) (void)hipEventRecord(t1[id % 8], s); }
    void release() {
        for (int i = 0; i < 8; ++i) { if (t0[i]) (void)hipEventDestroy(t0[i]); if (t1[i]) (void)hipEventDestroy(t1[i]); t0[i] = t1[i] = nullptr; }
    }
    ~CopyTimer() { release(); }
};

struct Lane {
    pa_index* idx = nullptr;
    int device = 0;
    IngestCache* cache = nullptr;        // its buffers and its four streams: stream (kernels), copy_stream, scan_stream, back_stream
    hipEvent_t last_h2d = nullptr;       // behind the lane's last window copy (an event of one of its slots)
    int64_t unfinished = -1;             // the window whose kernels were launched last on the kernels' stream and have not been waited for
    uint64_t text_job[LANE_SLOTS] = {0, 0, 0, 0};   // the writer's job that reads the slot's pinned text (0: none)
};

struct Win {
    uint64_t id = 0;
    int lane = 0, slot = 0;
    uint64_t from = 0;          // text offset of its first record
    uint64_t first_read = 0;    // number of the reads before it
    bool launched = false;      // its kernels are on the lane's stream
};

struct Pre {   // a window whose text is being read into its slot, or has been
    WindowPlan plan;
    uint64_t id = 0;
    BatchCtx* c = nullptr;
    Lane* l = nullptr;
};

constexpr int WIN_ODD = 1, WIN_EMPTY = 2;   // what resolve() answers besides a pa_status

struct TextPipe {
    const char* fastq_path;
    FastqText& text;
    Pool& pool;
    Writer& writer;
    std::vector<Lane>& lanes;
    const Options& opt;
    const double t_enter, t_begin;
    std::deque<Win> wins;       // launched or about to be, in order; the front is written first
    uint64_t next_id = 0, launched_reads = 0, reported = 0, flagged = 0, next_report = 1000000;
    double t_scan = 0, t_read = 0, t_wait = 0, t_launch = 0, t_text = 0, t_push = 0;
    uint64_t gpu_wins = 0, host_wins = 0, rescans = 0;   // windows whose records the GPU found, batches of the host's scan, scans run again
    InputStats stats{text.bgzf ? 2u : !text.inflated.empty() ? 1u : 0u, text.members.size()};
    CopyTimer timer{opt.verbose};
    uint64_t W = opt.window_of(text);
    const uint64_t KEEP = std::max<uint64_t>(4096, std::min<uint64_t>(W / 4, 1ull << 20));   // the end of the text is the host's: its rules for the last record live there
    uint64_t rec_start = 0;     // text offset of the first record no window has taken yet (known once the window before has been scanned)
    uint64_t read_to = 0;       // text read so far
    bool gpu_mode = false;      // windows are still handed to the GPU's scan
    bool have_pending = false;
    Win pending;                // the window whose records the GPU is finding
    Pre cur, nxt;               // the window being sent and scanned; the one whose text is being read behind it

    static double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
    int L() const { return (int)lanes.size(); }
    Lane& lane_of(uint64_t id) { return lanes[(size_t)(id % (uint64_t)L())]; }
    int slot_of(uint64_t id) const { return (int)((id / (uint64_t)L()) % LANE_SLOTS); }
    BatchCtx& ctx_of(const Win& w) { return lanes[(size_t)w.lane].cache->ctx[w.slot]; }
    int use(const Lane& l) { return hipSetDevice(l.device) == hipSuccess ? PA_OK : fail(PA_ERR_HIP, "hipSetDevice(%d) failed", l.device); }
    Win win_of(uint64_t id, uint64_t from) { Win w; w.id = id; w.lane = (int)(id % (uint64_t)L()); w.slot = slot_of(id); w.from = from; return w; }

    // lanes: one per handle; buffers and streams of an earlier call are taken from the handle
    int open_lanes(pa_index* const* idxs) {
        for (size_t i = 0; i < lanes.size(); ++i) {
            Lane& l = lanes[i];
            l.idx = idxs[i];
            const uint32_t *h_ec = nullptr, *h_class_ref = nullptr;
            index_host_classes(l.idx, &h_ec, &h_class_ref, &l.device);
            int e = use(l);
            if (e != PA_OK) return e;
            l.cache = static_cast<IngestCache*>(index_take_ingest_cache(l.idx));
            if (!l.cache) l.cache = new IngestCache();
            l.cache->idx = l.idx;
            for (hipStream_t* sp : {&l.cache->stream, &l.cache->copy_stream, &l.cache->scan_stream, &l.cache->back_stream})
                if (!*sp && hipStreamCreateWithFlags(sp, hipStreamNonBlocking) != hipSuccess) { *sp = nullptr; return fail(PA_ERR_HIP, "hipStreamCreate failed"); }
        }
        return PA_OK;
    }

    // [0, len) dealt in pieces of PIECE bytes: fn(a, b) copies bytes [a, b). One piece is copied by the caller, here. More go to the pool: all of them done on return
    // (wait), or left with the pool's workers (the answer is true: read_end waits for them)
    template <class F>
    bool deal_pieces(uint64_t len, bool wait, F fn) {
        if (len == 0) return false;
        const int ntask = (int)std::min<uint64_t>((len + PIECE - 1) / PIECE, 1u << 20);
        auto piece = [fn, len, ntask](int t) { fn(len * (uint64_t)t / (uint64_t)ntask, len * (uint64_t)(t + 1) / (uint64_t)ntask); };
        if (ntask == 1) { piece(0); return false; }
        if (wait) { pool.run(ntask, piece); return false; }
        pool.begin(ntask, piece);
        return true;
    }

    // bytes [off, off + len) of the text into dst (pinned): out of the file's mapping (read_piece), memcpy for text in memory (inflated gzip).
    // read_begin hands the pieces to the worker pool and returns; read_end waits for them (small reads are done at once by the caller)
    std::atomic<int> read_bad{0};
    bool read_async = false;
    // bytes of the mapping into a pinned window with streaming stores: the window is read next by the copy engine, never by this CPU, so no line of it
    // has to be fetched for ownership or kept in a cache
    static void copy_streaming(uint8_t* d, const uint8_t* s, size_t n) {
        size_t head = (64 - ((uintptr_t)d & 63)) & 63;
        if (head > n) head = n;
        memcpy(d, s, head);
        d += head; s += head; n -= head;
        const size_t body = n & ~(size_t)63;
        for (size_t i = 0; i < body; i += 64) {
            const __m128i v0 = _mm_loadu_si128((const __m128i*)(s + i)), v1 = _mm_loadu_si128((const __m128i*)(s + i + 16));
            const __m128i v2 = _mm_loadu_si128((const __m128i*)(s + i + 32)), v3 = _mm_loadu_si128((const __m128i*)(s + i + 48));
            _mm_stream_si128((__m128i*)(d + i), v0); _mm_stream_si128((__m128i*)(d + i + 16), v1);
            _mm_stream_si128((__m128i*)(d + i + 32), v2); _mm_stream_si128((__m128i*)(d + i + 48), v3);
        }
        _mm_sfence();
        memcpy(d + body, s + body, n - body);
    }
    void read_piece(uint64_t a, uint64_t b, uint8_t* dst) {   // text bytes [a, b) to dst
        if (text.mapped && text.data == text.map_base && !opt.use_pread) {
            // A file: out of its MAPPING. pread copies at 65 - 75 GB/s on 16 threads of the target host (one copy_to_user per page, the file's page-cache
            // lock) — 1.2 x the link, no margin — the same bytes out of the mapping at 127 GB/s INCLUDING the page tables of the piece, which are
            // filled in one call before the copy (MADV_POPULATE_READ, Linux 5.14; without it the copy faults them in: 115 GB/s) and dropped behind it
            // (a 100 GB file would otherwise keep 25 M entries mapped until the call ends)
            constexpr uint64_t PAGE = 4096;
            const bool big = b - a >= (256u << 10);
            if (big) {
                const uint64_t pa = a & ~(PAGE - 1), pb = std::min<uint64_t>((b + PAGE - 1) & ~(PAGE - 1), text.map_size);
#ifdef MADV_POPULATE_READ
                (void)madvise((void*)(text.map_base + pa), (size_t)(pb - pa), MADV_POPULATE_READ);
#else
                (void)madvise((void*)(text.map_base + pa), (size_t)(pb - pa), 22);
#endif
            }
            copy_streaming(dst, (const uint8_t*)text.data + a, (size_t)(b - a));
            if (big) {
                const uint64_t qa = (a + PAGE - 1) & ~(PAGE - 1), qb = b & ~(PAGE - 1);
                if (qb > qa) (void)madvise((void*)(text.map_base + qa), (size_t)(qb - qa), MADV_DONTNEED);
            }
        } else if (text.mapped && text.fd >= 0 && text.data == text.map_base) {
            uint64_t p = a;
            while (p < b) {
                const ssize_t got = pread(text.fd, dst + (p - a), (size_t)(b - p), (off_t)p);
                if (got < 0 && errno == EINTR) continue;
                if (got <= 0) { read_bad.store(1); return; }
                p += (uint64_t)got;
            }
        } else memcpy(dst, text.data + a, (size_t)(b - a));
    }
    void read_begin(uint64_t off, uint64_t len, uint8_t* dst) {
        read_async = deal_pieces(len, false, [this, off, dst](uint64_t a, uint64_t b) { read_piece(off + a, off + b, dst + a); });
    }
    int read_end() {
        if (read_async) { pool.end(); read_async = false; }
        return read_bad.exchange(0) ? fail(PA_ERR_IO, "%s: read failed: %s", fastq_path, strerror(errno)) : PA_OK;
    }
    // a BGZF window: bytes [off, off + len) of the COMPRESSED file into dst (pinned), by the pool, with streaming stores
    void read_comp_begin(uint64_t off, uint64_t len, uint8_t* dst) {
        const uint8_t* src = (const uint8_t*)text.map_base + off;
        read_async = deal_pieces(len, false, [src, dst](uint64_t a, uint64_t b) { copy_streaming(dst + a, src + a, (size_t)(b - a)); });
    }
    int read_small(uint64_t off, uint64_t len, uint8_t* dst) {   // by the caller itself, whatever the pool is doing (a window's head: <= 1 MiB)
        if (text.bgzf) return len ? bgzf_read_host(text, fastq_path, off, len, dst) : PA_OK;   // (the members that hold the unfinished record: inflated by this thread)
        if (len) read_piece(off, off + len, dst);
        return read_bad.load() ? fail(PA_ERR_IO, "%s: read failed: %s", fastq_path, strerror(errno)) : PA_OK;
    }

    // the kernels of the window launched before on this lane's stream: waited for (they share the stream's launch context inside the index)
    int finish_lane(Lane& l) {
        if (l.unfinished < 0) return PA_OK;
        for (Win& w : wins)
            if ((int64_t)w.id == l.unfinished) {
                const double t0 = now();
                int e = use(l);
                if (e == PA_OK) e = batch_finish(l.idx, ctx_of(w), l.cache->stream);
                t_wait += now() - t0;
                l.unfinished = -1;
                return e;
            }
        l.unfinished = -1;
        return PA_OK;
    }

    // the tuples of the windows whose kernels have been waited for: to the writer, in order, with the progress line of :497-503.
    // upto: also wait for the kernels of every window with id < upto (all of them at the end of the text)
    int retire_finished(uint64_t upto) {
        while (!wins.empty()) {
            Win& w = wins.front();
            if (!w.launched) break;   // (the window being launched right now)
            Lane& l = lanes[(size_t)w.lane];
            if (l.unfinished == (int64_t)w.id) {
                if (w.id >= upto) break;
                const int e = finish_lane(l);
                if (e != PA_OK) return e;
            }
            BatchCtx& c = ctx_of(w);
            const double t0 = now();
            int e = use(l);
            if (e == PA_OK) e = batch_text_wait(c);
            t_text += now() - t0;
            if (e != PA_OK) return e;
            uint64_t cum = 0, bucket = 0;
            while (next_report <= w.first_read + c.n) {   // :497-503: the counts of exactly the first 10^6 m reads
                if (bucket < FLAG_BUCKETS) cum += c.h_tot.get()[1 + bucket];
                ++bucket;
                fprintf(stderr, "\rDone Mapping %llu reads w/ Rate: %s", (unsigned long long)next_report,
                        rust_f32((float)(flagged + cum) * 100.0f / (float)next_report).c_str());
                fflush(stderr);
                next_report += 1000000;
            }
            flagged += c.flagged;
            reported += c.n;
            l.text_job[w.slot] = writer.push(c.h_text.get(), c.text_bytes);
            wins.pop_front();
        }
        return PA_OK;
    }

    // the slot of window `id`: the window that had it before (LANE_SLOTS windows of this lane earlier) has been handed to the writer
    int acquire(uint64_t id, BatchCtx** out) {
        const uint64_t span = (uint64_t)L() * LANE_SLOTS;
        if (id >= span) {
            const int e = retire_finished(id - span + 1);
            if (e != PA_OK) return e;
        }
        Lane& l = lane_of(id);
        BatchCtx& c = l.cache->ctx[slot_of(id)];
        int e = use(l);
        if (e != PA_OK) return e;
        if ((e = window_ensure_events(c)) != PA_OK) return e;
        c.back = l.cache->back_stream;
        *out = &c;
        return PA_OK;
    }

    // index.map_read (:451) for the window's records (c.n of them, c.wpr words each, found by the GPU scan or filled in by the host)
    int launch(Win& w) {
        Lane& l = lanes[(size_t)w.lane];
        BatchCtx& c = ctx_of(w);
        int e = finish_lane(l);
        if (e != PA_OK) return e;
        if ((e = retire_finished(0)) != PA_OK) return e;
        double t0 = now();
        if (l.text_job[w.slot]) { writer.wait(l.text_job[w.slot]); l.text_job[w.slot] = 0; }   // (the launch ends with the speculative copy of the tuples into the slot's pinned text)
        t_push += now() - t0; t0 = now();
        if ((e = use(l)) != PA_OK) return e;
        c.in_place = true;
        w.first_read = launched_reads;
        c.flag_mark = 1000000 - launched_reads % 1000000;
        if ((e = batch_ensure(l.idx, c, c.n, c.wpr, std::min<uint64_t>(std::max<uint64_t>(c.n + c.n / 8, 1 << 16), std::max<uint64_t>(opt.batch_reads, c.n)))) != PA_OK) return e;
        if ((e = batch_launch(l.idx, c, l.cache->stream)) != PA_OK) return e;
        l.unfinished = (int64_t)w.id;
        w.launched = true;
        launched_reads += c.n;
        t_launch += now() - t0;
        return PA_OK;
    }

    // the next window (plan_window: none when the text in front of the host's part has been read) gets its slot, and the pool's workers start to copy its bytes
    // into the slot's pinned memory: the text itself, or a BGZF window's compressed members with their rows of the member table
    int start_read(Pre& p, uint64_t id) {
        p.plan = gpu_mode ? plan_window(text, read_to, W, KEEP) : WindowPlan();
        const WindowPlan& plan = p.plan;
        if (!plan.active) return PA_OK;
        p.id = id;
        int e = acquire(id, &p.c);
        if (e != PA_OK) return e;
        p.l = &lane_of(id);
        if ((e = window_ensure_raw(*p.c, WINDOW_HEAD_ROOM + plan.text_len)) != PA_OK) return e;
        if (plan.n_members) {
            if ((e = window_ensure_comp(*p.c, plan.comp_len, plan.n_members)) != PA_OK) return e;
            for (uint64_t i = 0; i < plan.n_members; ++i) {
                pa_bgzf_member r = text.members[plan.first_member + i];
                r.in_off -= plan.comp_from;
                p.c->h_mrows.get()[i] = r;
            }
            read_comp_begin(plan.comp_from, plan.comp_len, p.c->h_comp.get());
        } else read_begin(plan.text_from, plan.text_len, p.c->h_raw.get() + WINDOW_HEAD_ROOM);
        read_to = plan.text_from + plan.text_len;
        return PA_OK;
    }

    // the window's bytes, now in pinned memory, go to the GPU on the lane's copy stream; a BGZF window's members are inflated there, behind their copy,
    // and their statuses come back ahead of ev_h2d
    int send_window(const Pre& p) {
        const WindowPlan& plan = p.plan;
        BatchCtx& c = *p.c;
        Lane& l = *p.l;
        const hipStream_t copy = l.cache->copy_stream;
        const double t0 = now();
        int e = read_end();
        if (e != PA_OK) return e;
        t_read += now() - t0;
        if ((e = use(l)) != PA_OK) return e;
        timer.begin(p.id, copy, plan.n_members ? plan.comp_len : plan.text_len);
        // lanes that share a GPU (a handle listed twice) send their windows one at a time: with two copies of one direction queued at once the runtime
        // runs one of them as a blit kernel, at a fraction of the DMA engine's rate (host_batch.cpp has the measurement)
        for (size_t o = 0; o < lanes.size() && opt.lane_serial; ++o)
            if (&lanes[o] != &l && lanes[o].device == l.device && lanes[o].last_h2d) PA_HIP_TRY(hipStreamWaitEvent(copy, lanes[o].last_h2d, 0));
        c.n_members = plan.n_members;
        if (plan.n_members) {   // BGZF: the compressed members cross the link, the text first exists in HBM
            PA_HIP_TRY(hipMemcpyAsync(c.d_comp.get(), c.h_comp.get(), plan.comp_len, hipMemcpyHostToDevice, copy));
            PA_HIP_TRY(hipMemcpyAsync(c.d_mrows.get(), c.h_mrows.get(), plan.n_members * sizeof(pa_bgzf_member), hipMemcpyHostToDevice, copy));
            if ((e = bgzf_inflate_launch(c.d_comp.get(), plan.comp_len, c.d_mrows.get(), plan.n_members, c.d_raw.get() + WINDOW_HEAD_ROOM, plan.text_len, c.d_mstat.get(), copy)) != PA_OK) return e;
            PA_HIP_TRY(hipMemcpyAsync(c.h_mstat.get(), c.d_mstat.get(), plan.n_members * sizeof(uint32_t), hipMemcpyDeviceToHost, copy));
            stats.members_gpu += plan.n_members;
            stats.bytes_h2d += plan.comp_len + plan.n_members * sizeof(pa_bgzf_member);
            stats.text_bytes_gpu += plan.text_len;
        } else {
            PA_HIP_TRY(hipMemcpyAsync(c.d_raw.get() + WINDOW_HEAD_ROOM, c.h_raw.get() + WINDOW_HEAD_ROOM, plan.text_len, hipMemcpyHostToDevice, copy));
            stats.bytes_h2d += plan.text_len;
        }
        PA_HIP_TRY(hipEventRecord(c.ev_h2d, copy));
        l.last_h2d = c.ev_h2d;
        timer.end(p.id, copy);
        return PA_OK;
    }

    // the pending window's scan: waited for; its records are launched, the next window's first record is known
    int resolve() {
        Lane& l = lanes[(size_t)pending.lane];
        BatchCtx& c = l.cache->ctx[pending.slot];
        const FqInfo& info = *c.h_info.get();
        have_pending = false;
        int e = use(l);
        if (e != PA_OK) return e;
        for (int attempt = 0;; ++attempt) {
            const double t0 = now();
            PA_HIP_TRY(hipEventSynchronize(c.ev_info));
            t_wait += now() - t0;
            if (!info.overflow) break;
            if (attempt == 2) return fail(PA_ERR_INTERNAL, "FASTQ scan: line table too small after regrowing");
            ++rescans;   // more lines than guessed (short reads): grow the line table, fill it again from the counts already there
            if ((e = window_ensure_scan(c, info.lines)) != PA_OK) return e;
            if ((e = window_scan_enqueue(c, true, l.cache->scan_stream)) != PA_OK) return e;
        }
        for (uint64_t i = 0; i < c.n_members; ++i)   // (they came back on the copy stream ahead of ev_h2d, which the scan waited for)
            if (c.h_mstat.get()[i] != PA_INFLATE_OK)
                return fail(PA_ERR_FORMAT, "%s: corrupt gzip stream: member at byte %llu: %s", fastq_path, (unsigned long long)c.h_mrows.get()[i].file_off,
                            pa_inflate_status_name(c.h_mstat.get()[i]));
        if (info.odd) return WIN_ODD;
        if (info.n == 0) return WIN_EMPTY;
        if (info.max_seq > PA_MAX_READ_LEN) return fail(PA_ERR_UNSUPPORTED, "read longer than %u bases", PA_MAX_READ_LEN);
        c.n = info.n;
        c.wpr = pa_words_per_read(info.max_seq ? info.max_seq : 1);
        rec_start = pending.from + info.consumed;
        wins.push_back(pending);
        ++gpu_wins;
        return launch(wins.back());
    }

    // a window is dropped: its text (and what was being read behind it) is read again, from the first record not yet taken
    int reread_from(uint64_t from) {
        if (nxt.plan.active) { (void)read_end(); nxt.plan.active = false; }
        (void)hipStreamSynchronize(cur.l->cache->copy_stream);
        read_to = from;
        if (W > (1ull << 31)) gpu_mode = false;   // (a record of gigabytes: the host's scan says what it is)
        return start_read(cur, next_id);
    }

    // the window's records are to be found: the unfinished record of the window before goes in front of the window's own text as its head (on the scan stream,
    // which then waits for the text itself: ev_h2d only), the scan follows and the window is the pending one
    int enqueue_scan(const Pre& p, uint64_t head, uint64_t skip) {
        BatchCtx& c = *p.c;
        const hipStream_t scan = p.l->cache->scan_stream;
        double t0 = now();
        if (head) {
            uint8_t* const h = c.h_raw.get() + WINDOW_HEAD_ROOM - head;
            const int e = read_small(rec_start, head, h);
            if (e != PA_OK) return e;
            PA_HIP_TRY(hipMemcpyAsync(c.d_raw.get() + WINDOW_HEAD_ROOM - head, h, head, hipMemcpyHostToDevice, scan));
            stats.bytes_h2d += head;
        }
        t_read += now() - t0; t0 = now();
        c.raw_begin = WINDOW_HEAD_ROOM - head + skip;
        c.raw_end = WINDOW_HEAD_ROOM + p.plan.text_len;
        int e = window_ensure_scan(c, 0);
        if (e != PA_OK) return e;
        PA_HIP_TRY(hipStreamWaitEvent(scan, c.ev_h2d, 0));
        if ((e = window_scan_enqueue(c, false, scan)) != PA_OK) return e;
        t_launch += now() - t0;
        pending = win_of(p.id, rec_start);
        have_pending = true;
        next_id = p.id + 1;
        return PA_OK;
    }

    // ---- windows the GPU scans ----
    // The text of window w + 1 is read (by the pool's workers, asynchronously) while this thread waits for window w - 1's scan, launches its kernels and
    // enqueues window w's scan: the reads follow each other without a gap, and so do the copies to the GPU behind them.
    int gpu_windows_loop() {
        int e = start_read(cur, next_id);
        while (e == PA_OK && cur.plan.active) {
            if ((e = send_window(cur)) != PA_OK) break;
            if ((e = start_read(nxt, cur.id + 1)) != PA_OK) break;      // the next window's text starts to arrive
            const uint64_t main_from = cur.plan.text_from;
            bool discard = false;
            if (have_pending) {
                const int r = resolve();
                if (r == WIN_ODD) { gpu_mode = false; discard = true; rec_start = pending.from; next_id = pending.id; }               // not four-line text from here on: the host's scan takes over
                else if (r == WIN_EMPTY) { W = std::max<uint64_t>(2 * W, 2 * (main_from - pending.from)); discard = true; rec_start = pending.from; next_id = pending.id; }   // no whole record in the window: a longer one
                else if (r != PA_OK) { e = r; break; }
            }
            if ((e = use(*cur.l)) != PA_OK) break;
            const uint64_t head = main_from > rec_start ? main_from - rec_start : 0;   // the unfinished record of the window before
            const uint64_t skip = rec_start > main_from ? rec_start - main_from : 0;   // (BGZF behind a discarded window: the first record starts inside the first member)
            if (!discard && head > WINDOW_HEAD_ROOM) { W = std::max<uint64_t>(W, 2 * head); discard = true; }
            if (discard) { e = reread_from(rec_start); continue; }
            if ((e = enqueue_scan(cur, head, skip)) != PA_OK) break;
            if ((e = retire_finished(0)) != PA_OK) break;
            cur = nxt;
            nxt.plan.active = false;
        }
        return e;
    }
    int gpu_windows() {
        gpu_mode = !opt.host_only && text.fsize > KEEP;
        int e = gpu_windows_loop();
        (void)read_end();   // (an error path: nothing of the pool's job is left behind)
        gpu_mode = false;
        if (e == PA_OK && have_pending) {
            const int r = resolve();
            if (r == WIN_ODD || r == WIN_EMPTY) { rec_start = pending.from; next_id = pending.id; }
            else e = r;
        }
        return e;
    }

    // a batch of the host-scanned text: records rp[0, n), whose text ends at `end` (ws's offsets). Text and records go to the GPU, the same kernels follow
    int host_batch(const WindowScan& ws, const RecPos* rp, uint64_t n, uint64_t end) {
        const uint64_t first = rp[0].start, bytes = end - first, id = next_id;
        if (bytes > (3ull << 30)) return fail(PA_ERR_UNSUPPORTED, "%s: record %llu is longer than 3 GiB", fastq_path, (unsigned long long)launched_reads);
        BatchCtx* cp = nullptr;
        int e = acquire(id, &cp);
        if (e != PA_OK) return e;
        BatchCtx& c = *cp;
        if ((e = window_ensure_raw(c, WINDOW_HEAD_ROOM + bytes)) != PA_OK) return e;
        if ((e = window_ensure_recs(c, n, true)) != PA_OK) return e;
        const double t0 = now();
        // the batch's text (plain memcpy: the bytes were just read by the scan and lie in the caches) and where its records lie in it
        const char* const src = ws.base + first;
        uint8_t* const dst = c.h_raw.get() + WINDOW_HEAD_ROOM;
        deal_pieces(bytes, true, [src, dst](uint64_t a, uint64_t b) { memcpy(dst + a, src + a, (size_t)(b - a)); });
        const int T4 = pool.size() * 4;
        std::vector<uint32_t> tmax((size_t)T4, 0);
        pool.run(T4, [&](int t) {
            uint32_t mx = 0;
            for (uint64_t i = n * (uint64_t)t / (uint64_t)T4; i < n * (uint64_t)(t + 1) / (uint64_t)T4; ++i) {
                const RecPos& r = rp[i];
                const uint64_t seq_off = std::min<uint64_t>(r.start + r.hdr + 1, ws.size);
                const uint32_t seq_len = (uint32_t)std::min<uint64_t>(r.seq_len, ws.size - seq_off);
                c.h_rec.get()[i] = make_uint4((uint32_t)(WINDOW_HEAD_ROOM + r.start + 1 - first), r.id_len, (uint32_t)(WINDOW_HEAD_ROOM + seq_off - first), seq_len);
                mx = std::max(mx, seq_len);
            }
            tmax[(size_t)t] = mx;
        });
        uint32_t maxlen = 1;
        for (uint32_t m : tmax) maxlen = std::max(maxlen, m);
        t_read += now() - t0;
        if (maxlen > PA_MAX_READ_LEN) return fail(PA_ERR_UNSUPPORTED, "read longer than %u bases", PA_MAX_READ_LEN);
        // (the copies ride on the lane's kernel stream: this path is bound by the host's scan, not by the link)
        const hipStream_t stream = lane_of(id).cache->stream;
        PA_HIP_TRY(hipMemcpyAsync(c.d_raw.get() + WINDOW_HEAD_ROOM, dst, bytes, hipMemcpyHostToDevice, stream));
        PA_HIP_TRY(hipMemcpyAsync(c.d_rec.get(), c.h_rec.get(), n * sizeof(uint4), hipMemcpyHostToDevice, stream));
        stats.bytes_h2d += bytes + n * sizeof(uint4);
        c.n_members = 0;
        c.raw_begin = WINDOW_HEAD_ROOM;
        c.raw_end = WINDOW_HEAD_ROOM + bytes;
        c.n = n;
        c.wpr = pa_words_per_read(maxlen);
        next_id = id + 1;
        wins.push_back(win_of(id, 0));
        ++host_wins;
        return launch(wins.back());
    }

    // ---- the rest of the text (its end; all of it when it is not in four-line shape): the host's scan, the same kernels ----
    int host_tail() {
        int e = PA_OK;
        // BGZF: what is left (the last KEEP bytes; everything from here on when the text is not in four-line shape) is inflated by the host's pool
        if (text.bgzf && (e = bgzf_materialise(text, fastq_path, pool, &rec_start)) != PA_OK) return e;
        IngestCache* const hc = lanes[0].cache;   // (the scan's lists are parked with lane 0's buffers)
        text.off = rec_start;
        WindowScan ws(text);
        uint64_t records_before = launched_reads;
        for (;;) {
            const double t0 = now();
            e = ws.next(fastq_path, records_before, pool, hc->rec_pos, hc->brk);
            t_scan += now() - t0;
            if (e != PA_OK || ws.nrec == 0) return e;
            records_before += ws.nrec;
            const RecPos* const rp = hc->rec_pos.data();
            auto end_of = [&](uint64_t i) { return i < ws.nrec ? rp[i].start : ws.size; };
            for (uint64_t i0 = 0; i0 < ws.nrec;) {
                // a batch of whole records whose text fits a window of 2 GiB (offsets into it are 32 bits)
                uint64_t i1 = std::min<uint64_t>(ws.nrec, i0 + opt.batch_reads);
                while (i1 > i0 + 1 && end_of(i1) - rp[i0].start > (1ull << 31)) i1 = i0 + (i1 - i0) / 2;
                if ((e = host_batch(ws, rp + i0, i1 - i0, end_of(i1))) != PA_OK) return e;
                i0 = i1;
            }
        }
    }

    // the end of a call, good or bad (rc): the figures of the call are left for their getters, every stream is waited for, the writer ends, and the lanes' buffers
    // are parked on their handles (or destroyed behind an error, whose message is kept)
    int finish(int rc, const char* out_path) {
        const double st[PA_INGEST_STAGES] = {t_scan, t_read, t_wait, t_launch, t_text, t_push, now() - t_begin, (double)reported};
        memcpy(pa::ingest::last_stage_seconds(), st, sizeof st);
        if (stats.text_kind == 2) stats.members_host = text.members_host;
        memcpy(last_input_stats(), &stats, sizeof stats);
        if (opt.verbose)
            fprintf(stderr, "\n[pa ingest] %llu reads, %d threads, %d lane(s): %llu windows scanned on the GPU (%llu scanned twice), %llu batches by the host; host scan %.3f s, read %.3f s, wait GPU %.3f s, launch %.3f s, wait text %.3f s, wait writer %.3f s, total %.3f s (before the first window %.3f s)\n",
                    (unsigned long long)reported, pool.size(), L(), (unsigned long long)gpu_wins, (unsigned long long)rescans, (unsigned long long)host_wins, t_scan, t_read, t_wait,
                    t_launch, t_text, t_push, now() - t_begin, t_begin - t_enter);
        if (opt.verbose && timer.ms > 0) fprintf(stderr, "[pa ingest] windows to the GPU: %.1f MB in %.2f ms of copies = %.1f GB/s\n", timer.total / 1e6, timer.ms, timer.total / timer.ms / 1e6);
        timer.release();
        if (reported >= 1000000) fputc('\n', stderr);   // (`eprintln!()` behind the progress line, :508)
        for (Lane& l : lanes) {
            if (!l.cache) continue;
            (void)hipSetDevice(l.device);
            for (hipStream_t s : {l.cache->copy_stream, l.cache->scan_stream, l.cache->back_stream, l.cache->stream})   // (the streams stay with the parked buffers; IngestCache::destroy releases them)
                if (s) (void)hipStreamSynchronize(s);
        }
        bool wrote = true;
        try { wrote = writer.finish(); } catch (...) { wrote = false; }
        if (rc == PA_OK && !wrote) rc = fail(PA_ERR_IO, "short write to %s", out_path);
        const std::string why = rc != PA_OK ? last_error_ref() : std::string();
        for (Lane& l : lanes) {
            if (!l.cache) continue;
            (void)hipSetDevice(l.device);
            if (l.cache->rec_pos.capacity() > ((size_t)64 << 20)) { std::vector<RecPos>().swap(l.cache->rec_pos); std::vector<std::vector<uint32_t>>().swap(l.cache->brk); }   // (do not park more than 1 GB of it)
            if (rc == PA_OK) index_put_ingest_cache(l.idx, l.cache, IngestCache::destroy);   // the next call starts with warm buffers
            else IngestCache::destroy(l.cache);
            l.cache = nullptr;
        }
        if (rc != PA_OK && !why.empty()) last_error_ref() = why;
        return rc;
    }
};

int check_replicas(pa_index* const* idxs, int nidx) {
    pa_index_stats s0, si;
    if (pa_index_get_stats(idxs[0], &s0) != PA_OK) return PA_ERR_INVALID_ARG;
    for (int i = 1; i < nidx; ++i) {
        if (pa_index_get_stats(idxs[i], &si) != PA_OK) return PA_ERR_INVALID_ARG;
        if (si.k != s0.k || si.num_nodes != s0.num_nodes || si.num_classes != s0.num_classes || si.num_kmers != s0.num_kmers)
            return fail(PA_ERR_INVALID_ARG, "handle %d is not a replica of handle 0 (k / nodes / classes / k-mers differ)", i);
    }
    return PA_OK;
}

int process_reads_impl(pa_index* const* idxs, int nidx, const char* fastq_path, const char* out_path, int num_threads, uint64_t* n_reads_out, uint64_t* n_flagged_out) {
    if (!idxs || nidx < 1 || !fastq_path || !out_path) return fail(PA_ERR_INVALID_ARG, "null argument");
    for (int i = 0; i < nidx; ++i)
        if (!idxs[i]) return fail(PA_ERR_INVALID_ARG, "null index handle");
    const double t_enter = TextPipe::now();
    if (num_threads < 1) num_threads = 1;
    if (n_reads_out) *n_reads_out = 0;
    if (n_flagged_out) *n_flagged_out = 0;
    int rc = check_replicas(idxs, nidx);
    if (rc != PA_OK) return rc;
    const Options opt;

    FastqText text;
    if (opt.bgzf) open_bgzf(fastq_path, text);
    if (!text.bgzf && (rc = open_fastq(fastq_path, text)) != PA_OK) return rc;
    FILE* out = strcmp(out_path, "-") == 0 ? stdout : fopen(out_path, "wb");
    if (!out) { text.release(); return fail(PA_ERR_IO, "cannot create %s: %s", out_path, strerror(errno)); }
    // a private 4 MiB stdio buffer only for a file this function opened (and closes before the buffer dies); the process-wide
    // stdout keeps its own buffering: handing it a function-local buffer would leave it dangling after the return
    std::vector<char> obuf(out != stdout ? (size_t)1 << 22 : 0);
    if (out != stdout) setvbuf(out, obuf.data(), _IOFBF, obuf.size());

    const double t_begin = TextPipe::now();
    Pool pool(num_threads);
    std::vector<Lane> lanes((size_t)nidx);
    Writer writer(out);
    TextPipe tp{fastq_path, text, pool, writer, lanes, opt, t_enter, t_begin};
    rc = no_throw("pa_process_reads", [&] {
        int e = tp.open_lanes(idxs);
        if (e == PA_OK) e = tp.gpu_windows();             // the text in windows as the file holds them: records found by the GPU
        if (e == PA_OK) e = tp.host_tail();               // its end, and text that is not in four-line shape: records found by the host
        return e == PA_OK ? tp.retire_finished(~0ull) : e;
    });
    rc = tp.finish(rc, out_path);
    text.release();
    if (out != stdout) { if (fclose(out) != 0 && rc == PA_OK) rc = fail(PA_ERR_IO, "close %s: %s", out_path, strerror(errno)); }
    else fflush(stdout);
    if (n_reads_out) *n_reads_out = tp.reported;
    if (n_flagged_out) *n_flagged_out = tp.flagged;
    return rc;
}

}  // namespace

extern "C" int pa_process_reads(pa_index* idx, const char* fastq_path, const char* out_path, int num_threads, uint64_t* n_reads_out,
                                uint64_t* n_flagged_out) {
    pa_index* one[1] = {idx};
    return no_throw("pa_process_reads", [&] { return process_reads_impl(one, 1, fastq_path, out_path, num_threads, n_reads_out, n_flagged_out); });
}

extern "C" int pa_process_reads_multi(pa_index* const* idx, int n_idx, const char* fastq_path, const char* out_path, int num_threads, uint64_t* n_reads_out,
                                      uint64_t* n_flagged_out) {
    return no_throw("pa_process_reads_multi", [&] { return process_reads_impl(idx, n_idx, fastq_path, out_path, num_threads, n_reads_out, n_flagged_out); });
}

extern "C" int pa_process_reads_input_stats(uint64_t out[PA_INGEST_INPUT_STATS]) {
    if (!out) return fail(PA_ERR_INVALID_ARG, "null argument");
    memcpy(out, last_input_stats(), sizeof(uint64_t) * PA_INGEST_INPUT_STATS);
    return PA_OK;
}

extern "C" int pa_process_reads_stage_seconds(double out[PA_INGEST_STAGES]) {
    if (!out) return fail(PA_ERR_INVALID_ARG, "null argument");
    memcpy(out, pa::ingest::last_stage_seconds(), sizeof(double) * PA_INGEST_STAGES);
    return PA_OK;
}
