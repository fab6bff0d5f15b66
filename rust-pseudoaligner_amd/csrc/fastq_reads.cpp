// pa_process_reads / pa_process_reads_multi, mirroring process_reads (src/pseudoaligner.rs:420-514): FASTQ in, one Rust-Debug-formatted tuple per
// read out, in INPUT order, with the flag rule of :455 as it is (true iff coverage >= 32 and the class is EMPTY). The pipeline over windows of
// raw text is described where it starts, below; the text itself is fastq_text.cpp's.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <cerrno>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <deque>
#include <mutex>
#include <thread>

#include "text_window.hpp"

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
// filled and dropped piece by piece: read_piece), the window goes to HBM as it is on a copy stream, the GPU finds its records (fastq_scan.hip) and the encode /
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
// What those steps do to a window — the pieces into pinned memory, the copies and the inflate, head and scan, the wait with its regrow, the window-size rule,
// the host-scanned batch — is text_window.hpp's (window_fill, window_send, window_enqueue_scan, window_scan_wait, window_rule, host_tail_cut, window_fill_host),
// shared with the paired drivers' WindowFeed. TextPipe is the scheduler: lanes and slots, reads that run behind the caller's back (window_fill without wait:
// the link is the bound and the host's read has no margin), the writer, the copy timer, the lane-serial wait, and the kernels of a window.
constexpr int LANE_SLOTS = 4;            // windows of a lane in flight: read | scan | map + render | write
constexpr uint32_t FLAG_BUCKETS = PA_RENDER_FLAG_BUCKETS;

struct Options {   // every switch the environment has for this driver, read once at the top of a call
    bool bgzf;              // PA_INGEST_BGZF=0 (diagnosis and A/B): a BGZF file is inflated on the host like any other .gz
    uint64_t batch_reads = DEFAULT_BATCH_READS;   // PA_INGEST_BATCH, rounded down to whole tiles of 64 reads; values below 64 are ignored
    uint64_t window;        // bytes of a window the GPU scans (window_from_env: PA_INGEST_WINDOW, clamped by the batch)
    bool verbose;           // PA_VERBOSE
    bool lane_serial;       // PA_LANE_SERIAL (knobs builds: A/B of the one-window-at-a-time rule for lanes that share a GPU)
    bool host_only;         // PA_INGEST_HOST_SCAN (diagnosis: every window through the host's scan)
    bool use_pread;         // PA_INGEST_PREAD (knobs builds: the windows through pread, as before; tools/microbench/host_read.cpp has both side by side)
    Options() {
        const char* v = getenv("PA_INGEST_BGZF");
        bgzf = !(v && *v && atoi(v) == 0);
        if ((v = getenv("PA_INGEST_BATCH"))) { const long long x = atoll(v); if (x >= 64) batch_reads = (uint64_t)x / 64 * 64; }
        window = window_from_env(batch_reads);
        verbose = getenv("PA_VERBOSE") != nullptr;
        lane_serial = knob_int("PA_LANE_SERIAL", 1) != 0;
        host_only = getenv("PA_INGEST_HOST_SCAN") != nullptr;
        use_pread = knob_int("PA_INGEST_PREAD", 0) != 0;
    }
};

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

struct LanePre : Pre {   // a window whose text is being read into its slot, or has been: on this lane
    Lane* l = nullptr;
};

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
    double st[6] = {0, 0, 0, 0, 0, 0};   // the call's stage seconds, by ST_*: the window steps add to the first four
    WindowCtx x{fastq_path, text, pool, st, opt.use_pread};   // the file as the window steps see it: input statistics, rescans, the read-error flag
    uint64_t gpu_wins = 0, host_wins = 0;   // windows whose records the GPU found, batches of the host's scan
    CopyTimer timer{opt.verbose};
    uint64_t W = window_of(text, opt.window);
    const uint64_t KEEP = keep_of(W);
    uint64_t rec_start = 0;     // text offset of the first record no window has taken yet (known once the window before has been scanned)
    uint64_t read_to = 0;       // text read so far
    bool gpu_mode = false;      // windows are still handed to the GPU's scan
    bool have_pending = false;
    Win pending;                // the window whose records the GPU is finding
    LanePre cur, nxt;           // the window being sent and scanned; the one whose text is being read behind it

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

    // the kernels of the window launched before on this lane's stream: waited for (they share the stream's launch context inside the index)
    int finish_lane(Lane& l) {
        if (l.unfinished < 0) return PA_OK;
        for (Win& w : wins)
            if ((int64_t)w.id == l.unfinished) {
                const double t0 = now();
                int e = use(l);
                if (e == PA_OK) e = batch_finish(l.idx, ctx_of(w), l.cache->stream);
                st[ST_WAIT] += now() - t0;
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
            st[ST_TEXT] += now() - t0;
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
        st[ST_PUSH] += now() - t0; t0 = now();
        if ((e = use(l)) != PA_OK) return e;
        c.in_place = true;
        w.first_read = launched_reads;
        c.flag_mark = 1000000 - launched_reads % 1000000;
        if ((e = batch_ensure(l.idx, c, c.n, c.wpr, std::min<uint64_t>(std::max<uint64_t>(c.n + c.n / 8, 1 << 16), std::max<uint64_t>(opt.batch_reads, c.n)))) != PA_OK) return e;
        if ((e = batch_launch(l.idx, c, l.cache->stream)) != PA_OK) return e;
        l.unfinished = (int64_t)w.id;
        w.launched = true;
        launched_reads += c.n;
        st[ST_LAUNCH] += now() - t0;
        return PA_OK;
    }

    // the next window (plan_window: none when the text in front of the host's part has been read) gets its slot, and the pool's workers start to copy its bytes
    // into the slot's pinned memory (window_fill without wait: the read goes on behind this thread's back until send_window asks for it)
    int start_read(LanePre& p, uint64_t id) {
        p.plan = gpu_mode ? plan_window(text, read_to, W, KEEP) : WindowPlan();
        if (!p.plan.active) return PA_OK;
        p.id = id;
        int e = acquire(id, &p.c);
        if (e != PA_OK) return e;
        p.l = &lane_of(id);
        if ((e = window_fill(x, p.plan, *p.c, false)) != PA_OK) return e;
        read_to = p.plan.text_from + p.plan.text_len;
        return PA_OK;
    }

    // the window's bytes, now in pinned memory, go to the GPU on the lane's copy stream (window_send), timed for PA_VERBOSE
    int send_window(const LanePre& p) {
        Lane& l = *p.l;
        const hipStream_t copy = l.cache->copy_stream;
        int e = window_fill_end(x);
        if (e != PA_OK) return e;
        if ((e = use(l)) != PA_OK) return e;
        timer.begin(p.id, copy, p.plan.n_members ? p.plan.comp_len : p.plan.text_len);
        // lanes that share a GPU (a handle listed twice) send their windows one at a time: with two copies of one direction queued at once the runtime
        // runs one of them as a blit kernel, at a fraction of the DMA engine's rate (host_batch.cpp has the measurement)
        for (size_t o = 0; o < lanes.size() && opt.lane_serial; ++o)
            if (&lanes[o] != &l && lanes[o].device == l.device && lanes[o].last_h2d) PA_HIP_TRY(hipStreamWaitEvent(copy, lanes[o].last_h2d, 0));
        if ((e = window_send(x, p.plan, *p.c, copy)) != PA_OK) return e;
        l.last_h2d = p.c->ev_h2d;
        timer.end(p.id, copy);
        return PA_OK;
    }

    // the pending window's scan: waited for (window_scan_wait); its records are launched, the next window's first record is known
    int resolve() {
        Lane& l = lanes[(size_t)pending.lane];
        BatchCtx& c = l.cache->ctx[pending.slot];
        have_pending = false;
        int e = use(l);
        if (e != PA_OK) return e;
        if ((e = window_scan_wait(x, c, l.cache->scan_stream)) != WIN_OK) return e;
        const FqInfo& info = *c.h_info.get();
        // (every read of this driver is encoded whole. The feed has no such line: its consumers refuse a long read where they encode it — WindowFeed::resolve)
        if (info.max_seq > PA_MAX_READ_LEN) return fail(PA_ERR_UNSUPPORTED, "read longer than %u bases", PA_MAX_READ_LEN);
        c.n = info.n;
        c.wpr = pa_words_per_read(info.max_seq ? info.max_seq : 1);
        rec_start = pending.from + info.consumed;
        wins.push_back(pending);
        ++gpu_wins;
        return launch(wins.back());
    }

    // a window is dropped: its text (and what was being read behind it) is read again, from the first record not yet taken — unless the host's scan takes over there
    int reread_from(uint64_t from, bool host) {
        if (nxt.plan.active) { (void)window_fill_end(x); nxt.plan.active = false; }
        (void)hipStreamSynchronize(cur.l->cache->copy_stream);
        read_to = from;
        if (host) gpu_mode = false;
        return start_read(cur, next_id);
    }

    // the window's records are to be found (window_enqueue_scan: head, then the scan behind ev_h2d), and the window is the pending one. WIN_HEAD: it is not
    int enqueue_scan(const LanePre& p) {
        const int r = window_enqueue_scan(x, p.plan, *p.c, rec_start, p.l->cache->scan_stream);
        if (r != WIN_OK) return r;
        pending = win_of(p.id, rec_start);
        have_pending = true;
        next_id = p.id + 1;
        return WIN_OK;
    }

    // ---- windows the GPU scans ----
    // The text of window w + 1 is read (by the pool's workers, asynchronously) while this thread waits for window w - 1's scan, launches its kernels and
    // enqueues window w's scan: the reads follow each other without a gap, and so do the copies to the GPU behind them.
    int gpu_windows_loop() {
        int e = start_read(cur, next_id);
        while (e == PA_OK && cur.plan.active) {
            if ((e = send_window(cur)) != PA_OK) break;
            if ((e = start_read(nxt, cur.id + 1)) != PA_OK) break;      // the next window's text starts to arrive
            int r = WIN_OK;   // what became of the pending window, then of cur
            if (have_pending) {
                r = resolve();
                if (r == WIN_ODD || r == WIN_EMPTY) { rec_start = pending.from; next_id = pending.id; }   // the pending window is dropped, and cur behind it
                else if (r != WIN_OK) { e = r; break; }
            }
            if ((e = use(*cur.l)) != PA_OK) break;
            if (r == WIN_OK && (r = enqueue_scan(cur)) < 0) { e = r; break; }
            if (r != WIN_OK) {   // odd, empty, or cur's head beyond the head room: a longer window from rec_start on, or the host's scan from there
                const WindowRule rule = window_rule(r, W, cur.plan.text_from, rec_start, true);
                W = rule.W;
                e = reread_from(rec_start, rule.host);
                continue;
            }
            if ((e = retire_finished(0)) != PA_OK) break;
            cur = nxt;
            nxt.plan.active = false;
        }
        return e;
    }
    int gpu_windows() {
        gpu_mode = !opt.host_only && text.fsize > KEEP;
        int e = gpu_windows_loop();
        (void)window_fill_end(x);   // (an error path: nothing of the pool's job is left behind)
        gpu_mode = false;
        if (e == PA_OK && have_pending) {   // (no window behind the last one: odd or empty, the rest is the host's)
            const int r = resolve();
            if (r == WIN_ODD || r == WIN_EMPTY) { rec_start = pending.from; next_id = pending.id; }
            else e = r;
        }
        return e;
    }

    // a batch of the host-scanned text: records rp[i0, i1) of ws. Text and records go to the GPU (window_fill_host, window_send_host), the same kernels follow
    int host_batch(const WindowScan& ws, const RecPos* rp, uint64_t i0, uint64_t i1) {
        const uint64_t id = next_id, n = i1 - i0;
        BatchCtx* cp = nullptr;
        int e = acquire(id, &cp);
        if (e != PA_OK) return e;
        BatchCtx& c = *cp;
        uint32_t maxlen = 0;
        if ((e = window_fill_host(x, ws, rp, i0, i1, launched_reads, c, &maxlen)) != PA_OK) return e;
        if (maxlen > PA_MAX_READ_LEN) return fail(PA_ERR_UNSUPPORTED, "read longer than %u bases", PA_MAX_READ_LEN);
        // (the copies ride on the lane's kernel stream: this path is bound by the host's scan, not by the link)
        if ((e = window_send_host(x, c, n, lane_of(id).cache->stream)) != PA_OK) return e;
        c.n = n;
        c.wpr = pa_words_per_read(maxlen ? maxlen : 1);   // (a batch of empty reads still has a word per read)
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
            st[ST_SCAN] += now() - t0;
            if (e != PA_OK || ws.nrec == 0) return e;
            records_before += ws.nrec;
            const RecPos* const rp = hc->rec_pos.data();
            for (uint64_t i0 = 0; i0 < ws.nrec;) {
                const uint64_t i1 = host_tail_cut(rp, ws.nrec, ws.size, i0, opt.batch_reads);
                if ((e = host_batch(ws, rp, i0, i1)) != PA_OK) return e;
                i0 = i1;
            }
        }
    }

    // the end of a call, good or bad (rc): the figures of the call are left for their getters, every stream is waited for, the writer ends, and the lanes' buffers
    // are parked on their handles (or destroyed behind an error, whose message is kept)
    int finish(int rc, const char* out_path) {
        const double all[PA_INGEST_STAGES] = {st[ST_SCAN], st[ST_READ], st[ST_WAIT], st[ST_LAUNCH], st[ST_TEXT], st[ST_PUSH], now() - t_begin, (double)reported};
        memcpy(pa::ingest::last_stage_seconds(), all, sizeof all);
        const InputStats stats = x.final_stats();
        memcpy(last_input_stats(), &stats, sizeof stats);
        if (opt.verbose)
            fprintf(stderr, "\n[pa ingest] %llu reads, %d threads, %d lane(s): %llu windows scanned on the GPU (%llu scanned twice), %llu batches by the host; host scan %.3f s, read %.3f s, wait GPU %.3f s, launch %.3f s, wait text %.3f s, wait writer %.3f s, total %.3f s (before the first window %.3f s)\n",
                    (unsigned long long)reported, pool.size(), L(), (unsigned long long)gpu_wins, (unsigned long long)x.rescans, (unsigned long long)host_wins, st[ST_SCAN], st[ST_READ], st[ST_WAIT],
                    st[ST_LAUNCH], st[ST_TEXT], st[ST_PUSH], now() - t_begin, t_begin - t_enter);
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
    const double t_enter = now();
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

    const double t_begin = now();
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
