// Host ingest pipeline mirroring process_reads (src/pseudoaligner.rs:420-514): FASTQ in, one Rust-Debug-formatted tuple
// per read out, in INPUT order. The reference's per-record mutex around the reader (src/utils.rs:152-157), bounded
// channel (:430,:464) and serial println consumer (:490) become a batch pipeline whose stages overlap:
//
//   scan     the FASTQ file is memory-mapped; all host threads count line breaks in their byte range, then record the
//            start of every 4-line record (no thread ever parses a byte twice, nobody takes a lock)
//   pack     per batch: threads 2-bit pack their reads straight into pinned tiles (the layout the kernel reads)
//   GPU      one stream: tiles H2D -> pa_map_batch_device -> results D2H; runs while the host formats the previous batch
//            and packs the next one
//   format   threads render "(flag, id, [ids], coverage)" (:455-461,:490) into per-thread buffers; classes returned by
//            reference are read from the host copy of the class table
//   write    a writer thread streams the buffers to the output in order
//
// The flag rule of :455 is kept as is (true iff coverage >= 32 and the class is EMPTY).
#include <fcntl.h>
#include <hip/hip_runtime.h>
#include <emmintrin.h>
#include <sys/mman.h>
#include <sys/resource.h>
#include <sys/stat.h>
#include <unistd.h>
#include <zlib.h>

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
#include <functional>
#include <memory>
#include <mutex>
#include <thread>
#include <unordered_set>

#include "ingest.hpp"
#include "pa_common.hpp"

using namespace pa;
using namespace pa::ingest;

namespace {

constexpr uint64_t DEFAULT_BATCH_READS = 2u << 20;   // (4 Mi reads left 1.3 GB of the mapping and 0.23 GB of text to the last, unoverlapped batch: 33 ms of tear-down per 8 M reads against 12)   // PA_INGEST_BATCH overrides (tests exercise the batch seams with small values)


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


const char* line_end(const char* p, const char* end) {
    const char* e = (const char*)memchr(p, '\n', (size_t)(end - p));
    return e ? e : end;
}

// Line breaks, 64 bytes at a time (SSE2, part of every x86-64): FASTQ lines are short — a header, a '+' — and one memchr call per
// line costs more than the bytes it looks at.
inline uint64_t nl_mask64(const char* p) {
    const __m128i nl = _mm_set1_epi8('\n');
    const uint64_t m0 = (uint32_t)_mm_movemask_epi8(_mm_cmpeq_epi8(_mm_loadu_si128((const __m128i*)p), nl));
    const uint64_t m1 = (uint32_t)_mm_movemask_epi8(_mm_cmpeq_epi8(_mm_loadu_si128((const __m128i*)(p + 16)), nl));
    const uint64_t m2 = (uint32_t)_mm_movemask_epi8(_mm_cmpeq_epi8(_mm_loadu_si128((const __m128i*)(p + 32)), nl));
    const uint64_t m3 = (uint32_t)_mm_movemask_epi8(_mm_cmpeq_epi8(_mm_loadu_si128((const __m128i*)(p + 48)), nl));
    return m0 | (m1 << 16) | (m2 << 32) | (m3 << 48);
}
uint64_t count_newlines(const char* d, uint64_t a, uint64_t b) {
    uint64_t c = 0, i = a;
    for (; i + 64 <= b; i += 64) c += (uint64_t)__builtin_popcountll(nl_mask64(d + i));
    for (; i < b; ++i) c += d[i] == '\n';
    return c;
}
// fn(position of a line break) for every line break in [from, to), in order, until fn returns false
template <class F>
void for_each_newline(const char* d, uint64_t from, uint64_t to, F&& fn) {
    uint64_t i = from;
    for (; i + 64 <= to; i += 64)
        for (uint64_t m = nl_mask64(d + i); m; m &= m - 1)
            if (!fn(i + (uint64_t)__builtin_ctzll(m))) return;
    for (; i < to; ++i)
        if (d[i] == '\n' && !fn(i)) return;
}

// The parallel scan finds records by counting lines, four to a record. A file that does not have that shape — sequence or
// qualities wrapped over several lines, which bio's fastq::Reader (the reference's reader) accepts — is first rewritten
// into it by this sequential reader: header line '@...', sequence lines up to the line that starts with '+', then as many
// quality lines as there were sequence lines (what bio 1.5's Reader::read does). Returns false (with the 0-based record
// number) when the text is no FASTQ at all; trailing blank lines are tolerated as everywhere in this file.
bool normalize_fastq(const char* d, uint64_t n, std::vector<char>& out, uint64_t& bad_rec) {
    out.clear();
    out.reserve(n + 16);
    const char* p = d;
    const char* const end = d + n;
    auto next_line = [&](const char*& b, const char*& e) -> bool {   // [b, e) without the line break; false at the end of the text
        if (p >= end) return false;
        b = p;
        const char* nl = (const char*)memchr(p, '\n', (size_t)(end - p));
        e = nl ? nl : end;
        p = nl ? nl + 1 : end;
        if (e > b && e[-1] == '\r') --e;
        return true;
    };
    uint64_t rec = 0;
    const char *b, *e;
    for (;;) {
        if (!next_line(b, e)) return true;
        if (b == e) {   // blank line: fine only if nothing but blank lines follows
            while (next_line(b, e))
                if (b != e) { bad_rec = rec; return false; }
            return true;
        }
        if (*b != '@') { bad_rec = rec; return false; }
        out.insert(out.end(), b, e);
        out.push_back('\n');
        uint64_t seq_lines = 0;
        bool plus = false;
        while (next_line(b, e)) {
            if (b != e && *b == '+') { plus = true; break; }
            out.insert(out.end(), b, e);
            ++seq_lines;
        }
        if (!plus) { bad_rec = rec; return false; }   // the text ends inside a record
        out.push_back('\n');
        out.push_back('+');
        out.push_back('\n');
        for (uint64_t i = 0; i < seq_lines; ++i) {
            if (!next_line(b, e)) break;   // (bio leaves the qualities short; the reference never looks at them)
            out.insert(out.end(), b, e);
        }
        out.push_back('\n');
        ++rec;
    }
}

struct FastqText {   // the text of a FASTQ file as the scan sees it: the mapped file, an inflated gzip stream, or the rewritten records
    const char* data = nullptr;
    uint64_t fsize = 0;
    bool mapped = false;
    std::vector<char> inflated;     // a gzip'ed FASTQ (utils::open_with_gz, src/utils.rs:45-57) is inflated into memory first
    std::vector<char> normalized;   // the text rewritten into four-line records, if it did not have that shape
    uint64_t off = 0;               // text before this offset has been handed out as records (windowed scan of pa_process_reads)
    const char* map_base = nullptr; // the mapping as mmap returned it (data moves on when the rest of a file is rewritten)
    uint64_t map_size = 0;
    int fd = -1;                    // of a mapped file (kept open for the call)
    void release() {
        if (mapped) munmap((void*)map_base, map_size);   // (the whole mapping: nobody gives parts of it back any more)
        if (fd >= 0) close(fd);
        fd = -1;
        mapped = false;
        data = nullptr;
        fsize = 0;
    }
};

int open_fastq(const char* fastq_path, FastqText& t) {
    const char*& data = t.data;
    uint64_t& fsize = t.fsize;
    bool& mapped = t.mapped;
    std::vector<char>& inflated = t.inflated;
    // ---- map the file ----
    const int fd = open(fastq_path, O_RDONLY);
    if (fd < 0) return fail(PA_ERR_IO, "cannot open %s: %s", fastq_path, strerror(errno));
    struct stat st;
    if (fstat(fd, &st) != 0) { close(fd); return fail(PA_ERR_IO, "cannot stat %s: %s", fastq_path, strerror(errno)); }
    fsize = (uint64_t)st.st_size;
    unsigned char magic[2] = {0, 0};
    const bool gz = fsize >= 2 && pread(fd, magic, 2, 0) == 2 && magic[0] == 0x1f && magic[1] == 0x8b;
    if (gz) {
        gzFile g = gzdopen(dup(fd), "rb");   // every member of a multi-member file, like flate2's MultiGzDecoder
        if (!g) { close(fd); return fail(PA_ERR_IO, "cannot read %s as gzip", fastq_path); }
        (void)gzbuffer(g, 1 << 20);
        inflated.resize(std::max<uint64_t>(fsize * 4, 1 << 20));
        uint64_t have = 0;
        for (;;) {
            if (have == inflated.size()) inflated.resize(inflated.size() * 2);
            const int got = gzread(g, inflated.data() + have, (unsigned)std::min<uint64_t>(inflated.size() - have, 1u << 30));
            if (got < 0) { int e = 0; const char* why = gzerror(g, &e); gzclose(g); close(fd); return fail(PA_ERR_FORMAT, "%s: corrupt gzip stream: %s", fastq_path, why); }
            if (got == 0) break;
            have += (uint64_t)got;
        }
        {
            int e = Z_OK;
            const char* why = gzerror(g, &e);   // a truncated member hands out what it has and reports Z_BUF_ERROR
            if (e != Z_OK && e != Z_STREAM_END) { const int rc_ = fail(PA_ERR_FORMAT, "%s: corrupt gzip stream: %s", fastq_path, why); gzclose(g); close(fd); return rc_; }
        }
        gzclose(g);
        fsize = have;
        data = inflated.data();
    } else if (fsize) {
        void* m = mmap(nullptr, fsize, PROT_READ, MAP_PRIVATE, fd, 0);
        if (m == MAP_FAILED) { close(fd); return fail(PA_ERR_IO, "cannot map %s: %s", fastq_path, strerror(errno)); }
        (void)madvise(m, fsize, MADV_SEQUENTIAL);
        data = (const char*)m;
        mapped = true;
        t.map_base = data;
        t.map_size = fsize;
        t.fd = fd;
        return PA_OK;
    }
    close(fd);
    return PA_OK;
}

constexpr int SCAN_NOT_FOUR_LINE = 1, SCAN_WINDOW_TOO_SMALL = 2;   // (what a window's scan may answer besides a pa_status)

// Records of the text t.data[t.off, t.off + avail): line breaks per byte range, then what every line is (scan of pa_process_reads;
// pa_fastq_scan_host runs it alone, over the whole text). rec_pos[i] = where record i lies, counted from t.data + t.off.
//   last   the text ends with these bytes: trailing blank lines are tolerated, a last record may lack its quality line, and a text that
//          is not in four-line shape is rewritten once (t.data / t.fsize / t.off then describe the rewritten text) and scanned again
//   !last  a WINDOW of a longer text: only whole records are taken, *consumed = the bytes they are (the next window starts behind them).
//          SCAN_NOT_FOUR_LINE: a record of the window lacks its '@' or '+' — the caller scans the rest of the file as one text;
//          SCAN_WINDOW_TOO_SMALL: the window holds no whole record
// rec_base: records before this text (error messages count records from the file's first).
int scan_fastq(const char* fastq_path, FastqText& t, uint64_t avail, bool last, uint64_t rec_base, Pool& pool, std::vector<RecPos>& rec_pos, uint64_t& nrec,
               std::vector<std::vector<uint32_t>>& brk, uint64_t* consumed) {
    bool& mapped = t.mapped;
    std::vector<char>& inflated = t.inflated;
    std::vector<char>& normalized = t.normalized;
    const int T = pool.size();
    int rc = PA_OK;
    nrec = 0;
    if (consumed) *consumed = 0;
    // ---- scan: line breaks per byte range, then the start of every fourth line ----
    for (int attempt = 0; attempt < 2; ++attempt) {
        const char* const data = t.data + t.off;
        const uint64_t fsize = attempt == 0 ? avail : t.fsize - t.off;
        std::atomic<uint64_t> odd_record{~0ull};   // first record whose first line lacks the '@' or whose third the '+'
        rc = PA_OK;
        // ONE pass over the text: every range notes where its line breaks are (32-bit offsets from the range's start: ranges are
        // kept below 2 GiB); what every line is follows from these lists alone, once the prefix sum has given each range its first
        // line number (a second pass over the text cost as much as the first: 2.5 GB per 8 M reads)
        const int R = (int)std::min<uint64_t>(std::max<uint64_t>((uint64_t)T * 4, fsize / (1ull << 30) + 1), fsize / (1 << 16) + 1);
        std::vector<uint64_t> nl((size_t)R + 1, 0);
        if (brk.size() < (size_t)R) brk.resize((size_t)R);   // (the caller keeps the lists between calls: 128 MB per 8 M reads that would otherwise be paged in again)
        auto range = [&](int r, uint64_t& a, uint64_t& b) { a = fsize * (uint64_t)r / R; b = fsize * (uint64_t)(r + 1) / R; };
        pool.run(R, [&](int r) {
            uint64_t a, b;
            range(r, a, b);
#ifdef MADV_POPULATE_READ
            // a fresh mapping of a file in the page cache costs a minor fault per 4 KiB page on first touch (0.6 M of them for 8 M reads):
            // let the kernel fill this range's page table entries in one call instead (Linux >= 5.14; elsewhere the faults simply happen)
            if (mapped && attempt == 0) {
                const uint64_t pa_ = (uint64_t)(data + a - t.map_base) & ~4095ull;   // (page-aligned in the mapping)
                (void)madvise((void*)(t.map_base + pa_), (size_t)((uint64_t)(data + b - t.map_base) - pa_), MADV_POPULATE_READ);
            }
#endif
            std::vector<uint32_t>& v = brk[(size_t)r];
            v.clear();
            v.reserve((size_t)((b - a) / 64 + 16));   // (FASTQ of 150-base reads: one line break per ~79 bytes)
            for_each_newline(data, a, b, [&](uint64_t e) { v.push_back((uint32_t)(e - a)); return true; });
            nl[(size_t)r + 1] = v.size();
        });
        for (int r = 0; r < R; ++r) nl[(size_t)r + 1] += nl[(size_t)r];
        uint64_t content_lines = 0;
        if (!last) {   // a window: the whole records among its lines; the next window starts behind their last line break
            nrec = nl[(size_t)R] / 4;
            if (nrec == 0) return SCAN_WINDOW_TOO_SMALL;
            content_lines = 4 * nrec;
            int r = 0;
            while (nl[(size_t)r + 1] < content_lines) ++r;
            uint64_t a, b;
            range(r, a, b);
            *consumed = a + brk[(size_t)r][(size_t)(content_lines - 1 - nl[(size_t)r])] + 1;
        } else {
        // trailing empty lines are tolerated: lines = line breaks before the last content byte + 1
        uint64_t tail = fsize, trailing_nl = 0;
        while (tail > 0 && (data[tail - 1] == '\n' || data[tail - 1] == '\r')) { trailing_nl += data[tail - 1] == '\n'; --tail; }
        content_lines = tail ? nl[(size_t)R] - trailing_nl + 1 : 0;
        if (content_lines % 4 == 3) {
            // a last record with an EMPTY sequence: its empty quality line looks like a trailing blank line (or is missing
            // altogether when the file ends after the '+'; bio's reader reads nothing there and hands the record out). Taken as
            // that record when the text ends "...\n<empty line>\n+..."
            uint64_t ls = tail;                                            // start of the last content line
            while (ls > 0 && data[ls - 1] != '\n') --ls;
            if (data[ls] == '+' && ls >= 2) {
                uint64_t pe = ls - 1;                                      // the line break that ends the sequence line
                if (pe > 0 && data[pe - 1] == '\r') --pe;
                if (pe > 0 && data[pe - 1] == '\n') content_lines += 1;    // the sequence line is empty
            }
        }
        if (content_lines % 4 != 0)
            rc = fail(PA_ERR_FORMAT, "%s: malformed FASTQ record %llu (file ends inside a record)", fastq_path, (unsigned long long)(rec_base + content_lines / 4));
        nrec = content_lines / 4;
        if (consumed) *consumed = fsize;
        }
        if (rc == PA_OK && nrec) {
            rec_pos.resize(nrec);   // (every field is written below: each line starts in exactly one range)
            RecPos* const rp = rec_pos.data();
            pool.run(R, [&](int r) {
                uint64_t a, b;
                range(r, a, b);
                auto odd = [&](uint64_t rec) {
                    uint64_t cur = odd_record.load();
                    while (rec < cur && !odd_record.compare_exchange_weak(cur, rec)) {}
                };
                // line li = bytes [p, e) (e = its line break, or the end of the text)
                auto line = [&](uint64_t p, uint64_t e, uint64_t li) {
                    const uint64_t rec = li >> 2;
                    if (rec >= nrec) return;
                    switch (li & 3) {
                        case 0: {
                            rp[rec].start = p;
                            rp[rec].hdr = (uint32_t)std::min<uint64_t>(e - p, 0xFFFFFFFFull);
                            if (data[p] != '@') odd(rec);
                            // record.id() (:456) = header[1..].trim_end().splitn(2, ' ').next() in bio 1.5: cut at the first SPACE only (a tab stays
                            // part of the id), after trailing white space was trimmed. Found here, while the header's bytes are in the cache
                            uint64_t hend = e, ide = p + 1;
                            while (hend > p + 1 && (data[hend - 1] == '\r' || data[hend - 1] == ' ' || data[hend - 1] == '\t' || data[hend - 1] == '\n')) --hend;
                            while (ide < hend && data[ide] != ' ') ++ide;
                            rp[rec].id_len = e > p ? (uint32_t)std::min<uint64_t>(ide - (p + 1), 0xFFFFFFFFull) : 0u;
                            break;
                        }
                        case 1: {
                            const uint64_t len = e - p;
                            rp[rec].seq = (uint32_t)std::min<uint64_t>(len, 0xFFFFFFFFull);
                            rp[rec].seq_len = (uint32_t)std::min<uint64_t>(len && data[e - 1] == '\r' ? len - 1 : len, 0xFFFFFFFFull);
                            break;
                        }
                        case 2: if (data[p] != '+') odd(rec); break;
                        default: break;
                    }
                };
                // the lines that START in [a, b): the first one begins after the first line break at or after a - 1. Their ends are
                // this range's line breaks and, for the last of them, the first line break of the ranges behind it
                uint64_t li = nl[(size_t)r], p = a;
                bool started = a == 0 || data[a - 1] == '\n';
                if (!started) li += 1;   // (the line break that ends the straddling line is counted in this range or a later one)
                bool open = true;        // a line that started in this range still waits for its end
                for (int q = r; q < R && open; ++q) {
                    uint64_t qa, qb;
                    range(q, qa, qb);
                    for (const uint32_t rel : brk[(size_t)q]) {
                        const uint64_t e = qa + rel;
                        if (!started) { started = true; p = e + 1; if (p >= b) { open = false; break; } continue; }
                        line(p, e, li);
                        p = e + 1;
                        ++li;
                        if (p >= b) { open = false; break; }
                    }
                }
                if (open && started && p < b && p < fsize) line(p, fsize, li);   // a last line without a line break
            });
        }
        if (rc == PA_OK && odd_record.load() == ~0ull) break;   // four lines to a record, markers in place
        if (!last) return SCAN_NOT_FOUR_LINE;
        if (attempt == 1) {
            if (rc == PA_OK) rc = fail(PA_ERR_FORMAT, "%s: malformed FASTQ record %llu", fastq_path, (unsigned long long)(rec_base + odd_record.load()));
            break;
        }
        // not that shape: wrapped sequence / quality lines? rewrite and scan again
        uint64_t bad = 0;
        std::vector<char> rewritten;
        if (!normalize_fastq(data, fsize, rewritten, bad)) {
            rc = fail(PA_ERR_FORMAT, "%s: malformed FASTQ record %llu (no '@' header, or the file ends inside the record)", fastq_path, (unsigned long long)(rec_base + bad));
            break;
        }
        t.release();   // (the mapping, if the text was one)
        inflated = std::vector<char>();
        normalized.swap(rewritten);
        t.data = normalized.data();
        t.fsize = normalized.size();
        t.off = 0;
        nrec = 0;
    }

    return rc;
}

// The text in WINDOWS: a mapped file is scanned a window at a time (PA_INGEST_WINDOW bytes), so that pa_process_reads has its first batch on
// the GPU while the rest of the file is still being scanned; a window ends behind its last whole record. A text held in memory (gzip), a
// window that is not in four-line shape (then: the rest of the file as one text, rewritten) and the last window are scanned as one text.
struct WindowScan {
    FastqText& text;
    uint64_t window = 256ull << 20;
    bool windowed, done = false;
    uint64_t nrec = 0;            // records of the current window
    const char* base = nullptr;   // the window's text: rec_pos counts from here
    uint64_t size = 0;            // its bytes
    uint64_t abs = ~0ull;         // its offset in the file's mapping (~0: not part of one)
    explicit WindowScan(FastqText& t) : text(t), windowed(t.mapped) {
        if (const char* v = getenv("PA_INGEST_WINDOW")) { const long long x = atoll(v); if (x >= 1) window = (uint64_t)x; }
    }
    // the next window with records in it (nrec = 0: the text has ended). records_before: records of the windows before (error messages)
    int next(const char* fastq_path, uint64_t records_before, Pool& pool, std::vector<RecPos>& rec_pos, std::vector<std::vector<uint32_t>>& brk) {
        nrec = 0;
        while (!done) {
            const uint64_t rest = text.fsize - text.off;
            if (rest == 0) { done = true; break; }
            const uint64_t avail = windowed ? std::min<uint64_t>(window, rest) : rest;
            const bool last = avail == rest;
            uint64_t consumed = 0;
            const int r = scan_fastq(fastq_path, text, avail, last, records_before, pool, rec_pos, nrec, brk, &consumed);
            if (r == SCAN_WINDOW_TOO_SMALL) { window *= 2; continue; }   // (a record longer than the window)
            if (r == SCAN_NOT_FOUR_LINE) { windowed = false; continue; }
            if (r != PA_OK) return r;
            base = text.data + text.off;
            size = consumed;
            abs = text.mapped ? (uint64_t)(base - text.map_base) : ~0ull;
            text.off += consumed;
            if (last) done = true;
            if (nrec) break;
        }
        return PA_OK;
    }
};

}  // namespace

// The scan stage of pa_process_reads by itself (no GPU): how many records the text holds and where their header and sequence
// lines lie. Offsets refer to the text as scanned: the file itself (*text_kind 0), the inflated gzip stream (1) or the text
// rewritten into four-line records (2, wrapped input).
extern "C" int pa_fastq_scan_host(const char* fastq_path, int num_threads, uint64_t* n_records, uint64_t* starts, uint32_t* header_len,
                                  uint32_t* seq_len, uint64_t capacity, int* text_kind) {
    if (!fastq_path || !n_records) return fail(PA_ERR_INVALID_ARG, "null argument");
    *n_records = 0;
    FastqText text;
    int rc = open_fastq(fastq_path, text);
    if (rc != PA_OK) return rc;
    const bool was_gz = !text.mapped && text.fsize != 0;
    Pool pool(num_threads < 1 ? 1 : num_threads);
    std::vector<RecPos> rec_pos;
    std::vector<std::vector<uint32_t>> brk;
    // window by window, as pa_process_reads walks the text. Offsets refer to the text the LAST window was part of: when a window turns out
    // not to be in four-line shape the rest of the file is rewritten, and records from there on lie in the rewritten text (*text_kind 2)
    uint64_t nrec = 0;
    WindowScan ws(text);
    while (rc == PA_OK) {
        rc = ws.next(fastq_path, nrec, pool, rec_pos, brk);
        if (rc != PA_OK || ws.nrec == 0) break;
        const uint64_t at = (uint64_t)(ws.base - text.data);   // of the window in the text it belongs to
        for (uint64_t i = 0; i < ws.nrec && nrec + i < capacity; ++i) {
            if (starts) starts[nrec + i] = at + rec_pos[i].start;
            if (header_len) header_len[nrec + i] = rec_pos[i].hdr;
            if (seq_len) seq_len[nrec + i] = rec_pos[i].seq_len;   // a CR before the line break is not sequence
        }
        nrec += ws.nrec;
    }
    if (rc == PA_OK) {
        *n_records = nrec;
        if (text_kind) *text_kind = !text.normalized.empty() ? 2 : was_gz ? 1 : 0;
    }
    text.release();
    return rc;
}

namespace {

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
constexpr int LANE_SLOTS = 4;            // windows of a lane in flight: read | scan | map + render | write
constexpr uint32_t FLAG_BUCKETS = PA_RENDER_FLAG_BUCKETS;

struct Lane {
    pa_index* idx = nullptr;
    int device = 0;
    IngestCache* cache = nullptr;
    hipStream_t stream = nullptr, copy = nullptr, scan = nullptr, back = nullptr;
    hipEvent_t last_h2d = nullptr;       // behind the lane's last window copy (an event of one of its slots)
    int64_t unfinished = -1;             // the window whose kernels were launched last on `stream` and have not been waited for
    uint64_t text_job[LANE_SLOTS] = {0, 0, 0, 0};   // the writer's job that reads the slot's pinned text (0: none)
};

struct Win {
    uint64_t id = 0;
    int lane = 0, slot = 0;
    uint64_t from = 0;          // text offset of its first record
    uint64_t first_read = 0;    // number of the reads before it
    bool launched = false;      // its kernels are on the lane's stream
};

struct TextPipe {
    const char* fastq_path;
    FastqText& text;
    Pool& pool;
    Writer& writer;
    std::vector<Lane>& lanes;
    uint64_t batch_reads;
    std::deque<Win> wins;       // launched or about to be, in order; the front is written first
    uint64_t next_id = 0, launched_reads = 0, reported = 0, flagged = 0, next_report = 1000000;
    double t_scan = 0, t_read = 0, t_wait = 0, t_launch = 0, t_text = 0, t_push = 0;
    uint64_t gpu_windows = 0, host_windows = 0, rescans = 0;

    static double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
    int L() const { return (int)lanes.size(); }
    Lane& lane_of(uint64_t id) { return lanes[(size_t)(id % (uint64_t)L())]; }
    int slot_of(uint64_t id) const { return (int)((id / (uint64_t)L()) % LANE_SLOTS); }
    BatchCtx& ctx_of(const Win& w) { return lanes[(size_t)w.lane].cache->ctx[w.slot]; }
    int use(const Lane& l) { return hipSetDevice(l.device) == hipSuccess ? PA_OK : fail(PA_ERR_HIP, "hipSetDevice(%d) failed", l.device); }

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
    bool use_pread = false;   // (knobs builds: the windows through pread, as before; tools/microbench/host_read.cpp has both side by side)
    void read_piece(uint64_t off, uint64_t len, uint8_t* dst, int t, int ntask) {
        const uint64_t a = off + len * (uint64_t)t / (uint64_t)ntask, b = off + len * (uint64_t)(t + 1) / (uint64_t)ntask;
        if (text.mapped && text.data == text.map_base && !use_pread) {
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
            copy_streaming(dst + (a - off), (const uint8_t*)text.data + a, (size_t)(b - a));
            if (big) {
                const uint64_t qa = (a + PAGE - 1) & ~(PAGE - 1), qb = b & ~(PAGE - 1);
                if (qb > qa) (void)madvise((void*)(text.map_base + qa), (size_t)(qb - qa), MADV_DONTNEED);
            }
        } else if (text.mapped && text.fd >= 0 && text.data == text.map_base) {
            uint64_t p = a;
            while (p < b) {
                const ssize_t got = pread(text.fd, dst + (p - off), (size_t)(b - p), (off_t)p);
                if (got < 0 && errno == EINTR) continue;
                if (got <= 0) { read_bad.store(1); return; }
                p += (uint64_t)got;
            }
        } else memcpy(dst + (a - off), text.data + a, (size_t)(b - a));
    }
    void read_begin(uint64_t off, uint64_t len, uint8_t* dst) {
        read_async = false;
        if (len == 0) return;
        const uint64_t PIECE = 2ull << 20;
        const int ntask = (int)std::min<uint64_t>((len + PIECE - 1) / PIECE, 1u << 20);
        if (ntask == 1) { read_piece(off, len, dst, 0, 1); return; }
        read_async = true;
        pool.begin(ntask, [this, off, len, dst, ntask](int t) { read_piece(off, len, dst, t, ntask); });
    }
    int read_end() {
        if (read_async) { pool.end(); read_async = false; }
        return read_bad.exchange(0) ? fail(PA_ERR_IO, "%s: read failed: %s", fastq_path, strerror(errno)) : PA_OK;
    }
    int read_text(uint64_t off, uint64_t len, uint8_t* dst) {
        read_begin(off, len, dst);
        return read_end();
    }
    int read_small(uint64_t off, uint64_t len, uint8_t* dst) {   // by the caller itself, whatever the pool is doing (a window's head: <= 1 MiB)
        if (len) read_piece(off, len, dst, 0, 1);
        return read_bad.load() ? fail(PA_ERR_IO, "%s: read failed: %s", fastq_path, strerror(errno)) : PA_OK;
    }

    // the kernels of the window launched before on this lane's stream: waited for (they share the stream's launch context inside the index)
    int finish_lane(Lane& l) {
        if (l.unfinished < 0) return PA_OK;
        for (Win& w : wins)
            if ((int64_t)w.id == l.unfinished) {
                const double t0 = now();
                int e = use(l);
                if (e == PA_OK) e = batch_finish(l.idx, ctx_of(w), l.stream);
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
        c.back = l.back;
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
        if ((e = batch_ensure(l.idx, c, c.n, c.wpr, std::min<uint64_t>(std::max<uint64_t>(c.n + c.n / 8, 1 << 16), std::max<uint64_t>(batch_reads, c.n)))) != PA_OK) return e;
        if ((e = batch_launch(l.idx, c, l.stream)) != PA_OK) return e;
        l.unfinished = (int64_t)w.id;
        w.launched = true;
        launched_reads += c.n;
        t_launch += now() - t0;
        return PA_OK;
    }
};

constexpr int WIN_OK = 0, WIN_ODD = 1, WIN_EMPTY = 2;

int process_reads_impl(pa_index* const* idxs, int nidx, const char* fastq_path, const char* out_path, int num_threads, uint64_t* n_reads_out, uint64_t* n_flagged_out) {
    if (!idxs || nidx < 1 || !fastq_path || !out_path) return fail(PA_ERR_INVALID_ARG, "null argument");
    for (int i = 0; i < nidx; ++i)
        if (!idxs[i]) return fail(PA_ERR_INVALID_ARG, "null index handle");
    const double t_enter = TextPipe::now();
    if (num_threads < 1) num_threads = 1;
    if (n_reads_out) *n_reads_out = 0;
    if (n_flagged_out) *n_flagged_out = 0;
    {
        pa_index_stats s0, si;
        if (pa_index_get_stats(idxs[0], &s0) != PA_OK) return PA_ERR_INVALID_ARG;
        for (int i = 1; i < nidx; ++i) {
            if (pa_index_get_stats(idxs[i], &si) != PA_OK) return PA_ERR_INVALID_ARG;
            if (si.k != s0.k || si.num_nodes != s0.num_nodes || si.num_classes != s0.num_classes || si.num_kmers != s0.num_kmers)
                return fail(PA_ERR_INVALID_ARG, "handle %d is not a replica of handle 0 (k / nodes / classes / k-mers differ)", i);
        }
    }

    FastqText text;
    {
        const int orc = open_fastq(fastq_path, text);
        if (orc != PA_OK) return orc;
    }
    FILE* out = strcmp(out_path, "-") == 0 ? stdout : fopen(out_path, "wb");
    if (!out) { text.release(); return fail(PA_ERR_IO, "cannot create %s: %s", out_path, strerror(errno)); }
    // a private 4 MiB stdio buffer only for a file this function opened (and closes before the buffer dies); the process-wide
    // stdout keeps its own buffering: handing it a function-local buffer would leave it dangling after the return
    std::vector<char> obuf(out != stdout ? (size_t)1 << 22 : 0);
    if (out != stdout) setvbuf(out, obuf.data(), _IOFBF, obuf.size());

    uint64_t BATCH_READS = DEFAULT_BATCH_READS;
    if (const char* v = getenv("PA_INGEST_BATCH")) { const long long x = atoll(v); if (x >= 64) BATCH_READS = (uint64_t)x / 64 * 64; }
    uint64_t W = 64ull << 20;   // bytes of a window the GPU scans (64 MiB: 128 MiB leaves more of the first read and the last kernels unoverlapped, 16 MiB costs launches) (PA_INGEST_WINDOW; never more than 256 bytes per read of a batch: the tests' small batches give small windows)
    if (const char* v = getenv("PA_INGEST_WINDOW")) { const long long x = atoll(v); if (x >= 1) W = (uint64_t)x; }
    W = std::min<uint64_t>(std::min<uint64_t>(W, BATCH_READS * 256), 1ull << 31);
    const bool verbose = getenv("PA_VERBOSE") != nullptr;
    const bool lane_serial = knob_int("PA_LANE_SERIAL", 1) != 0;   // (knobs builds: A/B of the one-window-at-a-time rule for lanes that share a GPU)
    const bool host_only = getenv("PA_INGEST_HOST_SCAN") != nullptr;   // (diagnosis: every window through the host's scan)
    const double t_begin = TextPipe::now();
    Pool pool(num_threads);
    int rc = PA_OK;

    // ---- lanes: one per handle; buffers and streams of an earlier call are taken from the handle ----
    std::vector<Lane> lanes((size_t)nidx);
    for (int i = 0; i < nidx && rc == PA_OK; ++i) {
        Lane& l = lanes[(size_t)i];
        l.idx = idxs[i];
        const uint32_t *h_ec = nullptr, *h_class_ref = nullptr;
        index_host_classes(l.idx, &h_ec, &h_class_ref, &l.device);
        if (hipSetDevice(l.device) != hipSuccess) { rc = fail(PA_ERR_HIP, "hipSetDevice(%d) failed", l.device); break; }
        l.cache = static_cast<IngestCache*>(index_take_ingest_cache(l.idx));
        if (!l.cache) l.cache = new IngestCache();
        l.cache->idx = l.idx;
        if (!l.cache->stream && hipStreamCreateWithFlags(&l.cache->stream, hipStreamNonBlocking) != hipSuccess) { l.cache->stream = nullptr; rc = fail(PA_ERR_HIP, "hipStreamCreate failed"); break; }
        if (!l.cache->copy_stream && hipStreamCreateWithFlags(&l.cache->copy_stream, hipStreamNonBlocking) != hipSuccess) { l.cache->copy_stream = nullptr; rc = fail(PA_ERR_HIP, "hipStreamCreate failed"); break; }
        for (hipStream_t* sp : {&l.cache->scan_stream, &l.cache->back_stream})
            if (rc == PA_OK && !*sp && hipStreamCreateWithFlags(sp, hipStreamNonBlocking) != hipSuccess) { *sp = nullptr; rc = fail(PA_ERR_HIP, "hipStreamCreate failed"); }
        if (rc != PA_OK) break;
        l.stream = l.cache->stream;
        l.copy = l.cache->copy_stream;
        l.scan = l.cache->scan_stream;
        l.back = l.cache->back_stream;
    }

    Writer writer(out);
    TextPipe tp{fastq_path, text, pool, writer, lanes, BATCH_READS};
    tp.use_pread = knob_int("PA_INGEST_PREAD", 0) != 0;
    const uint64_t fsize0 = text.fsize;
    const uint64_t KEEP = std::max<uint64_t>(4096, std::min<uint64_t>(W / 4, 1ull << 20));   // the end of the text is the host's: its rules for the last record live there
    uint64_t rec_start = 0;   // text offset of the first record no window has taken yet (known once the window before has been scanned)
    uint64_t read_to = 0;     // text read so far
    bool gpu_mode = rc == PA_OK && !host_only && fsize0 > KEEP;
    bool have_pending = false;
    Win pending;              // the window whose records the GPU is finding
    hipEvent_t vt0[8] = {nullptr}, vt1[8] = {nullptr};   // PA_VERBOSE: how long the windows' copies to the GPU took (eight windows back)
    uint64_t vbytes[8] = {0};
    double v_h2d_ms = 0, v_h2d_bytes = 0;

    // the pending window's scan: waited for; its records are launched, the next window's first record is known
    auto resolve = [&]() -> int {
        Lane& l = lanes[(size_t)pending.lane];
        BatchCtx& c = l.cache->ctx[pending.slot];
        have_pending = false;
        int e = tp.use(l);
        if (e != PA_OK) return e;
        for (int attempt = 0;; ++attempt) {
            const double t0 = TextPipe::now();
            if (hipEventSynchronize(c.ev_info) != hipSuccess) return fail(PA_ERR_HIP, "waiting for the FASTQ scan failed");
            tp.t_wait += TextPipe::now() - t0;
            if (!c.h_info.get()->overflow) break;
            if (attempt == 2) return fail(PA_ERR_INTERNAL, "FASTQ scan: line table too small after regrowing");
            ++tp.rescans;   // more lines than guessed (short reads): grow the line table, fill it again from the counts already there
            if ((e = window_ensure_scan(c, c.h_info.get()->lines)) != PA_OK) return e;
            if ((e = window_scan_enqueue(c, true, l.scan)) != PA_OK) return e;
        }
        if (c.h_info.get()->odd) return WIN_ODD;
        if (c.h_info.get()->n == 0) return WIN_EMPTY;
        if (c.h_info.get()->max_seq > PA_MAX_READ_LEN) return fail(PA_ERR_UNSUPPORTED, "read longer than %u bases", PA_MAX_READ_LEN);
        c.n = c.h_info.get()->n;
        c.wpr = pa_words_per_read(c.h_info.get()->max_seq ? c.h_info.get()->max_seq : 1);
        rec_start = pending.from + c.h_info.get()->consumed;
        tp.wins.push_back(pending);
        ++tp.gpu_windows;
        return tp.launch(tp.wins.back());
    };

    try {
    // ---- windows the GPU scans ----
    // The text of window w + 1 is read (by the pool's workers, asynchronously) while this thread waits for window w - 1's scan, launches its kernels and
    // enqueues window w's scan: the reads follow each other without a gap, and so do the copies to the GPU behind them.
    struct Pre { bool active = false; uint64_t id = 0, main_from = 0, main_len = 0; BatchCtx* c = nullptr; Lane* l = nullptr; };
    auto start_read = [&](Pre& p, uint64_t id) -> int {
        p.active = false;
        if (!gpu_mode || read_to + KEEP >= text.fsize) return PA_OK;
        p.main_len = std::min<uint64_t>(W, text.fsize - KEEP - read_to);
        p.main_from = read_to;
        p.id = id;
        int e = tp.acquire(id, &p.c);
        if (e != PA_OK) return e;
        p.l = &tp.lane_of(id);
        if ((e = window_ensure_raw(*p.c, WINDOW_HEAD_ROOM + p.main_len)) != PA_OK) return e;
        tp.read_begin(read_to, p.main_len, p.c->h_raw.get() + WINDOW_HEAD_ROOM);
        read_to += p.main_len;
        p.active = true;
        return PA_OK;
    };
    Pre cur, nxt;
    if (rc == PA_OK) rc = start_read(cur, tp.next_id);
    while (rc == PA_OK && cur.active) {
        const uint64_t id = cur.id, main_len = cur.main_len, main_from = cur.main_from;
        BatchCtx& c = *cur.c;
        Lane& l = *cur.l;
        double t0 = TextPipe::now();
        if ((rc = tp.read_end()) != PA_OK) break;                       // this window's text is in pinned memory
        tp.t_read += TextPipe::now() - t0;
        if ((rc = tp.use(l)) != PA_OK) break;
        if (verbose) {
            if (!vt0[id % 8]) { (void)hipEventCreate(&vt0[id % 8]); (void)hipEventCreate(&vt1[id % 8]); }
            else { float ms = 0; if (hipEventElapsedTime(&ms, vt0[id % 8], vt1[id % 8]) == hipSuccess) { v_h2d_ms += ms; v_h2d_bytes += vbytes[id % 8]; } }
            (void)hipEventRecord(vt0[id % 8], l.copy);
            vbytes[id % 8] = main_len;
        }
        // lanes that share a GPU (a handle listed twice) send their windows one at a time: with two copies of one direction queued at once the runtime
        // runs one of them as a blit kernel, at a fraction of the DMA engine's rate (host_batch.cpp has the measurement)
        for (size_t o = 0; o < lanes.size() && lane_serial; ++o)
            if (&lanes[o] != &l && lanes[o].device == l.device && lanes[o].last_h2d && hipStreamWaitEvent(l.copy, lanes[o].last_h2d, 0) != hipSuccess) { rc = fail(PA_ERR_HIP, "hipStreamWaitEvent failed"); break; }
        if (rc != PA_OK) break;
        if (hipMemcpyAsync(c.d_raw.get() + WINDOW_HEAD_ROOM, c.h_raw.get() + WINDOW_HEAD_ROOM, main_len, hipMemcpyHostToDevice, l.copy) != hipSuccess ||
            hipEventRecord(c.ev_h2d, l.copy) != hipSuccess) { rc = fail(PA_ERR_HIP, "copy of a text window to the GPU failed"); break; }
        l.last_h2d = c.ev_h2d;
        if (verbose) (void)hipEventRecord(vt1[id % 8], l.copy);
        if ((rc = start_read(nxt, id + 1)) != PA_OK) break;             // the next window's text starts to arrive
        bool discard = false;
        if (have_pending) {
            const int r = resolve();
            if (r == WIN_ODD) { gpu_mode = false; discard = true; rec_start = pending.from; tp.next_id = pending.id; }               // not four-line text from here on: the host's scan takes over
            else if (r == WIN_EMPTY) { W = std::max<uint64_t>(2 * W, 2 * (main_from - pending.from)); discard = true; rec_start = pending.from; tp.next_id = pending.id; }   // no whole record in the window: a longer one
            else if (r != PA_OK) { rc = r; break; }
        }
        if ((rc = tp.use(l)) != PA_OK) break;
        const uint64_t head = main_from - rec_start;   // the unfinished record of the window before
        if (!discard && head > WINDOW_HEAD_ROOM) { W = std::max<uint64_t>(W, 2 * head); discard = true; }
        if (discard) {   // this window's text (and what was being read behind it) is read again, from the first record not yet taken
            if (nxt.active) { (void)tp.read_end(); nxt.active = false; }
            (void)hipStreamSynchronize(l.copy);
            read_to = rec_start;
            if (W > (1ull << 31)) gpu_mode = false;   // (a record of gigabytes: the host's scan says what it is)
            if ((rc = start_read(cur, tp.next_id)) != PA_OK) break;
            continue;
        }
        t0 = TextPipe::now();
        if (head) {
            if ((rc = tp.read_small(rec_start, head, c.h_raw.get() + WINDOW_HEAD_ROOM - head)) != PA_OK) break;
            if (hipMemcpyAsync(c.d_raw.get() + WINDOW_HEAD_ROOM - head, c.h_raw.get() + WINDOW_HEAD_ROOM - head, head, hipMemcpyHostToDevice, l.scan) != hipSuccess) { rc = fail(PA_ERR_HIP, "copy of a window's head failed"); break; }
        }
        tp.t_read += TextPipe::now() - t0; t0 = TextPipe::now();
        c.raw_begin = WINDOW_HEAD_ROOM - head;
        c.raw_end = WINDOW_HEAD_ROOM + main_len;
        if ((rc = window_ensure_scan(c, 0)) != PA_OK) break;
        if (hipStreamWaitEvent(l.scan, c.ev_h2d, 0) != hipSuccess) { rc = fail(PA_ERR_HIP, "hipStreamWaitEvent failed"); break; }
        if ((rc = window_scan_enqueue(c, false, l.scan)) != PA_OK) break;
        tp.t_launch += TextPipe::now() - t0;
        pending = Win();
        pending.id = id;
        pending.lane = (int)(id % (uint64_t)nidx);
        pending.slot = tp.slot_of(id);
        pending.from = rec_start;
        have_pending = true;
        tp.next_id = id + 1;
        if ((rc = tp.retire_finished(0)) != PA_OK) break;
        cur = nxt;
        nxt.active = false;
    }
    if (cur.active || nxt.active) (void)tp.read_end();   // (an error path: nothing of the pool's job is left behind)
    gpu_mode = false;
    if (rc == PA_OK && have_pending) {
        const int r = resolve();
        if (r == WIN_ODD || r == WIN_EMPTY) { rec_start = pending.from; tp.next_id = pending.id; }
        else if (r != PA_OK) rc = r;
    }

    // ---- the rest of the text (its end; all of it when it is not in four-line shape): the host's scan, the same kernels ----
    if (rc == PA_OK) {
        IngestCache* const hc = lanes[0].cache;   // (the scan's lists are parked with lane 0's buffers)
        text.off = rec_start;
        WindowScan ws(text);
        uint64_t records_before = tp.launched_reads;
        for (;;) {
            double t0 = TextPipe::now();
            rc = ws.next(fastq_path, records_before, pool, hc->rec_pos, hc->brk);
            tp.t_scan += TextPipe::now() - t0;
            if (rc != PA_OK || ws.nrec == 0) break;
            records_before += ws.nrec;
            const RecPos* const rp = hc->rec_pos.data();
            for (uint64_t i0 = 0; i0 < ws.nrec && rc == PA_OK;) {
                // a batch of whole records whose text fits a window of 2 GiB (offsets into it are 32 bits)
                uint64_t i1 = std::min<uint64_t>(ws.nrec, i0 + BATCH_READS);
                const uint64_t first = rp[i0].start;
                auto end_of = [&](uint64_t i) { return i < ws.nrec ? rp[i].start : ws.size; };
                while (i1 > i0 + 1 && end_of(i1) - first > (1ull << 31)) i1 = i0 + (i1 - i0) / 2;
                const uint64_t bytes = end_of(i1) - first, n = i1 - i0;
                if (bytes > (3ull << 30)) { rc = fail(PA_ERR_UNSUPPORTED, "%s: record %llu is longer than 3 GiB", fastq_path, (unsigned long long)(tp.launched_reads)); break; }
                const uint64_t id = tp.next_id;
                BatchCtx* cp = nullptr;
                if ((rc = tp.acquire(id, &cp)) != PA_OK) break;
                BatchCtx& c = *cp;
                Lane& l = tp.lane_of(id);
                if ((rc = window_ensure_raw(c, WINDOW_HEAD_ROOM + bytes)) != PA_OK) break;
                if ((rc = window_ensure_recs(c, n, true)) != PA_OK) break;
                t0 = TextPipe::now();
                {   // the batch's text and where its records lie in it
                    const char* const src = ws.base + first;
                    const uint64_t PIECE = 2ull << 20;
                    const int ntask = (int)std::max<uint64_t>(1, std::min<uint64_t>((bytes + PIECE - 1) / PIECE, 1u << 20));
                    pool.run(ntask, [&](int t) {
                        const uint64_t a = bytes * (uint64_t)t / (uint64_t)ntask, b = bytes * (uint64_t)(t + 1) / (uint64_t)ntask;
                        memcpy(c.h_raw.get() + WINDOW_HEAD_ROOM + a, src + a, (size_t)(b - a));
                    });
                }
                const int T4 = pool.size() * 4;
                std::vector<uint32_t> tmax((size_t)T4, 0);
                pool.run(T4, [&](int t) {
                    uint32_t mx = 0;
                    for (uint64_t i = n * (uint64_t)t / (uint64_t)T4; i < n * (uint64_t)(t + 1) / (uint64_t)T4; ++i) {
                        const RecPos& r = rp[i0 + i];
                        const uint64_t seq_off = std::min<uint64_t>(r.start + r.hdr + 1, ws.size);
                        const uint32_t seq_len = (uint32_t)std::min<uint64_t>(r.seq_len, ws.size - seq_off);
                        c.h_rec.get()[i] = make_uint4((uint32_t)(WINDOW_HEAD_ROOM + r.start + 1 - first), r.id_len, (uint32_t)(WINDOW_HEAD_ROOM + seq_off - first), seq_len);
                        mx = std::max(mx, seq_len);
                    }
                    tmax[(size_t)t] = mx;
                });
                uint32_t maxlen = 1;
                for (uint32_t m : tmax) maxlen = std::max(maxlen, m);
                tp.t_read += TextPipe::now() - t0;
                if (maxlen > PA_MAX_READ_LEN) { rc = fail(PA_ERR_UNSUPPORTED, "read longer than %u bases", PA_MAX_READ_LEN); break; }
                // (the copies ride on the lane's kernel stream: this path is bound by the host's scan, not by the link)
                if (hipMemcpyAsync(c.d_raw.get() + WINDOW_HEAD_ROOM, c.h_raw.get() + WINDOW_HEAD_ROOM, bytes, hipMemcpyHostToDevice, l.stream) != hipSuccess ||
                    hipMemcpyAsync(c.d_rec.get(), c.h_rec.get(), n * sizeof(uint4), hipMemcpyHostToDevice, l.stream) != hipSuccess) { rc = fail(PA_ERR_HIP, "copy of a text window to the GPU failed"); break; }
                c.raw_begin = WINDOW_HEAD_ROOM;
                c.raw_end = WINDOW_HEAD_ROOM + bytes;
                c.n = n;
                c.wpr = pa_words_per_read(maxlen);
                Win w;
                w.id = id;
                w.lane = (int)(id % (uint64_t)nidx);
                w.slot = tp.slot_of(id);
                w.from = 0;
                tp.next_id = id + 1;
                tp.wins.push_back(w);
                ++tp.host_windows;
                rc = tp.launch(tp.wins.back());
                i0 = i1;
            }
            if (rc != PA_OK) break;
        }
    }
    if (rc == PA_OK) rc = tp.retire_finished(~0ull);
    } catch (const std::bad_alloc&) {
        rc = fail(PA_ERR_OOM, "out of host memory in pa_process_reads");
    } catch (const std::exception& ex) {
        rc = fail(PA_ERR_INTERNAL, "pa_process_reads: %s", ex.what());
    }
    {
        double* st = pa::ingest::last_stage_seconds();
        st[0] = tp.t_scan; st[1] = tp.t_read; st[2] = tp.t_wait; st[3] = tp.t_launch; st[4] = tp.t_text; st[5] = tp.t_push; st[6] = TextPipe::now() - t_begin; st[7] = (double)tp.reported;
    }
    if (verbose)
        fprintf(stderr, "\n[pa ingest] %llu reads, %d threads, %d lane(s): %llu windows scanned on the GPU (%llu scanned twice), %llu batches by the host; host scan %.3f s, read %.3f s, wait GPU %.3f s, launch %.3f s, wait text %.3f s, wait writer %.3f s, total %.3f s (before the first window %.3f s)\n",
                (unsigned long long)tp.reported, pool.size(), nidx, (unsigned long long)tp.gpu_windows, (unsigned long long)tp.rescans, (unsigned long long)tp.host_windows, tp.t_scan, tp.t_read, tp.t_wait,
                tp.t_launch, tp.t_text, tp.t_push, TextPipe::now() - t_begin, t_begin - t_enter);
    if (verbose && v_h2d_ms > 0) fprintf(stderr, "[pa ingest] windows to the GPU: %.1f MB in %.2f ms of copies = %.1f GB/s\n", v_h2d_bytes / 1e6, v_h2d_ms, v_h2d_bytes / v_h2d_ms / 1e6);
    for (int i = 0; i < 8; ++i) { if (vt0[i]) (void)hipEventDestroy(vt0[i]); if (vt1[i]) (void)hipEventDestroy(vt1[i]); }
    if (tp.reported >= 1000000) fputc('\n', stderr);   // (`eprintln!()` behind the progress line, :508)
    for (Lane& l : lanes) {
        if (!l.cache) continue;
        (void)hipSetDevice(l.device);
        for (hipStream_t s : {l.copy, l.scan, l.back})
            if (s) (void)hipStreamSynchronize(s);
        if (l.stream) (void)hipStreamSynchronize(l.stream);   // (the streams stay with the parked buffers; IngestCache::destroy releases them)
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
    text.release();
    if (out != stdout) { if (fclose(out) != 0 && rc == PA_OK) rc = fail(PA_ERR_IO, "close %s: %s", out_path, strerror(errno)); }
    else fflush(stdout);
    if (rc != PA_OK && !why.empty()) last_error_ref() = why;
    if (n_reads_out) *n_reads_out = tp.reported;
    if (n_flagged_out) *n_flagged_out = tp.flagged;
    return rc;
}

}  // namespace

extern "C" int pa_process_reads(pa_index* idx, const char* fastq_path, const char* out_path, int num_threads, uint64_t* n_reads_out,
                                uint64_t* n_flagged_out) {
    pa_index* one[1] = {idx};
    try {
        return process_reads_impl(one, 1, fastq_path, out_path, num_threads, n_reads_out, n_flagged_out);
    } catch (const std::bad_alloc&) {
        return fail(PA_ERR_OOM, "out of host memory in pa_process_reads");
    } catch (const std::exception& ex) {   // (thread creation: std::system_error) — nothing crosses the C ABI
        return fail(PA_ERR_INTERNAL, "pa_process_reads: %s", ex.what());
    }
}

extern "C" int pa_process_reads_multi(pa_index* const* idx, int n_idx, const char* fastq_path, const char* out_path, int num_threads, uint64_t* n_reads_out,
                                      uint64_t* n_flagged_out) {
    try {
        return process_reads_impl(idx, n_idx, fastq_path, out_path, num_threads, n_reads_out, n_flagged_out);
    } catch (const std::bad_alloc&) {
        return fail(PA_ERR_OOM, "out of host memory in pa_process_reads_multi");
    } catch (const std::exception& ex) {
        return fail(PA_ERR_INTERNAL, "pa_process_reads_multi: %s", ex.what());
    }
}

extern "C" int pa_process_reads_stage_seconds(double out[PA_INGEST_STAGES]) {
    if (!out) return fail(PA_ERR_INVALID_ARG, "null argument");
    memcpy(out, pa::ingest::last_stage_seconds(), sizeof(double) * PA_INGEST_STAGES);
    return PA_OK;
}

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
    int open(const char* p) {
        path = p;
        const int rc = open_fastq(p, text);
        if (rc == PA_OK) ws.reset(new WindowScan(text));
        return rc;
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

struct CellBatch {   // one batch of pairs: R2 (all of it) and the R1 prefixes, pinned + on the device, and the mapping's outputs
    PinnedBuffer<uint8_t> h_r2, h_r1;
    PinnedBuffer<uint64_t> h_r2off, h_r1off;
    DeviceBuffer<uint8_t> d_r2, d_r1;
    DeviceBuffer<uint64_t> d_r2off, d_r1off, d_tiles;
    DeviceBuffer<uint32_t> d_lens, d_arena;
    DeviceBuffer<pa_read_result> d_results;
    uint64_t n = 0, r2_bytes = 0, r1_bytes = 0;
    uint32_t max_len = 0, max_len1 = 0;   // longest R2 / longest gathered piece of R1
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

// The pair scan and gather shared by pa_count_cells and pa_count_pairs: the two files a window of records at a time, record counts and
// record.id() (after a trailing "/1" or "/2" is cut) compared on the way, whole windows' worth of pairs gathered into a batch — all of
// R2 and the first `prefix` bytes of every R1 (0xFFFFFFFF: all of it) — each piece copied before its window is given up.
struct PairReader {
    const char *r1_path, *r2_path;
    Pool& pool;
    const uint32_t prefix;
    double* st;                    // stage seconds: [0] scan, [1] gather
    PairCursor f1, f2;
    uint64_t batch_pairs = DEFAULT_BATCH_READS;
    int ntask;
    std::vector<uint64_t> part, part1;
    std::vector<uint32_t> part_max, part_max1;
    uint64_t pairs = 0;            // pairs of the batches launched so far (the caller adds a batch when it launches it)
    bool ended = false;
    PairReader(const char* r1, const char* r2, Pool& pl, uint32_t prefix_, double* st_)
        : r1_path(r1), r2_path(r2), pool(pl), prefix(prefix_), st(st_), ntask(pl.size() * 4), part((size_t)ntask + 1), part1((size_t)ntask + 1), part_max((size_t)ntask),
          part_max1((size_t)ntask) {
        if (const char* v = getenv("PA_INGEST_BATCH")) { const long long x = atoll(v); if (x >= 1) batch_pairs = (uint64_t)x; }
    }
    int open() {
        int rc;
        if ((rc = f1.open(r1_path)) != PA_OK || (rc = f2.open(r2_path)) != PA_OK) return rc;
        return PA_OK;
    }
    void release() { f1.text.release(); f2.text.release(); }
    // gather the next batch into b
    int gather(CellBatch& b) {
        b.n = 0; b.r2_bytes = 0; b.r1_bytes = 0; b.max_len = 0; b.max_len1 = 0;
        int e = PA_OK;
        if ((e = grow_pinned(b.h_r2off, batch_pairs + 1, 0)) || (e = grow_pinned(b.h_r1off, batch_pairs + 1, 0))) return e;
        if (prefix != 0xFFFFFFFFu && (e = grow_pinned(b.h_r1, (size_t)batch_pairs * prefix + 64, 0))) return e;
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
            part[0] = b.r2_bytes;
            part1[0] = b.r1_bytes;
            for (int t = 0; t < ntask; ++t) {
                part[(size_t)t + 1] += part[(size_t)t];
                part1[(size_t)t + 1] += part1[(size_t)t];
                b.max_len = std::max(b.max_len, part_max[(size_t)t]);
                b.max_len1 = std::max(b.max_len1, part_max1[(size_t)t]);
            }
            if ((e = grow_pinned(b.h_r2, part[(size_t)ntask] + 64, b.r2_bytes)) != PA_OK) return e;
            if ((e = grow_pinned(b.h_r1, part1[(size_t)ntask] + 64, b.r1_bytes)) != PA_OK) return e;   // (a bounded prefix: sized above, nothing to do)
            pool.run(ntask, [&](int t) {   // all of R2, the first `prefix` bytes of R1
                uint64_t o2 = part[(size_t)t], o1 = part1[(size_t)t];
                for (uint64_t i = m * (uint64_t)t / ntask; i < m * (uint64_t)(t + 1) / ntask; ++i) {
                    const uint32_t len2 = f2.rec[a2 + i].seq_len;
                    b.h_r2off.get()[base + i] = o2;
                    memcpy(b.h_r2.get() + o2, f2.seq(a2 + i), len2);
                    o2 += len2;
                    const uint32_t len1 = std::min(f1.rec[a1 + i].seq_len, prefix);
                    b.h_r1off.get()[base + i] = o1;
                    memcpy(b.h_r1.get() + o1, f1.seq(a1 + i), len1);
                    o1 += len1;
                }
            });
            b.r1_bytes = part1[(size_t)ntask];
            b.r2_bytes = part[(size_t)ntask];
            b.n += m;
            f1.at += m;
            f2.at += m;
            st[1] += secs_since(t0);
        }
        b.h_r2off.get()[b.n] = b.r2_bytes;
        b.h_r1off.get()[b.n] = b.r1_bytes;
        return PA_OK;
    }
};

// the batch's GPU leg up to the mapping: copies, encode, map (asynchronous on s)
int cell_batch_map(pa_index* idx, CellBatch& b, hipStream_t s) {
    const uint32_t wpr = pa_words_per_read(std::max(1u, b.max_len));
    int e = PA_OK;
    if ((e = b.d_r2.reserve(b.r2_bytes + 64, b.h_r2.size())) || (e = b.d_r1.reserve(b.r1_bytes + 64, b.h_r1.size())) ||
        (e = b.d_r2off.reserve(b.n + 1, b.h_r2off.size())) || (e = b.d_r1off.reserve(b.n + 1, b.h_r1off.size())) ||
        (e = b.d_tiles.reserve(pa_tiles_words(b.n, wpr) + 1, pa_tiles_words(b.n, wpr) + 1)) || (e = b.d_lens.reserve(b.n + 64, b.h_r1off.size())) ||
        (e = b.d_results.reserve(b.n + 64, b.h_r1off.size())))
        return e;
    const uint64_t hint = pa_map_arena_hint(idx, b.n);
    if ((e = b.d_arena.reserve(hint, hint)) != PA_OK) return e;
    PA_HIP_TRY(hipMemcpyAsync(b.d_r2.get(), b.h_r2.get(), b.r2_bytes, hipMemcpyHostToDevice, s));
    PA_HIP_TRY(hipMemcpyAsync(b.d_r2off.get(), b.h_r2off.get(), (b.n + 1) * 8, hipMemcpyHostToDevice, s));
    PA_HIP_TRY(hipMemcpyAsync(b.d_r1.get(), b.h_r1.get(), b.r1_bytes, hipMemcpyHostToDevice, s));
    PA_HIP_TRY(hipMemcpyAsync(b.d_r1off.get(), b.h_r1off.get(), (b.n + 1) * 8, hipMemcpyHostToDevice, s));
    if ((e = pa_encode_reads_device(idx, b.d_r2.get(), b.d_r2off.get(), b.n, wpr, b.d_tiles.get(), b.d_lens.get(), s)) != PA_OK) return e;
    return pa_map_batch_device(idx, b.d_tiles.get(), b.d_lens.get(), b.n, wpr, PA_DEFAULT_ALLOWED_MISMATCHES, b.d_results.get(), b.d_arena.get(),
                               b.d_arena.size(), nullptr, s);
}

// waits for the mapping (regrowing the arena as pa_map_finish asks), then counts the batch
int cell_batch_count(pa_index* idx, pa_cell_counter* counter, CellBatch& b, hipStream_t s, double* st) {
    auto t0 = std::chrono::steady_clock::now();
    uint64_t used = 0, need = 0;
    int e = pa_map_finish(idx, s, &used, &need);
    for (int attempt = 0; e == PA_ERR_ARENA_FULL && attempt < 3; ++attempt) {
        if ((e = b.d_arena.alloc(need + need / 8 + 4096)) != PA_OK) return e;
        const uint32_t wpr = pa_words_per_read(std::max(1u, b.max_len));
        e = pa_map_batch_device(idx, b.d_tiles.get(), b.d_lens.get(), b.n, wpr, PA_DEFAULT_ALLOWED_MISMATCHES, b.d_results.get(), b.d_arena.get(),
                                b.d_arena.size(), nullptr, s);
        if (e == PA_OK) e = pa_map_finish(idx, s, &used, &need);
    }
    st[2] += secs_since(t0);
    if (e != PA_OK) return e;
    t0 = std::chrono::steady_clock::now();
    e = pa_cell_counter_add_device(counter, b.d_results.get(), b.d_arena.get(), b.d_r1.get(), b.d_r1off.get(), b.n, s);
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
    hipStream_t s = nullptr;
    PA_HIP_TRY(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    struct StreamGuard { pa_index* idx; hipStream_t s; ~StreamGuard() { (void)hipStreamSynchronize(s); (void)pa_index_release_stream(idx, s); (void)hipStreamDestroy(s); } } guard{idx, s};
    CellBatch batches[2];
    uint64_t& pairs = rd.pairs;
    bool in_flight = false;
    bool& ended = rd.ended;
    int cur = 0;
    auto gather = [&](CellBatch& b) -> int { return rd.gather(b); };
    for (;;) {
        CellBatch& b = batches[cur];
        b.n = 0;
        rc = ended ? PA_OK : gather(b);   // (while the batch before is on the GPU)
        if (rc != PA_OK) break;
        if (in_flight) {
            if ((rc = cell_batch_count(idx, counter, batches[cur ^ 1], s, st)) != PA_OK) break;
            in_flight = false;
        }
        if (b.n == 0) break;
        const auto t0 = std::chrono::steady_clock::now();
        if ((rc = cell_batch_map(idx, b, s)) != PA_OK) break;
        st[3] += secs_since(t0);
        pairs += b.n;
        in_flight = true;
        cur ^= 1;
    }
    rd.release();
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
    st[7] = (double)pairs;
    return PA_OK;
}


// ---- pa_count_pairs: two FASTQ files -> the class-count table of the pairs ----
struct PairBatch : CellBatch {   // + mate 1's tiles and mapping, the reverse-complemented tiles of one mate, the pair stage's outputs
    DeviceBuffer<uint64_t> d_tiles1, d_rc;
    DeviceBuffer<uint32_t> d_lens1, d_arena1, d_parena;
    DeviceBuffer<pa_read_result> d_results1, d_presults;
    DeviceBuffer<uint8_t> d_scratch;
};

int pair_map_mate(pa_index* idx, const uint64_t* tiles, const uint32_t* lens, uint64_t n, uint32_t wpr, uint32_t allowed, pa_read_result* res, DeviceBuffer<uint32_t>& arena,
                  hipStream_t s) {
    return pa_map_batch_device(idx, tiles, lens, n, wpr, allowed, res, arena.get(), arena.size(), nullptr, s);
}

// the batch's GPU leg up to the two mappings: mate 1 on s1, mate 2 on s2 (each stream has its own launch context on idx), all asynchronous
int pair_batch_map(pa_index* idx, PairBatch& b, int orient, uint32_t allowed, hipStream_t s1, hipStream_t s2) {
    const uint32_t wpr1 = pa_words_per_read(std::max(1u, b.max_len1)), wpr2 = pa_words_per_read(std::max(1u, b.max_len));
    const size_t tw1 = pa_tiles_words(b.n, wpr1) + 1, tw2 = pa_tiles_words(b.n, wpr2) + 1;
    const uint64_t hint = pa_map_arena_hint(idx, b.n);
    int e = PA_OK;
    if ((e = b.d_r2.reserve(b.r2_bytes + 64, b.h_r2.size())) || (e = b.d_r1.reserve(b.r1_bytes + 64, b.h_r1.size())) ||
        (e = b.d_r2off.reserve(b.n + 1, b.h_r2off.size())) || (e = b.d_r1off.reserve(b.n + 1, b.h_r1off.size())) ||
        (e = b.d_tiles.reserve(tw2, tw2)) || (e = b.d_tiles1.reserve(tw1, tw1)) || (e = b.d_rc.reserve(std::max(tw1, tw2), std::max(tw1, tw2))) ||
        (e = b.d_lens.reserve(b.n + 64, b.h_r1off.size() + 64)) || (e = b.d_lens1.reserve(b.n + 64, b.h_r1off.size() + 64)) ||
        (e = b.d_results.reserve(b.n + 64, b.h_r1off.size() + 64)) || (e = b.d_results1.reserve(b.n + 64, b.h_r1off.size() + 64)) ||
        (e = b.d_presults.reserve(b.n + 64, b.h_r1off.size() + 64)) || (e = b.d_arena.reserve(hint, hint)) || (e = b.d_arena1.reserve(hint, hint)))
        return e;
    PA_HIP_TRY(hipMemcpyAsync(b.d_r1.get(), b.h_r1.get(), b.r1_bytes, hipMemcpyHostToDevice, s1));
    PA_HIP_TRY(hipMemcpyAsync(b.d_r1off.get(), b.h_r1off.get(), (b.n + 1) * 8, hipMemcpyHostToDevice, s1));
    PA_HIP_TRY(hipMemcpyAsync(b.d_r2.get(), b.h_r2.get(), b.r2_bytes, hipMemcpyHostToDevice, s2));
    PA_HIP_TRY(hipMemcpyAsync(b.d_r2off.get(), b.h_r2off.get(), (b.n + 1) * 8, hipMemcpyHostToDevice, s2));
    if ((e = pa_encode_reads_device(idx, b.d_r1.get(), b.d_r1off.get(), b.n, wpr1, b.d_tiles1.get(), b.d_lens1.get(), s1)) != PA_OK) return e;
    if ((e = pa_encode_reads_device(idx, b.d_r2.get(), b.d_r2off.get(), b.n, wpr2, b.d_tiles.get(), b.d_lens.get(), s2)) != PA_OK) return e;
    const uint64_t *t1 = b.d_tiles1.get(), *t2 = b.d_tiles.get();
    if (orient == PA_PAIR_RF) {
        if ((e = pa_revcomp_tiles_device(idx, b.d_tiles1.get(), b.d_lens1.get(), b.n, wpr1, b.d_rc.get(), s1)) != PA_OK) return e;
        t1 = b.d_rc.get();
    } else if (orient == PA_PAIR_FR) {
        if ((e = pa_revcomp_tiles_device(idx, b.d_tiles.get(), b.d_lens.get(), b.n, wpr2, b.d_rc.get(), s2)) != PA_OK) return e;
        t2 = b.d_rc.get();
    }
    if ((e = pair_map_mate(idx, t1, b.d_lens1.get(), b.n, wpr1, allowed, b.d_results1.get(), b.d_arena1, s1)) != PA_OK) return e;
    return pair_map_mate(idx, t2, b.d_lens.get(), b.n, wpr2, allowed, b.d_results.get(), b.d_arena, s2);
}

// waits for the two mappings (regrowing an arena as pa_map_finish asks), then combines and counts the batch on s1
int pair_batch_count(pa_index* idx, PairBatch& b, int orient, uint32_t allowed, uint64_t* d_counts, hipStream_t s1, hipStream_t s2, uint64_t* stats, double* st) {
    auto t0 = std::chrono::steady_clock::now();
    const uint32_t wpr1 = pa_words_per_read(std::max(1u, b.max_len1)), wpr2 = pa_words_per_read(std::max(1u, b.max_len));
    for (int mate = 0; mate < 2; ++mate) {
        hipStream_t s = mate ? s2 : s1;
        DeviceBuffer<uint32_t>& arena = mate ? b.d_arena : b.d_arena1;
        const bool rc = mate ? orient == PA_PAIR_FR : orient == PA_PAIR_RF;
        const uint64_t* tiles = rc ? b.d_rc.get() : mate ? b.d_tiles.get() : b.d_tiles1.get();
        uint64_t used = 0, need = 0;
        int e = pa_map_finish(idx, s, &used, &need);
        for (int attempt = 0; e == PA_ERR_ARENA_FULL && attempt < 3; ++attempt) {
            if ((e = arena.alloc(need + need / 8 + 4096)) != PA_OK) return e;
            e = pair_map_mate(idx, tiles, mate ? b.d_lens.get() : b.d_lens1.get(), b.n, mate ? wpr2 : wpr1, allowed, mate ? b.d_results.get() : b.d_results1.get(), arena, s);
            if (e == PA_OK) e = pa_map_finish(idx, s, &used, &need);
        }
        if (e != PA_OK) return e;
    }
    st[2] += secs_since(t0);
    t0 = std::chrono::steady_clock::now();
    // the pair arena is sized by a bound on what the batch can need, so that the counted launch cannot run out of it (a re-run would count twice)
    uint64_t bound = 0;
    const size_t scratch_bytes = pa_pairs_scratch_bytes(b.n);
    int e = b.d_scratch.reserve(scratch_bytes, scratch_bytes + scratch_bytes / 4);
    if (e != PA_OK) return e;
    if ((e = pairs_arena_bound(idx, b.d_results1.get(), b.d_results.get(), b.n, b.d_scratch.get(), s1, &bound)) != PA_OK) return e;
    if (bound > PA_MAX_ARENA_ENTRIES) return fail(PA_ERR_UNSUPPORTED, "a batch of %llu pairs may need %llu arena entries: lower PA_INGEST_BATCH", (unsigned long long)b.n, (unsigned long long)bound);
    if ((e = b.d_parena.reserve(bound + 64, bound + bound / 4 + 4096)) != PA_OK) return e;
    if ((e = pa_pairs_combine_device(idx, b.d_results1.get(), b.d_arena1.get(), b.d_results.get(), b.d_arena.get(), b.n, b.d_presults.get(), b.d_parena.get(), b.d_parena.size(),
                                     d_counts, b.d_scratch.get(), scratch_bytes, s1)) != PA_OK)
        return e;
    uint64_t bst[PA_PAIR_STATS], used = 0, need = 0;
    if ((e = pa_pairs_finish(idx, b.d_scratch.get(), s1, bst, &used, &need)) != PA_OK) return e;
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
    hipStream_t s1 = nullptr, s2 = nullptr;
    PA_HIP_TRY(hipStreamCreateWithFlags(&s1, hipStreamNonBlocking));
    struct StreamGuard { pa_index* idx; hipStream_t s; ~StreamGuard() { (void)hipStreamSynchronize(s); (void)pa_index_release_stream(idx, s); (void)hipStreamDestroy(s); } } g1{idx, s1};
    PA_HIP_TRY(hipStreamCreateWithFlags(&s2, hipStreamNonBlocking));
    StreamGuard g2{idx, s2};
    PA_HIP_TRY(hipMemsetAsync(d_counts.get(), 0, counts_len * 8, s1));
    PairBatch batches[2];
    uint64_t stats[PA_PAIR_STATS] = {0};
    bool in_flight = false;
    int cur = 0;
    for (;;) {
        PairBatch& b = batches[cur];
        b.n = 0;
        rc = rd.ended ? PA_OK : rd.gather(b);   // (while the batch before is on the GPU)
        if (rc != PA_OK) break;
        if (in_flight) {
            if ((rc = pair_batch_count(idx, batches[cur ^ 1], orient, allowed, d_counts.get(), s1, s2, stats, st)) != PA_OK) break;
            in_flight = false;
        }
        if (b.n == 0) break;
        const auto t0 = std::chrono::steady_clock::now();
        if ((rc = pair_batch_map(idx, b, orient, allowed, s1, s2)) != PA_OK) break;
        st[3] += secs_since(t0);
        rd.pairs += b.n;
        in_flight = true;
        cur ^= 1;
    }
    rd.release();
    if (rc != PA_OK) return rc;
    PA_HIP_TRY(hipMemcpyAsync(h_counts, d_counts.get(), counts_len * 8, hipMemcpyDeviceToHost, s1));
    PA_HIP_TRY(hipStreamSynchronize(s1));
    if (n_pairs) *n_pairs = rd.pairs;
    if (stats_out) for (int j = 0; j < PA_PAIR_STATS; ++j) stats_out[j] = stats[j];
    st[6] = secs_since(t_call);
    st[7] = (double)rd.pairs;
    return PA_OK;
}

}  // namespace

extern "C" int pa_count_cells(pa_index* idx, const pa_host_index* h, const char* r1_path, const char* r2_path, const char* whitelist_path, uint32_t bc_len,
                              uint32_t umi_len, const char* out_dir, int num_threads, uint64_t stats[PA_CELL_STATS]) {
    try {
        return count_cells_impl(idx, h, r1_path, r2_path, whitelist_path, bc_len, umi_len, out_dir, num_threads, stats);
    } catch (const std::bad_alloc&) {
        return fail(PA_ERR_OOM, "out of host memory in pa_count_cells");
    } catch (const std::exception& ex) {
        return fail(PA_ERR_INTERNAL, "pa_count_cells: %s", ex.what());
    }
}

extern "C" int pa_count_pairs(pa_index* idx, const char* r1_path, const char* r2_path, int orient, uint32_t allowed_mismatches, int num_threads, uint64_t* h_counts,
                              uint64_t* n_pairs, uint64_t stats[PA_PAIR_STATS]) {
    try {
        return count_pairs_impl(idx, r1_path, r2_path, orient, allowed_mismatches, num_threads, h_counts, n_pairs, stats);
    } catch (const std::bad_alloc&) {
        return fail(PA_ERR_OOM, "out of host memory in pa_count_pairs");
    } catch (const std::exception& ex) {
        return fail(PA_ERR_INTERNAL, "pa_count_pairs: %s", ex.what());
    }
}
