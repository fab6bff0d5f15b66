// The steps that turn a FASTQ text into scanned windows in HBM, written once for the two schedulers that run them: TextPipe
// (fastq_reads.cpp: lanes, four slots, asynchronous reads, a writer) and WindowFeed (window_feed.cpp: one file, three slots, synchronous reads). A step is a
// plain function over a WindowCtx (what a call knows about one file) and the BatchCtx of the window's slot; which slot, which stream and what happens between
// two steps is the scheduler's. Per window, in order: window_fill (plan's bytes into pinned memory by the pool) | window_fill_end | window_send (copy stream:
// H2D, BGZF inflate, statuses back, ev_h2d) | window_enqueue_scan (head of the unfinished record, scan behind ev_h2d) | window_scan_wait (regrow on overflow,
// member statuses, WIN_*) | window_rule (what an odd or empty window or a head beyond the head room does to W). The host-scanned tail: host_tail_cut |
// window_fill_host | window_send_host. What is arithmetic is inline here and driven without a GPU by tests/winsteps/.
#pragma once
#include <emmintrin.h>

#include <atomic>
#include <chrono>

#include "fastq_text.hpp"

namespace pa {
namespace ingest {

constexpr uint64_t PIECE = 2ull << 20;   // bytes of a window that one task of the pool copies

enum { WIN_OK = 0, WIN_ODD = 1, WIN_EMPTY = 2, WIN_HEAD = 3 };   // what a step answers besides a pa_status (those are negative): not four-line text | no whole record | the head does not fit the head room
enum { ST_SCAN = 0, ST_READ = 1, ST_WAIT = 2, ST_LAUNCH = 3, ST_TEXT = 4, ST_PUSH = 5 };   // stage seconds a step or a scheduler adds to (pa_process_reads_stage_seconds: [6] whole call, [7] reads)
enum { ST_TALLY = 4, ST_WRITE = 5, ST_CALL = 6, ST_RECORDS = 7 };   // the paired drivers' names for the same array: [ST_READ] is their host gather, then count | output files | whole call | pairs

struct InputStats {   // pa_process_reads_input_stats, in the ABI's order: filled as the call goes
    uint64_t text_kind = 0, members_total = 0, members_gpu = 0, members_host = 0, bytes_h2d = 0, text_bytes_gpu = 0;
};
static_assert(sizeof(InputStats) == sizeof(uint64_t) * PA_INGEST_INPUT_STATS, "one field per entry of the ABI's array");

inline double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

struct WindowCtx {   // one file of a call, filled once
    const char* path;
    FastqText& text;
    Pool& pool;
    double* st;                      // the call's stage seconds: the steps add host scan -> [ST_SCAN], read -> [ST_READ], wait -> [ST_WAIT], launch -> [ST_LAUNCH]
    bool use_pread = false;          // PA_INGEST_PREAD (knobs builds, pa_process_reads only)
    InputStats stats;
    uint64_t rescans = 0;            // scans run again with a longer line table
    std::atomic<int> read_bad{0};    // a piece's pread failed
    bool read_async = false;         // pieces of window_fill are with the pool's workers
    WindowCtx(const char* p, FastqText& t, Pool& pl, double* st_, bool pread = false) : path(p), text(t), pool(pl), st(st_), use_pread(pread) {
        stats.text_kind = t.bgzf ? 2u : !t.inflated.empty() ? 1u : 0u;
        stats.members_total = t.members.size();
    }
    InputStats final_stats() const {   // with the members the host inflated (counted in the text itself)
        InputStats s = stats;
        if (s.text_kind == 2) s.members_host = text.members_host;
        return s;
    }
};

struct Pre {   // a window whose text is being read into its slot or has been sent; plan.active: there is one
    WindowPlan plan;
    uint64_t id = 0;
    uint64_t from = 0;       // text offset of its first record (known when its scan is enqueued)
    BatchCtx* c = nullptr;   // its slot
};

// ---- the window size ----
// PA_INGEST_WINDOW (64 MiB: 128 MiB leaves more of the first read and the last kernels unoverlapped, 16 MiB costs launches), never more than 256 bytes per
// read of a batch (the tests' small batches give small windows) or than 2 GiB (offsets into a window are 32 bits)
inline uint64_t window_clamp(uint64_t window, uint64_t batch) { return std::min<uint64_t>(std::min<uint64_t>(window, batch * 256), 1ull << 31); }
uint64_t window_from_env(uint64_t batch);
inline uint64_t window_of(const FastqText& t, uint64_t window) { return t.bgzf ? std::max<uint64_t>(window, PA_BGZF_MAX_ISIZE) : window; }   // a BGZF window's own text is a run of whole members
inline uint64_t keep_of(uint64_t W) { return std::max<uint64_t>(4096, std::min<uint64_t>(W / 4, 1ull << 20)); }   // the end of the text is the host's: its rules for the last record live there

// A window's own text starts at main_from, the first record no window has taken at rec_start: in front of it lies the HEAD, the unfinished record of the
// window before (or, BGZF behind a dropped window, the first record starts `skip` bytes inside the first member). false: the head does not fit the head room
inline bool window_head(uint64_t main_from, uint64_t rec_start, uint64_t* head, uint64_t* skip) {
    *head = main_from > rec_start ? main_from - rec_start : 0;
    *skip = rec_start > main_from ? rec_start - main_from : 0;
    return *head <= WINDOW_HEAD_ROOM;
}

// What a window that cannot be used means. The text is read again from `from`, the first record not yet taken (the start of the dropped window's records;
// for WIN_HEAD the start of the head), and main_from is where the own text of the window BEHIND it starts (`more`: there is one; for WIN_HEAD the window itself).
// WIN_ODD: not four-line text from here on, the host's scan takes over. WIN_EMPTY: no whole record in the window, a longer one — at least twice as long,
// and twice what lay in front of the window behind; with no window behind it the rest of the text is the host's anyway. WIN_HEAD: a window of at least twice
// the head. A window beyond 2 GiB is a record of gigabytes: the host's scan says what it is.
struct WindowRule {
    uint64_t W;
    bool host;
};
inline WindowRule window_rule(int answer, uint64_t W, uint64_t main_from, uint64_t from, bool more) {
    if (answer == WIN_ODD || !more) return {W, true};
    const uint64_t front = main_from > from ? main_from - from : 0;
    W = answer == WIN_EMPTY ? std::max<uint64_t>(2 * W, 2 * front) : std::max<uint64_t>(W, 2 * front);
    return {W, W > (1ull << 31)};
}

// ---- pieces ----
// bytes of the mapping into a pinned window with streaming stores: the window is read next by the copy engine, never by this CPU, so no line of it
// has to be fetched for ownership or kept in a cache
inline void copy_streaming(uint8_t* d, const uint8_t* s, size_t n) {
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

// [0, len) dealt in pieces of PIECE bytes: fn(a, b) copies bytes [a, b). One piece is copied by the caller, here. More go to the pool: all of them done on return
// (wait), or left with the pool's workers (the answer is true: Pool::end waits for them)
template <class F>
bool deal_pieces(Pool& pool, uint64_t len, bool wait, F fn) {
    if (len == 0) return false;
    const int ntask = (int)std::min<uint64_t>((len + PIECE - 1) / PIECE, 1u << 20);
    auto piece = [fn, len, ntask](int t) { fn(len * (uint64_t)t / (uint64_t)ntask, len * (uint64_t)(t + 1) / (uint64_t)ntask); };
    if (ntask == 1) { piece(0); return false; }
    if (wait) { pool.run(ntask, piece); return false; }
    pool.begin(ntask, piece);
    return true;
}

// text bytes [a, b) to dst (pinned): out of the file's mapping (page tables filled before the copy and dropped behind it), by pread (x.use_pread), or memcpy
// for text in memory (inflated gzip). A feed's text is always the mapped kind (WindowFeed::takes)
void read_piece(WindowCtx& x, uint64_t a, uint64_t b, uint8_t* dst);

// ---- a window the GPU scans ----
// h_raw (and h_comp, with the members' rows rebased on the window's first compressed byte) sized, the plan's bytes dealt to the pool: the text itself, or a
// BGZF window's compressed members. wait: done on return, with window_fill_end's answer; otherwise pieces may be left with the workers until window_fill_end
int window_fill(WindowCtx& x, const WindowPlan& plan, BatchCtx& c, bool wait);
int window_fill_end(WindowCtx& x);   // the pieces are in pinned memory, or "read failed"
// the window's bytes to the GPU on the copy stream; a BGZF window's members are inflated there, behind their copy, and their statuses come back ahead of ev_h2d
int window_send(WindowCtx& x, const WindowPlan& plan, BatchCtx& c, hipStream_t copy);
// the window's records are to be found: the head goes in front of the window's own text (read by the caller itself; on the scan stream, which then waits for
// the text: ev_h2d only), the scan follows. WIN_HEAD: the head does not fit, nothing has been touched
int window_enqueue_scan(WindowCtx& x, const WindowPlan& plan, BatchCtx& c, uint64_t rec_start, hipStream_t scan);
// the window's scan waited for (ev_info), run again with a longer line table while FqInfo.overflow says so (three attempts), then the members' statuses:
// WIN_OK (c.h_info holds n, max_seq, consumed), WIN_ODD, WIN_EMPTY, or "corrupt gzip stream" / "line table too small"
int window_scan_wait(WindowCtx& x, BatchCtx& c, hipStream_t scan);

// ---- the host-scanned tail ----
// records [i0, i1) of a host-scanned window (rp[0, nrec), text of `size` bytes) make the next batch: at most `batch` of them, halved until their text fits
// 2 GiB (offsets into a window are 32 bits) or one record is left
inline uint64_t host_tail_cut(const RecPos* rp, uint64_t nrec, uint64_t size, uint64_t i0, uint64_t batch) {
    auto end_of = [&](uint64_t i) { return i < nrec ? rp[i].start : size; };
    uint64_t i1 = std::min<uint64_t>(nrec, i0 + batch);
    while (i1 > i0 + 1 && end_of(i1) - rp[i0].start > (1ull << 31)) i1 = i0 + (i1 - i0) / 2;
    return i1;
}
// records rp[i0, i1) of ws into the slot: their text behind the head room of h_raw (plain memcpy: the bytes were just read by the scan and lie in the caches),
// their rows in h_rec, the longest sequence in *maxlen. record_no: of rp[i0] in the file ("record N is longer than 3 GiB")
int window_fill_host(WindowCtx& x, const WindowScan& ws, const RecPos* rp, uint64_t i0, uint64_t i1, uint64_t record_no, BatchCtx& c, uint32_t* maxlen);
int window_send_host(WindowCtx& x, BatchCtx& c, uint64_t n, hipStream_t stream);   // text and rows to the GPU, asynchronous on `stream`

}  // namespace ingest
}  // namespace pa
