// A window feed for ONE FASTQ file: the text — a plain mapped file or the BGZF kind — becomes a sequence of windows in HBM, each with its
// records {id offset, id length, sequence offset, sequence length} (the layout of fastq_scan.hip) beside it. The rules are TextPipe's (fastq_reads.cpp), without
// its lanes and its writer: plan_window with the same W / KEEP arithmetic, pieces copied into pinned memory by the pool with streaming stores, copy and
// inflate on a copy stream, the scan on a scan stream behind ev_h2d, the unfinished record of the window before copied in front of the window (BGZF:
// bgzf_read_host), FqInfo.overflow -> regrow and rescan, an empty window or a head beyond the head room -> a longer window, FqInfo.odd or nothing left to plan
// -> the rest of the file through bgzf_materialise and the host's WindowScan, uploaded as windows of the same form. The paired drivers (fastq_pairs.cpp) run
// two of them side by side.
#pragma once
#include <memory>

#include "fastq_text.hpp"

namespace pa {
namespace ingest {

struct FeedWindow {
    const uint8_t* d_raw = nullptr;   // the window's text in HBM; the records' offsets count from here
    uint64_t raw_bytes = 0;           // bytes of it that may be read
    const uint4* d_rec = nullptr;
    uint64_t n = 0;                   // records (0: the file has ended)
    uint32_t max_seq = 0;             // the longest sequence among them
    hipEvent_t ready = nullptr;       // d_raw and d_rec are valid behind it
    int slot = -1;
};

struct FeedStats {   // pa_process_reads_input_stats' entries, for this file
    uint64_t text_kind = 0, members_total = 0, members_gpu = 0, members_host = 0, bytes_h2d = 0, text_bytes_gpu = 0;
};

// What of the feed is arithmetic (tests/pairplan drives these over made-up sequences without a GPU):
// the slot of window `id` ...
constexpr int FEED_SLOTS = 3;   // the window being consumed, the one being scanned, the one being read
inline int feed_slot_of(uint64_t id) { return (int)(id % (uint64_t)FEED_SLOTS); }
// ... and the pairs of the next segment of a batch: what both windows still hold, and what the batch still takes
inline uint64_t segment_pairs(uint64_t left1, uint64_t left2, uint64_t batch_pairs, uint64_t n) {
    const uint64_t room = batch_pairs > n ? batch_pairs - n : 0;
    return left1 < left2 ? (left1 < room ? left1 : room) : (left2 < room ? left2 : room);
}

class WindowFeed {
public:
    // st: the call's stage seconds ([0] host scan, [1] reading into pinned memory, [2] waiting for the GPU, [3] launch)
    WindowFeed(const char* path, FastqText& text, Pool& pool, double* st, uint64_t window, uint64_t host_batch_recs);
    ~WindowFeed();
    WindowFeed(const WindowFeed&) = delete;
    WindowFeed& operator=(const WindowFeed&) = delete;
    // a text the feed takes: a plain mapped file or the BGZF kind
    static bool takes(const FastqText& t) { return t.bgzf || (t.mapped && t.data == t.map_base); }
    int start();                                   // its two streams
    int next(FeedWindow& w);                       // the next window with records in it; w.n == 0: the file has ended
    int release(int slot, hipStream_t last_reader);   // the slot may be reused behind everything enqueued on last_reader so far
    FeedStats stats() const;
    uint64_t delivered() const { return delivered_; }   // records of the windows handed out

private:
    struct Slot {
        BatchCtx c;
        hipEvent_t ev_free = nullptr;
        bool wait_free = false;
    };
    struct Pre {   // a window whose text has been sent (or is the one being scanned)
        WindowPlan plan;
        uint64_t id = 0, from = 0;   // from: text offset of its first record (known when its scan is enqueued)
        bool active = false;
    };
    enum { WIN_OK = 0, WIN_ODD = 1, WIN_EMPTY = 2 };
    static double now();
    template <class F> void deal_pieces(uint64_t len, F fn);
    void read_piece(uint64_t a, uint64_t b, uint8_t* dst);
    int read_small(uint64_t off, uint64_t len, uint8_t* dst);
    int acquire(uint64_t id, Slot** out);
    int start_window(Pre& p, uint64_t id);            // plan | read | send
    int enqueue_scan(Pre& p);                         // head | scan; answers WIN_EMPTY when the head does not fit (the window is dropped, W grown)
    int resolve(const Pre& p, FeedWindow& w);         // WIN_OK / WIN_ODD / WIN_EMPTY or a pa_status
    int drop_unscanned(Pre& p);                       // a sent window that is not going to be scanned
    int enter_host(uint64_t from);
    int host_next(FeedWindow& w);

    const char* path_;
    FastqText& text_;
    Pool& pool_;
    double* st_;
    uint64_t W_, KEEP_, host_batch_recs_;
    Slot slots_[FEED_SLOTS];
    hipStream_t copy_ = nullptr, scan_ = nullptr;
    FeedStats stats_;
    uint64_t next_id_ = 0, rec_start_ = 0, read_to_ = 0, delivered_ = 0;
    bool gpu_mode_ = false, host_mode_ = false, ended_ = false;
    Pre cur_, scanning_;
    // the host's part
    std::unique_ptr<WindowScan> ws_;
    std::vector<RecPos> rec_pos_;
    std::vector<std::vector<uint32_t>> brk_;
    uint64_t host_at_ = 0, host_before_ = 0;
};

}  // namespace ingest
}  // namespace pa
