// A window feed for ONE FASTQ file: the text — a plain mapped file or the BGZF kind — becomes a sequence of windows in HBM, each with its
// records {id offset, id length, sequence offset, sequence length} (the layout of fastq_scan.hip) beside it. The steps are text_window.hpp's, the same bodies
// that TextPipe (fastq_reads.cpp) runs; the feed is the scheduler around them for a consumer that pulls: three slots, a slot taken again behind an event of its
// consumer, reads of a window's text synchronous on the pool (two feeds share it, and the pool runs one job at a time), next() handing out a window while the
// one behind it is scanned and the one behind that read and sent. FqInfo.odd or nothing left to plan -> the rest of the file through bgzf_materialise and the
// host's WindowScan, uploaded as windows of the same form. The paired drivers' device reader (pair_reader.cpp) runs two of them side by side.
#pragma once
#include <memory>

#include "text_window.hpp"

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
    // st: the call's stage seconds (the steps add to ST_SCAN, ST_READ, ST_WAIT, ST_LAUNCH)
    WindowFeed(const char* path, FastqText& text, Pool& pool, double* st, uint64_t window, uint64_t host_batch_recs);
    ~WindowFeed();
    WindowFeed(const WindowFeed&) = delete;
    WindowFeed& operator=(const WindowFeed&) = delete;
    // a text the feed takes: a plain mapped file or the BGZF kind
    static bool takes(const FastqText& t) { return t.bgzf || (t.mapped && t.data == t.map_base); }
    int start();                                   // its two streams
    int next(FeedWindow& w);                       // the next window with records in it; w.n == 0: the file has ended
    int release(int slot, hipStream_t last_reader);   // the slot may be reused behind everything enqueued on last_reader so far
    InputStats stats() const { return x_.final_stats(); }   // pa_process_reads_input_stats' entries, for this file
    uint64_t delivered() const { return delivered_; }   // records of the windows handed out

private:
    struct Slot {
        BatchCtx c;
        hipEvent_t ev_free = nullptr;
        bool wait_free = false;
    };
    int acquire(uint64_t id, Slot** out);
    int start_window(Pre& p, uint64_t id);            // plan | window_fill | window_send
    int enqueue_scan(Pre& p);                         // window_enqueue_scan; WIN_HEAD: the window is dropped, W grown or the host takes over
    int resolve(const Pre& p, FeedWindow& w);         // window_scan_wait: WIN_OK fills in w
    int drop_unscanned(Pre& p);                       // a sent window that is not going to be scanned
    int regrow(int answer, uint64_t main_from, bool more);   // window_rule applied: W, and where the text is read again or the host takes over
    int enter_host(uint64_t from);
    int host_next(FeedWindow& w);

    WindowCtx x_;
    uint64_t W_, KEEP_, host_batch_recs_;
    Slot slots_[FEED_SLOTS];
    hipStream_t copy_ = nullptr, scan_ = nullptr;
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
