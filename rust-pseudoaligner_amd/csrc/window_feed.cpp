// WindowFeed (window_feed.hpp): one FASTQ file as windows in HBM with their records beside them. What is done to a window is text_window.cpp's; here are the
// slots, the two streams and the order of the steps.
#include "window_feed.hpp"

namespace pa {
namespace ingest {

WindowFeed::WindowFeed(const char* path, FastqText& text, Pool& pool, double* st, uint64_t window, uint64_t host_batch_recs)
    : x_(path, text, pool, st), W_(window_of(text, window)), KEEP_(keep_of(W_)), host_batch_recs_(std::max<uint64_t>(1, host_batch_recs)) {}

WindowFeed::~WindowFeed() {
    for (hipStream_t s : {copy_, scan_})
        if (s) { (void)hipStreamSynchronize(s); (void)hipStreamDestroy(s); }
    for (Slot& s : slots_) {
        if (s.ev_free) (void)hipEventDestroy(s.ev_free);
        s.c.release();
    }
}

int WindowFeed::start() {
    for (hipStream_t* sp : {&copy_, &scan_})
        if (hipStreamCreateWithFlags(sp, hipStreamNonBlocking) != hipSuccess) { *sp = nullptr; return fail(PA_ERR_HIP, "hipStreamCreate failed"); }
    gpu_mode_ = x_.text.fsize > KEEP_;
    return PA_OK;
}

// the slot of window `id`: the copy stream waits for the last kernel that read what the slot held before
int WindowFeed::acquire(uint64_t id, Slot** out) {
    Slot& s = slots_[feed_slot_of(id)];
    int e = window_ensure_events(s.c);
    if (e != PA_OK) return e;
    if (!s.ev_free) PA_HIP_TRY(hipEventCreateWithFlags(&s.ev_free, hipEventDisableTiming));
    if (s.wait_free) {
        PA_HIP_TRY(hipStreamWaitEvent(copy_, s.ev_free, 0));
        PA_HIP_TRY(hipStreamWaitEvent(scan_, s.ev_free, 0));   // (a window's head goes in on the scan stream, ahead of ev_h2d)
        s.wait_free = false;
    }
    *out = &s;
    return PA_OK;
}

int WindowFeed::release(int slot, hipStream_t last_reader) {
    if (slot < 0 || slot >= FEED_SLOTS) return fail(PA_ERR_INTERNAL, "window feed: slot %d", slot);
    Slot& s = slots_[slot];
    PA_HIP_TRY(hipEventRecord(s.ev_free, last_reader));
    s.wait_free = true;
    return PA_OK;
}

// the next window (plan_window: none when the text in front of the host's part has been read): its bytes into the slot's pinned memory — the read is waited
// for here: two feeds take turns on the one pool — then to the GPU on the copy stream
int WindowFeed::start_window(Pre& p, uint64_t id) {
    p.plan = WindowPlan();
    const WindowPlan plan = gpu_mode_ ? plan_window(x_.text, read_to_, W_, KEEP_) : WindowPlan();
    if (!plan.active) return PA_OK;
    Slot* sp = nullptr;
    int e = acquire(id, &sp);
    if (e != PA_OK) return e;
    if ((e = window_fill(x_, plan, sp->c, true)) != PA_OK) return e;
    read_to_ = plan.text_from + plan.text_len;
    if ((e = window_send(x_, plan, sp->c, copy_)) != PA_OK) return e;
    p.plan = plan;
    p.id = id;
    p.c = &sp->c;
    return PA_OK;
}

// a sent window that will not be scanned (the text is read again from an earlier offset, or the host's scan takes over): its copy is waited for
int WindowFeed::drop_unscanned(Pre& p) {
    if (!p.plan.active) return PA_OK;
    p.plan.active = false;
    PA_HIP_TRY(hipStreamSynchronize(copy_));
    return PA_OK;
}

// a window could not be used (window_rule): the text is read again from rec_start_ for a longer window, or the host's scan takes over there
int WindowFeed::regrow(int answer, uint64_t main_from, bool more) {
    const WindowRule r = window_rule(answer, W_, main_from, rec_start_, more);
    W_ = r.W;
    if (r.host) return enter_host(rec_start_);
    read_to_ = rec_start_;
    return PA_OK;
}

// WIN_OK: p is the window being scanned. WIN_HEAD: a record longer than the head room — p has been dropped, the next one starts at the record
int WindowFeed::enqueue_scan(Pre& p) {
    const int r = window_enqueue_scan(x_, p.plan, *p.c, rec_start_, scan_);
    if (r == WIN_HEAD) {
        const uint64_t main_from = p.plan.text_from;
        int e = drop_unscanned(p);
        if (e == PA_OK) e = regrow(WIN_HEAD, main_from, true);
        return e != PA_OK ? e : WIN_HEAD;
    }
    if (r != WIN_OK) return r;
    p.from = rec_start_;
    scanning_ = p;
    p.plan.active = false;
    next_id_ = scanning_.id + 1;
    return WIN_OK;
}

int WindowFeed::resolve(const Pre& p, FeedWindow& w) {
    BatchCtx& c = *p.c;
    const int r = window_scan_wait(x_, c, scan_);
    if (r != WIN_OK) return r;
    // (TextPipe refuses a window whose max_seq is beyond PA_MAX_READ_LEN right here. The feed does not, here or in host_next: its consumer may keep only a
    // prefix of a read — R1 of pa_count_cells / pa_write_bus — and the paired host path refuses a long read where it is encoded, so the device path does too)
    const FqInfo& info = *c.h_info.get();
    w.d_raw = c.d_raw.get();
    w.raw_bytes = c.raw_end;
    w.d_rec = c.d_rec.get();
    w.n = info.n;
    w.max_seq = info.max_seq;
    w.ready = c.ev_info;
    w.slot = feed_slot_of(p.id);
    rec_start_ = p.from + info.consumed;
    return WIN_OK;
}

int WindowFeed::next(FeedWindow& w) {
    w = FeedWindow();
    int e = PA_OK;
    for (;;) {
        if (ended_) return PA_OK;
        if (host_mode_) return host_next(w);
        if (!scanning_.plan.active) {
            if (!cur_.plan.active && (e = start_window(cur_, next_id_)) != PA_OK) return e;
            if (!cur_.plan.active) { if ((e = enter_host(rec_start_)) != PA_OK) return e; continue; }   // nothing (more) for the GPU's scan
            const int r = enqueue_scan(cur_);
            if (r == WIN_HEAD) continue;
            if (r != WIN_OK) return r;
        }
        // the next window's text is read and sent while the GPU finds this one's records
        if (!cur_.plan.active && (e = start_window(cur_, next_id_)) != PA_OK) return e;
        const Pre done = scanning_;
        scanning_.plan.active = false;
        const int r = resolve(done, w);
        if (r == WIN_ODD || r == WIN_EMPTY) {   // the window is dropped, and the one sent behind it
            const bool more = cur_.plan.active;
            const uint64_t main_from = cur_.plan.text_from;
            if ((e = drop_unscanned(cur_)) != PA_OK) return e;
            rec_start_ = done.from;
            next_id_ = done.id;
            w = FeedWindow();
            if ((e = regrow(r, main_from, more)) != PA_OK) return e;
            continue;
        }
        if (r != WIN_OK) return r;
        delivered_ += w.n;
        if (cur_.plan.active) {   // its scan runs while the caller works on the window handed out now
            const int q = enqueue_scan(cur_);
            if (q != WIN_OK && q != WIN_HEAD) return q;
        }
        return PA_OK;
    }
}

// ---- the rest of the text (its end; all of it when it is not in four-line shape): the host's scan, uploaded as windows of the same form ----
int WindowFeed::enter_host(uint64_t from) {
    gpu_mode_ = false;
    host_mode_ = true;
    PA_HIP_TRY(hipStreamSynchronize(copy_));
    PA_HIP_TRY(hipStreamSynchronize(scan_));
    uint64_t at = from;
    int e = PA_OK;
    // BGZF: what is left (the last KEEP bytes; everything from here on when the text is not in four-line shape) is inflated by the host's pool
    if (x_.text.bgzf && (e = bgzf_materialise(x_.text, x_.path, x_.pool, &at)) != PA_OK) return e;
    x_.text.off = at;
    ws_.reset(new WindowScan(x_.text));
    host_at_ = 0;
    host_before_ = delivered_;
    return PA_OK;
}

int WindowFeed::host_next(FeedWindow& w) {
    WindowScan& ws = *ws_;
    if (host_at_ >= ws.nrec) {
        const double t0 = now();
        host_before_ += ws.nrec;
        const int e = ws.next(x_.path, host_before_, x_.pool, rec_pos_, brk_);
        x_.st[ST_SCAN] += now() - t0;
        if (e != PA_OK) return e;
        host_at_ = 0;
        if (ws.nrec == 0) { ended_ = true; return PA_OK; }
    }
    const uint64_t i0 = host_at_, i1 = host_tail_cut(rec_pos_.data(), ws.nrec, ws.size, i0, host_batch_recs_), id = next_id_;
    Slot* sp = nullptr;
    int e = acquire(id, &sp);
    if (e != PA_OK) return e;
    BatchCtx& c = sp->c;
    if ((e = window_fill_host(x_, ws, rec_pos_.data(), i0, i1, delivered_, c, &w.max_seq)) != PA_OK) return e;   // (no floor for max_seq: a window of empty reads has 0)
    const double t0 = now();
    if ((e = window_send_host(x_, c, i1 - i0, copy_)) != PA_OK) return e;
    PA_HIP_TRY(hipEventRecord(c.ev_info, copy_));
    // (the pinned text and records of the slot are written again only when the slot comes round: the copies out of them are waited for here, at the price of
    // one wait per host window — this part is bound by the host's scan)
    PA_HIP_TRY(hipEventSynchronize(c.ev_info));
    x_.st[ST_LAUNCH] += now() - t0;
    w.d_raw = c.d_raw.get();
    w.raw_bytes = c.raw_end;
    w.d_rec = c.d_rec.get();
    w.n = i1 - i0;
    w.ready = c.ev_info;
    w.slot = feed_slot_of(id);
    host_at_ = i1;
    next_id_ = id + 1;
    delivered_ += w.n;
    return PA_OK;
}

}  // namespace ingest
}  // namespace pa
