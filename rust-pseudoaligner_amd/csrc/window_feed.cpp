// WindowFeed (window_feed.hpp): one FASTQ file as windows in HBM with their records beside them. The steps are TextPipe's (fastq_reads.cpp), which stays
// as it is: the two helpers that copy a piece of the mapping into pinned memory are written out here a second time (see DESIGN.md §4b.2 for the follow-up).
#include "window_feed.hpp"

#include <emmintrin.h>

#include <cerrno>
#include <chrono>

namespace pa {
namespace ingest {

namespace {

constexpr uint64_t PIECE = 2ull << 20;   // bytes of a window that one task of the pool copies

// bytes of the mapping into a pinned window with streaming stores: the window is read next by the copy engine, never by this CPU
void copy_streaming(uint8_t* d, const uint8_t* s, size_t n) {
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

}  // namespace

double WindowFeed::now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

WindowFeed::WindowFeed(const char* path, FastqText& text, Pool& pool, double* st, uint64_t window, uint64_t host_batch_recs)
    : path_(path), text_(text), pool_(pool), st_(st), W_(text.bgzf ? std::max<uint64_t>(window, PA_BGZF_MAX_ISIZE) : window),
      KEEP_(std::max<uint64_t>(4096, std::min<uint64_t>(W_ / 4, 1ull << 20))), host_batch_recs_(std::max<uint64_t>(1, host_batch_recs)) {
    stats_.text_kind = text.bgzf ? 2u : 0u;
    stats_.members_total = text.members.size();
}

WindowFeed::~WindowFeed() {
    for (hipStream_t s : {copy_, scan_})
        if (s) { (void)hipStreamSynchronize(s); (void)hipStreamDestroy(s); }
    for (Slot& s : slots_) {
        if (s.ev_free) (void)hipEventDestroy(s.ev_free);
        s.c.release();
    }
}

FeedStats WindowFeed::stats() const {
    FeedStats s = stats_;
    if (s.text_kind == 2) s.members_host = text_.members_host;
    return s;
}

int WindowFeed::start() {
    for (hipStream_t* sp : {&copy_, &scan_})
        if (hipStreamCreateWithFlags(sp, hipStreamNonBlocking) != hipSuccess) { *sp = nullptr; return fail(PA_ERR_HIP, "hipStreamCreate failed"); }
    gpu_mode_ = text_.fsize > KEEP_;
    return PA_OK;
}

// [0, len) dealt in pieces of PIECE bytes to the pool (and the caller): all of them done on return
template <class F>
void WindowFeed::deal_pieces(uint64_t len, F fn) {
    if (len == 0) return;
    const int ntask = (int)std::min<uint64_t>((len + PIECE - 1) / PIECE, 1u << 20);
    auto piece = [fn, len, ntask](int t) { fn(len * (uint64_t)t / (uint64_t)ntask, len * (uint64_t)(t + 1) / (uint64_t)ntask); };
    if (ntask == 1) piece(0);
    else pool_.run(ntask, piece);
}

// text bytes [a, b) of a plain mapped file to dst: out of the mapping, its page tables filled before the copy and dropped behind it (TextPipe::read_piece)
void WindowFeed::read_piece(uint64_t a, uint64_t b, uint8_t* dst) {
    constexpr uint64_t PAGE = 4096;
    const bool big = b - a >= (256u << 10);
    if (big) {
        const uint64_t pa = a & ~(PAGE - 1), pb = std::min<uint64_t>((b + PAGE - 1) & ~(PAGE - 1), text_.map_size);
#ifdef MADV_POPULATE_READ
        (void)madvise((void*)(text_.map_base + pa), (size_t)(pb - pa), MADV_POPULATE_READ);
#else
        (void)madvise((void*)(text_.map_base + pa), (size_t)(pb - pa), 22);
#endif
    }
    copy_streaming(dst, (const uint8_t*)text_.data + a, (size_t)(b - a));
    if (big) {
        const uint64_t qa = (a + PAGE - 1) & ~(PAGE - 1), qb = b & ~(PAGE - 1);
        if (qb > qa) (void)madvise((void*)(text_.map_base + qa), (size_t)(qb - qa), MADV_DONTNEED);
    }
}

int WindowFeed::read_small(uint64_t off, uint64_t len, uint8_t* dst) {   // a window's head (<= WINDOW_HEAD_ROOM), by the caller itself
    if (len == 0) return PA_OK;
    if (text_.bgzf) return bgzf_read_host(text_, path_, off, len, dst);   // (the members that hold the unfinished record: inflated by this thread)
    read_piece(off, off + len, dst);
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

// the next window (plan_window: none when the text in front of the host's part has been read): its bytes into the slot's pinned memory by the pool, then to
// the GPU on the copy stream; a BGZF window's members are inflated there, behind their copy, and their statuses come back ahead of ev_h2d
int WindowFeed::start_window(Pre& p, uint64_t id) {
    p.active = false;
    p.plan = gpu_mode_ ? plan_window(text_, read_to_, W_, KEEP_) : WindowPlan();
    const WindowPlan& plan = p.plan;
    if (!plan.active) return PA_OK;
    Slot* sp = nullptr;
    int e = acquire(id, &sp);
    if (e != PA_OK) return e;
    BatchCtx& c = sp->c;
    if ((e = window_ensure_raw(c, WINDOW_HEAD_ROOM + plan.text_len)) != PA_OK) return e;
    double t0 = now();
    if (plan.n_members) {
        if ((e = window_ensure_comp(c, plan.comp_len, plan.n_members)) != PA_OK) return e;
        for (uint64_t i = 0; i < plan.n_members; ++i) {
            pa_bgzf_member r = text_.members[plan.first_member + i];
            r.in_off -= plan.comp_from;
            c.h_mrows.get()[i] = r;
        }
        const uint8_t* const src = (const uint8_t*)text_.map_base + plan.comp_from;
        uint8_t* const dst = c.h_comp.get();
        deal_pieces(plan.comp_len, [src, dst](uint64_t a, uint64_t b) { copy_streaming(dst + a, src + a, (size_t)(b - a)); });
    } else {
        uint8_t* const dst = c.h_raw.get() + WINDOW_HEAD_ROOM;
        const uint64_t off = plan.text_from;
        deal_pieces(plan.text_len, [this, off, dst](uint64_t a, uint64_t b) { read_piece(off + a, off + b, dst + a); });
    }
    st_[1] += now() - t0; t0 = now();
    read_to_ = plan.text_from + plan.text_len;
    c.n_members = plan.n_members;
    if (plan.n_members) {   // BGZF: the compressed members cross the link, the text first exists in HBM
        PA_HIP_TRY(hipMemcpyAsync(c.d_comp.get(), c.h_comp.get(), plan.comp_len, hipMemcpyHostToDevice, copy_));
        PA_HIP_TRY(hipMemcpyAsync(c.d_mrows.get(), c.h_mrows.get(), plan.n_members * sizeof(pa_bgzf_member), hipMemcpyHostToDevice, copy_));
        if ((e = bgzf_inflate_launch(c.d_comp.get(), plan.comp_len, c.d_mrows.get(), plan.n_members, c.d_raw.get() + WINDOW_HEAD_ROOM, plan.text_len, c.d_mstat.get(), copy_)) != PA_OK) return e;
        PA_HIP_TRY(hipMemcpyAsync(c.h_mstat.get(), c.d_mstat.get(), plan.n_members * sizeof(uint32_t), hipMemcpyDeviceToHost, copy_));
        stats_.members_gpu += plan.n_members;
        stats_.bytes_h2d += plan.comp_len + plan.n_members * sizeof(pa_bgzf_member);
        stats_.text_bytes_gpu += plan.text_len;
    } else {
        PA_HIP_TRY(hipMemcpyAsync(c.d_raw.get() + WINDOW_HEAD_ROOM, c.h_raw.get() + WINDOW_HEAD_ROOM, plan.text_len, hipMemcpyHostToDevice, copy_));
        stats_.bytes_h2d += plan.text_len;
    }
    PA_HIP_TRY(hipEventRecord(c.ev_h2d, copy_));
    st_[3] += now() - t0;
    p.id = id;
    p.active = true;
    return PA_OK;
}

// a sent window that will not be scanned (the text is read again from an earlier offset, or the host's scan takes over): its copy is waited for
int WindowFeed::drop_unscanned(Pre& p) {
    if (!p.active) return PA_OK;
    p.active = false;
    PA_HIP_TRY(hipStreamSynchronize(copy_));
    return PA_OK;
}

// the window's records are to be found: the unfinished record of the window before goes in front of the window's own text as its head (on the scan stream,
// which then waits for the text itself), the scan follows
int WindowFeed::enqueue_scan(Pre& p) {
    BatchCtx& c = slots_[feed_slot_of(p.id)].c;
    const uint64_t main_from = p.plan.text_from;
    const uint64_t head = main_from > rec_start_ ? main_from - rec_start_ : 0;   // the unfinished record of the window before
    const uint64_t skip = rec_start_ > main_from ? rec_start_ - main_from : 0;   // (BGZF behind a dropped window: the first record starts inside the first member)
    if (head > WINDOW_HEAD_ROOM) {   // a record longer than the head room: a longer window, read again from the record's start
        W_ = std::max<uint64_t>(W_, 2 * head);
        return WIN_EMPTY;
    }
    double t0 = now();
    if (head) {
        uint8_t* const h = c.h_raw.get() + WINDOW_HEAD_ROOM - head;
        const int e = read_small(rec_start_, head, h);
        if (e != PA_OK) return e;
        PA_HIP_TRY(hipMemcpyAsync(c.d_raw.get() + WINDOW_HEAD_ROOM - head, h, head, hipMemcpyHostToDevice, scan_));
        stats_.bytes_h2d += head;
    }
    st_[1] += now() - t0; t0 = now();
    c.raw_begin = WINDOW_HEAD_ROOM - head + skip;
    c.raw_end = WINDOW_HEAD_ROOM + p.plan.text_len;
    int e = window_ensure_scan(c, 0);
    if (e != PA_OK) return e;
    PA_HIP_TRY(hipStreamWaitEvent(scan_, c.ev_h2d, 0));
    if ((e = window_scan_enqueue(c, false, scan_)) != PA_OK) return e;
    st_[3] += now() - t0;
    p.from = rec_start_;
    return WIN_OK;
}

// the window's scan: waited for; WIN_OK fills in w
int WindowFeed::resolve(const Pre& p, FeedWindow& w) {
    const int slot = feed_slot_of(p.id);
    BatchCtx& c = slots_[slot].c;
    const FqInfo& info = *c.h_info.get();
    for (int attempt = 0;; ++attempt) {
        const double t0 = now();
        PA_HIP_TRY(hipEventSynchronize(c.ev_info));
        st_[2] += now() - t0;
        if (!info.overflow) break;
        if (attempt == 2) return fail(PA_ERR_INTERNAL, "FASTQ scan: line table too small after regrowing");
        int e = window_ensure_scan(c, info.lines);   // more lines than guessed (short reads): grow the line table, fill it again from the counts already there
        if (e != PA_OK) return e;
        if ((e = window_scan_enqueue(c, true, scan_)) != PA_OK) return e;
    }
    for (uint64_t i = 0; i < c.n_members; ++i)   // (they came back on the copy stream ahead of ev_h2d, which the scan waited for)
        if (c.h_mstat.get()[i] != PA_INFLATE_OK)
            return fail(PA_ERR_FORMAT, "%s: corrupt gzip stream: member at byte %llu: %s", path_, (unsigned long long)c.h_mrows.get()[i].file_off,
                        pa_inflate_status_name(c.h_mstat.get()[i]));
    if (info.odd) return WIN_ODD;
    if (info.n == 0) return WIN_EMPTY;
    // (TextPipe refuses a window whose max_seq is beyond PA_MAX_READ_LEN right here. The feed does not, here or in host_next: its consumer may keep only a
    // prefix of a read — R1 of pa_count_cells / pa_write_bus — and the paired host path refuses a long read where it is encoded, so the device path does too)
    w.d_raw = c.d_raw.get();
    w.raw_bytes = c.raw_end;
    w.d_rec = c.d_rec.get();
    w.n = info.n;
    w.max_seq = info.max_seq;
    w.ready = c.ev_info;
    w.slot = slot;
    rec_start_ = p.from + info.consumed;
    return WIN_OK;
}

int WindowFeed::next(FeedWindow& w) {
    w = FeedWindow();
    int e = PA_OK;
    for (;;) {
        if (ended_) return PA_OK;
        if (host_mode_) return host_next(w);
        if (!scanning_.active) {
            if (!cur_.active && (e = start_window(cur_, next_id_)) != PA_OK) return e;
            if (!cur_.active) { if ((e = enter_host(rec_start_)) != PA_OK) return e; continue; }   // nothing (more) for the GPU's scan
            const int r = enqueue_scan(cur_);
            if (r == WIN_EMPTY) { if ((e = drop_unscanned(cur_)) != PA_OK) return e; read_to_ = rec_start_; continue; }
            if (r != WIN_OK) return r;
            scanning_ = cur_;
            cur_.active = false;
            next_id_ = scanning_.id + 1;
        }
        // the next window's text is read and sent while the GPU finds this one's records
        if (!cur_.active && (e = start_window(cur_, next_id_)) != PA_OK) return e;
        const Pre done = scanning_;
        scanning_.active = false;
        const int r = resolve(done, w);
        if (r == WIN_ODD || r == WIN_EMPTY) {   // not four-line text from here on: the host's scan takes over; no whole record in the window: a longer one
            const bool more = cur_.active;
            const uint64_t main_from = cur_.plan.text_from;
            if ((e = drop_unscanned(cur_)) != PA_OK) return e;
            rec_start_ = done.from;
            next_id_ = done.id;
            w = FeedWindow();
            if (r == WIN_ODD || !more) { if ((e = enter_host(rec_start_)) != PA_OK) return e; continue; }
            W_ = std::max<uint64_t>(2 * W_, 2 * (main_from - done.from));
            if (W_ > (1ull << 31)) { if ((e = enter_host(rec_start_)) != PA_OK) return e; continue; }   // (a record of gigabytes: the host's scan says what it is)
            read_to_ = rec_start_;
            continue;
        }
        if (r != WIN_OK) return r;
        if (cur_.active) {   // its scan runs while the caller works on the window handed out now
            const int q = enqueue_scan(cur_);
            if (q == WIN_EMPTY) { if ((e = drop_unscanned(cur_)) != PA_OK) return e; read_to_ = rec_start_; }
            else if (q != WIN_OK) return q;
            else { scanning_ = cur_; cur_.active = false; next_id_ = scanning_.id + 1; }
        }
        delivered_ += w.n;
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
    if (text_.bgzf && (e = bgzf_materialise(text_, path_, pool_, &at)) != PA_OK) return e;
    text_.off = at;
    ws_.reset(new WindowScan(text_));
    host_at_ = 0;
    host_before_ = delivered_;
    return PA_OK;
}

int WindowFeed::host_next(FeedWindow& w) {
    WindowScan& ws = *ws_;
    if (host_at_ >= ws.nrec) {
        const double t0 = now();
        host_before_ += ws.nrec;
        const int e = ws.next(path_, host_before_, pool_, rec_pos_, brk_);
        st_[0] += now() - t0;
        if (e != PA_OK) return e;
        host_at_ = 0;
        if (ws.nrec == 0) { ended_ = true; return PA_OK; }
    }
    const RecPos* const rp = rec_pos_.data();
    auto end_of = [&](uint64_t i) { return i < ws.nrec ? rp[i].start : ws.size; };
    // a batch of whole records whose text fits a window of 2 GiB (offsets into it are 32 bits)
    const uint64_t i0 = host_at_;
    uint64_t i1 = std::min<uint64_t>(ws.nrec, i0 + host_batch_recs_);
    while (i1 > i0 + 1 && end_of(i1) - rp[i0].start > (1ull << 31)) i1 = i0 + (i1 - i0) / 2;
    const uint64_t n = i1 - i0, first = rp[i0].start, bytes = end_of(i1) - first, id = next_id_;
    if (bytes > (3ull << 30)) return fail(PA_ERR_UNSUPPORTED, "%s: record %llu is longer than 3 GiB", path_, (unsigned long long)delivered_);
    Slot* sp = nullptr;
    int e = acquire(id, &sp);
    if (e != PA_OK) return e;
    BatchCtx& c = sp->c;
    if ((e = window_ensure_raw(c, WINDOW_HEAD_ROOM + bytes)) != PA_OK) return e;
    if ((e = window_ensure_recs(c, n, true)) != PA_OK) return e;
    double t0 = now();
    const char* const src = ws.base + first;
    uint8_t* const dst = c.h_raw.get() + WINDOW_HEAD_ROOM;
    deal_pieces(bytes, [src, dst](uint64_t a, uint64_t b) { memcpy(dst + a, src + a, (size_t)(b - a)); });
    const int T4 = pool_.size() * 4;
    std::vector<uint32_t> tmax((size_t)T4, 0);
    const RecPos* const rp0 = rp + i0;
    pool_.run(T4, [&](int t) {
        uint32_t mx = 0;
        for (uint64_t i = n * (uint64_t)t / (uint64_t)T4; i < n * (uint64_t)(t + 1) / (uint64_t)T4; ++i) {
            const RecPos& r = rp0[i];
            const uint64_t seq_off = std::min<uint64_t>(r.start + r.hdr + 1, ws.size);
            const uint32_t seq_len = (uint32_t)std::min<uint64_t>(r.seq_len, ws.size - seq_off);
            c.h_rec.get()[i] = make_uint4((uint32_t)(WINDOW_HEAD_ROOM + r.start + 1 - first), r.id_len, (uint32_t)(WINDOW_HEAD_ROOM + seq_off - first), seq_len);
            mx = std::max(mx, seq_len);
        }
        tmax[(size_t)t] = mx;
    });
    uint32_t maxlen = 0;
    for (uint32_t m : tmax) maxlen = std::max(maxlen, m);
    st_[1] += now() - t0; t0 = now();
    PA_HIP_TRY(hipMemcpyAsync(c.d_raw.get() + WINDOW_HEAD_ROOM, dst, bytes, hipMemcpyHostToDevice, copy_));
    PA_HIP_TRY(hipMemcpyAsync(c.d_rec.get(), c.h_rec.get(), n * sizeof(uint4), hipMemcpyHostToDevice, copy_));
    PA_HIP_TRY(hipEventRecord(c.ev_info, copy_));
    // (the pinned text and records of the slot are written again only when the slot comes round: the copies out of them are waited for here, at the price of
    // one wait per host window — this part is bound by the host's scan)
    PA_HIP_TRY(hipEventSynchronize(c.ev_info));
    st_[3] += now() - t0;
    stats_.bytes_h2d += bytes + n * sizeof(uint4);
    c.n_members = 0;
    c.raw_begin = WINDOW_HEAD_ROOM;
    c.raw_end = WINDOW_HEAD_ROOM + bytes;
    w.d_raw = c.d_raw.get();
    w.raw_bytes = c.raw_end;
    w.d_rec = c.d_rec.get();
    w.n = n;
    w.max_seq = maxlen;
    w.ready = c.ev_info;
    w.slot = feed_slot_of(id);
    host_at_ = i1;
    next_id_ = id + 1;
    delivered_ += n;
    return PA_OK;
}

}  // namespace ingest
}  // namespace pa
