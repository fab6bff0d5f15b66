// The window steps of text_window.hpp that touch the file, the pool or the GPU.
#include "text_window.hpp"

#include <cerrno>

namespace pa {
namespace ingest {

uint64_t window_from_env(uint64_t batch) {
    uint64_t window = 64ull << 20;
    if (const char* v = getenv("PA_INGEST_WINDOW")) { const long long x = atoll(v); if (x >= 1) window = (uint64_t)x; }
    return window_clamp(window, batch);
}

void read_piece(WindowCtx& x, uint64_t a, uint64_t b, uint8_t* dst) {
    const FastqText& text = x.text;
    if (text.mapped && text.data == text.map_base && !x.use_pread) {
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
            if (got <= 0) { x.read_bad.store(1); return; }
            p += (uint64_t)got;
        }
    } else memcpy(dst, text.data + a, (size_t)(b - a));
}

int window_fill(WindowCtx& x, const WindowPlan& plan, BatchCtx& c, bool wait) {
    int e = window_ensure_raw(c, WINDOW_HEAD_ROOM + plan.text_len);
    if (e != PA_OK) return e;
    const double t0 = now();
    if (plan.n_members) {
        if ((e = window_ensure_comp(c, plan.comp_len, plan.n_members)) != PA_OK) return e;
        for (uint64_t i = 0; i < plan.n_members; ++i) {
            pa_bgzf_member r = x.text.members[plan.first_member + i];
            r.in_off -= plan.comp_from;
            c.h_mrows.get()[i] = r;
        }
        const uint8_t* const src = (const uint8_t*)x.text.map_base + plan.comp_from;
        uint8_t* const dst = c.h_comp.get();
        x.read_async = deal_pieces(x.pool, plan.comp_len, wait, [src, dst](uint64_t a, uint64_t b) { copy_streaming(dst + a, src + a, (size_t)(b - a)); });
    } else {
        WindowCtx* const xp = &x;
        uint8_t* const dst = c.h_raw.get() + WINDOW_HEAD_ROOM;
        const uint64_t off = plan.text_from;
        x.read_async = deal_pieces(x.pool, plan.text_len, wait, [xp, off, dst](uint64_t a, uint64_t b) { read_piece(*xp, off + a, off + b, dst + a); });
    }
    x.st[ST_READ] += now() - t0;
    return wait ? window_fill_end(x) : PA_OK;
}

int window_fill_end(WindowCtx& x) {
    const double t0 = now();
    if (x.read_async) { x.pool.end(); x.read_async = false; }
    x.st[ST_READ] += now() - t0;
    return x.read_bad.exchange(0) ? fail(PA_ERR_IO, "%s: read failed: %s", x.path, strerror(errno)) : PA_OK;
}

int window_send(WindowCtx& x, const WindowPlan& plan, BatchCtx& c, hipStream_t copy) {
    const double t0 = now();
    c.n_members = plan.n_members;
    if (plan.n_members) {   // BGZF: the compressed members cross the link, the text first exists in HBM
        PA_HIP_TRY(hipMemcpyAsync(c.d_comp.get(), c.h_comp.get(), plan.comp_len, hipMemcpyHostToDevice, copy));
        PA_HIP_TRY(hipMemcpyAsync(c.d_mrows.get(), c.h_mrows.get(), plan.n_members * sizeof(pa_bgzf_member), hipMemcpyHostToDevice, copy));
        const int e = bgzf_inflate_launch(c.d_comp.get(), plan.comp_len, c.d_mrows.get(), plan.n_members, c.d_raw.get() + WINDOW_HEAD_ROOM, plan.text_len, c.d_mstat.get(), copy);
        if (e != PA_OK) return e;
        PA_HIP_TRY(hipMemcpyAsync(c.h_mstat.get(), c.d_mstat.get(), plan.n_members * sizeof(uint32_t), hipMemcpyDeviceToHost, copy));
        x.stats.members_gpu += plan.n_members;
        x.stats.bytes_h2d += plan.comp_len + plan.n_members * sizeof(pa_bgzf_member);
        x.stats.text_bytes_gpu += plan.text_len;
    } else {
        PA_HIP_TRY(hipMemcpyAsync(c.d_raw.get() + WINDOW_HEAD_ROOM, c.h_raw.get() + WINDOW_HEAD_ROOM, plan.text_len, hipMemcpyHostToDevice, copy));
        x.stats.bytes_h2d += plan.text_len;
    }
    PA_HIP_TRY(hipEventRecord(c.ev_h2d, copy));
    x.st[ST_LAUNCH] += now() - t0;
    return PA_OK;
}

int window_enqueue_scan(WindowCtx& x, const WindowPlan& plan, BatchCtx& c, uint64_t rec_start, hipStream_t scan) {
    uint64_t head = 0, skip = 0;
    if (!window_head(plan.text_from, rec_start, &head, &skip)) return WIN_HEAD;
    double t0 = now();
    if (head) {
        uint8_t* const h = c.h_raw.get() + WINDOW_HEAD_ROOM - head;
        // (BGZF: the members that hold the unfinished record are inflated by this thread; otherwise one small piece, whatever the pool is doing)
        if (x.text.bgzf) { const int e = bgzf_read_host(x.text, x.path, rec_start, head, h); if (e != PA_OK) return e; }
        else read_piece(x, rec_start, rec_start + head, h);
        if (x.read_bad.exchange(0)) return fail(PA_ERR_IO, "%s: read failed: %s", x.path, strerror(errno));
        PA_HIP_TRY(hipMemcpyAsync(c.d_raw.get() + WINDOW_HEAD_ROOM - head, h, head, hipMemcpyHostToDevice, scan));
        x.stats.bytes_h2d += head;
    }
    x.st[ST_READ] += now() - t0; t0 = now();
    c.raw_begin = WINDOW_HEAD_ROOM - head + skip;
    c.raw_end = WINDOW_HEAD_ROOM + plan.text_len;
    int e = window_ensure_scan(c, 0);
    if (e != PA_OK) return e;
    PA_HIP_TRY(hipStreamWaitEvent(scan, c.ev_h2d, 0));
    if ((e = window_scan_enqueue(c, false, scan)) != PA_OK) return e;
    x.st[ST_LAUNCH] += now() - t0;
    return WIN_OK;
}

int window_scan_wait(WindowCtx& x, BatchCtx& c, hipStream_t scan) {
    const FqInfo& info = *c.h_info.get();
    for (int attempt = 0;; ++attempt) {
        const double t0 = now();
        PA_HIP_TRY(hipEventSynchronize(c.ev_info));
        x.st[ST_WAIT] += now() - t0;
        if (!info.overflow) break;
        if (attempt == 2) return fail(PA_ERR_INTERNAL, "FASTQ scan: line table too small after regrowing");
        ++x.rescans;   // more lines than guessed (short reads): grow the line table, fill it again from the counts already there
        int e = window_ensure_scan(c, info.lines);
        if (e != PA_OK) return e;
        if ((e = window_scan_enqueue(c, true, scan)) != PA_OK) return e;
    }
    for (uint64_t i = 0; i < c.n_members; ++i)   // (they came back on the copy stream ahead of ev_h2d, which the scan waited for)
        if (c.h_mstat.get()[i] != PA_INFLATE_OK)
            return fail(PA_ERR_FORMAT, "%s: corrupt gzip stream: member at byte %llu: %s", x.path, (unsigned long long)c.h_mrows.get()[i].file_off,
                        pa_inflate_status_name(c.h_mstat.get()[i]));
    return info.odd ? WIN_ODD : info.n == 0 ? WIN_EMPTY : WIN_OK;
}

int window_fill_host(WindowCtx& x, const WindowScan& ws, const RecPos* rp, uint64_t i0, uint64_t i1, uint64_t record_no, BatchCtx& c, uint32_t* maxlen) {
    const uint64_t n = i1 - i0, first = rp[i0].start, bytes = (i1 < ws.nrec ? rp[i1].start : ws.size) - first;
    rp += i0;
    if (bytes > (3ull << 30)) return fail(PA_ERR_UNSUPPORTED, "%s: record %llu is longer than 3 GiB", x.path, (unsigned long long)record_no);
    int e = window_ensure_raw(c, WINDOW_HEAD_ROOM + bytes);
    if (e != PA_OK) return e;
    if ((e = window_ensure_recs(c, n, true)) != PA_OK) return e;
    const double t0 = now();
    const char* const src = ws.base + first;
    uint8_t* const dst = c.h_raw.get() + WINDOW_HEAD_ROOM;
    deal_pieces(x.pool, bytes, true, [src, dst](uint64_t a, uint64_t b) { memcpy(dst + a, src + a, (size_t)(b - a)); });
    const int T4 = x.pool.size() * 4;
    std::vector<uint32_t> tmax((size_t)T4, 0);
    x.pool.run(T4, [&](int t) {
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
    *maxlen = 0;
    for (uint32_t m : tmax) *maxlen = std::max(*maxlen, m);
    x.st[ST_READ] += now() - t0;
    c.n_members = 0;
    c.raw_begin = WINDOW_HEAD_ROOM;
    c.raw_end = WINDOW_HEAD_ROOM + bytes;
    return PA_OK;
}

int window_send_host(WindowCtx& x, BatchCtx& c, uint64_t n, hipStream_t stream) {
    const uint64_t bytes = c.raw_end - c.raw_begin;
    PA_HIP_TRY(hipMemcpyAsync(c.d_raw.get() + WINDOW_HEAD_ROOM, c.h_raw.get() + WINDOW_HEAD_ROOM, bytes, hipMemcpyHostToDevice, stream));
    PA_HIP_TRY(hipMemcpyAsync(c.d_rec.get(), c.h_rec.get(), n * sizeof(uint4), hipMemcpyHostToDevice, stream));
    x.stats.bytes_h2d += bytes + n * sizeof(uint4);
    return PA_OK;
}

}  // namespace ingest
}  // namespace pa
