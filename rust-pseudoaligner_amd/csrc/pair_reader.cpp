// The paired drivers' reader in its two types, the function that chooses between them, and the call frame's open (pair_reader.hpp).
#include "pair_reader.hpp"

#include <atomic>
#include <string>

namespace pa {
namespace ingest {

uint64_t* last_pairs_input() {
    static thread_local uint64_t st[2 * PA_INGEST_INPUT_STATS + 1] = {0};
    return st;
}

namespace {

// an env switch: set to a number other than 0 (unset or empty: dflt)
bool env_on(const char* name, bool dflt = false) {
    const char* v = getenv(name);
    return v && *v ? atoi(v) != 0 : dflt;
}

void start_batch(MateBatch& b) {
    b.n = 0;
    for (Mate& m : b.mate) { m.bytes = 0; m.max_len = 0; }
}

// ---- the host type ----

// one FASTQ file of the pair, a window of records at a time (host memory follows the window, not the file; gzip is inflated whole)
struct PairCursor {
    const char* path = nullptr;
    FastqText text;
    std::unique_ptr<WindowScan> ws;
    std::vector<RecPos> rec;
    std::vector<std::vector<uint32_t>> brk;
    uint64_t at = 0, before = 0;   // next record of the window, records of the windows before it
    void adopt(const char* p, FastqText& opened) {   // a text that open_fastq has opened
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
    const char* id(uint64_t i, uint32_t& len) const {   // the id the pair is compared under
        const char* s = ws->base + rec[i].start + 1;
        len = pair_id_len(s, rec[i].id_len);
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

struct HostPairReader final : PairReader {
    PairCursor f[2];                    // R1, R2
    const int ntask;
    std::vector<uint64_t> part[2];      // per mate: the bytes in front of every task's pairs
    std::vector<uint32_t> part_max[2];  // ... and every task's longest piece
    HostPairReader(const char* r1, const char* r2, Pool& pl, uint32_t prefix_, double* st_, uint64_t batch, FastqText (&text)[2])
        : PairReader(r1, r2, pl, prefix_, st_, batch, false), ntask(pl.size() * 4) {
        for (int k = 0; k < 2; ++k) {
            f[k].adopt(k ? r2 : r1, text[k]);
            part[k].resize((size_t)ntask + 1);
            part_max[k].resize((size_t)ntask);
        }
    }
    ~HostPairReader() override { release(); }
    void release() override { f[0].text.release(); f[1].text.release(); }
    // the bytes of mate k's record i that are gathered: all of R2, the first `prefix` of R1
    uint32_t piece(int k, uint64_t i) const { return k ? f[1].rec[i].seq_len : std::min(f[0].rec[i].seq_len, prefix); }
    int gather(MateBatch& b) override {
        start_batch(b);
        int e = PA_OK;
        for (Mate& x : b.mate)
            if ((e = grow_pinned(x.h_off, batch_pairs + 1, 0)) != PA_OK) return e;
        if (prefix != 0xFFFFFFFFu && (e = grow_pinned(b.mate[0].h_bytes, (size_t)batch_pairs * prefix + 64, 0))) return e;
        while (b.n < batch_pairs) {
            uint64_t left[2] = {0, 0};
            double t0 = now();
            if ((e = f[0].ready(pool, left[0])) != PA_OK || (e = f[1].ready(pool, left[1])) != PA_OK) return e;
            st[ST_SCAN] += now() - t0;
            if (left[0] == 0 || left[1] == 0) {
                if (left[0] != left[1]) return no_mate(left[0], pairs + b.n);
                ended = true;
                break;
            }
            t0 = now();
            const uint64_t m = std::min(std::min(left[0], left[1]), batch_pairs - b.n), base = b.n;
            const uint64_t a[2] = {f[0].at, f[1].at};
            std::atomic<uint64_t> bad{~0ull};
            pool.run(ntask, [&](int t) {   // bytes of both mates per task, ids compared on the way
                uint64_t sum[2] = {0, 0};
                uint32_t mx[2] = {0, 0};
                for (uint64_t i = m * (uint64_t)t / ntask; i < m * (uint64_t)(t + 1) / ntask; ++i) {
                    uint32_t l1, l2;
                    const char* id1 = f[0].id(a[0] + i, l1);
                    const char* id2 = f[1].id(a[1] + i, l2);
                    if (l1 != l2 || memcmp(id1, id2, l1) != 0) {
                        uint64_t first = bad.load();
                        while (i < first && !bad.compare_exchange_weak(first, i)) {}
                    }
                    for (int k = 0; k < 2; ++k) {
                        const uint32_t len = piece(k, a[k] + i);
                        sum[k] += len;
                        mx[k] = std::max(mx[k], len);
                    }
                }
                for (int k = 0; k < 2; ++k) { part[k][(size_t)t + 1] = sum[k]; part_max[k][(size_t)t] = mx[k]; }
            });
            if (bad.load() != ~0ull) return ids_differ(pairs + base + bad.load());
            for (int k = 0; k < 2; ++k) {
                Mate& x = b.mate[k];
                part[k][0] = x.bytes;
                for (int t = 0; t < ntask; ++t) {
                    part[k][(size_t)t + 1] += part[k][(size_t)t];
                    x.max_len = std::max(x.max_len, part_max[k][(size_t)t]);
                }
                if ((e = grow_pinned(x.h_bytes, part[k][(size_t)ntask] + 64, x.bytes)) != PA_OK) return e;   // (a bounded prefix: sized above, nothing to do)
            }
            pool.run(ntask, [&](int t) {   // every task's pieces, back to back behind the tasks before
                for (int k = 0; k < 2; ++k) {
                    Mate& x = b.mate[k];
                    uint64_t o = part[k][(size_t)t];
                    for (uint64_t i = m * (uint64_t)t / ntask; i < m * (uint64_t)(t + 1) / ntask; ++i) {
                        const uint32_t len = piece(k, a[k] + i);
                        x.h_off.get()[base + i] = o;
                        memcpy(x.h_bytes.get() + o, f[k].seq(a[k] + i), len);
                        o += len;
                    }
                }
            });
            for (int k = 0; k < 2; ++k) { b.mate[k].bytes = part[k][(size_t)ntask]; f[k].at += m; }
            b.n += m;
            st[ST_READ] += now() - t0;
        }
        for (Mate& x : b.mate) x.h_off.get()[b.n] = x.bytes;
        return PA_OK;
    }
};

// ---- the device type ----

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

// the two files as window feeds, one stream for match + gather, the batch's control block
struct DevicePairReader final : PairReader {
    FastqText text[2];
    std::unique_ptr<WindowFeed> feed[2];
    FeedWindow win[2];
    uint64_t at[2] = {0, 0};       // next record of each file's window
    hipStream_t gs = nullptr;
    std::vector<hipStream_t> consumers;   // the streams the batches are consumed on
    DeviceBuffer<uint64_t> d_ctl;
    PinnedBuffer<uint64_t> h_ctl;
    DeviceBuffer<uint8_t> d_scratch;
    bool live = true;              // release() has work to do
    DevicePairReader(const char* r1, const char* r2, Pool& pl, uint32_t prefix_, double* st_, uint64_t batch, FastqText (&opened)[2])
        : PairReader(r1, r2, pl, prefix_, st_, batch, true) {
        for (int i = 0; i < 2; ++i) { text[i] = std::move(opened[i]); opened[i] = FastqText(); }
    }
    ~DevicePairReader() override { release(); }
    void consume_on(const hipStream_t* s, int n) override { consumers.assign(s, s + n); }
    int start() {
        const uint64_t window = window_from_env(batch_pairs);   // (PA_INGEST_BATCH as the paired drivers read it: any value >= 1)
        const char* const paths[2] = {r1_path, r2_path};
        int rc = PA_OK;
        PA_HIP_TRY(hipStreamCreateWithFlags(&gs, hipStreamNonBlocking));
        if ((rc = d_ctl.alloc(PA_PAIRS_CTL_WORDS)) != PA_OK || (rc = h_ctl.alloc(PA_PAIRS_CTL_WORDS)) != PA_OK) return rc;
        for (int i = 0; i < 2; ++i) {
            feed[i].reset(new WindowFeed(paths[i], text[i], pool, st, window, batch_pairs));
            if ((rc = feed[i]->start()) != PA_OK) return rc;
        }
        return PA_OK;
    }
    void release() override {
        if (!live) return;
        live = false;
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
        for (FastqText& t : text) { t.release(); t = FastqText(); }
    }
    // the next gather into the batch's buffers waits, on gs, for what its consumers were given last
    int consumed(MateBatch& b) override {
        for (size_t i = 0; i < consumers.size() && i < 2; ++i) {
            const int e = b.consumed[i].record(consumers[i]);
            if (e != PA_OK) return e;
            b.consumed[i].pending = true;
        }
        return PA_OK;
    }
    // the batch's control block, once, behind its gathers: the first bad id, the longest pieces, the bytes
    int close_device_batch(MateBatch& b) {
        Mate &m1 = b.mate[0], &m2 = b.mate[1];
        if (b.n == 0) return PA_OK;
        const double t0 = now();
        PA_HIP_TRY(hipMemcpyAsync(h_ctl.get(), d_ctl.get(), PA_PAIRS_CTL_WORDS * 8, hipMemcpyDeviceToHost, gs));
        PA_HIP_TRY(hipStreamSynchronize(gs));
        st[ST_WAIT] += now() - t0;
        const uint64_t* const c = h_ctl.get();
        if (c[5] != ~0ull) return fail(PA_ERR_INTERNAL, "pair scan: the record of pair %llu lies outside its window", (unsigned long long)(pairs + c[5]));
        if (c[0] != ~0ull) return ids_differ(pairs + c[0]);
        if (c[3] > m1.d_bytes.size() || c[4] > m2.d_bytes.size()) return fail(PA_ERR_INTERNAL, "pair scan: a batch of %llu + %llu bytes did not fit its buffers", (unsigned long long)c[3], (unsigned long long)c[4]);
        m1.max_len = (uint32_t)c[1];
        m2.max_len = (uint32_t)c[2];
        m1.bytes = c[3];
        m2.bytes = c[4];
        return PA_OK;
    }
    // segments of m = min(records left in R1's window, in R2's window, room in the batch) pairs, matched and gathered on gs
    int gather(MateBatch& b) override {
        Mate &m1 = b.mate[0], &m2 = b.mate[1];
        start_batch(b);
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
                if ((e = feed[i]->next(win[i])) != PA_OK) {   // (an id that differs in the pairs gathered so far is the earlier error, as with the host type)
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
                if (left1 != left2) return no_mate(left1, pairs + b.n);
                ended = true;
                return PA_OK;
            }
            const double t0 = now();
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
            st[ST_LAUNCH] += now() - t0;
        }
        return close_device_batch(b);
    }
};

}  // namespace

int open_pair_reader(const char* r1_path, const char* r2_path, Pool& pool, uint32_t prefix, double* st, std::unique_ptr<PairReader>& out) {
    uint64_t batch_pairs = DEFAULT_BATCH_READS;
    if (const char* v = getenv("PA_INGEST_BATCH")) { const long long x = atoll(v); if (x >= 1) batch_pairs = (uint64_t)x; }
    const bool host_only = env_on("PA_PAIRS_HOST_SCAN"), bgzf = !host_only && env_on("PA_INGEST_BGZF", true), plain_too = env_on("PA_PAIRS_DEVICE_PLAIN");
    const char* const paths[2] = {r1_path, r2_path};
    FastqText text[2];
    auto give_up = [&](int rc) { for (FastqText& t : text) t.release(); return rc; };
    int rc = PA_OK;
    bool takes = !host_only;
    for (int i = 0; i < 2; ++i) {
        if (bgzf) open_bgzf(paths[i], text[i]);
        if (!text[i].bgzf && (rc = open_fastq(paths[i], text[i])) != PA_OK) return give_up(rc);
        takes = takes && WindowFeed::takes(text[i]) && (text[i].bgzf || plain_too);
    }
    uint64_t* const is = last_pairs_input();
    memset(is, 0, sizeof(uint64_t) * (2 * PA_INGEST_INPUT_STATS + 1));
    if (takes) {   // (from here on the reader's release() reports the call's input, a call that ends in an error included)
        std::unique_ptr<DevicePairReader> dev(new DevicePairReader(r1_path, r2_path, pool, prefix, st, batch_pairs, text));
        if ((rc = dev->start()) != PA_OK) return rc;
        out = std::move(dev);
        return PA_OK;
    }
    // the host type for the whole call (a BGZF file is then inflated like any other .gz)
    for (int i = 0; i < 2; ++i)
        if (text[i].bgzf) { text[i].release(); text[i] = FastqText(); if ((rc = open_fastq(paths[i], text[i])) != PA_OK) return give_up(rc); }
    for (int i = 0; i < 2; ++i) is[i * PA_INGEST_INPUT_STATS] = text[i].inflated.empty() ? 0u : 1u;
    out.reset(new HostPairReader(r1_path, r2_path, pool, prefix, st, batch_pairs, text));
    return PA_OK;
}

int PairedCall::open(pa_index* idx, const char* r1_path, const char* r2_path, uint32_t prefix, int n_streams, int n_consumers) {
    pool.emplace(num_threads < 1 ? usable_threads() : num_threads);
    int rc = open_pair_reader(r1_path, r2_path, *pool, prefix, st, rd);
    if (rc != PA_OK) return rc;
    for (int j = 0; j < n_streams; ++j) {
        if ((rc = streams[j].create(idx)) != PA_OK) return rc;
        s[j] = streams[j].get();
    }
    rd->consume_on(s, n_consumers);
    return PA_OK;
}

int size_stage(pa_index* idx, ArenaBound bound_of, const pa_read_result* d_a, const pa_read_result* d_b, uint64_t n, size_t scratch_bytes, DeviceBuffer<uint8_t>& scratch,
               DeviceBuffer<uint32_t>& arena, hipStream_t s) {
    uint64_t bound = 0;
    int e = scratch.reserve(scratch_bytes, scratch_bytes + scratch_bytes / 4);
    if (e != PA_OK || (e = bound_of(idx, d_a, d_b, n, scratch.get(), s, &bound)) != PA_OK) return e;
    if (bound > PA_MAX_ARENA_ENTRIES) return fail(PA_ERR_UNSUPPORTED, "a batch of %llu pairs may need %llu arena entries: lower PA_INGEST_BATCH", (unsigned long long)n, (unsigned long long)bound);
    return arena.reserve(bound + 64, bound + bound / 4 + 4096);
}

}  // namespace ingest
}  // namespace pa
