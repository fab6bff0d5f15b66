// Test-only probe of the text kernels of process_reads (tests/test_gpu_text_kernels.py; never linked into the product): record finding and
// in-place encode (csrc/fastq_scan.hip), tuple rendering (csrc/render.hip). tests/text/build.py compiles this file TOGETHER WITH those two
// sources (and csrc/fastq_text.cpp, the host's scan), as the product compiles them; the probe calls their launch functions on host arrays:
// every entry allocates device buffers, uploads the inputs AND the outputs (whatever pattern the caller filled an output with is what an
// element the kernels do not write still holds afterwards: guard elements behind every output show a write past its end), launches on the
// null stream, synchronises and downloads.
//
// Every entry checks on the host that what it is asked to launch stays inside the buffers it allocates (PA_ERR_INVALID_ARG otherwise): a
// wrong test must fail, never fault.
//
//   tp_scan         launch_fq_scan on text[begin, end), optionally again with rescan = true and other capacities on the same chunk tables
//   tp_encode_rec   launch_encode_rec
//   tp_render       launch_render_len + launch_render_write (scratch: render_scan_bytes)
//   tp_host_scan    the host's scan (WindowScan, fastq_text.cpp) with the id lengths pa_fastq_scan_host does not hand out; no GPU
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <string>
#include <vector>

#include "fastq_text.hpp"
#include "hip_buffer.hpp"
#include "kernels.hpp"
#include "pa_common.hpp"

// the two symbols of the host runtime the sources need (the product has them in host_index.cpp)
namespace pa {
std::string& last_error_ref() {
    static thread_local std::string s;
    return s;
}
int fail(int code, const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    last_error_ref() = buf;
    return code;
}
}  // namespace pa

using namespace pa;
typedef unsigned long long ull;
constexpr uint64_t TP_GUARD = 4;              // elements behind every output array
constexpr uint64_t TP_TEXT_SLACK = 64 << 10;  // sentinel bytes behind text_cap in the device's text buffer

namespace {

template <class T>
struct Dev {   // n elements of T in HBM holding a copy of h[0 .. n) (at least one element is allocated)
    DeviceBuffer<T> b;
    size_t n = 0;
    int up(const T* h, size_t count) {
        n = count;
        const int e = b.alloc(std::max<size_t>(count, 1));
        if (e != PA_OK) return e;
        if (count) PA_HIP_TRY(hipMemcpy(b.get(), h, count * sizeof(T), hipMemcpyHostToDevice));
        return PA_OK;
    }
    int down(T* h) const {
        if (n) PA_HIP_TRY(hipMemcpy(h, b.get(), n * sizeof(T), hipMemcpyDeviceToHost));
        return PA_OK;
    }
    T* get() const { return b.get(); }
};

int dev_sync() {
    PA_HIP_TRY(hipStreamSynchronize(nullptr));
    return PA_OK;
}

#define TRY(x) do { const int e_ = (x); if (e_ != PA_OK) return e_; } while (0)
#define LAUNCH(x) do { const int k_ = (x); if (k_) return fail(PA_ERR_HIP, "%s: %s", #x, hipGetErrorString((hipError_t)k_)); } while (0)

}  // namespace

extern "C" {

const char* tp_last_error(void) { return last_error_ref().c_str(); }
int tp_device_count(void) {
    int n = 0;
    return hipGetDeviceCount(&n) == hipSuccess ? n : 0;
}
uint64_t tp_guard(void) { return TP_GUARD; }
uint64_t tp_text_slack(void) { return TP_TEXT_SLACK; }
uint64_t tp_info_bytes(void) { return sizeof(FqInfo); }
uint32_t tp_flag_buckets(void) { return PA_RENDER_FLAG_BUCKETS; }
uint32_t tp_chunks(uint64_t begin, uint64_t end) { return fq_chunks(begin, end); }

// The records of text[begin, end). text has text_bytes >= end + 16 bytes (the product's window buffer has 64 spare bytes: the kernels load
// whole 16-byte groups). line_start has cap_lines + TP_GUARD elements, rec 4 * (cap_recs + TP_GUARD) (uint4 each), chunk and first
// tp_chunks(begin, end) + 1 + TP_GUARD. With cap_lines2 != 0 a second call with rescan = true follows on the same chunk tables, as
// ingest.hpp makes it after an overflow: line_start2 / rec2 / info2 receive its answer.
int tp_scan(const uint8_t* text, uint64_t text_bytes, uint64_t begin, uint64_t end, uint32_t* line_start, uint64_t cap_lines, uint32_t* rec, uint64_t cap_recs,
            FqInfo* info, uint32_t* line_start2, uint64_t cap_lines2, uint32_t* rec2, uint64_t cap_recs2, FqInfo* info2, uint32_t* chunk, uint32_t* first) {
    if (!text || begin >= end || end + 16 > text_bytes || end >= (1ull << 32) || cap_lines == 0)
        return fail(PA_ERR_INVALID_ARG, "tp_scan: window [%llu, %llu) of %llu bytes, %llu line starts", (ull)begin, (ull)end, (ull)text_bytes, (ull)cap_lines);
    const uint32_t n_chunks = fq_chunks(begin, end);
    const size_t tmp_bytes = fq_scan_tmp_bytes(n_chunks);
    Dev<uint8_t> dtext, dtmp;
    Dev<uint32_t> dls, dchunk, dfirst, dls2;
    Dev<uint4> drec, drec2;
    Dev<FqInfo> dinfo;
    TRY(dtext.up(text, text_bytes));
    TRY(dtmp.b.alloc(std::max<size_t>(tmp_bytes, 16)));
    TRY(dls.up(line_start, cap_lines + TP_GUARD));
    TRY(drec.up(reinterpret_cast<const uint4*>(rec), cap_recs + TP_GUARD));
    TRY(dchunk.up(chunk, n_chunks + 1 + TP_GUARD));
    TRY(dfirst.up(first, n_chunks + 1 + TP_GUARD));
    TRY(dinfo.up(info, 1));
    LAUNCH(launch_fq_scan(dtext.get(), begin, end, dchunk.get(), dfirst.get(), dtmp.get(), tmp_bytes, dls.get(), cap_lines, drec.get(), cap_recs, dinfo.get(), false, nullptr));
    TRY(dev_sync());
    TRY(dls.down(line_start));
    TRY(drec.down(reinterpret_cast<uint4*>(rec)));
    TRY(dinfo.down(info));
    if (cap_lines2) {
        TRY(dls2.up(line_start2, cap_lines2 + TP_GUARD));
        TRY(drec2.up(reinterpret_cast<const uint4*>(rec2), cap_recs2 + TP_GUARD));
        LAUNCH(launch_fq_scan(dtext.get(), begin, end, dchunk.get(), dfirst.get(), dtmp.get(), tmp_bytes, dls2.get(), cap_lines2, drec2.get(), cap_recs2, dinfo.get(), true, nullptr));
        TRY(dev_sync());
        TRY(dls2.down(line_start2));
        TRY(drec2.down(reinterpret_cast<uint4*>(rec2)));
        TRY(dinfo.down(info2));
    }
    TRY(dchunk.down(chunk));
    return dfirst.down(first);
}

// rec[n] = {-, -, sequence offset, sequence length} into text -> tiles[ceil(n / 64) * wpr * 64 + TP_GUARD], lens[n + TP_GUARD]
int tp_encode_rec(const uint8_t* text, uint64_t text_bytes, const uint32_t* rec, uint64_t n, uint32_t wpr, uint64_t* tiles, uint32_t* lens) {
    if (wpr == 0) return fail(PA_ERR_INVALID_ARG, "tp_encode_rec: wpr 0");
    for (uint64_t i = 0; i < n; ++i)
        if ((uint64_t)rec[4 * i + 2] + std::min<uint64_t>(rec[4 * i + 3], 32ull * wpr) > text_bytes)
            return fail(PA_ERR_INVALID_ARG, "tp_encode_rec: record %llu reads beyond the text", (ull)i);
    const uint64_t words = ((n + 63) / 64) * wpr * 64;
    Dev<uint8_t> dtext;
    Dev<uint4> drec;
    Dev<uint64_t> dtiles;
    Dev<uint32_t> dlens;
    TRY(dtext.up(text, text_bytes));
    TRY(drec.up(reinterpret_cast<const uint4*>(rec), n));
    TRY(dtiles.up(tiles, words + TP_GUARD));
    TRY(dlens.up(lens, n + TP_GUARD));
    LAUNCH(launch_encode_rec(dtext.get(), drec.get(), n, wpr, dtiles.get(), dlens.get(), nullptr));
    TRY(dev_sync());
    TRY(dtiles.down(tiles));
    return dlens.down(lens);
}

// The tuples of results[n]. The ids are ids[id_off[i] .. id_off[i + 1]) (rec == nullptr) or ids[rec[4i] .. rec[4i] + rec[4i + 1]); the arena's
// arena_cap entries lie at the END of their allocation; cls_off[num_classes + 1] into cls_txt. len and off have n + 1 + TP_GUARD elements,
// flagged PA_RENDER_FLAG_BUCKETS (added to). The device's text buffer has text_cap + TP_TEXT_SLACK bytes, all `sentinel` before the launch;
// afterwards its bytes [w0, w0 + w0_len) and [w1, w1 + w1_len) are copied to out0 / out1.
int tp_render(const pa_read_result* results, uint64_t n, const uint32_t* arena, uint64_t arena_cap, const uint8_t* ids, uint64_t ids_bytes, const uint64_t* id_off,
              const uint32_t* rec, const uint64_t* cls_off, uint64_t num_classes, const uint8_t* cls_txt, uint64_t flag_mark, uint64_t text_cap, uint8_t sentinel,
              uint32_t* len, uint64_t* off, ull* flagged, uint64_t w0, uint64_t w0_len, uint8_t* out0, uint64_t w1, uint64_t w1_len, uint8_t* out1) {
    const uint64_t text_alloc = text_cap + TP_TEXT_SLACK;
    if (w0 + w0_len > text_alloc || w1 + w1_len > text_alloc) return fail(PA_ERR_INVALID_ARG, "tp_render: a window beyond the text buffer");
    if (!id_off == !rec) return fail(PA_ERR_INVALID_ARG, "tp_render: id_off or rec");
    for (uint64_t i = 0; i < n; ++i) {
        const uint64_t b = rec ? rec[4 * i] : id_off[i], e = rec ? (uint64_t)rec[4 * i] + rec[4 * i + 1] : id_off[i + 1];
        if (b > e || e > ids_bytes) return fail(PA_ERR_INVALID_ARG, "tp_render: id %llu lies beyond the id bytes", (ull)i);
        if ((results[i].class_off & PA_CLASS_REF) && (results[i].class_off & ~PA_CLASS_REF) >= num_classes)
            return fail(PA_ERR_INVALID_ARG, "tp_render: record %llu refers to class %u of %llu", (ull)i, results[i].class_off & ~PA_CLASS_REF, (ull)num_classes);
    }
    for (uint64_t c = 0; c < num_classes; ++c)
        if (cls_off[c] > cls_off[c + 1]) return fail(PA_ERR_INVALID_ARG, "tp_render: class offsets descend");
    const size_t scan_bytes = render_scan_bytes(n);
    Dev<pa_read_result> dres;
    Dev<uint8_t> dids, dtxt, dscan, dtext;
    Dev<uint64_t> didoff, dclsoff, doff;
    Dev<uint4> drec;
    Dev<uint32_t> darena, dlen;
    Dev<ull> dflag;
    TRY(dres.up(results, n));
    TRY(dids.up(ids, ids_bytes));
    if (id_off) TRY(didoff.up(id_off, n + 1));
    if (rec) TRY(drec.up(reinterpret_cast<const uint4*>(rec), n));
    TRY(dclsoff.up(cls_off, num_classes + 1));
    TRY(dtxt.up(cls_txt, cls_off[num_classes]));
    // the arena at the end of an allocation of whole 4 KiB pages
    const size_t arena_alloc = (std::max<size_t>(arena_cap, 1) + 1023) / 1024 * 1024;
    TRY(darena.b.alloc(arena_alloc));
    uint32_t* const d_arena = darena.get() + (arena_alloc - arena_cap);
    PA_HIP_TRY(hipMemset(darena.get(), 0xEE, arena_alloc * 4));
    if (arena_cap) PA_HIP_TRY(hipMemcpy(d_arena, arena, arena_cap * 4, hipMemcpyHostToDevice));
    TRY(dlen.up(len, n + 1 + TP_GUARD));
    TRY(doff.up(off, n + 1 + TP_GUARD));
    TRY(dflag.up(flagged, PA_RENDER_FLAG_BUCKETS));
    TRY(dscan.b.alloc(std::max<size_t>(scan_bytes, 16)));
    TRY(dtext.b.alloc(text_alloc));
    PA_HIP_TRY(hipMemset(dtext.get(), sentinel, text_alloc));
    LAUNCH(launch_render_len(dres.get(), d_arena, dids.get(), id_off ? didoff.get() : nullptr, rec ? drec.get() : nullptr, dclsoff.get(), dtxt.get(), n, arena_cap, flag_mark,
                             dlen.get(), doff.get(), dflag.get(), dscan.get(), scan_bytes, nullptr));
    LAUNCH(launch_render_write(dres.get(), d_arena, dids.get(), id_off ? didoff.get() : nullptr, rec ? drec.get() : nullptr, dclsoff.get(), dtxt.get(), n, arena_cap,
                               doff.get(), dtext.get(), text_cap, nullptr));
    TRY(dev_sync());
    TRY(dlen.down(len));
    TRY(doff.down(off));
    TRY(dflag.down(flagged));
    if (w0_len) PA_HIP_TRY(hipMemcpy(out0, dtext.get() + w0, w0_len, hipMemcpyDeviceToHost));
    if (w1_len) PA_HIP_TRY(hipMemcpy(out1, dtext.get() + w1, w1_len, hipMemcpyDeviceToHost));
    return PA_OK;
}

// The host's scan of a FASTQ file, window by window as pa_fastq_scan_host walks it, with record.id()'s length: for the first `capacity`
// records the start of the '@', the bytes of the header line, the id's and the sequence's length. No GPU.
int tp_host_scan(const char* path, int threads, uint64_t* n_records, uint64_t* starts, uint32_t* header_len, uint32_t* id_len, uint32_t* seq_len, uint64_t capacity) {
    using namespace pa::ingest;
    *n_records = 0;
    FastqText text;
    int rc = open_fastq(path, text);
    if (rc != PA_OK) return rc;
    Pool pool(threads < 1 ? 1 : threads);
    std::vector<RecPos> rec_pos;
    std::vector<std::vector<uint32_t>> brk;
    uint64_t nrec = 0;
    WindowScan ws(text);
    while (rc == PA_OK) {
        rc = ws.next(path, nrec, pool, rec_pos, brk);
        if (rc != PA_OK || ws.nrec == 0) break;
        const uint64_t at = (uint64_t)(ws.base - text.data);
        for (uint64_t i = 0; i < ws.nrec && nrec + i < capacity; ++i) {
            starts[nrec + i] = at + rec_pos[i].start;
            header_len[nrec + i] = rec_pos[i].hdr;
            id_len[nrec + i] = rec_pos[i].id_len;
            seq_len[nrec + i] = rec_pos[i].seq_len;
        }
        nrec += ws.nrec;
    }
    if (rc == PA_OK) *n_records = nrec;
    text.release();
    return rc;
}

}  // extern "C"
