// The FASTQ text on the host: a file opened (mapped; gzip inflated), its records found by counting lines — every host thread its byte
// range, nobody parses a byte twice or takes a lock — with the tolerances of bio's fastq::Reader (the reference's reader): CRLF, trailing
// blank lines, a last record without its quality line, wrapped sequence / quality lines (rewritten first). pa_fastq_scan_host runs the scan
// alone; the file drivers (fastq_reads.cpp, pair_reader.cpp) take their windows of records from it (fastq_text.hpp).
#include <fcntl.h>
#include <emmintrin.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>
#include <zlib.h>

#include <algorithm>
#include <atomic>
#include <cerrno>
#include <cstdlib>

#include "fastq_text.hpp"

using namespace pa;
using namespace pa::ingest;

namespace {

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

}  // namespace

namespace {
// one member inflated into out[0, out_len): nullptr, or what is wrong with it
const char* inflate_member_host(const uint8_t* comp, const pa_bgzf_member& m, uint8_t* out) {
    z_stream z;
    memset(&z, 0, sizeof z);
    if (inflateInit2(&z, -15) != Z_OK) return "zlib failed to start";
    uint8_t spare[8];
    z.next_in = const_cast<Bytef*>(comp + m.in_off);
    z.avail_in = m.in_len;
    z.next_out = m.out_len ? out : spare;
    z.avail_out = m.out_len ? m.out_len : 0;
    int r = inflate(&z, Z_FINISH);
    if (r != Z_STREAM_END && z.avail_out == 0) {   // the text is complete but the end-of-block bits are still to be read, or there is more text than ISIZE: spare room tells
        z.next_out = spare;
        z.avail_out = sizeof spare;
        r = inflate(&z, Z_FINISH);
    }
    const char* why = nullptr;
    if (r != Z_STREAM_END) why = z.msg ? "invalid deflate stream" : z.total_out > m.out_len ? "more text than ISIZE" : "input exhausted";
    else if (z.avail_in) why = "bytes behind the end of the stream";
    else if (z.total_out != m.out_len) why = z.total_out > m.out_len ? "more text than ISIZE" : "less text than ISIZE";
    else if ((uint32_t)crc32(crc32(0L, Z_NULL, 0), out, m.out_len) != m.crc32) why = "crc mismatch";
    inflateEnd(&z);
    return why;
}
}  // namespace

uint64_t pa::ingest::bgzf_member_at(const FastqText& t, uint64_t off) {
    uint64_t lo = 0, hi = t.members.size();   // the last member with out_off <= off
    while (hi - lo > 1) {
        const uint64_t mid = (lo + hi) / 2;
        if (t.members[mid].out_off <= off) lo = mid; else hi = mid;
    }
    return lo;
}

WindowPlan pa::ingest::plan_window(const FastqText& t, uint64_t read_to, uint64_t W, uint64_t KEEP) {
    WindowPlan p;
    if (read_to + KEEP >= t.fsize) return p;
    if (!t.bgzf) {
        p.text_from = read_to;
        p.text_len = std::min<uint64_t>(W, t.fsize - KEEP - read_to);
        p.active = true;
        return p;
    }
    auto end_of = [&t](uint64_t m) { return t.members[m].out_off + t.members[m].out_len; };
    const uint64_t m0 = bgzf_member_at(t, read_to), from = t.members[m0].out_off, limit = std::min<uint64_t>(from + W, t.fsize - KEEP);
    uint64_t m1 = m0;
    while (m1 < t.members.size() && end_of(m1) <= limit) ++m1;
    if (m1 == m0 || end_of(m1 - 1) <= read_to) return p;   // no whole member left in front of the host's part
    p.text_from = from;
    p.text_len = end_of(m1 - 1) - from;
    p.first_member = m0;
    p.n_members = m1 - m0;
    p.comp_from = t.members[m0].file_off;
    p.comp_len = (m1 < t.members.size() ? t.members[m1].file_off : t.map_size) - p.comp_from;
    p.active = true;
    return p;
}

int pa::ingest::bgzf_read_host(FastqText& t, const char* fastq_path, uint64_t off, uint64_t len, uint8_t* dst) {
    std::vector<uint8_t> tmp(PA_BGZF_MAX_ISIZE);
    const uint8_t* comp = (const uint8_t*)t.map_base;
    for (uint64_t i = bgzf_member_at(t, off); i < t.members.size() && t.members[i].out_off < off + len; ++i) {
        const pa_bgzf_member& m = t.members[i];
        if (m.out_len == 0) continue;
        if (const char* why = inflate_member_host(comp, m, tmp.data()))
            return fail(PA_ERR_FORMAT, "%s: corrupt gzip stream: member at byte %llu: %s", fastq_path, (unsigned long long)m.file_off, why);
        ++t.members_host;
        const uint64_t a = std::max<uint64_t>(off, m.out_off), b = std::min<uint64_t>(off + len, m.out_off + m.out_len);
        if (b > a) memcpy(dst + (a - off), tmp.data() + (a - m.out_off), (size_t)(b - a));
    }
    return PA_OK;
}

int pa::ingest::bgzf_materialise(FastqText& t, const char* fastq_path, Pool& pool, uint64_t* from) {
    const uint64_t first = t.fsize ? bgzf_member_at(t, std::min(*from, t.fsize - 1)) : 0, n = t.members.size() - first;
    const uint64_t base = t.members.empty() ? 0 : t.members[first].out_off;
    t.inflated.resize((size_t)(t.fsize - base));
    const uint8_t* comp = (const uint8_t*)t.map_base;
    std::atomic<uint64_t> bad{~0ull};
    const int ntask = (int)std::max<uint64_t>(1, std::min<uint64_t>(n, (uint64_t)pool.size() * 4));
    pool.run(ntask, [&](int k) {
        uint8_t spare[8];
        for (uint64_t i = first + n * (uint64_t)k / (uint64_t)ntask; i < first + n * (uint64_t)(k + 1) / (uint64_t)ntask; ++i) {
            const pa_bgzf_member& m = t.members[i];
            if (inflate_member_host(comp, m, m.out_len ? (uint8_t*)t.inflated.data() + (m.out_off - base) : spare)) {
                uint64_t cur = bad.load();
                while (i < cur && !bad.compare_exchange_weak(cur, i)) {}
            }
        }
    });
    if (bad.load() != ~0ull) {   // (said again by one thread, for the message)
        const pa_bgzf_member& m = t.members[bad.load()];
        std::vector<uint8_t> tmp(PA_BGZF_MAX_ISIZE + 8);
        const char* why = inflate_member_host(comp, m, tmp.data());
        return fail(PA_ERR_FORMAT, "%s: corrupt gzip stream: member at byte %llu: %s", fastq_path, (unsigned long long)m.file_off, why ? why : "corrupt");
    }
    t.members_host += n;
    *from -= base;
    t.data = t.inflated.data();
    t.fsize -= base;
    return PA_OK;
}

int pa::ingest::open_fastq(const char* fastq_path, FastqText& t) {
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

namespace {

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
                            // part of the id), after trailing white space was trimmed (str::trim_end: White_Space, in ASCII 0x09-0x0D — VT and FF too — and
                            // the blank). Found here, while the header's bytes are in the cache
                            uint64_t hend = e, ide = p + 1;
                            while (hend > p + 1 && (data[hend - 1] == ' ' || (uint8_t)(data[hend - 1] - 0x09) <= 0x0D - 0x09)) --hend;
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

}  // namespace

pa::ingest::WindowScan::WindowScan(FastqText& t) : text(t), windowed(t.mapped) {
    if (const char* v = getenv("PA_INGEST_WINDOW")) { const long long x = atoll(v); if (x >= 1) window = (uint64_t)x; }
}

int pa::ingest::WindowScan::next(const char* fastq_path, uint64_t records_before, Pool& pool, std::vector<RecPos>& rec_pos, std::vector<std::vector<uint32_t>>& brk) {
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
