// The text of a FASTQ file as the host sees it (fastq_text.cpp): opened (mapped, or inflated when gzip'ed), scanned for its records a window
// at a time with the tolerant rules of bio's reader. What the file drivers share: pa_process_reads (fastq_reads.cpp) hands the host's scan
// the text its GPU scan does not take, the paired drivers (pair_reader.cpp under fastq_cells.cpp and fastq_pairs.cpp) walk their two files with it. What is done to a window of
// this text on its way to the GPU and behind it — for both of them — is text_window.hpp's.
#pragma once
#include <sys/mman.h>
#include <unistd.h>

#include <cstdint>
#include <new>
#include <vector>

#include "ingest.hpp"

namespace pa {
namespace ingest {

constexpr uint64_t DEFAULT_BATCH_READS = 2u << 20;   // (4 Mi reads left 1.3 GB of the mapping and 0.23 GB of text to the last, unoverlapped batch: 33 ms of tear-down per 8 M reads against 12)   // PA_INGEST_BATCH overrides (tests exercise the batch seams with small values)

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
    // A BGZF file (pa_bgzf_scan accepts it; pa_process_reads and the paired drivers' window feeds): the mapping is the COMPRESSED file (map_base / map_size, `mapped` stays false: nothing
    // may read text out of it), fsize = the bytes of text (sum of ISIZE), offsets everywhere are text offsets, `members` finds the bytes behind them.
    // data stays null until materialise() has inflated the text's tail on the host (the part the GPU windows do not take).
    bool bgzf = false;
    std::vector<pa_bgzf_member> members;
    uint64_t members_host = 0;      // members inflated by the host so far (pa_process_reads_input_stats)
    void release() {
        if (mapped || bgzf) munmap((void*)map_base, map_size);   // (the whole mapping: nobody gives parts of it back any more)
        if (fd >= 0) close(fd);
        fd = -1;
        mapped = false;
        bgzf = false;
        data = nullptr;
        fsize = 0;
    }
};

int open_fastq(const char* fastq_path, FastqText& t);
// bgzf.cpp (pa_process_reads, and the paired drivers when they take the device form): a file that is BGZF from first byte to last is opened as the BGZF kind above (t.bgzf set); anything else, an unreadable
// file included, leaves t untouched for open_fastq, with its results and its errors
void open_bgzf(const char* fastq_path, FastqText& t);
// BGZF kind: the index of the member that holds text offset `off` (the last member that starts at or before it: empty members in front are skipped)
uint64_t bgzf_member_at(const FastqText& t, uint64_t off);
// The next window of pa_process_reads: the text [text_from, text_from + text_len) behind read_to that the GPU scans, at most W bytes of it and none of the text's
// last KEEP bytes (the end of the text is the host's). Plain text: starts at read_to. BGZF kind: a run of whole members, from the member that holds read_to
// (read_to is a member's first byte except behind a discarded window: the scan then starts inside the member) to the last member boundary at or below
// text_from + W and fsize - KEEP; comp_from / comp_len are those members' bytes in the file. !active: nothing (no whole member) is left in front of the host's part.
// Arithmetic only: no buffer, no pool, no GPU (tests/plan drives it over made-up texts)
struct WindowPlan {
    bool active = false;
    uint64_t text_from = 0, text_len = 0;
    uint64_t first_member = 0, n_members = 0, comp_from = 0, comp_len = 0;   // (BGZF kind only)
};
WindowPlan plan_window(const FastqText& t, uint64_t read_to, uint64_t W, uint64_t KEEP);
// BGZF kind: text bytes [off, off + len) into dst, the members that hold them inflated by the calling thread with zlib, each checked (stream end, ISIZE, CRC-32).
// PA_ERR_FORMAT "corrupt gzip stream" naming the member's file offset otherwise
int bgzf_read_host(FastqText& t, const char* fastq_path, uint64_t off, uint64_t len, uint8_t* dst);
// BGZF kind: the text from the member that holds `from` to the end inflated into t.inflated by the pool; t.data / t.fsize then describe that tail as a text in
// memory and *from is rewritten to the same byte's offset in it
int bgzf_materialise(FastqText& t, const char* fastq_path, Pool& pool, uint64_t* from);

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
    explicit WindowScan(FastqText& t);
    // the next window with records in it (nrec = 0: the text has ended). records_before: records of the windows before (error messages)
    int next(const char* fastq_path, uint64_t records_before, Pool& pool, std::vector<RecPos>& rec_pos, std::vector<std::vector<uint32_t>>& brk);
};

// The id under which the two records of a pair are compared: record.id() of `len` bytes at s with one trailing "/1" or "/2" cut, and only from an id of at
// least two bytes. The host's pair reader calls it per record (pair_reader.cpp), tests/pairplan drives it over ids in buffers of exactly their length, and
// tests/pairscan_model.py states the same rule for the GPU's pair scan (pair_scan.hip)
inline uint32_t pair_id_len(const char* s, uint32_t len) {
    return len >= 2 && s[len - 2] == '/' && (s[len - 1] == '1' || s[len - 1] == '2') ? len - 2 : len;
}

// The C ABI's edge of a file driver: nothing thrown crosses it (std::bad_alloc out of the growable buffers, std::system_error out of thread creation)
template <class F>
int no_throw(const char* entry, F&& body) {
    try {
        return body();
    } catch (const std::bad_alloc&) {
        return fail(PA_ERR_OOM, "out of host memory in %s", entry);
    } catch (const std::exception& ex) {
        return fail(PA_ERR_INTERNAL, "%s: %s", entry, ex.what());
    }
}

}  // namespace ingest
}  // namespace pa
