// pa_bgzf_scan: the member table of a BGZF file, found from header to header without inflating (host only; include/pseudoaligner_amd.h has the rules).
#include <fcntl.h>
#include <sys/stat.h>

#include "fastq_text.hpp"
#include "pa_common.hpp"

using namespace pa;

namespace {

inline uint32_t le16(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }
inline uint32_t le32(const uint8_t* p) { return le16(p) | (le16(p + 2) << 16); }

// one member at data[at ..): its row (in_off, in_len, out_len, crc32, file_off) and *block = its size in the file. false = not BGZF
bool parse_member(const uint8_t* data, uint64_t size, uint64_t at, pa_bgzf_member* m, uint64_t* block) {
    if (size - at < 12 + 6 + 8) return false;   // fixed header, XLEN, the BC subfield, trailer
    const uint8_t* h = data + at;
    if (h[0] != 0x1f || h[1] != 0x8b || h[2] != 8) return false;
    const uint32_t flg = h[3];
    if (!(flg & 4) || (flg & 0xE0)) return false;   // FEXTRA is what makes it BGZF; zlib refuses the reserved bits
    const uint32_t xlen = le16(h + 10);
    uint64_t p = 12;
    if (size - at < p + xlen) return false;
    uint32_t bsize = 0;
    bool have = false;
    uint64_t x = p;
    while (x < p + xlen) {   // every subfield is at least its four header bytes: the loop advances
        if (p + xlen - x < 4) return false;
        const uint32_t slen = le16(h + x + 2);
        if (p + xlen - x - 4 < slen) return false;
        if (h[x] == 'B' && h[x + 1] == 'C') {
            if (slen != 2) return false;
            if (!have) bsize = le16(h + x + 4);
            have = true;
        }
        x += 4 + slen;
    }
    if (!have) return false;
    const uint64_t blk = (uint64_t)bsize + 1;
    if (blk > size - at) return false;   // BSIZE beyond the end / truncated last member
    p += xlen;
    for (uint32_t bit = 8; bit <= 16; bit <<= 1) {   // FNAME, FCOMMENT: zero-terminated
        if (!(flg & bit)) continue;
        while (p < blk && h[p]) p++;
        if (p >= blk) return false;
        p++;
    }
    if (flg & 2) p += 2;   // FHCRC
    if (p + 8 > blk) return false;
    const uint32_t isize = le32(h + blk - 4);
    if (isize > PA_BGZF_MAX_ISIZE) return false;
    m->in_off = at + p;
    m->in_len = (uint32_t)(blk - 8 - p);
    m->out_len = isize;
    m->crc32 = le32(h + blk - 8);
    m->file_off = at;
    m->reserved = 0;
    *block = blk;
    return true;
}

}  // namespace

extern "C" int pa_bgzf_scan(const uint8_t* data, uint64_t size, pa_bgzf_member* members, uint64_t cap, uint64_t* n, uint64_t* text_bytes) {
    if (n) *n = 0;
    if (text_bytes) *text_bytes = 0;
    if (!n || (size && !data)) return fail(PA_ERR_INVALID_ARG, "pa_bgzf_scan: null argument");
    uint64_t at = 0, count = 0, text = 0;
    while (at < size) {   // every member is at least 26 bytes: the loop advances
        pa_bgzf_member m;
        uint64_t block = 0;
        if (!parse_member(data, size, at, &m, &block)) return fail(PA_ERR_NOT_BGZF, "not BGZF: member %llu at byte %llu", (unsigned long long)count, (unsigned long long)at);
        m.out_off = text;
        if (members && count < cap) members[count] = m;
        text += m.out_len;
        count++;
        at += block;
    }
    if (count == 0) return fail(PA_ERR_NOT_BGZF, "not BGZF: no bytes");
    *n = count;
    if (text_bytes) *text_bytes = text;
    if (members && cap < count) return fail(PA_ERR_BUFFER_TOO_SMALL, "pa_bgzf_scan: %llu members, room for %llu", (unsigned long long)count, (unsigned long long)cap);
    return PA_OK;
}

void pa::ingest::open_bgzf(const char* fastq_path, FastqText& t) {
    const int fd = open(fastq_path, O_RDONLY);
    if (fd < 0) return;
    struct stat st;
    if (fstat(fd, &st) != 0 || st.st_size < 28) { close(fd); return; }
    const uint64_t size = (uint64_t)st.st_size;
    void* m = mmap(nullptr, size, PROT_READ, MAP_PRIVATE, fd, 0);
    if (m == MAP_FAILED) { close(fd); return; }
    uint64_t n = 0, text_bytes = 0;
    const std::string before = last_error_ref();   // (a file that is not BGZF is no error of the call)
    if (pa_bgzf_scan((const uint8_t*)m, size, nullptr, 0, &n, &text_bytes) == PA_OK) {
        t.members.resize((size_t)n);
        if (pa_bgzf_scan((const uint8_t*)m, size, t.members.data(), n, &n, &text_bytes) == PA_OK) {
            t.bgzf = true;
            t.map_base = (const char*)m;
            t.map_size = size;
            t.fd = fd;
            t.fsize = text_bytes;
            t.data = nullptr;
            return;
        }
        t.members.clear();
    }
    last_error_ref() = before;
    munmap(m, size);
    close(fd);
}
