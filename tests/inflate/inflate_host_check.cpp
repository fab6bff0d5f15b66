// The decoder of csrc/inflate_core.hpp on a CPU, under ASan + UBSan (tests/inflate/build.py): every vector of tests/bgzf_cases.py goes through
// the same decode decisions here before it is sent to a GPU. A stand-alone program; never loaded into Python, never run on a GPU.
// The cooperative parts have scalar stand-ins: one lane, no barrier, the XOR over one value, a staged window copied byte by byte.
// The text buffer is exactly out_len bytes and the payload exactly in_len bytes on the heap, so one byte outside either is a sanitizer report.
//
// usage: inflate_host_check CASEFILE     CASEFILE: "PAIC" u32 n, then per member u32 in_len, u32 out_len, u32 crc32, in_len payload bytes
// prints one line per member: "<status> <crc32 of the text, 8 hex digits> <fnv1a of the text, 16 hex digits>"
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "inflate_core.hpp"

using namespace pa_inflate;

struct HostEnv {
    const uint8_t* comp;
    uint32_t in_len;
    uint32_t lane() const { return 0; }
    uint32_t lanes() const { return 1; }
    void sync() const {}
    uint32_t xor_all(uint32_t v) const { return v; }
    uint8_t payload(uint32_t i) const { return comp[i]; }   // unguarded on purpose: the caller's bound is what is under test
    void stage(uint8_t* win, int32_t origin) const {
        for (uint32_t i = 0; i < IN_WIN; i++) {
            const int64_t at = (int64_t)origin + i;
            win[i] = at >= 0 && at < (int64_t)in_len ? comp[at] : 0;
        }
    }
};

static bool rd32(FILE* f, uint32_t* v) {
    uint8_t b[4];
    if (fread(b, 1, 4, f) != 4) return false;
    *v = b[0] | (b[1] << 8) | (b[2] << 16) | ((uint32_t)b[3] << 24);
    return true;
}

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s CASEFILE\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    char magic[4];
    uint32_t n = 0;
    if (fread(magic, 1, 4, f) != 4 || memcmp(magic, "PAIC", 4) != 0 || !rd32(f, &n)) { fprintf(stderr, "bad case file\n"); return 2; }
    auto work = std::make_unique<Work>();
    for (uint32_t i = 0; i < n; i++) {
        uint32_t in_len, out_len, crc;
        if (!rd32(f, &in_len) || !rd32(f, &out_len) || !rd32(f, &crc) || in_len > (1u << 20) || out_len > PA_BGZF_MAX_ISIZE) { fprintf(stderr, "bad member %u\n", i); return 2; }
        std::vector<uint8_t> comp(in_len), text(out_len, 0xA5);
        if (in_len && fread(comp.data(), 1, in_len, f) != in_len) { fprintf(stderr, "short member %u\n", i); return 2; }
        HostEnv env{comp.data(), in_len};
        uint32_t got = 0;
        // the first window starts up to 15 bytes in front of the payload, as on the device (where it depends on the payload's address)
        const uint32_t st = inflate_member(env, *work, in_len, text.data(), out_len, crc, -(int32_t)(i % 16), &got);
        uint64_t h = 0xcbf29ce484222325ull;
        for (uint8_t b : text) h = (h ^ b) * 0x100000001b3ull;
        printf("%u %08x %016llx\n", st, got, (unsigned long long)h);
    }
    fclose(f);
    return 0;
}
