// What of the window steps (csrc/text_window.hpp) is arithmetic or plain host code, driven without a GPU: copy_streaming against memcpy over every alignment,
// the window-size rule (window_head, window_rule, window_clamp, keep_of, window_of) over hand-written cases held against the formulas written out here, and
// host_tail_cut over made-up record starts. A stand-alone host program (tests/winsteps/build.py builds it under AddressSanitizer + UndefinedBehaviorSanitizer,
// tests/test_winsteps.py runs it); the functions are the product's own, included from the header. Prints one line per group, exits 1 on a miss.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "text_window.hpp"

using namespace pa::ingest;

namespace {

int misses = 0;
#define CHECK(cond, ...)                                        \
    do {                                                        \
        if (!(cond)) { if (++misses <= 20) { printf("MISS %s:%d %s: ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } } \
    } while (0)

typedef unsigned long long ull;

// ---- copy_streaming == memcpy, byte for byte, and nothing beside the destination is written ----
void check_copy() {
    constexpr size_t GUARD = 64, MAXLEN = 4096 + 63;
    std::vector<size_t> lens;
    for (size_t n = 0; n <= 200; ++n) lens.push_back(n);
    for (size_t extra : {0, 1, 63}) lens.push_back(4096 + extra);
    constexpr size_t DBYTES = (GUARD + 64 + MAXLEN + GUARD + 63) / 64 * 64, SBYTES = (16 + MAXLEN + 63) / 64 * 64;
    uint8_t* const dbuf = (uint8_t*)aligned_alloc(64, DBYTES);   // (64-byte aligned: destination offset 0 is a whole line's start)
    uint8_t* const sbuf = (uint8_t*)aligned_alloc(64, SBYTES);
    uint64_t s = 99;
    for (size_t i = 0; i < SBYTES; ++i) sbuf[i] = (uint8_t)pa::splitmix64(s);
    uint64_t copies = 0;
    for (size_t doff = 0; doff < 64; ++doff)
        for (size_t soff = 0; soff < 16; ++soff)
            for (size_t n : lens) {
                uint8_t* const d = dbuf + GUARD + doff;
                const uint8_t* const src = sbuf + soff;
                memset(dbuf + doff, 0xA5, GUARD + n + GUARD);   // the guards on both sides, and the destination itself
                copy_streaming(d, src, n);
                ++copies;
                bool same = memcmp(d, src, n) == 0, guards = true;
                for (size_t g = 0; g < GUARD; ++g) guards = guards && d[-(ptrdiff_t)g - 1] == 0xA5 && d[n + g] == 0xA5;
                CHECK(same, "destination offset %zu, source offset %zu, %zu bytes: the copy differs from memcpy", doff, soff, n);
                CHECK(guards, "destination offset %zu, source offset %zu, %zu bytes: a byte beside the destination was written", doff, soff, n);
            }
    free(dbuf);
    free(sbuf);
    printf("copy_streaming: %llu copies\n", (ull)copies);
}

// ---- the window-size rule ----
void expect_rule(const char* name, int answer, uint64_t W, uint64_t main_from, uint64_t from, bool more, uint64_t want_W, bool want_host) {
    const WindowRule r = window_rule(answer, W, main_from, from, more);
    CHECK(r.W == want_W && r.host == want_host, "%s: W %llu host %d, expected W %llu host %d", name, (ull)r.W, (int)r.host, (ull)want_W, (int)want_host);
}

void check_rule() {
    const uint64_t G2 = 1ull << 31, ROOM = WINDOW_HEAD_ROOM;
    // an empty window with a window behind it: max(2 W, 2 (main_from - from)), the host beyond 2^31
    expect_rule("empty, the window is what was short", WIN_EMPTY, 1000, 5000, 4200, true, std::max<uint64_t>(2 * 1000, 2 * (5000 - 4200)), false);
    expect_rule("empty, the text in front is longer than W", WIN_EMPTY, 1000, 5000, 1000, true, std::max<uint64_t>(2 * 1000, 2 * (5000 - 1000)), false);
    // ... and without one (the last window the GPU was given): the rest is the host's, W stays
    expect_rule("empty, nothing behind it", WIN_EMPTY, 1000, 0, 4200, false, 1000, true);
    expect_rule("odd", WIN_ODD, 1000, 5000, 4200, true, 1000, true);
    expect_rule("odd, nothing behind it", WIN_ODD, 1000, 0, 4200, false, 1000, true);
    // the head: exactly the head room fits; one more byte does not, and the window becomes max(W, 2 head)
    uint64_t head = 0, skip = 0;
    CHECK(window_head(5 * ROOM, 4 * ROOM, &head, &skip) && head == ROOM && skip == 0, "a head of exactly the head room: head %llu skip %llu", (ull)head, (ull)skip);
    CHECK(!window_head(5 * ROOM, 4 * ROOM - 1, &head, &skip) && head == ROOM + 1 && skip == 0, "a head of the head room + 1: head %llu skip %llu", (ull)head, (ull)skip);
    CHECK(window_head(700, 700, &head, &skip) && head == 0 && skip == 0, "no head: head %llu skip %llu", (ull)head, (ull)skip);
    CHECK(window_head(700, 912, &head, &skip) && head == 0 && skip == 212, "a first record inside the first member: head %llu skip %llu", (ull)head, (ull)skip);
    expect_rule("head one beyond the head room, small W", WIN_HEAD, 700, 5 * ROOM, 4 * ROOM - 1, true, std::max<uint64_t>(700, 2 * (ROOM + 1)), false);
    expect_rule("head one beyond the head room, large W", WIN_HEAD, 64 * ROOM, 5 * ROOM, 4 * ROOM - 1, true, std::max<uint64_t>(64 * ROOM, 2 * (ROOM + 1)), false);
    // the step that crosses 2^31: a window of exactly 2 GiB is still the GPU's, one beyond is the host's
    expect_rule("empty, 2 W = 2^31", WIN_EMPTY, G2 / 2, G2 / 2, 0, true, G2, false);
    expect_rule("empty, 2 W = 2^31 + 2", WIN_EMPTY, G2 / 2 + 1, G2 / 2 + 1, 0, true, std::max<uint64_t>(2 * (G2 / 2 + 1), 2 * (G2 / 2 + 1)), true);
    expect_rule("empty, the text in front crosses 2^31", WIN_EMPTY, 1000, 3 * G2, 3 * G2 - G2 / 2 - 1, true, 2 * (G2 / 2 + 1), true);
    expect_rule("head, 2 head = 2^31", WIN_HEAD, 1000, 3 * G2, 3 * G2 - G2 / 2, true, G2, false);
    expect_rule("head, 2 head = 2^31 + 2", WIN_HEAD, 1000, 3 * G2, 3 * G2 - G2 / 2 - 1, true, G2 + 2, true);
    // the window a call starts with: min(window, 256 bytes per read of a batch, 2^31); a BGZF window holds a whole member; KEEP = max(4096, min(W / 4, 2^20))
    CHECK(window_clamp(64ull << 20, 2u << 20) == (64ull << 20), "default window, default batch");
    CHECK(window_clamp(64ull << 20, 64) == 64 * 256, "a batch of 64 reads");
    CHECK(window_clamp(700, 333) == 700, "a window of 700 bytes");
    CHECK(window_clamp(1ull << 40, 1ull << 40) == G2, "nothing beyond 2^31");
    pa::ingest::FastqText plain, bgzf;
    bgzf.bgzf = true;
    CHECK(window_of(plain, 700) == 700 && window_of(bgzf, 700) == PA_BGZF_MAX_ISIZE && window_of(bgzf, 1u << 20) == (1u << 20), "window_of");
    CHECK(keep_of(700) == 4096 && keep_of(65536) == 16384 && keep_of(64ull << 20) == (1ull << 20) && keep_of(4 * 4096) == 4096 && keep_of(4 * 4097) == 4097, "keep_of");
    printf("window rule: done\n");
}

// ---- host_tail_cut: the batches cover every record exactly once, in order ----
void walk_cuts(const char* name, const std::vector<uint64_t>& starts, uint64_t size, uint64_t batch, uint64_t want_batches) {
    std::vector<RecPos> rp(starts.size());
    for (size_t i = 0; i < starts.size(); ++i) { rp[i] = RecPos(); rp[i].start = starts[i]; }
    const uint64_t nrec = rp.size();
    auto end_of = [&](uint64_t i) { return i < nrec ? starts[i] : size; };
    uint64_t i0 = 0, batches = 0, last_end = nrec ? starts[0] : 0;
    while (i0 < nrec) {
        const uint64_t i1 = host_tail_cut(rp.data(), nrec, size, i0, batch);
        CHECK(i1 > i0 && i1 <= nrec, "%s: cut [%llu, %llu) of %llu records", name, (ull)i0, (ull)i1, (ull)nrec);
        if (!(i1 > i0 && i1 <= nrec)) return;   // (would not end)
        CHECK(i1 - i0 <= batch, "%s: a batch of %llu records, at most %llu", name, (ull)(i1 - i0), (ull)batch);
        CHECK(end_of(i1) - starts[i0] <= (1ull << 31) || i1 == i0 + 1, "%s: a batch of %llu records holds %llu bytes", name, (ull)(i1 - i0), (ull)(end_of(i1) - starts[i0]));
        // the rule itself: the longest of batch, batch / 2, batch / 4, ... records (never more than are left) whose text fits 2 GiB
        uint64_t want = std::min<uint64_t>(nrec, i0 + batch);
        while (want > i0 + 1 && end_of(want) - starts[i0] > (1ull << 31)) want = i0 + (want - i0) / 2;
        CHECK(i1 == want, "%s: cut at %llu, the halving rule gives %llu", name, (ull)i1, (ull)want);
        CHECK(starts[i0] == last_end, "%s: the batch at record %llu starts at byte %llu, the one before ended at %llu", name, (ull)i0, (ull)starts[i0], (ull)last_end);
        last_end = end_of(i1);
        i0 = i1;
        ++batches;
    }
    CHECK(i0 == nrec && (nrec == 0 || last_end == size), "%s: the cuts end at record %llu, byte %llu of %llu", name, (ull)i0, (ull)last_end, (ull)size);
    CHECK(batches == want_batches, "%s: %llu batches, expected %llu", name, (ull)batches, (ull)want_batches);
    printf("host_tail_cut %s: %llu records in %llu batches\n", name, (ull)nrec, (ull)batches);
}

std::vector<uint64_t> every(uint64_t n, uint64_t step) {
    std::vector<uint64_t> v(n);
    for (uint64_t i = 0; i < n; ++i) v[i] = 17 + i * step;   // (the host's window does not have to start with a record)
    return v;
}

void check_cuts() {
    const uint64_t G = 1ull << 30;
    walk_cuts("a run that fits", every(1000, 316), 17 + 1000 * 316, 64, 16);                     // 15 batches of 64 and the last one of 40, ending at `size`
    walk_cuts("one batch", every(10, 316), 17 + 10 * 316 + 5, 64, 1);                             // (text behind the last record belongs to it)
    walk_cuts("batch of one", every(7, 316), 17 + 7 * 316, 1, 7);
    walk_cuts("records of 3 GiB", every(5, 3 * G), 17 + 5 * 3 * G, 8, 5);                         // 8 -> 4 -> 2 -> 1: down to one record, which no halving can shorten
    walk_cuts("records of 0.9 GiB", every(8, 9 * G / 10), 17 + 8 * (9 * G / 10), 8, 5);           // two records fit 2 GiB: 8 -> 4 -> 2 | 6 -> 3 -> 1 | 5 -> 2 | 3 -> 1 | 2
    walk_cuts("exactly 2 GiB", every(4, G), 17 + 4 * G, 2, 2);                                    // two records of 1 GiB are 2^31 bytes: they fit
    walk_cuts("no records", {}, 100, 64, 0);
}

}  // namespace

int main() {
    check_copy();
    check_rule();
    check_cuts();
    printf(misses ? "FAILED\n" : "OK\n");
    return misses ? 1 : 0;
}
