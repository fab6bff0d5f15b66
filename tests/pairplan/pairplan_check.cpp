// The arithmetic of the paired drivers' device path that needs no GPU (csrc/window_feed.hpp: segment_pairs, feed_slot_of), driven over made-up sequences
// of window record counts the way DevicePairReader::gather (csrc/pair_reader.cpp) drives it: windows are refilled when they are used up, a batch is built from segments, a window
// is released when its last segment has been launched. Checked: every pair is taken exactly once and in order, a batch never exceeds batch_pairs, a window
// is never released before its last segment, the two files end together or the longer one is named, and the slot of a window is not taken again while the
// window and the two windows behind it (being scanned, being read) are alive. Stand-alone host program, built with -fsanitize=address,undefined.
// What this pins is the ARITHMETIC only: segment_pairs() and feed_slot_of() are the product's, the loop around them and the model of which slots are busy
// are written here after that gather and WindowFeed::next. The order in which WindowFeed::next itself takes slots (the window after next read into its
// slot before the next one is resolved, the ids taken again after an empty or odd window) is not seen by this program: it runs on the GPU tier only
// (tests/test_gpu_pairs_ingest.py with windows of 700 bytes).
// Also pinned here: pair_id_len (csrc/fastq_text.hpp), the rule under which the host's reader compares the ids of a pair, the product's own inline function.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "window_feed.hpp"

using namespace pa::ingest;

namespace {

int misses = 0;
#define CHECK(cond, ...)                                        \
    do {                                                        \
        if (!(cond)) { ++misses; printf("MISS %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } \
    } while (0)

struct File {   // a file as its feed hands it out: windows of counts[k] records (a feed never hands out an empty window, so zeros are skipped), then the end
    std::vector<uint64_t> counts;
    size_t k = 0;
    uint64_t id = 0;          // windows handed out so far
    uint64_t n = 0, at = 0;   // the window held: its records, the next one
    uint64_t first = 0;       // the file's record number of the held window's first record
    bool held = false;
    std::vector<int> slot_busy = std::vector<int>(FEED_SLOTS, 0);
    uint64_t total() const { uint64_t s = 0; for (uint64_t c : counts) s += c; return s; }
    void release() {
        CHECK(held && at == n, "a window of %llu records released at record %llu", (unsigned long long)n, (unsigned long long)at);
        slot_busy[(size_t)feed_slot_of(id - 1)] = 0;
        held = false;
    }
    void next() {
        first += n;
        n = at = 0;
        while (k < counts.size() && counts[k] == 0) ++k;
        if (k == counts.size()) return;
        n = counts[k++];
        // the window handed out now and the two behind it (scanned, read) hold three different slots, none of them a held one
        for (uint64_t j = id; j < id + 3; ++j)
            for (uint64_t i = id; i < j; ++i) CHECK(feed_slot_of(i) != feed_slot_of(j), "windows %llu and %llu share slot %d", (unsigned long long)i, (unsigned long long)j, feed_slot_of(j));
        CHECK(!slot_busy[(size_t)feed_slot_of(id)], "slot %d taken while its window is held", feed_slot_of(id));
        slot_busy[(size_t)feed_slot_of(id)] = 1;
        held = true;
        ++id;
    }
};

// -> pairs taken; *longer: 0 none, 1 / 2 the file that had records left
uint64_t drive(std::vector<uint64_t> c1, std::vector<uint64_t> c2, uint64_t batch_pairs, int* longer) {
    File f[2];
    f[0].counts = c1;
    f[1].counts = c2;
    uint64_t pairs = 0;
    bool ended = false;
    *longer = 0;
    while (!ended) {
        uint64_t n = 0;
        while (n < batch_pairs) {
            for (File& x : f) {
                if (x.at < x.n) continue;
                if (x.held) x.release();
                x.next();
            }
            const uint64_t left1 = f[0].n - f[0].at, left2 = f[1].n - f[1].at;
            if (left1 == 0 || left2 == 0) {
                if (left1 != left2) *longer = left1 ? 1 : 2;
                ended = true;
                break;
            }
            const uint64_t m = segment_pairs(left1, left2, batch_pairs, n);
            CHECK(m >= 1 && m <= left1 && m <= left2 && n + m <= batch_pairs, "segment of %llu pairs (left %llu / %llu, batch %llu + it of %llu)", (unsigned long long)m,
                  (unsigned long long)left1, (unsigned long long)left2, (unsigned long long)n, (unsigned long long)batch_pairs);
            if (m == 0) return pairs;   // (would not end)
            // in order and exactly once: the segment's first pair is the next record of both files
            CHECK(f[0].first + f[0].at == pairs + n && f[1].first + f[1].at == pairs + n, "pair %llu taken from records %llu / %llu", (unsigned long long)(pairs + n),
                  (unsigned long long)(f[0].first + f[0].at), (unsigned long long)(f[1].first + f[1].at));
            n += m;
            f[0].at += m;
            f[1].at += m;
        }
        CHECK(n <= batch_pairs, "a batch of %llu pairs", (unsigned long long)n);
        pairs += n;
        if (n == 0) break;
    }
    return pairs;
}

void expect(const char* name, std::vector<uint64_t> c1, std::vector<uint64_t> c2, uint64_t batch) {
    File a, b;
    a.counts = c1;
    b.counts = c2;
    const uint64_t t1 = a.total(), t2 = b.total();
    int longer = 0;
    const uint64_t got = drive(c1, c2, batch, &longer);
    CHECK(got == (t1 < t2 ? t1 : t2), "%s: %llu pairs taken of %llu / %llu", name, (unsigned long long)got, (unsigned long long)t1, (unsigned long long)t2);
    CHECK(longer == (t1 == t2 ? 0 : t1 > t2 ? 1 : 2), "%s: longer file %d", name, longer);
    printf("%s: %llu pairs, batch %llu, longer %d\n", name, (unsigned long long)got, (unsigned long long)batch, longer);
}

// pair_id_len over an id in a heap buffer of exactly its length (a look in front of a one-byte or empty id is a sanitizer finding); silent unless it misses
void expect_id(const char* id, uint32_t want) {
    const uint32_t len = (uint32_t)strlen(id);
    std::unique_ptr<char[]> buf(new char[len]);
    memcpy(buf.get(), id, len);
    const uint32_t got = pair_id_len(buf.get(), len);
    CHECK(got == want, "pair_id_len(\"%s\") = %u, not %u", id, got, want);
}

}  // namespace

int main() {
    // the cases of test_id_cut (tests/test_pairscan_model.py): "/1" or "/2" is cut once, and only from an id of at least two bytes
    expect_id("read7/1", 5); expect_id("read7/2", 5); expect_id("read7/3", 7); expect_id("read7/", 6); expect_id("read71", 6);
    expect_id("/1", 0); expect_id("/2", 0); expect_id("1", 1); expect_id("/", 1); expect_id("", 0); expect_id("a/1/1", 3);
    expect("equal windows", {100, 100, 100}, {100, 100, 100}, 64);
    expect("different windows", {7, 300, 1, 1, 91}, {150, 150, 100}, 64);
    expect("batch larger than everything", {5, 5, 5}, {15}, 1000);
    expect("batch of one", {3, 2}, {1, 1, 1, 1, 1}, 1);
    expect("empty windows", {0, 10, 0, 0, 10, 0}, {20, 0}, 7);
    expect("first file ends first", {100, 50}, {100, 100}, 64);
    expect("second file ends first", {100, 100, 3}, {100, 50}, 333);
    expect("one file empty", {}, {10}, 8);
    expect("both empty", {}, {}, 8);
    uint64_t s = 12345;   // made-up sequences from a small generator
    for (int round = 0; round < 200; ++round) {
        std::vector<uint64_t> c[2];
        uint64_t tot[2] = {0, 0};
        for (int k = 0; k < 2; ++k)
            for (int i = 0, w = 1 + (int)(pa::splitmix64(s) % 12); i < w; ++i) { c[k].push_back(pa::splitmix64(s) % 5 == 0 ? 0 : pa::splitmix64(s) % 400); tot[k] += c[k].back(); }
        if (round % 2 && tot[0] != tot[1]) c[tot[0] < tot[1] ? 0 : 1].push_back(tot[0] < tot[1] ? tot[1] - tot[0] : tot[0] - tot[1]);   // every other round: equal files
        int longer = 0;
        const uint64_t batch = 1 + pa::splitmix64(s) % 500;
        File a, b;
        a.counts = c[0];
        b.counts = c[1];
        const uint64_t got = drive(c[0], c[1], batch, &longer);
        CHECK(got == (a.total() < b.total() ? a.total() : b.total()), "round %d: %llu pairs", round, (unsigned long long)got);
    }
    printf("random rounds done\n");
    printf(misses ? "FAILED\n" : "OK\n");
    return misses ? 1 : 0;
}
