// Stand-alone host check of the pair dictionary (csrc/device_layout.hpp, csrc/dict_slots.hpp): the mixing function and its inverse, the entry
// fields at their limits, the choice of format, and the builder's edges — keys placed by inverting the mixing function so that they land where
// a case needs them. TEST INFRASTRUCTURE ONLY (run as a child process by tests/test_dict_pairs.py, under ASan + UBSan).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <thread>
#include <vector>

#include "device_flatten.hpp"
#include "dict_slots.hpp"

using namespace pa;

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++failures; fprintf(stderr, "FAIL %s:%d: %s: ", __FILE__, __LINE__, #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } while (0)

// (HostAtomics: the CPU flattener's own policy type, csrc/dict_slots.hpp)

constexpr uint32_t B = 23;   // 2^23 pairs (128 MB): the smallest table whose tag has room for a displacement of three (pair_max_disp = 6)
constexpr uint32_t RBITS = PAIR_KEY_BITS - B;
constexpr uint32_t NPAIRS = 1u << B;

struct Key { uint64_t km; uint32_t handle, off; };
static Key key_at(uint32_t q, uint32_t r, uint32_t handle, uint32_t off) { return Key{pair_unmix(((uint64_t)q << RBITS) | r), handle, off}; }

struct Table {
    std::vector<uint64_t> w;
    std::vector<uint32_t> touched;   // pairs a case wrote (reset between cases instead of refilling 128 MB)
    Table() : w(2ull * NPAIRS, PAIR_EMPTY) {}
    void build(const std::vector<Key>& keys, int threads = 1) {
        auto pass = [&](auto fn) {
            if (threads <= 1) { for (const Key& k : keys) fn(k); return; }
            std::vector<std::thread> th;
            for (int t = 0; t < threads; ++t) th.emplace_back([&, t] { for (size_t i = t; i < keys.size(); i += threads) fn(keys[i]); });
            for (auto& x : th) x.join();
        };
        bool ok = true;
        pass([&](const Key& k) { if (!pair_insert<HostAtomics>(w.data(), B, k.km, k.handle, k.off)) ok = false; });
        CHECK(ok, "a key went further than pair_max_disp");
        pass([&](const Key& k) { pair_flag<HostAtomics>(w.data(), B, k.km); });
        for (const Key& k : keys) {
            const uint32_t q = (uint32_t)(pair_mix(k.km) >> RBITS);
            for (uint32_t d = 0; d <= pair_max_disp(B) + 1; ++d) touched.push_back((q + d) & (NPAIRS - 1));
        }
    }
    void reset() {
        for (uint32_t p : touched) w[2ull * p] = w[2ull * p + 1] = PAIR_EMPTY;
        touched.clear();
    }
    bool flagged(uint32_t p) const { return !((w[2ull * (p & (NPAIRS - 1))] >> PAIR_FLAG_BIT) & 1u); }
};

// every key is found where the layout says, with its handle and off
static void expect_found(const Table& t, const std::vector<Key>& keys, const std::vector<uint32_t>& probes, const char* what) {
    for (size_t i = 0; i < keys.size(); ++i) {
        uint32_t h = 0, o = 0, p = 99;
        const bool f = pair_find64(t.w.data(), B, keys[i].km, h, o, p);
        CHECK(f && h == keys[i].handle && o == keys[i].off && p == probes[i], "%s: key %zu found=%d handle=%u off=%u probes=%u (want %u %u %u)", what, i, (int)f, h, o, p,
              keys[i].handle, keys[i].off, probes[i]);
    }
}
static void expect_absent(const Table& t, uint64_t km, uint32_t probes, const char* what) {
    uint32_t h = 0, o = 0, p = 99;
    const bool f = pair_find64(t.w.data(), B, km, h, o, p);
    CHECK(!f && p == probes, "%s: absent key found=%d after %u further pairs (want %u)", what, (int)f, p, probes);
}
// no key that shares q with an inserted key and differs from it in one remainder bit is found
static void expect_neighbours_absent(const Table& t, const std::vector<Key>& keys, const char* what) {
    for (const Key& k : keys) {
        const uint64_t m = pair_mix(k.km);
        for (uint32_t bit = 0; bit < RBITS; ++bit) {
            const uint64_t other = pair_unmix(m ^ (1ull << bit));
            if (std::any_of(keys.begin(), keys.end(), [&](const Key& x) { return x.km == other; })) continue;
            uint32_t h, o, p;
            CHECK(!pair_find64(t.w.data(), B, other, h, o, p), "%s: a key one remainder bit from an inserted one is found", what);
        }
    }
}

static void test_mix() {
    std::mt19937_64 rng(1);
    std::vector<uint64_t> v{0, PAIR_KEY_MASK, 1, 1ull << 47};
    for (int i = 0; i < 200000; ++i) v.push_back(rng() & PAIR_KEY_MASK);
    for (uint64_t x : v) {
        const uint64_t m = pair_mix(x);
        CHECK(m <= PAIR_KEY_MASK && pair_unmix(m) == x && pair_mix(pair_unmix(x)) == x, "mix round trip of %llx", (unsigned long long)x);
    }
}

static void test_entry() {
    const uint32_t tags[] = {0u, (1u << 27) - 1u, (1u << PAIR_TAG_BITS) - 2u}, handles[] = {0u, PAIR_NO_HANDLE - 1u}, offs[] = {0u, PAIR_OFF_MASK};
    for (uint32_t t : tags)
        for (uint32_t h : handles)
            for (uint32_t o : offs) {
                const uint64_t e = pair_entry(t, h, o);
                CHECK(pair_entry_tag(e) == t && pair_entry_handle(e) == h && pair_entry_off(e) == o && ((e >> PAIR_FLAG_BIT) & 1u) && e != PAIR_EMPTY,
                      "entry round trip tag=%x handle=%x off=%x", t, h, o);
                const uint64_t f = e & ~(1ull << PAIR_FLAG_BIT);   // (the flag touches no field)
                CHECK(pair_entry_tag(f) == t && pair_entry_handle(f) == h && pair_entry_off(f) == o, "flagged entry tag=%x", t);
            }
    CHECK(pair_entry_handle(PAIR_EMPTY) == PAIR_NO_HANDLE, "the empty entry has the empty handle");
    CHECK(dict_entry_off(63, true, 3) <= PAIR_OFF_MASK && dict_entry_off(64 * 7 + 63, true, 3) == PAIR_OFF_MASK, "the off word has 11 bits");
    for (uint32_t b = PAIR_MIN_LOG2; b <= PAIR_MAX_LOG2; ++b) {   // the largest tag a lookup can ask for is not the empty entry's
        const uint32_t rbits = PAIR_KEY_BITS - b;
        const uint64_t top = (((uint64_t)pair_max_disp(b) << rbits) | ((1ull << rbits) - 1));
        CHECK(top < (1ull << PAIR_TAG_BITS) - 1, "b=%u: tag overflow", b);
    }
}

static void test_format() {
    const uint64_t nk = 1000000;
    CHECK(dict_pair_log2(24, 1000, nk, 0) == 21 && dict_pair_log2(21, 1000, nk, 0) == 21, "pair format at K = 24 and K = 21");
    CHECK(dict_pair_log2(25, 1000, nk, 0) == 0 && dict_pair_log2(31, 1000, nk, 0) == 0, "16-byte slots at K = 25 and K = 31");
    CHECK(dict_pair_log2(24, PAIR_MAX_BLOCKS, nk, 0) == 0 && dict_pair_log2(24, PAIR_MAX_BLOCKS - 1, nk, 0) != 0, "handle limit");
    CHECK(dict_pair_log2(24, 1000, 103900000ull, 0) == (PAIR_LOAD >= 0.7742 ? 27u : 28u), "config 3 sizing");
    CHECK(dict_pair_log2(24, 1000, (uint64_t)(PAIR_LOAD * (1u << 21)), 0) == 21 && dict_pair_log2(24, 1000, (uint64_t)(PAIR_LOAD * (1u << 21)) + 1, 0) == 22, "size threshold");
    CHECK(dict_pair_log2(24, 1000, nk, 2) == 23, "a table that was too small doubles");
    setenv("PA_PAIR_MAX_BLOCKS", "1000", 1);   // the hook only lowers the limit
    CHECK(dict_pair_log2(24, 1000, nk, 0) == 0 && dict_pair_log2(24, 999, nk, 0) == 21, "lowered handle limit");
    setenv("PA_PAIR_MAX_BLOCKS", "4000000000", 1);
    CHECK(dict_pair_log2(24, PAIR_MAX_BLOCKS, nk, 0) == 0, "the hook cannot raise the limit");
    unsetenv("PA_PAIR_MAX_BLOCKS");
    setenv("PA_PAIR_LOG2", "23", 1);
    CHECK(dict_pair_log2(24, 1000, nk, 0) == 23 && dict_pair_log2(31, 1000, nk, 0) == 0, "forced size");
    unsetenv("PA_PAIR_LOG2");
}

static void test_edges() {
    Table t;
    const uint32_t q = 12345;
    for (uint32_t n : {1u, 2u, 3u, 5u}) {   // n keys homed to one pair: the two smallest stay, the rest go on two by two
        std::vector<Key> keys;
        for (uint32_t i = 0; i < n; ++i) keys.push_back(key_at(q, 10 + 7 * i, 100 + i, (i * 0x2F5u) & PAIR_OFF_MASK));
        std::vector<Key> shuffled(keys.rbegin(), keys.rend());
        t.build(shuffled);
        std::vector<uint32_t> probes;
        for (uint32_t i = 0; i < n; ++i) probes.push_back(i / 2);
        expect_found(t, keys, probes, "keys of one home");
        expect_neighbours_absent(t, keys, "keys of one home");
        const uint32_t last = (n - 1) / 2;   // pairs q .. q + last hold keys; all but the last say that keys lie further on
        for (uint32_t d = 0; d <= last + 1; ++d) CHECK(t.flagged(q + d) == (d < last), "n=%u: flag of pair +%u", n, d);
        // an absent key of this home: one pair per flag it meets
        expect_absent(t, key_at(q, 5, 0, 0).km, last, n == 2 ? "absent, home full and not flagged" : "absent key of a shared home");
        // a carried key keeps its remainder: the key of the NEXT home with that remainder is another key, and absent
        if (n >= 3) expect_absent(t, key_at(q + 1, 10 + 7 * 2, 0, 0).km, n == 5 ? 1u : 0u, "the key a carried key would answer for without its displacement");
        t.reset();
    }
    for (uint32_t q0 : {777u, NPAIRS - 2u}) {   // a run of full pairs carries a key three pairs on (second: across the wrap to pair 0)
        std::vector<Key> keys{key_at(q0, 1, 1, 1), key_at(q0, 2, 2, 2), key_at(q0, 3, 3, 3)};
        const uint32_t m = NPAIRS - 1;
        keys.push_back(key_at((q0 + 1) & m, 50, 4, 4)); keys.push_back(key_at((q0 + 1) & m, 60, 5, 5));
        keys.push_back(key_at((q0 + 2) & m, 50, 6, 6)); keys.push_back(key_at((q0 + 2) & m, 60, 7, 7));
        keys.push_back(key_at((q0 + 3) & m, 50, 8, PAIR_OFF_MASK));
        t.build(keys, 4);
        expect_found(t, keys, {0, 0, 3, 0, 0, 0, 0, 0}, "carried three pairs on");
        expect_neighbours_absent(t, keys, "carried three pairs on");
        for (uint32_t d = 0; d < 5; ++d) CHECK(t.flagged(q0 + d) == (d < 3), "run from %u: flag of pair +%u", q0, d);
        expect_absent(t, key_at(q0, 9, 0, 0).km, 3, "absent, home full and flagged");                 // follows the flags to the first pair without one
        expect_absent(t, key_at((q0 + 1) & m, 9, 0, 0).km, 2, "absent, passes through flagged pairs of another home");
        expect_absent(t, key_at((q0 + 3) & m, 3, 0, 0).km, 0, "alias of the carried key at the pair it lies in");
        expect_absent(t, key_at((q0 + 4) & m, 9, 0, 0).km, 0, "absent, empty home");
        t.reset();
    }
    {   // the table does not depend on the order of insertion or on threads
        std::mt19937_64 rng(7);
        std::vector<Key> keys;
        for (uint32_t i = 0; i < 1500; ++i) keys.push_back(key_at(5000 + (uint32_t)(rng() % 2500), (uint32_t)(rng() & ((1u << RBITS) - 1)), i, i & PAIR_OFF_MASK));   // 0.6 keys per pair: by the Poisson figure of device_layout.hpp 4.6 % of the keys (69) lie off their home
        std::sort(keys.begin(), keys.end(), [](const Key& a, const Key& b) { return a.km < b.km; });
        keys.erase(std::unique(keys.begin(), keys.end(), [](const Key& a, const Key& b) { return a.km == b.km; }), keys.end());
        t.build(keys);
        std::vector<uint64_t> first(t.w.begin() + 2 * 4000, t.w.begin() + 2 * 8000);
        uint32_t far = 0;
        for (const Key& k : keys) { uint32_t h, o, p; CHECK(pair_find64(t.w.data(), B, k.km, h, o, p) && h == k.handle && o == k.off, "dense run: key lost"); far += p != 0; }
        CHECK(far > 30, "dense run: only %u keys off their home", far);
        for (int round = 0; round < 3; ++round) {
            t.reset();
            std::shuffle(keys.begin(), keys.end(), rng);
            t.build(keys, round == 0 ? 1 : 8);
            CHECK(std::equal(first.begin(), first.end(), t.w.begin() + 2 * 4000), "dense run: another order of insertion gives another table");
        }
        t.reset();
    }
}

int main() {
    test_mix();
    test_entry();
    test_format();
    test_edges();
    if (failures) { fprintf(stderr, "%d checks failed\n", failures); return 1; }
    printf("pairdict ok\n");
    return 0;
}
