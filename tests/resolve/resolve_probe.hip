// Test-only probe of pa_resolve_kernel (tests/test_gpu_resolve_edges.py; never linked into the product). This translation unit INCLUDES
// csrc/resolve.hip, so the kernel, launch_resolve and everything they inline (window_canon, window_class, class_of_list) are the product's own
// text compiled with the product's flags; the rest of the host runtime (pa::fail, pa::index_pair_view ...) comes from the product library the
// probe is linked against. The probe is linked -Bsymbolic: the launch_resolve it calls is the copy in here, whatever else the process has loaded.
//
// rsp_resolve takes a deferred-entry stream and every scalar of the launch as host values, VALIDATES them (nothing a test hands over can make
// the kernel read or write out of bounds), fills every output with a known pattern, runs launch_resolve once on one stream, synchronises and
// returns every buffer with guard words behind it. A HIP error comes back as PA_ERR_HIP with HIP's message in pa_last_error().
#include "resolve.hip"

#include <algorithm>
#include <vector>

#include "hip_buffer.hpp"

namespace {

using namespace pa;

constexpr uint32_t RSP_FILL = 0xA5C3B7E1u;                     // what every u32 output holds before the launch (no rid, no class, no key)
constexpr unsigned long long RSP_FILL64 = 0x5A17000000000000ull;   // counts[i] before the launch: this + i
constexpr uint64_t RSP_GUARD = 64;                            // words behind every buffer
constexpr uint32_t RSP_NO_KEYS = 1u, RSP_NO_COLOUR = 2u, RSP_NO_NOVEL = 4u;

uint32_t top_bit(uint32_t m) { return 31u - (uint32_t)__builtin_clz(m); }

// the entries the kernel may read, checked against everything it derives an address from
int entries_valid(const uint32_t* e, uint64_t n, uint64_t n_results, const uint32_t* arena, uint64_t arena_words, uint64_t num_tx) {
    std::vector<uint32_t> rids;
    rids.reserve(n);
    for (uint64_t i = 0; i < n; ++i) {
        const uint32_t* w = e + 8 * i;
        const unsigned long long at = i;
        if (w[0] == 0xFFFFFFFFu) continue;   // padding
        if (w[0] >= n_results) return fail(PA_ERR_INVALID_ARG, "entry %llu: rid %u outside the results", at, w[0]);
        rids.push_back(w[0]);
        const uint32_t kind = w[3] & 0xC0000000u, count = w[3] & 0x3FFFFFFFu;
        if (kind == PA_DEFER_WINDOW) {
            const uint32_t b1 = w[4], m1 = w[5], b2 = w[6], m2 = w[7];
            if (count == 0 || count != (uint32_t)(__builtin_popcount(m1) + __builtin_popcount(m2))) return fail(PA_ERR_INVALID_ARG, "entry %llu: count is not the bits of its masks", at);
            if (m2 && (uint64_t)b2 < (uint64_t)b1 + CLASS_WINDOW) return fail(PA_ERR_INVALID_ARG, "entry %llu: window 2 starts inside window 1", at);
            if (m1 && (uint64_t)b1 + top_bit(m1) >= num_tx) return fail(PA_ERR_INVALID_ARG, "entry %llu: window 1 holds an id that is no transcript", at);
            if (m2 && (uint64_t)b2 + top_bit(m2) >= num_tx) return fail(PA_ERR_INVALID_ARG, "entry %llu: window 2 holds an id that is no transcript", at);
        } else if (kind == PA_DEFER_LIST) {
            if (count == 0 || (uint64_t)w[4] + count > arena_words) return fail(PA_ERR_INVALID_ARG, "entry %llu: its list runs past the arena", at);
            for (uint32_t t = 0; t < count; ++t) {
                const uint32_t id = arena[w[4] + t];
                if (id >= num_tx || (t && id <= arena[w[4] + t - 1])) return fail(PA_ERR_INVALID_ARG, "entry %llu: its list is not ascending transcript ids", at);
            }
        } else return fail(PA_ERR_INVALID_ARG, "entry %llu is neither a window nor a list", at);
    }
    std::sort(rids.begin(), rids.end());
    if (std::adjacent_find(rids.begin(), rids.end()) != rids.end()) return fail(PA_ERR_INVALID_ARG, "two entries share a rid");
    return PA_OK;
}

template <class T> int put(DeviceBuffer<T>& d, const std::vector<T>& h, hipStream_t st) {
    if (const int e = d.alloc(h.size())) return e;
    PA_HIP_TRY(hipMemcpyAsync(d.get(), h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice, st));
    return PA_OK;
}

}  // namespace

extern "C" {

uint32_t rsp_fill() { return RSP_FILL; }
uint64_t rsp_fill64() { return RSP_FILL64; }
uint64_t rsp_guard() { return RSP_GUARD; }
uint32_t rsp_arena_chunk() { return PA_ARENA_CHUNK; }

// sizes of the index's two content tables; then (either may be NULL) wtable[16 wbuckets], class_table[class_table_size]
int rsp_tables(pa_index* idx, uint32_t* wbuckets, uint64_t* class_table_size, uint32_t* num_classes, int* num_cus, uint32_t* wtable, uint32_t* class_table) {
    if (!idx) return fail(PA_ERR_INVALID_ARG, "null argument");
    PairIndexView v;
    index_pair_view(idx, &v);
    PA_HIP_TRY(hipSetDevice(v.device));
    if (wbuckets) *wbuckets = v.dv.wbuckets;
    if (class_table_size) *class_table_size = v.class_table_size;
    if (num_classes) *num_classes = v.dv.num_classes;
    if (num_cus) *num_cus = v.num_cus;
    if (wtable) PA_HIP_TRY(hipMemcpy(wtable, v.dv.wtable, (size_t)v.dv.wbuckets * 64, hipMemcpyDeviceToHost));
    if (class_table) PA_HIP_TRY(hipMemcpy(class_table, v.class_table, v.class_table_size * 4, hipMemcpyDeviceToHost));
    return PA_OK;
}

// One launch_resolve. In: entries[8 n_entries] (the stream as the map kernel left it; min(defer_top, defer_cap) <= n_entries <= defer_cap),
// arena_in[arena_words] (what the arena holds at launch: the list entries' ids; arena_top0 is the launch's *arena_top), the scalars, flags
// (RSP_NO_*), num_tx (the index's transcript count). Out, each with rsp_guard() words behind it, all filled with rsp_fill() first (counts with
// rsp_fill64() + slot): results[4 n_results], arena_out[max(arena_words, arena_cap)], keys[keys_cap + defer_cap], colour[n_results],
// counts[num_classes + 3], novel[2 novel_cap], ctl[4] = {*arena_top, *status, *novel_ctr, *novel_status} (novel_ctr starts at novel_ctr0).
int rsp_resolve(pa_index* idx, const uint32_t* entries, uint64_t n_entries, uint64_t defer_top, uint64_t defer_cap, const uint32_t* arena_in, uint64_t arena_words,
                uint64_t arena_top0, uint64_t arena_cap, uint64_t n_results, uint64_t keys_top, uint64_t keys_cap, uint64_t novel_cap, uint64_t novel_ctr0, int num_cus,
                uint32_t flags, uint64_t num_tx, uint32_t* results, uint32_t* arena_out, uint32_t* keys, uint32_t* colour, unsigned long long* counts,
                uint32_t* novel, unsigned long long* ctl) {
    if (!idx || !results || !arena_out || !keys || !colour || !counts || !novel || !ctl || (n_entries && !entries) || (arena_words && !arena_in))
        return fail(PA_ERR_INVALID_ARG, "null argument");
    const uint64_t lim = 1ull << 28;   // nothing here comes near bit 31 of a class_off, and the sums below cannot wrap
    if (defer_cap > lim || arena_words > lim || arena_cap > lim || arena_top0 > lim || n_results > lim || keys_cap > lim || novel_cap > lim || num_cus < 1 || num_cus > 1024)
        return fail(PA_ERR_INVALID_ARG, "a size is out of range");
    if (n_entries > defer_cap || n_entries < std::min(defer_top, defer_cap)) return fail(PA_ERR_INVALID_ARG, "the stream does not hold what defer_top and defer_cap promise");
    PairIndexView v;
    index_pair_view(idx, &v);
    if (num_tx == 0 || num_tx > 32ull * (v.dv.bitmap_words - 2)) return fail(PA_ERR_INVALID_ARG, "num_tx is not the index's");
    if (const int e = entries_valid(entries, n_entries, n_results, arena_in, arena_words, num_tx)) return e;
    PA_HIP_TRY(hipSetDevice(v.device));
    hipStream_t st = nullptr;
    PA_HIP_TRY(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    struct StreamGuard { hipStream_t s; ~StreamGuard() { (void)hipStreamDestroy(s); } } sg{st};

    const uint64_t arena_n = std::max(arena_words, arena_cap), keys_n = keys_cap + defer_cap, counts_n = (uint64_t)v.dv.num_classes + 3;
    std::vector<uint32_t> h_defer(8 * std::max<uint64_t>(defer_cap, 1), RSP_FILL), h_res(4 * n_results + RSP_GUARD, RSP_FILL), h_arena(arena_n + RSP_GUARD, RSP_FILL),
        h_keys(keys_n + RSP_GUARD, RSP_FILL), h_col(n_results + RSP_GUARD, RSP_FILL), h_novel(2 * novel_cap + RSP_GUARD, RSP_FILL);
    std::vector<unsigned long long> h_counts(counts_n + RSP_GUARD), h_ctl(64, 0ull);   // a MapCtl's worth: the four words lie 64 bytes apart at least
    std::copy(entries, entries + 8 * n_entries, h_defer.begin());
    std::copy(arena_in, arena_in + arena_words, h_arena.begin());
    for (uint64_t i = 0; i < h_counts.size(); ++i) h_counts[i] = RSP_FILL64 + i;
    enum { C_ARENA_TOP = 0, C_STATUS = 8, C_NOVEL_CTR = 16, C_NOVEL_STATUS = 24, C_KEYS_TOP = 32, C_DEFER_TOP = 40 };
    h_ctl[C_ARENA_TOP] = arena_top0;
    h_ctl[C_NOVEL_CTR] = novel_ctr0;
    h_ctl[C_KEYS_TOP] = keys_top;
    h_ctl[C_DEFER_TOP] = defer_top;

    DeviceBuffer<uint32_t> d_defer, d_res, d_arena, d_keys, d_col, d_novel;
    DeviceBuffer<unsigned long long> d_counts, d_ctl;
    if (const int e = put(d_defer, h_defer, st)) return e;
    if (const int e = put(d_res, h_res, st)) return e;
    if (const int e = put(d_arena, h_arena, st)) return e;
    if (const int e = put(d_keys, h_keys, st)) return e;
    if (const int e = put(d_col, h_col, st)) return e;
    if (const int e = put(d_novel, h_novel, st)) return e;
    if (const int e = put(d_counts, h_counts, st)) return e;
    if (const int e = put(d_ctl, h_ctl, st)) return e;

    MapParams p{};
    p.ix = v.dv;
    p.results = reinterpret_cast<pa_read_result*>(d_res.get());
    p.arena = d_arena.get();
    p.arena_cap = arena_cap;
    p.colour_out = (flags & RSP_NO_COLOUR) ? nullptr : d_col.get();
    p.arena_top = d_ctl.get() + C_ARENA_TOP;
    p.status = reinterpret_cast<uint32_t*>(d_ctl.get() + C_STATUS);
    p.keys = (flags & RSP_NO_KEYS) ? nullptr : d_keys.get();
    p.keys_top = d_ctl.get() + C_KEYS_TOP;
    p.counts = d_counts.get();
    p.defer = d_defer.get();
    p.defer_top = d_ctl.get() + C_DEFER_TOP;
    p.keys_cap = keys_cap;
    p.defer_cap = defer_cap;
    p.class_table = v.class_table;
    p.class_table_size = v.class_table_size;
    p.novel_list = (flags & RSP_NO_NOVEL) ? nullptr : d_novel.get();
    p.novel_ctr = d_ctl.get() + C_NOVEL_CTR;
    p.novel_status = d_ctl.get() + C_NOVEL_STATUS;
    p.novel_cap = novel_cap;
    PA_HIP_TRY((hipError_t)launch_resolve(p, defer_cap, keys_cap, num_cus, st));

    PA_HIP_TRY(hipMemcpyAsync(results, d_res.get(), h_res.size() * 4, hipMemcpyDeviceToHost, st));
    PA_HIP_TRY(hipMemcpyAsync(arena_out, d_arena.get(), h_arena.size() * 4, hipMemcpyDeviceToHost, st));
    PA_HIP_TRY(hipMemcpyAsync(keys, d_keys.get(), h_keys.size() * 4, hipMemcpyDeviceToHost, st));
    PA_HIP_TRY(hipMemcpyAsync(colour, d_col.get(), h_col.size() * 4, hipMemcpyDeviceToHost, st));
    PA_HIP_TRY(hipMemcpyAsync(novel, d_novel.get(), h_novel.size() * 4, hipMemcpyDeviceToHost, st));
    PA_HIP_TRY(hipMemcpyAsync(counts, d_counts.get(), h_counts.size() * 8, hipMemcpyDeviceToHost, st));
    PA_HIP_TRY(hipMemcpyAsync(h_ctl.data(), d_ctl.get(), h_ctl.size() * 8, hipMemcpyDeviceToHost, st));
    PA_HIP_TRY(hipStreamSynchronize(st));
    ctl[0] = h_ctl[C_ARENA_TOP];
    ctl[1] = (uint32_t)h_ctl[C_STATUS];
    ctl[2] = h_ctl[C_NOVEL_CTR];
    ctl[3] = h_ctl[C_NOVEL_STATUS];
    if (h_ctl[C_KEYS_TOP] != keys_top || h_ctl[C_DEFER_TOP] != defer_top) return fail(PA_ERR_INTERNAL, "the kernel changed a stream head");
    return PA_OK;
}

}  // extern "C"
