// BUS output (pa_bus, include/pseudoaligner_amd.h): every read becomes one 128-bit key, high word barcode | UMI, low word
// the equivalence class — its ec, or for an arena list of two ids or more the 64-bit hash of its content with bit 63 set (a sentinel not
// below any valid key when the read drops). A batch is radix-sorted over the key's used bits, equal keys are collapsed into (key, reads)
// entries appended to an accumulator in HBM, and one list per distinct hash of the batch — after every list under that hash was compared
// with it — goes to the host. finish() sorts and reduces the accumulator, lets the host number the lists (bus_host.cpp), replaces the
// hashes by ecs, sorts and reduces once more (a list that equals an index class joins that class's record) and writes whole records.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <memory>
#include <new>
#include <unordered_map>
#include <vector>

#include "bus_host.hpp"
#include "bus_records_host.hpp"
#include "bus_state.hpp"
#include "device_prims.hpp"
#include "hip_buffer.hpp"
#include "kernel_utils.hpp"
#include "pa_common.hpp"

using namespace pa;

namespace {

constexpr uint64_t BUS_WRITE_PIECE = 1u << 18;    // records (8 MiB) per piece of pa_bus_write
constexpr ull BUS_LIST_BIT = 1ull << 63;          // low key word: the hash of an arena list, not an ec

__device__ inline uint32_t bus_base(uint8_t c) { return c == 'A' ? 0u : c == 'C' ? 1u : c == 'G' ? 2u : c == 'T' ? 3u : 4u; }

struct BusKeyParams {
    const pa_read_result* results;
    const uint32_t* arena;
    uint64_t arena_len;
    const uint8_t* r1;
    const uint64_t* r1_off;
    uint64_t n;
    const uint32_t* class_ec;   // [num_classes]: the ec of an index class, CLASS_EC_NONE for one without ids
    uint32_t num_classes, num_tx;
    uint32_t bc_len, umi_len;
    u128 sentinel;
    u128* keys;
    uint32_t* vals;             // the read's number in the batch
    ull* stats;
};

// one lane per read: the six fates in the header's order, the key of a recorded read; fate counts summed per wave
__global__ __launch_bounds__(BUS_BLOCK) void pa_bus_keys_kernel(const BusKeyParams p) {
    const uint64_t i = (uint64_t)blockIdx.x * BUS_BLOCK + threadIdx.x;
    bool r1_short = false, barcode_n = false, umi_n = false, unmapped = false, bad_class = false, recorded = false;
    if (i < p.n) {
        const uint64_t off = p.r1_off[i];
        const uint64_t len = p.r1_off[i + 1] - off;
        u128 key = p.sentinel;
        if (len < (uint64_t)p.bc_len + p.umi_len) r1_short = true;
        else {
            ull w = 0;
            uint32_t bad_bc = 0, bad_umi = 0;
            for (uint32_t j = 0; j < p.bc_len; ++j) {
                const uint32_t b = bus_base(p.r1[off + j]);
                bad_bc |= b >> 2;
                w = (w << 2) | (b & 3u);
            }
            for (uint32_t j = 0; j < p.umi_len; ++j) {
                const uint32_t b = bus_base(p.r1[off + p.bc_len + j]);
                bad_umi |= b >> 2;
                w = (w << 2) | (b & 3u);
            }
            if (bad_bc) barcode_n = true;
            else if (bad_umi) umi_n = true;
            else {
                const pa_read_result r = p.results[i];
                ull lo = 0;
                if (!(r.mismatches & PA_MAPPED_BIT) || r.class_len == 0) unmapped = true;
                else if (r.class_off & PA_CLASS_REF) {
                    const uint32_t c = r.class_off & ~PA_CLASS_REF;
                    if (c >= p.num_classes) bad_class = true;
                    else {
                        const uint32_t ec = p.class_ec[c];
                        if (ec == bus::CLASS_EC_NONE) unmapped = true;
                        else { recorded = true; lo = ec; }
                    }
                } else if ((uint64_t)r.class_off + r.class_len > p.arena_len) bad_class = true;
                else {
                    const uint32_t* ids = p.arena + r.class_off;
                    uint64_t h = 0x243f6a8885a308d3ull ^ r.class_len;   // pa_mix64 chained over the ascending ids
                    uint32_t prev = 0;
                    bool ok = true;
                    for (uint32_t j = 0; j < r.class_len; ++j) {
                        const uint32_t t = ids[j];
                        if (t >= p.num_tx || (j && t <= prev)) { ok = false; break; }
                        h = pa_mix64(h ^ t) + 0x9e3779b97f4a7c15ull;
                        prev = t;
                    }
                    if (!ok) bad_class = true;
                    else {
                        recorded = true;
                        // (bit 0 cleared: no key of a recorded read has a low word of all ones, as the sentinel has)
                        lo = r.class_len == 1 ? (ull)ids[0] : ((h | BUS_LIST_BIT) & ~1ull);
                    }
                }
                if (recorded) key = ((u128)w << 64) | lo;
            }
        }
        p.keys[i] = key;
        p.vals[i] = (uint32_t)i;
    }
    // one atomic per wave and fate (wave64: 64-bit ballots)
    const bool fates[7] = {i < p.n, r1_short, barcode_n, umi_n, unmapped, bad_class, recorded};
    for (int f = 0; f < 7; ++f) {
        const ull m = __ballot(fates[f]);
        if ((threadIdx.x & 63) == 0 && m) atomicAdd(p.stats + f, (ull)__popcll(m));
    }
}

// ---- the arena lists of a batch ----
__device__ inline bool same_list(const pa_read_result a, const pa_read_result b, const uint32_t* __restrict__ arena) {
    if (a.class_len != b.class_len) return false;
    if (a.class_off == b.class_off) return true;
    for (uint32_t j = 0; j < a.class_len; ++j)
        if (arena[a.class_off + j] != arena[b.class_off + j]) return false;
    return true;
}
// every recorded read whose key holds a hash against the first read of its run (equal hash means the same list only after the contents
// were compared): *err = the hash of a run with two different lists
__global__ __launch_bounds__(BUS_BLOCK) void pa_bus_verify_members_kernel(const u128* __restrict__ keys, const uint32_t* __restrict__ vals, const uint32_t* __restrict__ pos,
                                                                           const uint32_t* __restrict__ start, uint32_t n, const pa_read_result* __restrict__ results,
                                                                           const uint32_t* __restrict__ arena, ull* __restrict__ err) {
    const uint32_t i = blockIdx.x * BUS_BLOCK + threadIdx.x;
    if (i >= n) return;
    const ull lo = key_lo(keys[i]);
    if (!(lo & BUS_LIST_BIT)) return;
    const uint32_t first = start[pos[i] - 1];
    if (first != i && !same_list(results[vals[i]], results[vals[first]], arena)) *err = lo;
}
__global__ __launch_bounds__(BUS_BLOCK) void pa_bus_list_flags_kernel(const u128* __restrict__ unique, uint32_t runs, uint32_t* __restrict__ flags) {
    const uint32_t r = blockIdx.x * BUS_BLOCK + threadIdx.x;
    if (r < runs) flags[r] = (key_lo(unique[r]) & BUS_LIST_BIT) ? 1u : 0u;
}
// the flagged runs -> (hash, the read that stands for the run)
__global__ __launch_bounds__(BUS_BLOCK) void pa_bus_list_gather_kernel(const u128* __restrict__ unique, const uint32_t* __restrict__ start, const uint32_t* __restrict__ vals,
                                                                        const uint32_t* __restrict__ which, uint32_t n_lists, ull* __restrict__ hash, uint32_t* __restrict__ read) {
    const uint32_t j = blockIdx.x * BUS_BLOCK + threadIdx.x;
    if (j >= n_lists) return;
    const uint32_t r = which[j];
    hash[j] = key_lo(unique[r]);
    read[j] = vals[start[r]];
}
// (hash, read) sorted by hash: every member of a run of equal hashes against the run's first; the first's list length -> lens[run]
__global__ __launch_bounds__(BUS_BLOCK) void pa_bus_verify_runs_kernel(const ull* __restrict__ hash, const uint32_t* __restrict__ read, const uint32_t* __restrict__ pos,
                                                                        const uint32_t* __restrict__ start, uint32_t n, const pa_read_result* __restrict__ results,
                                                                        const uint32_t* __restrict__ arena, ull* __restrict__ lens, ull* __restrict__ err) {
    const uint32_t j = blockIdx.x * BUS_BLOCK + threadIdx.x;
    if (j >= n) return;
    const uint32_t run = pos[j] - 1, first = start[run];
    if (first == j) lens[run] = results[read[j]].class_len;
    else if (!same_list(results[read[j]], results[read[first]], arena)) *err = hash[j];
}
// one list per distinct hash -> the pool: ids[off[run] ..]
__global__ __launch_bounds__(BUS_BLOCK) void pa_bus_pool_copy_kernel(const uint32_t* __restrict__ read, const uint32_t* __restrict__ start, uint32_t runs,
                                                                      const pa_read_result* __restrict__ results, const uint32_t* __restrict__ arena,
                                                                      const ull* __restrict__ off, uint32_t* __restrict__ ids) {
    const uint32_t run = blockIdx.x * BUS_BLOCK + threadIdx.x;
    if (run >= runs) return;
    const pa_read_result r = results[read[start[run]]];
    for (uint32_t j = 0; j < r.class_len; ++j) ids[off[run] + j] = arena[r.class_off + j];
}

// ---- finish ----
// hashes -> ecs by binary search in the table sorted by hash; a hash the table lacks: *err
__global__ __launch_bounds__(BUS_BLOCK) void pa_bus_remap_kernel(u128* __restrict__ keys, uint32_t n, const ull* __restrict__ table_hash, const uint32_t* __restrict__ table_ec,
                                                                  uint32_t table_n, ull* __restrict__ err) {
    const uint32_t i = blockIdx.x * BUS_BLOCK + threadIdx.x;
    if (i >= n) return;
    const u128 k = keys[i];
    const ull lo = key_lo(k);
    if (!(lo & BUS_LIST_BIT)) return;
    uint32_t a = 0, b = table_n;
    while (a < b) {
        const uint32_t mid = a + (b - a) / 2;
        if (table_hash[mid] < lo) a = mid + 1;
        else b = mid;
    }
    if (a < table_n && table_hash[a] == lo) keys[i] = ((u128)key_hi(k) << 64) | table_ec[a];
    else *err = lo;
}
}  // namespace

namespace {

int fetch_stats(pa_bus* b, hipStream_t s) {
    ull d[BS_RECORDS];
    PA_HIP_TRY(hipMemcpyAsync(d, b->d_stats.get(), sizeof d, hipMemcpyDeviceToHost, s));
    PA_HIP_TRY(hipStreamSynchronize(s));
    for (uint32_t j = 0; j < BS_RECORDS; ++j) b->stats[j] = d[j];
    return PA_OK;
}

int check_err(pa_bus* b, hipStream_t s, const char* what) {
    ull err = 0;
    const int e = fetch(b->d_err.get(), s, err);
    if (e != PA_OK) return e;
    if (err) return fail(PA_ERR_INTERNAL, "%s %016llx", what, err);
    return PA_OK;
}

// sorted keys[0 .. n) -> unique[runs], b->start[runs + 1] (b->heads and b->pos hold the flags and their scan afterwards); n >= 1
template <class K>
int collapse_keys(pa_bus* b, hipStream_t s, const K* keys, uint32_t n, K* unique, uint32_t& runs) {
    int e;
    if ((e = grow(b->heads, n)) || (e = grow(b->pos, n)) || (e = grow(b->start, (size_t)n + 1)) || (e = b->d_n.reserve(1, 1))) return e;
    return collapse_runs(s, b->tmp, KeyArray<K>{keys}, n, b->heads.get(), b->pos.get(), unique, b->start.get(), runs);
}

// the arena lists among the batch's `runs` new accumulator entries at `unique` (sorted reads in b->sorted / b->svals, their runs in
// b->start): verified on the device, one list per distinct hash appended to the host's pool
int collect_lists(pa_bus* b, hipStream_t s, const u128* unique, uint32_t runs, const pa_read_result* d_results, const uint32_t* d_arena) {
    int e;
    uint32_t n_lists = 0;
    if ((e = grow(b->which, runs)) != PA_OK) return e;
    // (heads is free again: the flags of the runs)
    if ((e = launch(pa_bus_list_flags_kernel, grid_for(runs, BUS_BLOCK), BUS_BLOCK, s, unique, runs, b->heads.get()))) return e;
    if ((e = select_flagged_indices(s, b->tmp, (const uint32_t*)b->heads.get(), (size_t)runs, b->which.get(), b->d_n.get())) || (e = fetch_u32(b->d_n.get(), s, n_lists)))
        return e;
    if (n_lists == 0) return PA_OK;
    if ((e = grow(b->lhash, n_lists)) || (e = grow(b->lhash_s, n_lists)) || (e = grow(b->lhash_u, n_lists)) || (e = grow(b->lread, n_lists)) ||
        (e = grow(b->lread_s, n_lists)) || (e = grow(b->lens, n_lists)) || (e = grow(b->loff, n_lists)))
        return e;
    // `start` is overwritten by the collapse below: the reads that stand for the runs are gathered first
    if ((e = launch(pa_bus_list_gather_kernel, grid_for(n_lists, BUS_BLOCK), BUS_BLOCK, s, unique, (const uint32_t*)b->start.get(), (const uint32_t*)b->svals.get(),
            (const uint32_t*)b->which.get(), n_lists, b->lhash.get(), b->lread.get()))) return e;
    if ((e = sort_pairs(s, b->tmp, (const ull*)b->lhash.get(), b->lhash_s.get(), (const uint32_t*)b->lread.get(), b->lread_s.get(), (int)n_lists, 0, 64))) return e;
    uint32_t distinct = 0;
    if ((e = collapse_keys<ull>(b, s, b->lhash_s.get(), n_lists, b->lhash_u.get(), distinct)) != PA_OK) return e;
    if ((e = launch(pa_bus_verify_runs_kernel, grid_for(n_lists, BUS_BLOCK), BUS_BLOCK, s, (const ull*)b->lhash_s.get(), (const uint32_t*)b->lread_s.get(),
            (const uint32_t*)b->pos.get(), (const uint32_t*)b->start.get(), n_lists, d_results, d_arena, b->lens.get(), b->d_err.get()))) return e;
    if ((e = scan_exclusive(s, b->tmp, (const ull*)b->lens.get(), b->loff.get(), (size_t)distinct))) return e;
    std::vector<ull> h_hash(distinct), h_off(distinct), h_len(distinct);
    PA_HIP_TRY(hipMemcpyAsync(h_hash.data(), b->lhash_u.get(), distinct * 8ull, hipMemcpyDeviceToHost, s));
    PA_HIP_TRY(hipMemcpyAsync(h_off.data(), b->loff.get(), distinct * 8ull, hipMemcpyDeviceToHost, s));
    PA_HIP_TRY(hipMemcpyAsync(h_len.data(), b->lens.get(), distinct * 8ull, hipMemcpyDeviceToHost, s));
    if ((e = check_err(b, s, "two different id lists share the content hash")) != PA_OK) return e;   // (synchronises)
    const uint64_t total = h_off[distinct - 1] + h_len[distinct - 1];
    if ((e = grow(b->pool_ids, (size_t)total)) != PA_OK) return e;
    if ((e = launch(pa_bus_pool_copy_kernel, grid_for(distinct, BUS_BLOCK), BUS_BLOCK, s, (const uint32_t*)b->lread_s.get(), (const uint32_t*)b->start.get(), distinct, d_results,
            d_arena, (const ull*)b->loff.get(), b->pool_ids.get()))) return e;
    std::vector<uint32_t> h_ids((size_t)total);
    PA_HIP_TRY(hipMemcpyAsync(h_ids.data(), b->pool_ids.get(), total * 4, hipMemcpyDeviceToHost, s));
    PA_HIP_TRY(hipStreamSynchronize(s));
    // the host's pool: a hash met in an earlier batch must come with the same list
    for (uint32_t d = 0; d < distinct; ++d) {
        const uint32_t* ids = h_ids.data() + h_off[d];
        const auto it = b->list_of_hash.find(h_hash[d]);
        if (it != b->list_of_hash.end()) {
            const uint64_t l = it->second, a = b->list_off[l], len = b->list_off[l + 1] - a;
            if (len != h_len[d] || !std::equal(ids, ids + len, b->list_ids.data() + a))
                return fail(PA_ERR_INTERNAL, "two different id lists share the content hash %016llx", h_hash[d]);
            continue;
        }
        b->list_of_hash.emplace(h_hash[d], b->list_hash.size());
        b->list_hash.push_back(h_hash[d]);
        b->list_ids.insert(b->list_ids.end(), ids, ids + h_len[d]);
        b->list_off.push_back(b->list_ids.size());
    }
    return PA_OK;
}

// (keys, counts)[0 .. n) -> sorted, equal keys joined: (out_keys, out_counts)[runs]; scratch (k1, c1)[n]
int sort_reduce(pa_bus* b, hipStream_t s, const u128* keys, const uint32_t* counts, uint64_t n, u128* k1, uint32_t* c1, u128* out_keys, uint32_t* out_counts,
                uint32_t& runs) {
    int e;
    if ((e = sort_pairs(s, b->tmp, keys, k1, counts, c1, (size_t)n, 0, b->key_bits()))) return e;
    if ((e = collapse_keys<u128>(b, s, k1, (uint32_t)n, out_keys, runs)) != PA_OK) return e;
    return run_counts(s, b->start.get(), runs, c1, out_counts);
}

int bus_finish(pa_bus* b) {
    PA_HIP_TRY(hipSetDevice(b->device));
    hipStream_t s = nullptr;
    const HostIndex& hi = b->host->h;
    const std::vector<uint64_t> no_class{0};
    const uint64_t* ec_offset = hi.ec_offset.empty() ? no_class.data() : hi.ec_offset.data();
    std::vector<int32_t> list_ec;
    int e = bus::assign_ecs(b->num_tx, ec_offset, hi.ec_ids.data(), b->num_classes, b->list_off.data(), b->list_ids.data(), b->list_hash.size(), b->table, list_ec);
    if (e != PA_OK) return e;
    const uint64_t M0 = b->acc_n;
    if (M0) {
        DeviceBuffer<u128> k1, k2;
        DeviceBuffer<uint32_t> c1, c2;
        if ((e = k1.alloc(M0)) || (e = k2.alloc(M0)) || (e = c1.alloc(M0)) || (e = c2.alloc(M0))) return e;
        uint32_t M = 0;
        // 1. every batch's entries together: sort by key, sum the reads of equal keys -> (k2, c2)[M]
        if ((e = sort_reduce(b, s, b->acc_keys.get(), b->acc_counts.get(), M0, k1.get(), c1.get(), k2.get(), c2.get(), M)) != PA_OK) return e;
        b->acc_keys.release();
        b->acc_counts.release();
        if (!b->list_hash.empty()) {
            // 2. hash -> ec, sorted by hash, to HBM; the hashes are replaced
            std::vector<uint64_t> order(b->list_hash.size());
            for (uint64_t l = 0; l < order.size(); ++l) order[l] = l;
            std::sort(order.begin(), order.end(), [&](uint64_t x, uint64_t y) { return b->list_hash[x] < b->list_hash[y]; });
            std::vector<ull> th(order.size());
            std::vector<uint32_t> te(order.size());
            for (uint64_t j = 0; j < order.size(); ++j) { th[j] = b->list_hash[order[j]]; te[j] = (uint32_t)list_ec[order[j]]; }
            DeviceBuffer<ull> d_th;
            DeviceBuffer<uint32_t> d_te;
            if ((e = upload(d_th, th)) || (e = upload(d_te, te))) return e;
            if ((e = launch(pa_bus_remap_kernel, grid_for(M, BUS_BLOCK), BUS_BLOCK, s, k2.get(), M, (const ull*)d_th.get(), (const uint32_t*)d_te.get(), (uint32_t)th.size(),
                    b->d_err.get()))) return e;
            if ((e = check_err(b, s, "no id list was kept for the content hash")) != PA_OK) return e;
            // 3. a list that turned out to be an index class joins that class's record: sort and reduce once more -> (k2, c2)[M]
            DeviceBuffer<u128> k3;
            DeviceBuffer<uint32_t> c3;
            if ((e = k3.alloc(M)) || (e = c3.alloc(M))) return e;
            const uint32_t before = M;
            if ((e = sort_reduce(b, s, k2.get(), c2.get(), before, k1.get(), c1.get(), k3.get(), c3.get(), M)) != PA_OK) return e;
            k2 = std::move(k3);
            c2 = std::move(c3);
        }
        // 4. whole records
        if ((e = b->d_records.alloc(M)) != PA_OK) return e;
        if ((e = launch(pa_bus_records_kernel<64, 0>, grid_for(M, BUS_BLOCK), BUS_BLOCK, s, (const u128*)k2.get(), (const uint32_t*)c2.get(), M, 2 * b->umi_len,
                b->d_records.get()))) return e;
        PA_HIP_TRY(hipStreamSynchronize(s));
        b->n_records = M;
    }
    b->stats[BS_RECORDS] = b->n_records;
    b->finished = true;
    return PA_OK;
}

}  // namespace

int pa::bus_finished_view(const pa_bus* b, int* device, const pa_bus_record** d_records, uint64_t* n_records, const bus::EcTable** table, uint32_t* bc_len,
                          uint32_t* umi_len, uint32_t* num_tx) {
    if (!b->finished) return fail(PA_ERR_INVALID_ARG, "the records exist after pa_bus_finish");
    *device = b->device; *d_records = b->d_records.get(); *n_records = b->n_records; *table = &b->table;
    *bc_len = b->bc_len; *umi_len = b->umi_len; *num_tx = b->num_tx;
    return PA_OK;
}

extern "C" {

int pa_bus_create(pa_index* idx, const pa_host_index* h, uint32_t bc_len, uint32_t umi_len, pa_bus** out) {
    if (out) *out = nullptr;
    if (!idx || !h || !out) return fail(PA_ERR_INVALID_ARG, "null argument");
    int e = bus_records::check_lengths(bc_len, umi_len, PA_ERR_UNSUPPORTED, " (one 64-bit word)");
    if (e != PA_OK) return e;
    const HostIndex& hi = h->h;
    const uint32_t num_classes = hi.ec_offset.empty() ? 0 : (uint32_t)(hi.ec_offset.size() - 1);
    std::vector<uint32_t> class_ec;
    uint32_t M = 0;
    e = bus::class_ecs(hi.num_transcripts, hi.ec_offset.data(), hi.ec_ids.data(), num_classes, class_ec, &M);
    if (e != PA_OK) return e;
    pa_index_stats ist{};
    if ((e = pa_index_get_stats(idx, &ist)) != PA_OK) return e;
    if (ist.num_classes != num_classes) return fail(PA_ERR_INVALID_ARG, "host index has %u classes, the device index %u: not the index it was made from", num_classes, ist.num_classes);
    const uint32_t *h_ec = nullptr, *h_ref = nullptr;
    int device = 0;
    index_host_classes(idx, &h_ec, &h_ref, &device);
    PA_HIP_TRY(hipSetDevice(device));
    std::unique_ptr<pa_bus> b(new (std::nothrow) pa_bus());
    if (!b) return fail(PA_ERR_OOM, "out of host memory");
    b->device = device;
    b->bc_len = bc_len; b->umi_len = umi_len; b->num_classes = num_classes; b->num_tx = hi.num_transcripts; b->host = h;
    if ((e = upload(b->d_class_ec, class_ec)) || (e = b->d_stats.alloc(PA_BUS_STATS)) || (e = b->d_err.alloc(1))) return e;
    PA_HIP_TRY(hipMemset(b->d_stats.get(), 0, PA_BUS_STATS * 8));
    PA_HIP_TRY(hipMemset(b->d_err.get(), 0, 8));
    *out = b.release();
    return PA_OK;
}

int pa_bus_add_device(pa_bus* b, const pa_read_result* d_results, const uint32_t* d_arena, uint64_t arena_len, const uint8_t* d_r1, const uint64_t* d_r1_offsets,
                      uint64_t n_reads, void* stream) {
    if (!b || (n_reads && (!d_results || !d_r1 || !d_r1_offsets)) || (arena_len && !d_arena)) return fail(PA_ERR_INVALID_ARG, "null argument");
    if (b->finished) return fail(PA_ERR_INVALID_ARG, "the writer is finished: no batches after pa_bus_finish");
    if (n_reads > 0x7FFFFFFFull) return fail(PA_ERR_UNSUPPORTED, "at most 2^31-1 reads per batch");
    if (n_reads == 0) return PA_OK;
    PA_HIP_TRY(hipSetDevice(b->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    int e;
    if ((e = grow(b->keys, n_reads)) || (e = grow(b->sorted, n_reads)) || (e = grow(b->vals, n_reads)) || (e = grow(b->svals, n_reads))) return e;
    BusKeyParams p;
    p.results = d_results; p.arena = d_arena; p.arena_len = arena_len; p.r1 = d_r1; p.r1_off = d_r1_offsets; p.n = n_reads;
    p.class_ec = b->d_class_ec.get(); p.num_classes = b->num_classes; p.num_tx = b->num_tx; p.bc_len = b->bc_len; p.umi_len = b->umi_len;
    p.sentinel = ((u128)low_mask(2 * (b->bc_len + b->umi_len)) << 64) | ~0ull;   // >= every valid key: the dropped reads sort behind the recorded ones
    p.keys = b->keys.get(); p.vals = b->vals.get(); p.stats = b->d_stats.get();
    const uint64_t recorded_before = b->stats[BS_RECORDED];
    if ((e = launch(pa_bus_keys_kernel, grid_for(n_reads, BUS_BLOCK), BUS_BLOCK, s, p))) return e;
    if ((e = fetch_stats(b, s)) != PA_OK) return e;
    const uint64_t recorded = b->stats[BS_RECORDED] - recorded_before;
    if (recorded == 0) return PA_OK;
    if (b->acc_n + recorded > 0x7FFFFFFFull) return fail(PA_ERR_UNSUPPORTED, "more than 2^31-1 record entries before finish");
    if (b->acc_n + recorded > b->acc_keys.size()) {   // grow the accumulator (doubling), keeping what it holds
        const uint64_t want = std::max<uint64_t>(b->acc_n + recorded, 2 * b->acc_keys.size());
        DeviceBuffer<u128> nk;
        DeviceBuffer<uint32_t> nc;
        if ((e = nk.alloc(want)) || (e = nc.alloc(want))) return e;
        if (b->acc_n) {
            PA_HIP_TRY(hipMemcpyAsync(nk.get(), b->acc_keys.get(), b->acc_n * 16, hipMemcpyDeviceToDevice, s));
            PA_HIP_TRY(hipMemcpyAsync(nc.get(), b->acc_counts.get(), b->acc_n * 4, hipMemcpyDeviceToDevice, s));
            PA_HIP_TRY(hipStreamSynchronize(s));
        }
        b->acc_keys = std::move(nk);
        b->acc_counts = std::move(nc);
    }
    // only the key's used bits are sorted; the recorded reads are the first `recorded` sorted keys
    u128* unique = b->acc_keys.get() + b->acc_n;
    uint32_t runs = 0;
    if ((e = sort_pairs(s, b->tmp, (const u128*)b->keys.get(), b->sorted.get(), (const uint32_t*)b->vals.get(), b->svals.get(), (size_t)n_reads, 0, b->key_bits()))) return e;
    if ((e = collapse_keys<u128>(b, s, b->sorted.get(), (uint32_t)recorded, unique, runs)) != PA_OK) return e;
    if ((e = run_counts(s, b->start.get(), runs, nullptr, b->acc_counts.get() + b->acc_n))) return e;
    if ((e = launch(pa_bus_verify_members_kernel, grid_for(recorded, BUS_BLOCK), BUS_BLOCK, s, (const u128*)b->sorted.get(), (const uint32_t*)b->svals.get(),
            (const uint32_t*)b->pos.get(), (const uint32_t*)b->start.get(), (uint32_t)recorded, d_results, d_arena, b->d_err.get()))) return e;
    if ((e = collect_lists(b, s, unique, runs, d_results, d_arena)) != PA_OK) return e;
    if ((e = check_err(b, s, "two different id lists share the content hash")) != PA_OK) return e;   // (synchronises)
    b->acc_n += runs;
    return PA_OK;
}

int pa_bus_finish(pa_bus* b, uint64_t* n_records, uint32_t* n_ecs) {
    if (!b || !n_records || !n_ecs) return fail(PA_ERR_INVALID_ARG, "null argument");
    *n_records = 0;
    *n_ecs = 0;
    if (!b->finished) {
        const int e = bus_finish(b);
        if (e != PA_OK) return e;
    }
    *n_records = b->n_records;
    *n_ecs = (uint32_t)b->table.n_ecs();
    return PA_OK;
}

int pa_bus_records(const pa_bus* b, pa_bus_record* out, uint64_t cap) {
    if (!b) return fail(PA_ERR_INVALID_ARG, "null argument");
    if (!b->finished) return fail(PA_ERR_INVALID_ARG, "the records exist after pa_bus_finish");
    const uint64_t n = b->n_records;
    if (cap < n) return fail(PA_ERR_BUFFER_TOO_SMALL, "%llu records, room for %llu", (ull)n, (ull)cap);
    if (n && !out) return fail(PA_ERR_INVALID_ARG, "null argument");
    if (n) {
        PA_HIP_TRY(hipSetDevice(b->device));
        PA_HIP_TRY(hipMemcpy(out, b->d_records.get(), n * sizeof(pa_bus_record), hipMemcpyDeviceToHost));
    }
    return PA_OK;
}

int pa_bus_ecs(const pa_bus* b, uint64_t* offsets, uint32_t* ids, uint64_t ids_cap, uint64_t* n_ids) {
    if (!b || !n_ids) return fail(PA_ERR_INVALID_ARG, "null argument");
    if (!b->finished) return fail(PA_ERR_INVALID_ARG, "the ec table exists after pa_bus_finish");
    *n_ids = b->table.ids.size();
    if (!ids) return PA_OK;
    if (!offsets) return fail(PA_ERR_INVALID_ARG, "null argument");
    if (ids_cap < *n_ids) return fail(PA_ERR_BUFFER_TOO_SMALL, "%llu ids, room for %llu", (ull)*n_ids, (ull)ids_cap);
    memcpy(offsets, b->table.offsets.data(), b->table.offsets.size() * 8);
    if (*n_ids) memcpy(ids, b->table.ids.data(), *n_ids * 4);
    return PA_OK;
}

int pa_bus_stats(const pa_bus* b, uint64_t stats[PA_BUS_STATS]) {
    if (!b || !stats) return fail(PA_ERR_INVALID_ARG, "null argument");
    memcpy(stats, b->stats, sizeof b->stats);
    return PA_OK;
}

int pa_bus_write(const pa_bus* b, const char* out_dir) {
    if (!b || !out_dir) return fail(PA_ERR_INVALID_ARG, "null argument");
    if (!b->finished) return fail(PA_ERR_INVALID_ARG, "the files are written after pa_bus_finish");
    // the records come over the link in pieces of BUS_WRITE_PIECE through two pinned buffers: piece j + 1 is copied while piece j is written
    PA_HIP_TRY(hipSetDevice(b->device));
    PinnedBuffer<pa_bus_record> pinned[2];
    const uint64_t n = b->n_records, piece = std::min<uint64_t>(std::max<uint64_t>(n, 1), BUS_WRITE_PIECE);
    int e;
    if ((e = pinned[0].alloc(piece)) || (e = pinned[1].alloc(piece))) return e;
    uint64_t copied = 0, handed = 0;
    int cur = 0;
    auto start_copy = [&](int buf) -> int {   // the next piece into pinned[buf], asynchronous on the null stream
        const uint64_t m = std::min(piece, n - copied);
        if (m) PA_HIP_TRY(hipMemcpyAsync(pinned[buf].get(), b->d_records.get() + copied, m * sizeof(pa_bus_record), hipMemcpyDeviceToHost, nullptr));
        copied += m;
        return PA_OK;
    };
    if ((e = start_copy(0)) != PA_OK) return e;
    return bus::write_files(out_dir, b->bc_len, b->umi_len, [&](const pa_bus_record** p, uint64_t* m) -> int {
        PA_HIP_TRY(hipStreamSynchronize(nullptr));   // the piece in pinned[cur] has arrived
        *p = pinned[cur].get();
        *m = std::min(piece, n - handed);
        handed += *m;
        cur ^= 1;
        return start_copy(cur);
    }, b->table, b->host->h.tx_names);
}

void pa_bus_destroy(pa_bus* b) {
    if (!b) return;
    (void)hipSetDevice(b->device);
    delete b;
}

}  // extern "C"
