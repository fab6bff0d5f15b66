// BUS barcode correction (pa_bus_correct, include/pseudoaligner_amd.h): the `bustools correct` + re-sort step on the records where
// they lie. The whitelist becomes an open-addressing table in HBM (8-byte slots, the barcode is the key, linear probing from pa_mix64); the
// records' distinct barcodes are classified in two launches — one exact probe per barcode, then a group of CORRECT_GROUP lanes per missed
// barcode that deals its 3 bc_len single substitutions over the lanes and issues every probe before it looks at any; every record takes its
// barcode's target or is dropped, and the kept ones are sorted and collapsed again with collapse_runs, as bus.hip collapses a run (skipped when nothing moved).
// Integer arithmetic only; the stat counters are summed per wave and added with integer atomics, once per wave: the kernels that count run a bounded
// grid whose lanes stride over their items (a wave per 64 records adding to one address each was most of the rewrite's time).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "bus_correct_host.hpp"
#include "bus_state.hpp"
#include "device_prims.hpp"
#include "hip_buffer.hpp"
#include "kernel_utils.hpp"
#include "pa_common.hpp"
#include "phase_clock.hpp"

using namespace pa;

namespace {

constexpr uint32_t CORRECT_BLOCK = 256;        // 4 waves
constexpr uint32_t CORRECT_GROUP = 16;         // lanes that share the 3 bc_len candidates of one missed barcode: four barcodes per wave64
constexpr uint32_t CORRECT_MAX_ROUNDS = 6;     // candidates of one lane: ceil(3 * 31 / CORRECT_GROUP)
constexpr uint32_t CORRECT_MAX_GRID = 2048;    // blocks of a counting kernel: its lanes stride over the items and a wave adds its counters once, at its end
constexpr ull WL_EMPTY = ~0ull;                // an empty slot, and the target of a dropped barcode (a barcode has at most 62 bits)
enum : uint32_t { ERR_DUPLICATE = 0, ERR_TABLE = 1, ERR_WORDS = 2 };
enum : uint32_t { CS_RECORDS_IN = 0, CS_READS_IN, CS_BARCODES_IN, CS_EXACT, CS_CORRECTED, CS_NONE, CS_AMBIGUOUS, CS_RECORDS_EXACT, CS_RECORDS_CORRECTED, CS_RECORDS_DROPPED,
                  CS_READS_DROPPED, CS_RECORDS_OUT, CS_BARCODES_OUT };
static_assert(CS_BARCODES_OUT + 1 == PA_BUS_CORRECT_STATS, "the stats of the header");
static_assert(CORRECT_GROUP * CORRECT_MAX_ROUNDS >= 3 * 31 && 64 % CORRECT_GROUP == 0, "a group holds every candidate and divides a wave");

thread_local float g_phase_ms[PA_BUS_CORRECT_PHASES] = {};

// ---- 1. the whitelist table ----
// sorted whitelist -> table; equal neighbours: the error word names the barcode (+ 1); a table without a free slot: the other error word
__global__ __launch_bounds__(CORRECT_BLOCK) void pa_correct_insert_kernel(const ull* __restrict__ sorted, uint32_t n, ull* __restrict__ table, ull cap, ull* __restrict__ err) {
    const uint32_t i = blockIdx.x * CORRECT_BLOCK + threadIdx.x;
    if (i >= n) return;
    const ull k = sorted[i];
    if (i && sorted[i - 1] == k) { atomicMax(err + ERR_DUPLICATE, k + 1); return; }
    const ull mask = cap - 1;
    ull j = pa_mix64(k) & mask;
    bool placed = false;
    for (ull step = 0; step < cap; ++step) {
        const ull old = atomicCAS(table + j, WL_EMPTY, k);
        if (old == WL_EMPTY || old == k) { placed = true; break; }
        j = (j + 1) & mask;
    }
    if (!placed) atomicMax(err + ERR_TABLE, 1ull);
}

// 1 key is in the table, 0 it is not, -1 no empty slot met within `cap` steps (a damaged table)
__device__ inline int wl_lookup(const ull* __restrict__ table, ull cap, ull key) {
    const ull mask = cap - 1;
    ull j = pa_mix64(key) & mask;
    for (ull step = 0; step < cap; ++step) {
        const ull v = table[j];
        if (v == key) return 1;
        if (v == WL_EMPTY) return 0;
        j = (j + 1) & mask;
    }
    return -1;
}

// ---- 3a. one lane per distinct barcode: the exact probe ----
__global__ __launch_bounds__(CORRECT_BLOCK) void pa_correct_exact_kernel(const ull* __restrict__ ubc, const uint32_t* __restrict__ start, uint32_t B, const ull* __restrict__ table,
                                                                          ull cap, ull* __restrict__ target, uint32_t* __restrict__ missed, ull* __restrict__ stats,
                                                                          ull* __restrict__ err) {
    ull n_exact = 0, records = 0;
    for (uint64_t b = (uint64_t)blockIdx.x * CORRECT_BLOCK + threadIdx.x; b < B; b += (uint64_t)gridDim.x * CORRECT_BLOCK) {
        const ull bc = ubc[b];
        const int r = wl_lookup(table, cap, bc);
        if (r < 0) atomicMax(err + ERR_TABLE, 2ull);
        const bool exact = r == 1;
        target[b] = exact ? bc : WL_EMPTY;
        missed[b] = exact ? 0u : 1u;
        if (exact) { ++n_exact; records += start[b + 1] - start[b]; }
    }
    wave_add(stats + CS_EXACT, n_exact);
    wave_add(stats + CS_RECORDS_EXACT, records);
}

// ---- 3b. CORRECT_GROUP lanes per missed barcode: candidate c = position c / 3 (from the last base), substitution 1 + c % 3 (xor of the
// base's two bits); lane g of the group takes c = g, g + GROUP, ... Every round issues the loads of all the lane's candidates
// before any is compared; a candidate ends at its key (hit) or at an empty slot (miss), and the outcome is the number of hits in the
// group: 0 none, 1 corrected (the lane that holds the hit writes the target), >= 2 ambiguous ----
// ROUNDS = the candidates of a lane, ceil(3 bc_len / CORRECT_GROUP): the loads of a round are unconditional (a decided candidate reads the slot
// it read last, a candidate beyond 3 bc_len a slot it never looks at), so that no branch stands between them and they leave together
template <uint32_t ROUNDS>
__global__ __launch_bounds__(CORRECT_BLOCK) void pa_correct_neighbours_kernel(const ull* __restrict__ ubc, const uint32_t* __restrict__ start, const uint32_t* __restrict__ miss,
                                                                               uint32_t n_miss, uint32_t n_cand, const ull* __restrict__ table, ull cap,
                                                                               ull* __restrict__ target, ull* __restrict__ stats, ull* __restrict__ err) {
    const uint64_t t = (uint64_t)blockIdx.x * CORRECT_BLOCK + threadIdx.x;
    const uint32_t g = (uint32_t)(t % CORRECT_GROUP);
    const uint64_t wave_first = t / 64 * (64 / CORRECT_GROUP), all_groups = (uint64_t)gridDim.x * (CORRECT_BLOCK / CORRECT_GROUP);
    ull n_corrected = 0, n_none = 0, n_ambiguous = 0, records = 0;   // of the groups this lane leads
    // (the trip count is the wave's: the cross-lane sum below wants the whole group there, and the wave's last groups may be beyond the list)
    for (uint64_t m0 = wave_first; m0 < n_miss; m0 += all_groups) {
        const uint64_t m = m0 + (t % 64) / CORRECT_GROUP;
        const bool active = m < n_miss;
        const uint32_t b = active ? miss[m] : 0u;
        const ull bc = active ? ubc[b] : 0ull;
        const ull mask = cap - 1;
        ull cand[ROUNDS], slot[ROUNDS];
        uint32_t pending = 0;   // bit r: candidate r of this lane is not decided yet
#pragma unroll
        for (uint32_t r = 0; r < ROUNDS; ++r) {
            const uint32_t c = g + r * CORRECT_GROUP;
            cand[r] = bc ^ ((ull)(1 + c % 3) << (2 * (c / 3)));
            slot[r] = pa_mix64(cand[r]) & mask;
            if (active && c < n_cand) pending |= 1u << r;
        }
        uint32_t hits = 0;
        ull hit = WL_EMPTY;
        bool damaged = false;
        for (ull step = 0; pending != 0; ++step) {
            if (step >= cap) { damaged = true; break; }
            ull seen[ROUNDS];
#pragma unroll
            for (uint32_t r = 0; r < ROUNDS; ++r) seen[r] = table[slot[r]];   // (slot[r] < cap always)
#pragma unroll
            for (uint32_t r = 0; r < ROUNDS; ++r) {
                const bool open = (pending >> r) & 1u, found = seen[r] == cand[r], empty = seen[r] == WL_EMPTY;
                if (open && found) { ++hits; hit = cand[r]; }
                if (open && (found || empty)) pending &= ~(1u << r);
                else if (open) slot[r] = (slot[r] + 1) & mask;
            }
        }
        if (damaged) atomicMax(err + ERR_TABLE, 3ull);
        // the group's hits: xor butterflies below CORRECT_GROUP stay inside the group
        uint32_t total = hits;
#pragma unroll
        for (uint32_t off = CORRECT_GROUP / 2; off > 0; off >>= 1) total += __shfl_xor(total, (int)off);
        if (active && total == 1 && hits == 1) target[b] = hit;
        if (active && g == 0) {
            if (total == 0) ++n_none;
            else if (total == 1) { ++n_corrected; records += start[b + 1] - start[b]; }
            else ++n_ambiguous;
        }
    }
    wave_add(stats + CS_CORRECTED, n_corrected);
    wave_add(stats + CS_NONE, n_none);
    wave_add(stats + CS_AMBIGUOUS, n_ambiguous);
    wave_add(stats + CS_RECORDS_CORRECTED, records);
}

// ---- 4. rewrite and re-collapse ----
// one lane per record: kept[i] = its barcode has a target; the reads in and the reads dropped
__global__ __launch_bounds__(CORRECT_BLOCK) void pa_correct_keep_kernel(const pa_bus_record* __restrict__ rec, const uint32_t* __restrict__ pos, const ull* __restrict__ target,
                                                                         uint32_t n, uint32_t* __restrict__ kept, ull* __restrict__ stats) {
    ull reads = 0, dropped = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * CORRECT_BLOCK + threadIdx.x; i < n; i += (uint64_t)gridDim.x * CORRECT_BLOCK) {
        const bool keep = target[pos[i] - 1] != WL_EMPTY;
        const ull count = rec[i].count;
        kept[i] = keep ? 1u : 0u;
        reads += count;
        dropped += keep ? 0ull : count;
    }
    wave_add(stats + CS_READS_IN, reads);
    wave_add(stats + CS_READS_DROPPED, dropped);
}
// kpos = inclusive scan of kept: the kept records compacted as keys (target barcode | UMI) << 32 | ec + 2^31, with their counts
__global__ __launch_bounds__(CORRECT_BLOCK) void pa_correct_compact_kernel(const pa_bus_record* __restrict__ rec, const uint32_t* __restrict__ pos,
                                                                            const ull* __restrict__ target, const uint32_t* __restrict__ kept,
                                                                            const uint32_t* __restrict__ kpos, uint32_t n, uint32_t umi_bits, u128* __restrict__ keys,
                                                                            uint32_t* __restrict__ counts) {
    const uint32_t i = blockIdx.x * CORRECT_BLOCK + threadIdx.x;
    if (i >= n || !kept[i]) return;
    const RecordWords r = load_record(rec + i);
    const ull umi = (ull)r.a.z | ((ull)r.a.w << 32);
    const ull w = (target[pos[i] - 1] << umi_bits) | umi;
    const uint32_t d = kpos[i] - 1;
    keys[d] = ((u128)w << 32) | (u128)(r.c.x ^ EC_BIAS);
    counts[d] = r.c.y;
}
__global__ __launch_bounds__(CORRECT_BLOCK) void pa_correct_barcodes_out_kernel(const pa_bus_record* __restrict__ rec, uint32_t n, ull* __restrict__ stats) {
    ull heads = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * CORRECT_BLOCK + threadIdx.x; i < n; i += (uint64_t)gridDim.x * CORRECT_BLOCK)
        if (i == 0 || rec[i].barcode != rec[i - 1].barcode) ++heads;
    wave_add(stats + CS_BARCODES_OUT, heads);
}

// blocks of a kernel whose lanes stride over n items
uint32_t count_grid(uint64_t n) { return std::min(grid_for(n, CORRECT_BLOCK), CORRECT_MAX_GRID); }

int check_device_err(const ull* d_err, hipStream_t s) {
    ull err[ERR_WORDS] = {};
    PA_HIP_TRY(hipMemcpyAsync(err, d_err, sizeof err, hipMemcpyDeviceToHost, s));
    PA_HIP_TRY(hipStreamSynchronize(s));
    if (err[ERR_DUPLICATE]) return fail(PA_ERR_INVALID_ARG, "the whitelist holds barcode %llu twice", err[ERR_DUPLICATE] - 1);
    if (err[ERR_TABLE]) return fail(PA_ERR_INTERNAL, "the whitelist table is damaged: a probe met no free slot (where: %llu)", err[ERR_TABLE]);
    return PA_OK;
}

// d_in[n] (n >= 1, strictly ascending) on the current device, the whitelist (checked) on the host -> d_out[*n_out], stats
int correct_device(const pa_bus_record* d_in, uint32_t n, uint32_t bc_len, uint32_t umi_len, const uint64_t* whitelist, uint64_t n_whitelist,
                   DeviceBuffer<pa_bus_record>& d_out, uint64_t* n_out, uint64_t* stats) {
    hipStream_t s = nullptr;
    int e;
    PhaseClock<PA_BUS_CORRECT_PHASES> clock;
    if ((e = clock.open()) || (e = clock.mark(0))) return e;
    DeviceBuffer<uint8_t> tmp;
    DeviceBuffer<ull> d_stats, d_err;
    if ((e = d_stats.alloc(PA_BUS_CORRECT_STATS)) || (e = d_err.alloc(ERR_WORDS))) return e;
    PA_HIP_TRY(hipMemsetAsync(d_stats.get(), 0, PA_BUS_CORRECT_STATS * 8, s));
    PA_HIP_TRY(hipMemsetAsync(d_err.get(), 0, ERR_WORDS * 8, s));

    // 1. the table
    const uint32_t W = (uint32_t)n_whitelist;
    const ull cap = correct::table_capacity(n_whitelist);
    DeviceBuffer<ull> d_wl, d_wl_sorted, d_table;
    if ((e = upload(d_wl, (const ull*)whitelist, (size_t)W)) || (e = d_wl_sorted.alloc(W)) || (e = d_table.alloc((size_t)cap))) return e;
    PA_HIP_TRY(hipMemsetAsync(d_table.get(), 0xFF, (size_t)cap * 8, s));
    if ((e = sort_keys(s, tmp, (const ull*)d_wl.get(), d_wl_sorted.get(), (int)W, 0, 2 * bc_len))) return e;
    if ((e = launch(pa_correct_insert_kernel, grid_for(W, CORRECT_BLOCK), CORRECT_BLOCK, s, (const ull*)d_wl_sorted.get(), W, d_table.get(), cap, d_err.get()))) return e;
    if ((e = clock.mark(1)) || (e = check_device_err(d_err.get(), s))) return e;

    // 2. the distinct barcodes: the collapse in its two halves, the outputs sized by the run count
    DeviceBuffer<uint32_t> d_heads, d_pos, d_start, d_missed, d_miss, d_n;
    DeviceBuffer<ull> d_ubc, d_target;
    uint32_t B = 0, n_miss = 0;
    if ((e = d_heads.alloc(n)) || (e = d_pos.alloc(n)) || (e = d_n.alloc(1)) || (e = flag_runs(s, tmp, RecordBarcode{d_in}, n, d_heads.get(), d_pos.get(), B))) return e;
    if ((e = d_ubc.alloc(B)) || (e = d_target.alloc(B)) || (e = d_start.alloc((size_t)B + 1)) || (e = d_missed.alloc(B)) || (e = d_miss.alloc(B)) ||
        (e = scatter_runs(s, RecordBarcode{d_in}, (const uint32_t*)d_heads.get(), (const uint32_t*)d_pos.get(), n, B, d_ubc.get(), d_start.get())))
        return e;

    // 3a. exact
    if ((e = launch(pa_correct_exact_kernel, count_grid(B), CORRECT_BLOCK, s, (const ull*)d_ubc.get(), (const uint32_t*)d_start.get(), B, (const ull*)d_table.get(), cap,
            d_target.get(), d_missed.get(), d_stats.get(), d_err.get()))) return e;
    if ((e = select_flagged_indices(s, tmp, (const uint32_t*)d_missed.get(), (size_t)B, d_miss.get(), d_n.get())) || (e = clock.mark(2)) || (e = fetch_u32(d_n.get(), s, n_miss)))
        return e;
    // 3b. the neighbours of the missed ones
    if (n_miss) {
        const dim3 grid(count_grid((uint64_t)n_miss * CORRECT_GROUP)), block(CORRECT_BLOCK);
        auto neighbours = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, grid, block, 0, s, (const ull*)d_ubc.get(), (const uint32_t*)d_start.get(), (const uint32_t*)d_miss.get(), n_miss, 3 * bc_len,
                               (const ull*)d_table.get(), cap, d_target.get(), d_stats.get(), d_err.get());
        };
        switch ((3 * bc_len + CORRECT_GROUP - 1) / CORRECT_GROUP) {   // 1 .. CORRECT_MAX_ROUNDS for bc_len 1 .. 31
            case 1: neighbours(pa_correct_neighbours_kernel<1>); break;
            case 2: neighbours(pa_correct_neighbours_kernel<2>); break;
            case 3: neighbours(pa_correct_neighbours_kernel<3>); break;
            case 4: neighbours(pa_correct_neighbours_kernel<4>); break;
            case 5: neighbours(pa_correct_neighbours_kernel<5>); break;
            default: neighbours(pa_correct_neighbours_kernel<CORRECT_MAX_ROUNDS>); break;
        }
        PA_HIP_TRY(hipGetLastError());
    }
    if ((e = clock.mark(3))) return e;

    // 4. rewrite: the kept records as keys
    DeviceBuffer<uint32_t>& d_kept = d_heads;   // (the heads are used up)
    DeviceBuffer<uint32_t> d_kpos, d_counts;
    DeviceBuffer<u128> d_keys;
    uint32_t n_kept = 0;
    if ((e = d_kpos.alloc(n))) return e;
    if ((e = launch(pa_correct_keep_kernel, count_grid(n), CORRECT_BLOCK, s, d_in, (const uint32_t*)d_pos.get(), (const ull*)d_target.get(), n, d_kept.get(), d_stats.get()))) return e;
    if ((e = scan_inclusive_total(s, tmp, (const uint32_t*)d_kept.get(), d_kpos.get(), (size_t)n, n_kept))) return e;
    ull st[PA_BUS_CORRECT_STATS] = {};
    PA_HIP_TRY(hipMemcpyAsync(st, d_stats.get(), sizeof st, hipMemcpyDeviceToHost, s));
    if ((e = check_device_err(d_err.get(), s))) return e;   // (synchronises)
    uint32_t M = 0;
    if (n_kept) {
        const uint32_t umi_bits = 2 * umi_len, key_bits = 32 + 2 * (bc_len + umi_len);
        if ((e = d_keys.alloc(n_kept)) || (e = d_counts.alloc(n_kept))) return e;
        if ((e = launch(pa_correct_compact_kernel, grid_for(n, CORRECT_BLOCK), CORRECT_BLOCK, s, d_in, (const uint32_t*)d_pos.get(), (const ull*)d_target.get(),
                (const uint32_t*)d_kept.get(), (const uint32_t*)d_kpos.get(), n, umi_bits, d_keys.get(), d_counts.get()))) return e;
        // a barcode moved: sort, join equal keys. Otherwise the kept records are sorted and distinct as they were
        if ((e = records_from_keys(s, tmp, d_keys, d_counts, n_kept, st[CS_CORRECTED] != 0, key_bits, umi_bits, d_out, M))) return e;
        if ((e = launch(pa_correct_barcodes_out_kernel, count_grid(M), CORRECT_BLOCK, s, (const pa_bus_record*)d_out.get(), M, d_stats.get()))) return e;
        PA_HIP_TRY(hipMemcpyAsync(&st[CS_BARCODES_OUT], d_stats.get() + CS_BARCODES_OUT, 8, hipMemcpyDeviceToHost, s));
    } else {
        d_out.release();
    }
    if ((e = clock.mark(4)) || (e = clock.close(g_phase_ms, 4))) return e;   // (synchronises)
    st[CS_RECORDS_IN] = n;
    st[CS_BARCODES_IN] = B;
    st[CS_RECORDS_DROPPED] = (ull)n - st[CS_RECORDS_EXACT] - st[CS_RECORDS_CORRECTED];
    st[CS_RECORDS_OUT] = M;
    if (st[CS_EXACT] + st[CS_CORRECTED] + st[CS_NONE] + st[CS_AMBIGUOUS] != B || st[CS_RECORDS_EXACT] + st[CS_RECORDS_CORRECTED] != n_kept)
        return fail(PA_ERR_INTERNAL, "barcode correction: the counts of the classes do not add up");
    *n_out = M;
    if (stats) for (uint32_t j = 0; j < PA_BUS_CORRECT_STATS; ++j) stats[j] = st[j];
    return PA_OK;
}

}  // namespace

extern "C" {

int pa_bus_whitelist_pack(const char* whitelist, uint64_t n, uint32_t bc_len, uint64_t* packed) { return correct::pack_whitelist(whitelist, n, bc_len, packed); }

int pa_bus_correct_records(pa_index* idx, const pa_bus_record* in, uint64_t n, uint32_t bc_len, uint32_t umi_len, const uint64_t* whitelist, uint64_t n_whitelist,
                           pa_bus_record* out, uint64_t cap, uint64_t* n_out, uint64_t stats[PA_BUS_CORRECT_STATS]) {
    if (n_out) *n_out = 0;
    if (stats) memset(stats, 0, PA_BUS_CORRECT_STATS * 8);
    if (!n_out) return fail(PA_ERR_INVALID_ARG, "null argument");
    int e;
    if ((e = correct::check_lengths(bc_len, umi_len)) || (e = correct::check_whitelist(whitelist, n_whitelist, bc_len))) return e;
    if (n > 0x7FFFFFFFull) return fail(PA_ERR_UNSUPPORTED, "more than 2^31-1 records");
    if ((e = correct::check_records(in, n, bc_len, umi_len))) return e;
    DeviceBuffer<pa_bus_record> d_out;
    if ((e = on_host_records(idx, in, n, [&](const pa_bus_record* d_in, uint32_t m) { return correct_device(d_in, m, bc_len, umi_len, whitelist, n_whitelist, d_out, n_out, stats); },
                             empty_ok)))
        return e;
    return deliver_records(d_out, *n_out, out, cap);
}

int pa_bus_correct(pa_bus* b, const uint64_t* whitelist, uint64_t n_whitelist, uint64_t stats[PA_BUS_CORRECT_STATS]) {
    if (stats) memset(stats, 0, PA_BUS_CORRECT_STATS * 8);
    int e;
    if ((e = finished_writer(b, "the records are corrected after pa_bus_finish")) || (e = correct::check_whitelist(whitelist, n_whitelist, b->bc_len))) return e;
    return rewrite_writer_records(b, [&](const pa_bus_record* d_in, uint32_t n, DeviceBuffer<pa_bus_record>& d_out, uint64_t* n_out) {
        return correct_device(d_in, n, b->bc_len, b->umi_len, whitelist, n_whitelist, d_out, n_out, stats);
    }, empty_ok);
}

int pa_bus_correct_phase_ms(float out[PA_BUS_CORRECT_PHASES]) {
    if (!out) return fail(PA_ERR_INVALID_ARG, "null argument");
    for (int i = 0; i < PA_BUS_CORRECT_PHASES; ++i) out[i] = g_phase_ms[i];
    return PA_OK;
}

}  // extern "C"
