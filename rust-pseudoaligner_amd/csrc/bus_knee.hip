// Cell calling on BUS records (pa_bus_knee, pa_bus_keep; include/pseudoaligner_amd.h): the per-barcode table (records, molecules,
// reads) over the sorted records where they lie, the ranking of its rows by molecules, the curve of distinct molecule counts for the host's
// threshold rule, the called list and the rows; and the pure filter that keeps the records of listed barcodes.
// The table is reduce-then-scan over tiles of KNEE_TILE records: pass 1 sums every tile's barcode heads, molecule heads and reads, a scan over
// the tile totals gives every tile its carry, pass 2 recomputes the prefixes inside the tile (wave shuffles + one LDS exchange between the
// block's four waves) and writes one head row (barcode, start, molecules before, reads before) at every barcode head; a row of the table is the
// difference of two consecutive head rows. No loop is as long as a barcode and no atomic names a barcode's slot: the cost does not depend on
// how the records are shared out among the barcodes. Integer arithmetic only; the counters are summed per wave and added once per wave.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "bus_knee_host.hpp"
#include "bus_state.hpp"
#include "device_prims.hpp"
#include "hip_buffer.hpp"
#include "kernel_utils.hpp"
#include "pa_common.hpp"
#include "phase_clock.hpp"

using namespace pa;

namespace {

constexpr uint32_t KNEE_BLOCK = 256;                      // 4 waves
constexpr uint32_t KNEE_ITEMS = 8;                        // records of a lane in one tile: record k * KNEE_BLOCK + lane of the tile, k = 0 .. 7 (a wave reads 64 neighbours)
constexpr uint32_t KNEE_TILE = KNEE_BLOCK * KNEE_ITEMS;   // records of a tile
constexpr uint32_t KNEE_MAX_GRID = 1024;                  // blocks of a kernel whose blocks stride over the tiles (or whose lanes stride over the items)
constexpr uint32_t KNEE_WAVES = KNEE_BLOCK / 64;
enum : uint32_t { KS_RECORDS = 0, KS_READS, KS_MOLECULES, KS_BARCODES, KS_D, KS_L, KS_THRESHOLD, KS_CALLED, KS_CALLED_MOLECULES, KS_CALLED_READS };
enum : uint32_t { KP_RECORDS_IN = 0, KP_READS_IN, KP_BARCODES_IN, KP_BARCODES_KEPT, KP_RECORDS_OUT, KP_READS_OUT, KP_LISTED_ABSENT };
static_assert(KS_CALLED_READS + 1 == PA_KNEE_STATS && KP_LISTED_ABSENT + 1 == PA_BUS_KEEP_STATS, "the stats of the header");
static_assert(sizeof(pa_bus_barcode_row) == 32 && sizeof(pa_bus_record) == 32, "rows and records move as two 16-byte words");

// what pass 2 leaves at every barcode head (and once behind the last record): the table's rows are differences of neighbours
struct alignas(16) KneeHead {
    ull barcode, reads;      // reads of all records before this one
    uint32_t start, mols;    // the record's index; molecules that begin before this record
    uint32_t pad[2];
};
static_assert(sizeof(KneeHead) == 32, "two 16-byte stores");

thread_local float g_phase_ms[PA_KNEE_PHASES] = {};

// v of lanes 0 .. lane of the wave, summed (every lane calls)
__device__ inline ull wave_scan(ull v, uint32_t lane) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const ull o = __shfl_up(v, off);
        if ((int)lane >= off) v += o;
    }
    return v;
}

// record i of n as this lane sees it: (barcode, UMI) as one 16-byte load, count as one 4-byte load; its flags against the record before it, which
// the lane below holds (a wave's first lane loads it: for the tile's first record that is the record before the tile). A lane beyond n carries
// zeros. Every lane of the wave calls. heads = barcode head << 32 | molecule head
__device__ inline void knee_load(const pa_bus_record* __restrict__ rec, uint64_t i, uint32_t n, uint32_t lane, ull& barcode, ull& heads, ull& reads) {
    const bool live = i < n;
    ull umi = 0;
    barcode = 0;
    reads = 0;
    if (live) {
        const uint4 a = *reinterpret_cast<const uint4*>(rec + i);
        barcode = (ull)a.x | ((ull)a.y << 32);
        umi = (ull)a.z | ((ull)a.w << 32);
        reads = rec[i].count;
    }
    ull pbc = __shfl_up(barcode, 1), pumi = __shfl_up(umi, 1);
    if (lane == 0 && live && i > 0) {
        const uint4 a = *reinterpret_cast<const uint4*>(rec + (i - 1));
        pbc = (ull)a.x | ((ull)a.y << 32);
        pumi = (ull)a.z | ((ull)a.w << 32);
    }
    const bool bh = live && (i == 0 || pbc != barcode), mh = live && (bh || pumi != umi);
    heads = ((ull)bh << 32) | (ull)mh;
}

// ---- 1. the table ----
// pass 1: tile_heads[tile] = barcode heads << 32 | molecule heads, tile_reads[tile] = the reads of the tile
__global__ __launch_bounds__(KNEE_BLOCK) void pa_knee_tile_totals_kernel(const pa_bus_record* __restrict__ rec, uint32_t n, uint32_t n_tiles, ull* __restrict__ tile_heads,
                                                                          ull* __restrict__ tile_reads) {
    __shared__ ull lds_heads[KNEE_WAVES], lds_reads[KNEE_WAVES];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        ull heads = 0, reads = 0;
#pragma unroll
        for (uint32_t k = 0; k < KNEE_ITEMS; ++k) {
            ull bc, h, r;
            knee_load(rec, (uint64_t)tile * KNEE_TILE + k * KNEE_BLOCK + threadIdx.x, n, lane, bc, h, r);
            heads += h;
            reads += r;
        }
        heads = wave_sum(heads);
        reads = wave_sum(reads);
        if (lane == 0) { lds_heads[wave] = heads; lds_reads[wave] = reads; }
        __syncthreads();
        if (threadIdx.x == 0) {
            ull h = 0, r = 0;
#pragma unroll
            for (uint32_t w = 0; w < KNEE_WAVES; ++w) { h += lds_heads[w]; r += lds_reads[w]; }
            tile_heads[tile] = h;
            tile_reads[tile] = r;
        }
        __syncthreads();   // (the next tile writes the same words)
    }
}

// pass 2: scan_heads / scan_reads = the inclusive scans of pass 1's totals, so a tile's carry is the entry before its own. At every barcode head the
// head row `barcode heads before it` is written; the lane of the last record writes the sentinel row behind the last barcode
__global__ __launch_bounds__(KNEE_BLOCK) void pa_knee_heads_kernel(const pa_bus_record* __restrict__ rec, uint32_t n, uint32_t n_tiles, const ull* __restrict__ scan_heads,
                                                                    const ull* __restrict__ scan_reads, KneeHead* __restrict__ out, uint32_t B) {
    __shared__ ull lds_heads[2][KNEE_WAVES], lds_reads[2][KNEE_WAVES];   // (two sets, used in turn: one barrier per step)
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        ull carry_heads = tile ? scan_heads[tile - 1] : 0ull, carry_reads = tile ? scan_reads[tile - 1] : 0ull;
        ull bc[KNEE_ITEMS], h[KNEE_ITEMS], r[KNEE_ITEMS];
#pragma unroll
        for (uint32_t k = 0; k < KNEE_ITEMS; ++k)   // every load of the tile leaves before the first barrier
            knee_load(rec, (uint64_t)tile * KNEE_TILE + k * KNEE_BLOCK + threadIdx.x, n, lane, bc[k], h[k], r[k]);
#pragma unroll
        for (uint32_t k = 0; k < KNEE_ITEMS; ++k) {
            const uint64_t i = (uint64_t)tile * KNEE_TILE + k * KNEE_BLOCK + threadIdx.x;
            ull incl_heads = wave_scan(h[k], lane), incl_reads = wave_scan(r[k], lane);
            const uint32_t set = k & 1;
            if (lane == 63) { lds_heads[set][wave] = incl_heads; lds_reads[set][wave] = incl_reads; }
            __syncthreads();
            ull step_heads = 0, step_reads = 0;
#pragma unroll
            for (uint32_t w = 0; w < KNEE_WAVES; ++w) {
                const ull wh = lds_heads[set][w], wr = lds_reads[set][w];
                if (w < wave) { incl_heads += wh; incl_reads += wr; }
                step_heads += wh;
                step_reads += wr;
            }
            incl_heads += carry_heads;
            incl_reads += carry_reads;
            const uint32_t bheads = (uint32_t)(incl_heads >> 32), mheads = (uint32_t)incl_heads;   // up to and with this record
            if ((h[k] >> 32) && bheads - 1 < B) {   // a barcode head, so a molecule head too: row bheads - 1
                const ull before = incl_reads - r[k];
                uint4* o = reinterpret_cast<uint4*>(out + (bheads - 1));
                o[0] = make_uint4((uint32_t)bc[k], (uint32_t)(bc[k] >> 32), (uint32_t)before, (uint32_t)(before >> 32));
                o[1] = make_uint4((uint32_t)i, mheads - 1, 0u, 0u);
            }
            if (i == (uint64_t)n - 1 && bheads <= B) {   // the sentinel row: start = n, every molecule, every read
                uint4* o = reinterpret_cast<uint4*>(out + bheads);
                o[0] = make_uint4(0u, 0u, (uint32_t)incl_reads, (uint32_t)(incl_reads >> 32));
                o[1] = make_uint4(n, mheads, 0u, 0u);
            }
            carry_heads += step_heads;
            carry_reads += step_reads;
        }
        __syncthreads();   // (the next tile starts over with set 0)
    }
}

// rows as differences: umis / records / reads of barcode b, the identity permutation for the sort, the largest umis
__global__ __launch_bounds__(KNEE_BLOCK) void pa_knee_diff_kernel(const KneeHead* __restrict__ heads, uint32_t B, uint32_t* __restrict__ umis, uint32_t* __restrict__ records,
                                                                   ull* __restrict__ reads, uint32_t* __restrict__ index, uint32_t* __restrict__ max_umis) {
    uint32_t mx = 0;
    for (uint64_t b = (uint64_t)blockIdx.x * KNEE_BLOCK + threadIdx.x; b < B; b += (uint64_t)gridDim.x * KNEE_BLOCK) {
        const KneeHead h0 = heads[b], h1 = heads[b + 1];
        const uint32_t u = h1.mols - h0.mols;
        umis[b] = u;
        records[b] = h1.start - h0.start;
        reads[b] = h1.reads - h0.reads;
        index[b] = (uint32_t)b;
        mx = max(mx, u);
    }
    for (int off = 32; off > 0; off >>= 1) mx = max(mx, (uint32_t)__shfl_down(mx, off));
    if ((threadIdx.x & 63) == 0 && mx) atomicMax(max_umis, mx);
}

// ---- 2. rank ----
__global__ __launch_bounds__(KNEE_BLOCK) void pa_knee_rank_kernel(const uint32_t* __restrict__ sorted_index, uint32_t B, uint32_t* __restrict__ rank) {
    const uint32_t r = blockIdx.x * KNEE_BLOCK + threadIdx.x;
    if (r < B && sorted_index[r] < B) rank[sorted_index[r]] = r;
}

// ---- 3. the called barcodes and the rows: 32 bytes as two 16-byte stores; sums[0] molecules, sums[1] reads of the called barcodes ----
__global__ __launch_bounds__(KNEE_BLOCK) void pa_knee_rows_kernel(const KneeHead* __restrict__ heads, const uint32_t* __restrict__ umis, const uint32_t* __restrict__ records,
                                                                   const ull* __restrict__ reads, const uint32_t* __restrict__ rank, uint32_t B, ull threshold,
                                                                   pa_bus_barcode_row* __restrict__ rows, uint32_t* __restrict__ flags, ull* __restrict__ sums) {
    ull mols = 0, rds = 0;
    for (uint64_t b = (uint64_t)blockIdx.x * KNEE_BLOCK + threadIdx.x; b < B; b += (uint64_t)gridDim.x * KNEE_BLOCK) {
        const ull bc = heads[b].barcode, rd = reads[b];
        const uint32_t u = umis[b], called = (ull)u >= threshold ? 1u : 0u;
        flags[b] = called;
        uint4* o = reinterpret_cast<uint4*>(rows + b);
        o[0] = make_uint4((uint32_t)bc, (uint32_t)(bc >> 32), (uint32_t)rd, (uint32_t)(rd >> 32));
        o[1] = make_uint4(records[b], u, rank[b], called);
        if (called) { mols += u; rds += rd; }
    }
    wave_add(sums + 0, mols);
    wave_add(sums + 1, rds);
}
__global__ __launch_bounds__(KNEE_BLOCK) void pa_knee_called_kernel(const KneeHead* __restrict__ heads, const uint32_t* __restrict__ selected, uint32_t n_called, uint32_t B,
                                                                     ull* __restrict__ called) {
    const uint32_t j = blockIdx.x * KNEE_BLOCK + threadIdx.x;
    if (j < n_called && selected[j] < B) called[j] = heads[selected[j]].barcode;
}

// ---- pa_bus_keep ----
// one lane per record: its barcode-head flag; the reads in. The flagging half of the collapse with the sum of the reads fused into it, so that
// the 32-byte records are swept once; the scatter half is the shared one (scatter_runs)
__global__ __launch_bounds__(KNEE_BLOCK) void pa_keep_heads_kernel(const pa_bus_record* __restrict__ rec, uint32_t n, uint32_t* __restrict__ heads, ull* __restrict__ stats) {
    ull reads = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * KNEE_BLOCK + threadIdx.x; i < n; i += (uint64_t)gridDim.x * KNEE_BLOCK) {
        heads[i] = (i == 0 || rec[i].barcode != rec[i - 1].barcode) ? 1u : 0u;
        reads += rec[i].count;
    }
    wave_add(stats + KP_READS_IN, reads);
}
// one lane per distinct barcode: a binary search in the ascending list (at most 32 halvings of a list below 2^32)
__global__ __launch_bounds__(KNEE_BLOCK) void pa_keep_search_kernel(const ull* __restrict__ distinct, uint32_t B, const ull* __restrict__ list, uint32_t n_list,
                                                                     uint32_t* __restrict__ listed, ull* __restrict__ stats) {
    ull found = 0;
    for (uint64_t b = (uint64_t)blockIdx.x * KNEE_BLOCK + threadIdx.x; b < B; b += (uint64_t)gridDim.x * KNEE_BLOCK) {
        const ull bc = distinct[b];
        uint32_t lo = 0, hi = n_list;   // the first entry >= bc lies in [lo, hi]
        for (uint32_t step = 0; step < 32 && lo < hi; ++step) {
            const uint32_t mid = lo + (hi - lo) / 2;
            if (list[mid] < bc) lo = mid + 1;
            else hi = mid;
        }
        const bool hit = lo < n_list && list[lo] == bc;
        listed[b] = hit ? 1u : 0u;
        found += hit;
    }
    wave_add(stats + KP_BARCODES_KEPT, found);
}
// one lane per record: kept[i] = its barcode is listed; the reads out
__global__ __launch_bounds__(KNEE_BLOCK) void pa_keep_flag_kernel(const pa_bus_record* __restrict__ rec, const uint32_t* __restrict__ pos, const uint32_t* __restrict__ listed,
                                                                   uint32_t n, uint32_t B, uint32_t* __restrict__ kept, ull* __restrict__ stats) {
    ull reads = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * KNEE_BLOCK + threadIdx.x; i < n; i += (uint64_t)gridDim.x * KNEE_BLOCK) {
        const uint32_t b = pos[i] - 1;
        const bool keep = b < B && listed[b] != 0;
        kept[i] = keep ? 1u : 0u;
        if (keep) reads += rec[i].count;
    }
    wave_add(stats + KP_READS_OUT, reads);
}
// kpos = the inclusive scan of kept: record i moves to kpos[i] - 1, as two 16-byte loads and stores
__global__ __launch_bounds__(KNEE_BLOCK) void pa_keep_compact_kernel(const pa_bus_record* __restrict__ rec, const uint32_t* __restrict__ kept, const uint32_t* __restrict__ kpos,
                                                                      uint32_t n, uint32_t n_out, pa_bus_record* __restrict__ out) {
    const uint32_t i = blockIdx.x * KNEE_BLOCK + threadIdx.x;
    if (i >= n || !kept[i] || kpos[i] - 1 >= n_out) return;
    copy_record(out + (kpos[i] - 1), rec + i);
}

uint32_t strided_grid(uint64_t items) { return std::min(grid_for(items, KNEE_BLOCK), KNEE_MAX_GRID); }

// the result of one knee, in HBM
struct KneeResult {
    DeviceBuffer<pa_bus_barcode_row> d_rows;
    DeviceBuffer<ull> d_called;
    uint64_t n_rows = 0, n_called = 0;
    uint64_t stats[PA_KNEE_STATS] = {};
};

// the empty table: no device work; the threshold is the rule's on an empty curve
int knee_empty(const pa_knee_params& p, KneeResult& res) {
    uint64_t L = 0;
    res.stats[KS_THRESHOLD] = knee::threshold(p, nullptr, nullptr, 0, &L);
    return PA_OK;
}

// d_in[n] (n >= 1, strictly ascending) on the current device -> res
int knee_device(const pa_bus_record* d_in, uint32_t n, const pa_knee_params& p, KneeResult& res) {
    hipStream_t s = nullptr;
    int e;
    PhaseClock<PA_KNEE_PHASES> clock;
    if ((e = clock.open()) || (e = clock.mark(0))) return e;
    DeviceBuffer<uint8_t> tmp;
    uint64_t* st = res.stats;

    // 1. the table
    const uint32_t n_tiles = grid_for(n, KNEE_TILE), grid = std::min(n_tiles, KNEE_MAX_GRID);
    DeviceBuffer<ull> d_tile_heads, d_tile_reads, d_scan_heads, d_scan_reads;
    if ((e = d_tile_heads.alloc(n_tiles)) || (e = d_tile_reads.alloc(n_tiles)) || (e = d_scan_heads.alloc(n_tiles)) || (e = d_scan_reads.alloc(n_tiles))) return e;
    if ((e = launch(pa_knee_tile_totals_kernel, grid, KNEE_BLOCK, s, d_in, n, n_tiles, d_tile_heads.get(), d_tile_reads.get()))) return e;
    ull total_heads = 0, total_reads = 0;
    if ((e = scan_inclusive_total(s, tmp, (const ull*)d_tile_heads.get(), d_scan_heads.get(), (size_t)n_tiles, total_heads)) ||
        (e = scan_inclusive_total(s, tmp, (const ull*)d_tile_reads.get(), d_scan_reads.get(), (size_t)n_tiles, total_reads)))
        return e;
    const uint32_t B = (uint32_t)(total_heads >> 32), molecules = (uint32_t)total_heads;
    if (B < 1 || B > n || molecules < B || molecules > n) return fail(PA_ERR_INTERNAL, "knee: %u barcodes and %u molecules in %u records", B, molecules, n);
    DeviceBuffer<KneeHead> d_heads;
    DeviceBuffer<uint32_t> d_umis, d_records, d_index, d_max;
    DeviceBuffer<ull> d_reads;
    if ((e = d_heads.alloc((size_t)B + 1)) || (e = d_umis.alloc(B)) || (e = d_records.alloc(B)) || (e = d_index.alloc(B)) || (e = d_reads.alloc(B)) || (e = d_max.alloc(1))) return e;
    PA_HIP_TRY(hipMemsetAsync(d_max.get(), 0, 4, s));
    if ((e = launch(pa_knee_heads_kernel, grid, KNEE_BLOCK, s, d_in, n, n_tiles, (const ull*)d_scan_heads.get(), (const ull*)d_scan_reads.get(), d_heads.get(), B))) return e;
    if ((e = launch(pa_knee_diff_kernel, strided_grid(B), KNEE_BLOCK, s, (const KneeHead*)d_heads.get(), B, d_umis.get(), d_records.get(), d_reads.get(), d_index.get(),
            d_max.get()))) return e;
    uint32_t max_umis = 0;
    if ((e = clock.mark(1)) || (e = fetch_u32(d_max.get(), s, max_umis))) return e;

    // 2. rank and curve: a stable descending sort of umis keeps equal values in ascending row (= barcode) order
    DeviceBuffer<uint32_t> d_sorted, d_sorted_index, d_rank, d_values, d_counts, d_runs;
    DeviceBuffer<ull> d_atleast;
    if ((e = d_sorted.alloc(B)) || (e = d_sorted_index.alloc(B)) || (e = d_rank.alloc(B)) || (e = d_values.alloc(B)) || (e = d_counts.alloc(B)) || (e = d_runs.alloc(1)) ||
        (e = d_atleast.alloc(B)))
        return e;
    if ((e = sort_pairs_desc(s, tmp, (const uint32_t*)d_umis.get(), d_sorted.get(), (const uint32_t*)d_index.get(), d_sorted_index.get(), (int)B, 0,
                             std::max(1u, bits_for(max_umis)))))
        return e;
    if ((e = launch(pa_knee_rank_kernel, grid_for(B, KNEE_BLOCK), KNEE_BLOCK, s, (const uint32_t*)d_sorted_index.get(), B, d_rank.get()))) return e;
    uint32_t D = 0;
    if ((e = run_length_encode(s, tmp, (const uint32_t*)d_sorted.get(), (size_t)B, d_values.get(), d_counts.get(), d_runs.get())) || (e = fetch_u32(d_runs.get(), s, D))) return e;
    if (D < 1 || D > B) return fail(PA_ERR_INTERNAL, "knee: %u distinct molecule counts over %u barcodes", D, B);
    if ((e = scan_inclusive(s, tmp, (const uint32_t*)d_counts.get(), d_atleast.get(), (size_t)D))) return e;
    std::vector<uint32_t> v(D);
    std::vector<uint64_t> R(D);
    PA_HIP_TRY(hipMemcpyAsync(v.data(), d_values.get(), (size_t)D * 4, hipMemcpyDeviceToHost, s));
    PA_HIP_TRY(hipMemcpyAsync(R.data(), d_atleast.get(), (size_t)D * 8, hipMemcpyDeviceToHost, s));
    if ((e = clock.mark(2))) return e;
    PA_HIP_TRY(hipStreamSynchronize(s));
    if (R[D - 1] != B || v[0] != max_umis) return fail(PA_ERR_INTERNAL, "knee: the curve ends at %llu of %u barcodes", (ull)R[D - 1], B);

    // 3. the threshold (host), the called list, the rows
    uint64_t L = 0;
    const uint64_t t = knee::threshold(p, v.data(), R.data(), D, &L);
    DeviceBuffer<uint32_t> d_flags, d_selected, d_n;
    DeviceBuffer<ull> d_sums;
    if ((e = res.d_rows.alloc(B)) || (e = d_flags.alloc(B)) || (e = d_selected.alloc(B)) || (e = d_n.alloc(1)) || (e = d_sums.alloc(2))) return e;
    PA_HIP_TRY(hipMemsetAsync(d_sums.get(), 0, 16, s));
    if ((e = launch(pa_knee_rows_kernel, strided_grid(B), KNEE_BLOCK, s, (const KneeHead*)d_heads.get(), (const uint32_t*)d_umis.get(), (const uint32_t*)d_records.get(),
            (const ull*)d_reads.get(), (const uint32_t*)d_rank.get(), B, (ull)t, res.d_rows.get(), d_flags.get(), d_sums.get()))) return e;
    uint32_t n_called = 0;
    if ((e = select_flagged_indices(s, tmp, (const uint32_t*)d_flags.get(), (size_t)B, d_selected.get(), d_n.get())) || (e = fetch_u32(d_n.get(), s, n_called))) return e;
    if (n_called > B) return fail(PA_ERR_INTERNAL, "knee: %u of %u barcodes called", n_called, B);
    if ((e = res.d_called.alloc(n_called ? n_called : 1))) return e;
    if (n_called) {
        if ((e = launch(pa_knee_called_kernel, grid_for(n_called, KNEE_BLOCK), KNEE_BLOCK, s, (const KneeHead*)d_heads.get(), (const uint32_t*)d_selected.get(), n_called, B,
                res.d_called.get()))) return e;
    }
    ull sums[2] = {};
    PA_HIP_TRY(hipMemcpyAsync(sums, d_sums.get(), 16, hipMemcpyDeviceToHost, s));
    if ((e = clock.mark(3)) || (e = clock.close(g_phase_ms))) return e;   // (synchronises)
    st[KS_RECORDS] = n;
    st[KS_READS] = total_reads;
    st[KS_MOLECULES] = molecules;
    st[KS_BARCODES] = B;
    st[KS_D] = D;
    st[KS_L] = L;
    st[KS_THRESHOLD] = t;
    st[KS_CALLED] = n_called;
    st[KS_CALLED_MOLECULES] = sums[0];
    st[KS_CALLED_READS] = sums[1];
    if (sums[0] > molecules || sums[1] > total_reads) return fail(PA_ERR_INTERNAL, "knee: the called barcodes hold more than the table");
    res.n_rows = B;
    res.n_called = n_called;
    return PA_OK;
}

// res -> the caller's arrays (either may be NULL), the counts and the stats
int knee_deliver(const KneeResult& res, pa_bus_barcode_row* rows, uint64_t rows_cap, uint64_t* n_rows, uint64_t* called, uint64_t called_cap, uint64_t* n_called,
                 uint64_t* stats) {
    *n_rows = res.n_rows;
    *n_called = res.n_called;
    if (stats) for (uint32_t j = 0; j < PA_KNEE_STATS; ++j) stats[j] = res.stats[j];
    if (rows && rows_cap < res.n_rows) return fail(PA_ERR_BUFFER_TOO_SMALL, "%llu rows, room for %llu", (ull)res.n_rows, (ull)rows_cap);
    if (called && called_cap < res.n_called) return fail(PA_ERR_BUFFER_TOO_SMALL, "%llu called barcodes, room for %llu", (ull)res.n_called, (ull)called_cap);
    if (rows && res.n_rows) PA_HIP_TRY(hipMemcpy(rows, res.d_rows.get(), res.n_rows * sizeof(pa_bus_barcode_row), hipMemcpyDeviceToHost));
    if (called && res.n_called) PA_HIP_TRY(hipMemcpy(called, res.d_called.get(), res.n_called * 8, hipMemcpyDeviceToHost));
    return PA_OK;
}

// d_in[n] (n >= 1, strictly ascending) on the current device, the list (checked) on the host -> d_out[*n_out], stats
int keep_device(const pa_bus_record* d_in, uint32_t n, const uint64_t* barcodes, uint64_t n_barcodes, DeviceBuffer<pa_bus_record>& d_out, uint64_t* n_out, uint64_t* stats) {
    hipStream_t s = nullptr;
    int e;
    DeviceBuffer<uint8_t> tmp;
    DeviceBuffer<ull> d_stats, d_list, d_distinct;
    DeviceBuffer<uint32_t> d_heads, d_pos, d_listed, d_kpos;
    if ((e = d_stats.alloc(PA_BUS_KEEP_STATS)) || (e = upload(d_list, (const ull*)barcodes, (size_t)n_barcodes)) || (e = d_heads.alloc(n)) || (e = d_pos.alloc(n)) ||
        (e = d_kpos.alloc(n)))
        return e;
    PA_HIP_TRY(hipMemsetAsync(d_stats.get(), 0, PA_BUS_KEEP_STATS * 8, s));
    if ((e = launch(pa_keep_heads_kernel, strided_grid(n), KNEE_BLOCK, s, d_in, n, d_heads.get(), d_stats.get()))) return e;
    uint32_t B = 0, kept = 0;
    if ((e = scan_inclusive_total(s, tmp, (const uint32_t*)d_heads.get(), d_pos.get(), (size_t)n, B))) return e;
    if (B < 1 || B > n) return fail(PA_ERR_INTERNAL, "keep: %u barcodes in %u records", B, n);
    if ((e = d_distinct.alloc(B)) || (e = d_listed.alloc(B)) ||
        (e = scatter_runs(s, RecordBarcode{d_in}, (const uint32_t*)d_heads.get(), (const uint32_t*)d_pos.get(), n, B, d_distinct.get(), nullptr)))
        return e;
    if ((e = launch(pa_keep_search_kernel, strided_grid(B), KNEE_BLOCK, s, (const ull*)d_distinct.get(), B, (const ull*)d_list.get(), (uint32_t)n_barcodes, d_listed.get(),
            d_stats.get()))) return e;
    DeviceBuffer<uint32_t>& d_kept = d_heads;   // (the heads are used up)
    if ((e = launch(pa_keep_flag_kernel, strided_grid(n), KNEE_BLOCK, s, d_in, (const uint32_t*)d_pos.get(), (const uint32_t*)d_listed.get(), n, B, d_kept.get(),
            d_stats.get()))) return e;
    if ((e = scan_inclusive_total(s, tmp, (const uint32_t*)d_kept.get(), d_kpos.get(), (size_t)n, kept))) return e;
    if (kept > n) return fail(PA_ERR_INTERNAL, "keep: %u of %u records kept", kept, n);
    if (kept) {
        if ((e = d_out.alloc(kept))) return e;
        if ((e = launch(pa_keep_compact_kernel, grid_for(n, KNEE_BLOCK), KNEE_BLOCK, s, d_in, (const uint32_t*)d_kept.get(), (const uint32_t*)d_kpos.get(), n, kept,
                d_out.get()))) return e;
    } else {
        d_out.release();
    }
    ull st[PA_BUS_KEEP_STATS] = {};
    PA_HIP_TRY(hipMemcpyAsync(st, d_stats.get(), sizeof st, hipMemcpyDeviceToHost, s));
    PA_HIP_TRY(hipStreamSynchronize(s));
    st[KP_RECORDS_IN] = n;
    st[KP_BARCODES_IN] = B;
    st[KP_RECORDS_OUT] = kept;
    if (st[KP_BARCODES_KEPT] > n_barcodes || st[KP_BARCODES_KEPT] > B) return fail(PA_ERR_INTERNAL, "keep: %llu barcodes kept of %u", st[KP_BARCODES_KEPT], B);
    st[KP_LISTED_ABSENT] = n_barcodes - st[KP_BARCODES_KEPT];
    *n_out = kept;
    if (stats) for (uint32_t j = 0; j < PA_BUS_KEEP_STATS; ++j) stats[j] = st[j];
    return PA_OK;
}

// no records: every listed barcode is absent
int keep_empty(uint64_t n_barcodes, uint64_t* stats) {
    if (stats) stats[KP_LISTED_ABSENT] = n_barcodes;
    return PA_OK;
}

int knee_of_writer(const pa_bus* b, const pa_knee_params* p, KneeResult& res) {
    pa_knee_params params;
    int e;
    if ((e = finished_writer(b, "cells are called after pa_bus_finish")) || (e = knee::take_params(p, params))) return e;
    return on_writer_records(b, [&](const pa_bus_record* d_in, uint32_t n) { return knee_device(d_in, n, params, res); }, [&] { return knee_empty(params, res); });
}

}  // namespace

int pa_bus_knee_vectors(const pa_bus* b, const pa_knee_params* p, std::vector<pa_bus_barcode_row>& rows, std::vector<uint64_t>& called, uint64_t* stats) {
    KneeResult res;
    int e;
    if ((e = knee_of_writer(b, p, res))) return e;
    rows.resize((size_t)res.n_rows);
    called.resize((size_t)res.n_called);
    uint64_t n_rows = 0, n_called = 0;
    return knee_deliver(res, rows.data(), rows.size(), &n_rows, called.data(), called.size(), &n_called, stats);
}

extern "C" {

int pa_bus_knee_records(pa_index* idx, const pa_bus_record* in, uint64_t n, uint32_t bc_len, uint32_t umi_len, const pa_knee_params* p, pa_bus_barcode_row* rows,
                        uint64_t rows_cap, uint64_t* n_rows, uint64_t* called, uint64_t called_cap, uint64_t* n_called, uint64_t stats[PA_KNEE_STATS]) {
    if (n_rows) *n_rows = 0;
    if (n_called) *n_called = 0;
    if (stats) memset(stats, 0, PA_KNEE_STATS * 8);
    if (!n_rows || !n_called) return fail(PA_ERR_INVALID_ARG, "null argument");
    pa_knee_params params;
    int e;
    if ((e = knee::take_params(p, params))) return e;
    if (n > 0x7FFFFFFFull) return fail(PA_ERR_UNSUPPORTED, "more than 2^31-1 records");
    KneeResult res;
    if ((e = knee::check_records(in, n, bc_len, umi_len)) ||
        (e = on_host_records(idx, in, n, [&](const pa_bus_record* d_in, uint32_t m) { return knee_device(d_in, m, params, res); }, [&] { return knee_empty(params, res); })))
        return e;
    return knee_deliver(res, rows, rows_cap, n_rows, called, called_cap, n_called, stats);
}

int pa_bus_knee(const pa_bus* b, const pa_knee_params* p, pa_bus_barcode_row* rows, uint64_t rows_cap, uint64_t* n_rows, uint64_t* called, uint64_t called_cap,
                uint64_t* n_called, uint64_t stats[PA_KNEE_STATS]) {
    if (n_rows) *n_rows = 0;
    if (n_called) *n_called = 0;
    if (stats) memset(stats, 0, PA_KNEE_STATS * 8);
    if (!n_rows || !n_called) return fail(PA_ERR_INVALID_ARG, "null argument");
    KneeResult res;
    int e;
    if ((e = knee_of_writer(b, p, res))) return e;
    return knee_deliver(res, rows, rows_cap, n_rows, called, called_cap, n_called, stats);
}

int pa_bus_knee_phase_ms(float out[PA_KNEE_PHASES]) {
    if (!out) return fail(PA_ERR_INVALID_ARG, "null argument");
    for (int i = 0; i < PA_KNEE_PHASES; ++i) out[i] = g_phase_ms[i];
    return PA_OK;
}

int pa_bus_keep_records(pa_index* idx, const pa_bus_record* in, uint64_t n, uint32_t bc_len, uint32_t umi_len, const uint64_t* barcodes, uint64_t n_barcodes,
                        pa_bus_record* out, uint64_t cap, uint64_t* n_out, uint64_t stats[PA_BUS_KEEP_STATS]) {
    if (n_out) *n_out = 0;
    if (stats) memset(stats, 0, PA_BUS_KEEP_STATS * 8);
    if (!n_out) return fail(PA_ERR_INVALID_ARG, "null argument");
    int e;
    if (n > 0x7FFFFFFFull) return fail(PA_ERR_UNSUPPORTED, "more than 2^31-1 records");
    if (n_barcodes > 0x7FFFFFFFull) return fail(PA_ERR_UNSUPPORTED, "a list of more than 2^31-1 barcodes");
    DeviceBuffer<pa_bus_record> d_out;
    if ((e = knee::check_records(in, n, bc_len, umi_len)) || (e = knee::check_list(barcodes, n_barcodes, bc_len)) ||
        (e = on_host_records(idx, in, n, [&](const pa_bus_record* d_in, uint32_t m) { return keep_device(d_in, m, barcodes, n_barcodes, d_out, n_out, stats); },
                             [&] { return keep_empty(n_barcodes, stats); })))
        return e;
    return deliver_records(d_out, *n_out, out, cap);
}

int pa_bus_keep(pa_bus* b, const uint64_t* barcodes, uint64_t n_barcodes, uint64_t stats[PA_BUS_KEEP_STATS]) {
    if (stats) memset(stats, 0, PA_BUS_KEEP_STATS * 8);
    int e;
    if ((e = finished_writer(b, "the records are filtered after pa_bus_finish"))) return e;
    if (n_barcodes > 0x7FFFFFFFull) return fail(PA_ERR_UNSUPPORTED, "a list of more than 2^31-1 barcodes");
    if ((e = knee::check_list(barcodes, n_barcodes, b->bc_len))) return e;
    return rewrite_writer_records(b, [&](const pa_bus_record* d_in, uint32_t n, DeviceBuffer<pa_bus_record>& d_out, uint64_t* n_out) {
        return keep_device(d_in, n, barcodes, n_barcodes, d_out, n_out, stats);
    }, [&] { return keep_empty(n_barcodes, stats); });
}

}  // extern "C"
