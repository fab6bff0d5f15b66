// UMI correction on BUS records (pa_bus_umi_correct, include/pseudoaligner_amd.h): the `bustools umicorrect` step on the records where
// they lie, ahead of the gene counter. The molecule table is the gene counter's (molecule_stage.hpp: heads over (barcode, UMI), S(m) as (offset, length)
// into one id buffer) plus n(m) from a segmented u64 sum; barcode segments are the heads over the molecules' barcodes. The neighbour search writes
// target[m] and nothing else: a barcode's UMIs lie ascending and contiguous, so a small barcode is compared all against all by a lane per molecule,
// a larger one is staged into LDS by its block and each lane binary-searches the 3 umi_len single substitutions of its molecule there, and one beyond
// the LDS cap is searched the same way in HBM. Only a hit loads n(v) and S(v). Every decision reads the input state alone, no molecule's slot is
// written by more than its own lane, the counters are summed per wave and added with integer atomics once per wave. The records of moved
// molecules then take their target's UMI and go through the sort + collapse tail of the barcode correction (bus_state.hpp); nothing moved: a copy.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "bus_state.hpp"
#include "bus_umi_host.hpp"
#include "bus_umi_state.hpp"
#include "device_prims.hpp"
#include "genes_host.hpp"
#include "hip_buffer.hpp"
#include "kernel_utils.hpp"
#include "molecule_stage.hpp"
#include "pa_common.hpp"
#include "phase_clock.hpp"

using namespace pa;

namespace {

constexpr uint32_t UM_MAX_GRID = 2048;       // blocks of a kernel whose lanes stride over their items and add their counters once per wave
#ifdef PA_UMI_FORCE_HBM                      // a TEST build (tools/bench_umi.py): the barcodes of the block bin take the HBM variant
constexpr uint32_t UM_BLOCK_BIN_MAX = UM_LANE_MAX;
#else
constexpr uint32_t UM_BLOCK_BIN_MAX = UM_LDS_CAP;
#endif
constexpr uint32_t UM_NONE = 0xFFFFFFFFu;
enum : uint32_t { US_RECORDS_IN = 0, US_READS_IN, US_MOLECULES_IN, US_BARCODES, US_INERT, US_HAMMING1, US_NEIGHBOUR, US_MOVED, US_CHAINED, US_RECORDS_REWRITTEN, US_READS_MOVED,
                  US_RECORDS_OUT, US_MOLECULES_OUT, US_LARGEST, US_HBM };
static_assert(US_HBM + 1 == PA_BUS_UMI_STATS, "the stats of the header");
static_assert(UM_LANE_MAX >= 1 && UM_LANE_MAX < UM_LDS_CAP && UM_LDS_CAP * 8 <= 64 * 1024, "three bins; the u64 words of the block bin fill 64 KiB at most");
static_assert(UM_BLOCK == GN_BLOCK, "one block size for the molecule stage and the search");

thread_local float g_phase_ms[PA_BUS_UMI_PHASES] = {};

uint32_t stride_grid(uint64_t n) { return std::max(1u, std::min(grid_for(n, UM_BLOCK), UM_MAX_GRID)); }

__device__ inline ull wave_max(ull v) {   // valid in lane 0 (every lane calls)
    for (int off = 32; off > 0; off >>= 1) v = max(v, (ull)__shfl_down(v, off));
    return v;
}

// ---- 1. the molecule table: what the molecule stage leaves, plus n(m), the UMI and the barcode segments ----
__global__ __launch_bounds__(UM_BLOCK) void um_record_counts(const pa_bus_record* __restrict__ rec, uint32_t n, ull* __restrict__ cnt, ull* __restrict__ stats) {
    ull reads = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * UM_BLOCK + threadIdx.x; i < n; i += (uint64_t)gridDim.x * UM_BLOCK) {
        const ull c = rec[i].count;
        cnt[i] = c;
        reads += c;
    }
    wave_add(stats + US_READS_IN, reads);
}
__global__ __launch_bounds__(UM_BLOCK) void um_mol_info(const pa_bus_record* __restrict__ rec, const uint32_t* __restrict__ mol_start, const uint32_t* __restrict__ mol_len,
                                                        uint32_t n_mol, ull* __restrict__ mol_umi, uint32_t* __restrict__ bc_heads, ull* __restrict__ stats) {
    ull inert = 0;
    for (uint64_t m = (uint64_t)blockIdx.x * UM_BLOCK + threadIdx.x; m < n_mol; m += (uint64_t)gridDim.x * UM_BLOCK) {
        const pa_bus_record* r = rec + mol_start[m];
        mol_umi[m] = r->umi;
        bc_heads[m] = (m == 0 || r->barcode != rec[mol_start[m - 1]].barcode) ? 1u : 0u;
        inert += mol_len[m] ? 0u : 1u;
    }
    wave_add(stats + US_INERT, inert);
}
// barcode b = molecules [bc_start[b], bc_start[b + 1]) (the last one ends at n_mol): its bin, and the largest
__global__ __launch_bounds__(UM_BLOCK) void um_bins(const uint32_t* __restrict__ bc_start, uint32_t n_bc, uint32_t n_mol, uint32_t* __restrict__ in_block,
                                                    uint32_t* __restrict__ in_hbm, ull* __restrict__ stats) {
    ull largest = 0;
    for (uint64_t b = (uint64_t)blockIdx.x * UM_BLOCK + threadIdx.x; b < n_bc; b += (uint64_t)gridDim.x * UM_BLOCK) {
        const uint32_t size = (b + 1 < n_bc ? bc_start[b + 1] : n_mol) - bc_start[b];
        in_block[b] = (size > UM_LANE_MAX && size <= UM_BLOCK_BIN_MAX) ? 1u : 0u;
        in_hbm[b] = size > UM_BLOCK_BIN_MAX ? 1u : 0u;
        largest = max(largest, (ull)size);
    }
    largest = wave_max(largest);
    if ((threadIdx.x & 63) == 0 && largest) atomicMax(stats + US_LARGEST, largest);
}

// ---- 2. the neighbour search ----
struct SearchArgs {
    const ull* mol_umi;          // [n_mol] ascending inside a barcode
    const ull* mol_n;            // [n_mol] n(m)
    const ull* mol_off;          // S(m) = ids[mol_off .. mol_off + mol_len), ascending; mol_len 0: inert
    const uint32_t* mol_len;
    const uint32_t* ids;
    const uint32_t* bc_start;    // [n_bc]
    const uint32_t* bc_of;       // [n_mol] barcode number + 1 (the inclusive scan of the barcode heads)
    uint32_t n_mol, n_bc, umi_len, mode;
    uint32_t* target;            // [n_mol]
    ull* stats;
};
struct Best {
    ull n, umi;                  // the greatest (n, UMI) so far, m's own at the start
    uint32_t mol, hamming1, neighbour;
};
struct Tally { ull hamming1 = 0, neighbour = 0, moved = 0; };

__device__ __forceinline__ uint32_t bc_end(const SearchArgs& p, uint32_t b) { return b + 1 < p.n_bc ? p.bc_start[b + 1] : p.n_mol; }

// two ascending lists share an id (nearly always two singletons)
__device__ __forceinline__ bool um_sets_meet(const uint32_t* __restrict__ a, uint32_t la, const uint32_t* __restrict__ b, uint32_t lb) {
    uint32_t i = 0, j = 0;
    while (i < la && j < lb) {
        const uint32_t x = a[i], y = b[j];
        if (x == y) return true;
        if (x < y) ++i; else ++j;
    }
    return false;
}
// molecule v holds a UMI one substitution from m's: only now n(v) and S(v) are loaded
__device__ __forceinline__ void um_consider(const SearchArgs& p, uint32_t m, uint32_t v, Best& best) {
    best.hamming1 = 1;
    if (!um_sets_meet(p.ids + p.mol_off[m], p.mol_len[m], p.ids + p.mol_off[v], p.mol_len[v])) return;   // (an inert v has no ids)
    best.neighbour = 1;
    const ull nv = p.mol_n[v], uv = p.mol_umi[v];
    if (p.mode == PA_UMI_DIRECTIONAL && p.mol_n[m] > (nv + 1) / 2) return;   // n(v) >= 2 n(m) - 1, without the product (n(v) < 2^63)
    if (nv > best.n || (nv == best.n && uv > best.umi)) { best.n = nv; best.umi = uv; best.mol = v; }
}
__device__ __forceinline__ void um_decided(const SearchArgs& p, uint32_t m, const Best& best, Tally& t) {
    p.target[m] = best.mol;
    t.hamming1 += best.hamming1;
    t.neighbour += best.neighbour;
    t.moved += best.mol != m ? 1u : 0u;
}
__device__ __forceinline__ void um_tally(const SearchArgs& p, const Tally& t) {
    wave_add(p.stats + US_HAMMING1, t.hamming1);
    wave_add(p.stats + US_NEIGHBOUR, t.neighbour);
    wave_add(p.stats + US_MOVED, t.moved);
}

// the lane bin: a lane per molecule of a barcode of up to UM_LANE_MAX molecules, its UMI against every other one of the barcode. XOR, the two bits
// of each base ORed into one, one bit set = one base differs
__global__ __launch_bounds__(UM_BLOCK) void um_search_lane(const SearchArgs p) {
    Tally t;
    for (uint64_t i = (uint64_t)blockIdx.x * UM_BLOCK + threadIdx.x; i < p.n_mol; i += (uint64_t)gridDim.x * UM_BLOCK) {
        const uint32_t m = (uint32_t)i, b = p.bc_of[m] - 1, m0 = p.bc_start[b], m1 = bc_end(p, b);
        if (m1 - m0 > UM_LANE_MAX) continue;
        const ull u = p.mol_umi[m];
        Best best{p.mol_n[m], u, m, 0u, 0u};
        if (p.mol_len[m])
            for (uint32_t v = m0; v < m1; ++v) {
                const ull x = p.mol_umi[v] ^ u;
                if (__popcll((x | (x >> 1)) & 0x5555555555555555ull) == 1) um_consider(p, m, v, best);
            }
        um_decided(p, m, best, t);
    }
    um_tally(p, t);
}

// position of key in the ascending arr[cnt], or UM_NONE
template <class A>
__device__ __forceinline__ uint32_t um_find(const A* __restrict__ arr, uint32_t cnt, ull key) {
    uint32_t lo = 0, hi = cnt;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if ((ull)arr[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo < cnt && (ull)arr[lo] == key ? lo : UM_NONE;
}
// the block bin and the HBM variant: a block per listed barcode. W: the word its UMIs are staged in (u32 up to 16 bases); HBM: nothing is staged
// and the search reads the molecule table itself
template <class W, bool HBM>
__global__ __launch_bounds__(UM_BLOCK) void um_search_block(const SearchArgs p, const uint32_t* __restrict__ list) {
    __shared__ W lds[HBM ? 1 : UM_LDS_CAP];
    const uint32_t b = list[blockIdx.x], m0 = p.bc_start[b], cnt = bc_end(p, b) - m0;
    if (!HBM) {   // (cnt <= UM_LDS_CAP: the host put the barcode on this list)
        if (cnt > UM_LDS_CAP) return;
        for (uint32_t j = threadIdx.x; j < cnt; j += UM_BLOCK) lds[j] = (W)p.mol_umi[m0 + j];
        __syncthreads();
    }
    Tally t;
    for (uint32_t j = threadIdx.x; j < cnt; j += UM_BLOCK) {
        const uint32_t m = m0 + j;
        const ull u = p.mol_umi[m];
        Best best{p.mol_n[m], u, m, 0u, 0u};
        if (p.mol_len[m])
            for (uint32_t c = 0; c < 3 * p.umi_len; ++c) {   // base c / 3 from the last one, substitution 1 + c % 3 (xor of the base's two bits)
                const ull key = u ^ ((ull)(1 + c % 3) << (2 * (c / 3)));
                const uint32_t at = HBM ? um_find(p.mol_umi + m0, cnt, key) : um_find(lds, cnt, key);
                if (at != UM_NONE) um_consider(p, m, m0 + at, best);
            }
        um_decided(p, m, best, t);
    }
    um_tally(p, t);
}

// ---- 3. rewrite ----
// record i of molecule pos[i] - 1 as a key under its target's UMI
__global__ __launch_bounds__(UM_BLOCK) void um_rewrite(const pa_bus_record* __restrict__ rec, const uint32_t* __restrict__ pos, const uint32_t* __restrict__ target,
                                                       const ull* __restrict__ mol_umi, uint32_t n, uint32_t umi_bits, u128* __restrict__ keys, uint32_t* __restrict__ counts) {
    const uint32_t i = blockIdx.x * UM_BLOCK + threadIdx.x;
    if (i >= n) return;
    const RecordWords r = load_record(rec + i);
    const ull bc = (ull)r.a.x | ((ull)r.a.y << 32);
    const ull w = (bc << umi_bits) | mol_umi[target[pos[i] - 1]];
    keys[i] = ((u128)w << 32) | (u128)(r.c.x ^ EC_BIAS);
    counts[i] = r.c.y;
}
// nothing moved: the records as they are, flags and pad written as 0
__global__ __launch_bounds__(UM_BLOCK) void um_copy(const pa_bus_record* __restrict__ rec, uint32_t n, pa_bus_record* __restrict__ out) {
    const uint32_t i = blockIdx.x * UM_BLOCK + threadIdx.x;
    if (i >= n) return;
    RecordWords r = load_record(rec + i);
    r.c.z = r.c.w = 0u;
    store_record(out + i, r);
}

// ---- 4. stats ----
__global__ __launch_bounds__(UM_BLOCK) void um_moves(const uint32_t* __restrict__ target, const uint32_t* __restrict__ mol_start, const ull* __restrict__ mol_n, uint32_t n_mol,
                                                     uint32_t n, ull* __restrict__ stats) {
    ull chained = 0, records = 0, reads = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * UM_BLOCK + threadIdx.x; i < n_mol; i += (uint64_t)gridDim.x * UM_BLOCK) {
        const uint32_t m = (uint32_t)i, t = target[m];
        if (t == m) continue;
        chained += target[t] != t ? 1u : 0u;
        records += (m + 1 < n_mol ? mol_start[m + 1] : n) - mol_start[m];
        reads += mol_n[m];
    }
    wave_add(stats + US_CHAINED, chained);
    wave_add(stats + US_RECORDS_REWRITTEN, records);
    wave_add(stats + US_READS_MOVED, reads);
}
__global__ __launch_bounds__(UM_BLOCK) void um_molecules_out(const pa_bus_record* __restrict__ rec, uint32_t n, ull* __restrict__ stats) {
    ull heads = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * UM_BLOCK + threadIdx.x; i < n; i += (uint64_t)gridDim.x * UM_BLOCK)
        if (i == 0 || rec[i].barcode != rec[i - 1].barcode || rec[i].umi != rec[i - 1].umi) ++heads;
    wave_add(stats + US_MOLECULES_OUT, heads);
}

// d_in[n] (n >= 1, checked) on the current device, the ec -> gene-set table on the host -> d_out[*n_out], stats
int umi_device(const pa_bus_record* d_in, uint32_t n, uint32_t bc_len, uint32_t umi_len, const genes::GeneSets& gs, uint32_t mode, DeviceBuffer<pa_bus_record>& d_out,
               uint64_t* n_out, uint64_t* stats) {
    hipStream_t s = nullptr;
    int e;
    PhaseClock<PA_BUS_UMI_PHASES> clock;
    if ((e = clock.open()) || (e = clock.mark(0))) return e;
    DeviceBuffer<uint8_t> tmp;
    DeviceBuffer<ull> d_stats;
    DeviceBuffer<uint32_t> d_n;
    if ((e = d_stats.alloc(PA_BUS_UMI_STATS)) || (e = d_n.alloc(4))) return e;
    PA_HIP_TRY(hipMemsetAsync(d_stats.get(), 0, PA_BUS_UMI_STATS * 8, s));

    // 1. molecules: starts, S(m); a record's molecule number; n(m) by a segmented sum; UMIs and barcode segments
    DeviceBuffer<uint32_t> heads, flags, pos;
    MolTable mt;
    if ((e = heads.alloc(n)) || (e = flags.alloc(n)) || (e = pos.alloc(n)) || (e = molecule_table(s, tmp, d_n.get(), d_in, n, gs, heads.get(), flags.get(), mt))) return e;
    const uint32_t n_mol = mt.n_mol;
    DeviceBuffer<ull> cnt, mol_n, mol_umi;
    DeviceBuffer<uint32_t> mol_id, bc_heads, bc_of, bc_start, in_block, in_hbm, block_list, hbm_list, target;
    uint32_t n_bc = 0, n_runs = 0, n_block = 0, n_hbm = 0;
    if ((e = cnt.alloc(n)) || (e = mol_n.alloc(n_mol)) || (e = mol_umi.alloc(n_mol)) || (e = mol_id.alloc(n_mol)) || (e = bc_heads.alloc(n_mol)) || (e = bc_of.alloc(n_mol)) ||
        (e = target.alloc(n_mol)))
        return e;
    if ((e = scan_inclusive(s, tmp, (const uint32_t*)heads.get(), pos.get(), (size_t)n))) return e;
    if ((e = launch(um_record_counts, stride_grid(n), UM_BLOCK, s, d_in, n, cnt.get(), d_stats.get()))) return e;
    if ((e = reduce_by_key_sum(s, tmp, (const uint32_t*)pos.get(), (const ull*)cnt.get(), (size_t)n, mol_id.get(), mol_n.get(), d_n.get())) || (e = fetch_u32(d_n.get(), s, n_runs)))
        return e;
    if (n_runs != n_mol) return fail(PA_ERR_INTERNAL, "UMI correction: %u molecule sums for %u molecules", n_runs, n_mol);
    if ((e = launch(um_mol_info, stride_grid(n_mol), UM_BLOCK, s, d_in, (const uint32_t*)mt.mol_start.get(), (const uint32_t*)mt.mol_len.get(), n_mol, mol_umi.get(),
            bc_heads.get(), d_stats.get())))
        return e;
    if ((e = scan_inclusive_total(s, tmp, (const uint32_t*)bc_heads.get(), bc_of.get(), (size_t)n_mol, n_bc))) return e;
    if ((e = bc_start.alloc(n_bc)) || (e = in_block.alloc(n_bc)) || (e = in_hbm.alloc(n_bc)) || (e = block_list.alloc(n_bc)) || (e = hbm_list.alloc(n_bc))) return e;
    if ((e = select_flagged_indices(s, tmp, (const uint32_t*)bc_heads.get(), (size_t)n_mol, bc_start.get(), d_n.get()))) return e;
    if ((e = launch(um_bins, stride_grid(n_bc), UM_BLOCK, s, (const uint32_t*)bc_start.get(), n_bc, n_mol, in_block.get(), in_hbm.get(), d_stats.get()))) return e;
    if ((e = select_flagged_indices(s, tmp, (const uint32_t*)in_block.get(), (size_t)n_bc, block_list.get(), d_n.get())) || (e = fetch_u32(d_n.get(), s, n_block))) return e;
    if ((e = select_flagged_indices(s, tmp, (const uint32_t*)in_hbm.get(), (size_t)n_bc, hbm_list.get(), d_n.get())) || (e = fetch_u32(d_n.get(), s, n_hbm))) return e;
    if (n_block > n_bc || n_hbm > n_bc) return fail(PA_ERR_INTERNAL, "UMI correction: more listed barcodes than barcodes");
    if ((e = clock.mark(1))) return e;

    // 2. the search: one launch per bin
    SearchArgs p{};
    p.mol_umi = mol_umi.get(); p.mol_n = mol_n.get(); p.mol_off = mt.mol_off.get(); p.mol_len = mt.mol_len.get(); p.ids = mt.ids.get(); p.bc_start = bc_start.get();
    p.bc_of = bc_of.get(); p.n_mol = n_mol; p.n_bc = n_bc; p.umi_len = umi_len; p.mode = mode; p.target = target.get(); p.stats = d_stats.get();
    if ((e = launch(um_search_lane, stride_grid(n_mol), UM_BLOCK, s, p))) return e;
    if (n_block) {
        if (umi_len <= 16) e = launch(um_search_block<uint32_t, false>, n_block, UM_BLOCK, s, p, (const uint32_t*)block_list.get());
        else e = launch(um_search_block<ull, false>, n_block, UM_BLOCK, s, p, (const uint32_t*)block_list.get());
        if (e) return e;
    }
    if (n_hbm && (e = launch(um_search_block<ull, true>, n_hbm, UM_BLOCK, s, p, (const uint32_t*)hbm_list.get()))) return e;
    ull st[PA_BUS_UMI_STATS] = {};
    if ((e = clock.mark(2))) return e;
    PA_HIP_TRY(hipMemcpyAsync(st, d_stats.get(), sizeof st, hipMemcpyDeviceToHost, s));
    PA_HIP_TRY(hipStreamSynchronize(s));

    // 3. rewrite; a molecule moved: sort, join equal keys
    uint32_t M = n;
    if (st[US_MOVED]) {
        DeviceBuffer<u128> keys;
        DeviceBuffer<uint32_t> counts;
        if ((e = keys.alloc(n)) || (e = counts.alloc(n))) return e;
        if ((e = launch(um_rewrite, grid_for(n, UM_BLOCK), UM_BLOCK, s, d_in, (const uint32_t*)pos.get(), (const uint32_t*)target.get(), (const ull*)mol_umi.get(), n, 2 * umi_len,
                keys.get(), counts.get())))
            return e;
        if ((e = records_from_keys(s, tmp, keys, counts, n, true, 32 + 2 * (bc_len + umi_len), 2 * umi_len, d_out, M))) return e;
        PA_HIP_TRY(hipStreamSynchronize(s));   // (keys and counts leave scope)
    } else {
        if ((e = d_out.alloc(n)) || (e = launch(um_copy, grid_for(n, UM_BLOCK), UM_BLOCK, s, d_in, n, d_out.get()))) return e;
    }
    if ((e = clock.mark(3))) return e;

    // 4. stats
    if ((e = launch(um_moves, stride_grid(n_mol), UM_BLOCK, s, (const uint32_t*)target.get(), (const uint32_t*)mt.mol_start.get(), (const ull*)mol_n.get(), n_mol, n, d_stats.get())) ||
        (e = launch(um_molecules_out, stride_grid(M), UM_BLOCK, s, (const pa_bus_record*)d_out.get(), M, d_stats.get())))
        return e;
    PA_HIP_TRY(hipMemcpyAsync(st, d_stats.get(), sizeof st, hipMemcpyDeviceToHost, s));
    if ((e = clock.mark(4)) || (e = clock.close(g_phase_ms))) return e;   // (synchronises)
    st[US_RECORDS_IN] = n;
    st[US_MOLECULES_IN] = n_mol;
    st[US_BARCODES] = n_bc;
    st[US_RECORDS_OUT] = M;
    st[US_HBM] = n_hbm;
    if (st[US_MOVED] > st[US_NEIGHBOUR] || st[US_NEIGHBOUR] > st[US_HAMMING1] || st[US_HAMMING1] + st[US_INERT] > n_mol || M > n || st[US_MOLECULES_OUT] > n_mol)
        return fail(PA_ERR_INTERNAL, "UMI correction: the counts do not add up");
    *n_out = M;
    if (stats) for (uint32_t j = 0; j < PA_BUS_UMI_STATS; ++j) stats[j] = st[j];
    return PA_OK;
}

}  // namespace

extern "C" {

int pa_bus_umi_correct_records(pa_index* idx, const pa_bus_record* in, uint64_t n, const uint64_t* ec_offsets, const uint32_t* ec_ids, uint32_t n_ecs, uint32_t num_tx,
                               const uint32_t* tx_gene, uint32_t num_genes, uint32_t bc_len, uint32_t umi_len, uint32_t mode, pa_bus_record* out, uint64_t cap, uint64_t* n_out,
                               uint64_t stats[PA_BUS_UMI_STATS]) {
    if (n_out) *n_out = 0;
    if (stats) memset(stats, 0, PA_BUS_UMI_STATS * 8);
    if (!n_out) return fail(PA_ERR_INVALID_ARG, "null argument");
    int e;
    if ((e = umi::check_call(in, n, ec_offsets, ec_ids, n_ecs, num_tx, tx_gene, num_genes, bc_len, umi_len, mode))) return e;
    DeviceBuffer<pa_bus_record> d_out;
    if ((e = on_host_records(idx, in, n, [&](const pa_bus_record* d_in, uint32_t m) {
            genes::GeneSets gs;
            genes::gene_sets(ec_offsets, ec_ids, n_ecs, tx_gene, gs);
            return umi_device(d_in, m, bc_len, umi_len, gs, mode, d_out, n_out, stats);
        }, empty_ok)))
        return e;
    return deliver_records(d_out, *n_out, out, cap);
}

int pa_bus_umi_correct(pa_bus* b, const uint32_t* tx_gene, uint32_t num_genes, uint32_t mode, uint64_t stats[PA_BUS_UMI_STATS]) {
    if (stats) memset(stats, 0, PA_BUS_UMI_STATS * 8);
    int e;
    if ((e = finished_writer(b, "the UMIs are corrected after pa_bus_finish")) || (e = umi::check_mode(mode)) || (e = genes::check_lengths(b->bc_len, b->umi_len))) return e;
    const uint32_t n_ecs = (uint32_t)b->table.n_ecs();
    if ((e = genes::check_tables(b->table.offsets.data(), b->table.ids.data(), n_ecs, b->num_tx, tx_gene, num_genes))) return e;
    return rewrite_writer_records(b, [&](const pa_bus_record* d_in, uint32_t n, DeviceBuffer<pa_bus_record>& d_out, uint64_t* n_out) {
        genes::GeneSets gs;
        genes::gene_sets(b->table.offsets.data(), b->table.ids.data(), n_ecs, tx_gene, gs);
        return umi_device(d_in, n, b->bc_len, b->umi_len, gs, mode, d_out, n_out, stats);
    }, empty_ok);
}

int pa_bus_umi_correct_phase_ms(float out[PA_BUS_UMI_PHASES]) {
    if (!out) return fail(PA_ERR_INVALID_ARG, "null argument");
    for (int i = 0; i < PA_BUS_UMI_PHASES; ++i) out[i] = g_phase_ms[i];
    return PA_OK;
}

}  // extern "C"
