// The molecule stage over sorted BUS records, shared by the gene counter (genes.hip) and the UMI correction (bus_umi.hip): run heads over
// (barcode, UMI); every molecule's gene set = the intersection of its records' G(e) (one record: G(e) itself by reference into the table; up to
// GN_LANE_RECORDS records: a lane; more: a wave), counted, scanned and written behind the table in one id buffer. Private to those two sources.
#pragma once
#include <hip/hip_runtime.h>

#include "device_prims.hpp"
#include "genes_host.hpp"
#include "genes_state.hpp"
#include "hip_buffer.hpp"
#include "kernel_utils.hpp"
#include "pa_common.hpp"

namespace {   // (kernels and helpers of the including source: every code object gets its own)

typedef unsigned long long ull;
constexpr uint32_t B = pa::GN_BLOCK;
using pa::GN_LANE_RECORDS;

#define GN_LAUNCH(kernel, items, s, ...) do { const int e_ = pa::launch(kernel, pa::grid_for(items, B), B, s, __VA_ARGS__); if (e_ != PA_OK) return e_; } while (0)

// ---- molecule stage ----
__global__ __launch_bounds__(B) void gn_mol_heads(const pa_bus_record* __restrict__ rec, uint32_t n, uint32_t* __restrict__ heads) {
    const uint32_t i = blockIdx.x * B + threadIdx.x;
    if (i < n) heads[i] = (i == 0 || rec[i].barcode != rec[i - 1].barcode || rec[i].umi != rec[i - 1].umi) ? 1u : 0u;
}

struct MolArgs {
    const pa_bus_record* rec;
    uint32_t n, n_mol;
    const uint32_t* mol_start;   // [n_mol]
    const ull* gs_off;           // [n_ecs + 1]
    const ull* gs_hash;          // [n_ecs]
    const uint32_t* sets;        // G(e) lists (count pass: the table; fill pass: the id buffer, which begins with the table)
    ull table_ids;               // ids of the table: the molecules' own lists lie behind them
    uint32_t* need;              // [n_mol] ids of a molecule's own list (0 for a molecule of one record)
    const ull* aoff;             // [n_mol] exclusive scan of need
    uint32_t* out;               // the id buffer (fill pass)
    ull* mol_off;                // [n_mol] a molecule's set = ids[mol_off .. mol_off + mol_len)
    uint32_t* mol_len;
    ull* mol_hash;
    const uint32_t* long_idx;    // the molecules of more than GN_LANE_RECORDS records
    uint32_t n_long;
};

__device__ __forceinline__ uint32_t mol_end(const MolArgs& p, uint32_t i) { return i + 1 < p.n_mol ? p.mol_start[i + 1] : p.n; }
__device__ __forceinline__ bool gn_has(const uint32_t* __restrict__ v, uint32_t n, uint32_t x) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (v[mid] < x) lo = mid + 1; else hi = mid;
    }
    return lo < n && v[lo] == x;
}
// x in G(e) of every record of [a + 1, b)
__device__ __forceinline__ bool gn_in_all(const MolArgs& p, uint32_t a, uint32_t b, uint32_t x) {
    for (uint32_t r = a + 1; r < b; ++r) {
        const uint32_t ec = (uint32_t)p.rec[r].ec;
        const ull o = p.gs_off[ec];
        if (!gn_has(p.sets + o, (uint32_t)(p.gs_off[ec + 1] - o), x)) return false;
    }
    return true;
}

// a lane per molecule: one record -> G(e) by reference (count pass); 2 .. GN_LANE_RECORDS records -> counted, then written
template <bool FILL>
__global__ __launch_bounds__(B) void gn_intersect_lane(const MolArgs p) {
    const uint32_t i = blockIdx.x * B + threadIdx.x;
    if (i >= p.n_mol) return;
    const uint32_t a = p.mol_start[i], b = mol_end(p, i), m = b - a;
    const uint32_t ec0 = (uint32_t)p.rec[a].ec;
    const ull o0 = p.gs_off[ec0];
    const uint32_t l0 = (uint32_t)(p.gs_off[ec0 + 1] - o0);
    if (m == 1) {
        if (!FILL) { p.need[i] = 0; p.mol_off[i] = o0; p.mol_len[i] = l0; p.mol_hash[i] = p.gs_hash[ec0]; }
        return;
    }
    if (m > GN_LANE_RECORDS) {
        if (!FILL) p.need[i] = 0;   // (the wave kernel overwrites it)
        return;
    }
    uint32_t* dst = FILL ? p.out + p.table_ids + p.aoff[i] : nullptr;
    uint32_t cnt = 0;
    for (uint32_t j = 0; j < l0; ++j) {
        const uint32_t x = p.sets[o0 + j];
        if (gn_in_all(p, a, b, x)) {
            if (FILL) dst[cnt] = x;
            ++cnt;
        }
    }
    if (!FILL) p.need[i] = cnt;
}

// a wave per long molecule: 64 candidates of the first record's set at a time, kept ones written in order behind a ballot
template <bool FILL>
__global__ __launch_bounds__(B) void gn_intersect_wave(const MolArgs p) {
    const uint32_t w = (blockIdx.x * B + threadIdx.x) / 64, lane = threadIdx.x & 63;
    if (w >= p.n_long) return;
    const uint32_t i = p.long_idx[w];
    const uint32_t a = p.mol_start[i], b = mol_end(p, i);
    const uint32_t ec0 = (uint32_t)p.rec[a].ec;
    const ull o0 = p.gs_off[ec0];
    const uint32_t l0 = (uint32_t)(p.gs_off[ec0 + 1] - o0);
    uint32_t* dst = FILL ? p.out + p.table_ids + p.aoff[i] : nullptr;
    uint32_t cnt = 0;
    for (uint32_t base = 0; base < l0; base += 64) {
        const uint32_t j = base + lane;
        uint32_t x = 0;
        bool keep = false;
        if (j < l0) {
            x = p.sets[o0 + j];
            keep = gn_in_all(p, a, b, x);
        }
        const ull mask = __ballot(keep);
        if (FILL && keep) dst[cnt + __popcll(mask & ((1ull << lane) - 1))] = x;
        cnt += __popcll(mask);
    }
    if (!FILL && lane == 0) p.need[i] = cnt;
}

__global__ __launch_bounds__(B) void gn_long_flags(const MolArgs p, uint32_t* __restrict__ flags) {
    const uint32_t i = blockIdx.x * B + threadIdx.x;
    if (i < p.n_mol) flags[i] = mol_end(p, i) - p.mol_start[i] > GN_LANE_RECORDS ? 1u : 0u;
}

// the molecules of two records or more: where their list lies, its length and hash; then kept = a set that is not empty
__global__ __launch_bounds__(B) void gn_mol_finish(const MolArgs p, uint32_t* __restrict__ kept) {
    const uint32_t i = blockIdx.x * B + threadIdx.x;
    if (i >= p.n_mol) return;
    if (mol_end(p, i) - p.mol_start[i] > 1) {
        const ull off = p.table_ids + p.aoff[i];
        const uint32_t len = p.need[i];
        p.mol_off[i] = off;
        p.mol_len[i] = len;
        p.mol_hash[i] = pa::list_hash_dev(p.out + off, len);
    }
    kept[i] = p.mol_len[i] ? 1u : 0u;
}

template <class T>
int alloc_n(pa::DeviceBuffer<T>& b, size_t n) { return b.alloc(n ? n : 1); }

// what the stage leaves: molecule i = records [mol_start[i], mol_start[i + 1]) (the last one ends at n), its gene set = ids[mol_off[i] ..
// mol_off[i] + mol_len[i]), ascending, and the set's content hash. ids begins with the table's G(e) lists
struct MolTable {
    uint32_t n_mol = 0;
    pa::DeviceBuffer<uint32_t> mol_start, mol_len, ids;
    pa::DeviceBuffer<ull> mol_off, mol_hash;
};

// d_rec[n] (n >= 1, strictly ascending) -> t. heads[n] takes the run heads over (barcode, UMI); flags[n] is scratch and holds kept[n_mol] (1 for a
// set that is not empty) afterwards. The two may be one array: the heads are used up before the flags are written. d_n: one word of scratch
inline int molecule_table(hipStream_t s, pa::DeviceBuffer<uint8_t>& tmp, uint32_t* d_n, const pa_bus_record* d_rec, uint32_t n, const pa::genes::GeneSets& gs, uint32_t* heads,
                          uint32_t* flags, MolTable& t) {
    using namespace pa;
    int e;
    // 1. molecules
    if ((e = t.mol_start.alloc(n))) return e;
    GN_LAUNCH(gn_mol_heads, n, s, d_rec, n, heads);
    if ((e = select_flagged_indices(s, tmp, (const uint32_t*)heads, (size_t)n, t.mol_start.get(), d_n)) || (e = fetch_u32(d_n, s, t.n_mol))) return e;
    const uint32_t n_mol = t.n_mol;
    // 2. their gene sets: counted, scanned, written behind the table
    DeviceBuffer<uint64_t> gs_off, gs_hash;
    DeviceBuffer<ull> aoff;
    DeviceBuffer<uint32_t> gs_ids, need, long_idx;
    if ((e = upload(gs_off, gs.off)) || (e = upload(gs_hash, gs.hash)) || (e = upload(gs_ids, gs.ids)) || (e = need.alloc(n_mol)) || (e = aoff.alloc(n_mol)) ||
        (e = t.mol_off.alloc(n_mol)) || (e = t.mol_len.alloc(n_mol)) || (e = t.mol_hash.alloc(n_mol)) || (e = long_idx.alloc(n_mol)))
        return e;
    MolArgs m{};
    m.rec = d_rec; m.n = n; m.n_mol = n_mol; m.mol_start = t.mol_start.get(); m.gs_off = (const ull*)gs_off.get(); m.gs_hash = (const ull*)gs_hash.get(); m.sets = gs_ids.get();
    m.table_ids = gs.ids.size(); m.need = need.get(); m.aoff = aoff.get(); m.out = nullptr; m.mol_off = t.mol_off.get(); m.mol_len = t.mol_len.get();
    m.mol_hash = t.mol_hash.get(); m.long_idx = long_idx.get(); m.n_long = 0;
    GN_LAUNCH(gn_long_flags, n_mol, s, m, flags);
    if ((e = select_flagged_indices(s, tmp, (const uint32_t*)flags, (size_t)n_mol, long_idx.get(), d_n)) || (e = fetch_u32(d_n, s, m.n_long))) return e;
    GN_LAUNCH(gn_intersect_lane<false>, n_mol, s, m);
    if (m.n_long) GN_LAUNCH(gn_intersect_wave<false>, (uint64_t)m.n_long * 64, s, m);
    if ((e = scan_exclusive(s, tmp, (const uint32_t*)need.get(), aoff.get(), (size_t)n_mol))) return e;
    ull last_off = 0;
    uint32_t last_need = 0;
    PA_HIP_TRY(hipMemcpyAsync(&last_off, aoff.get() + (n_mol - 1), 8, hipMemcpyDeviceToHost, s));
    if ((e = fetch_u32(need.get() + (n_mol - 1), s, last_need))) return e;
    const ull own_ids = last_off + last_need;
    if ((e = alloc_n(t.ids, (size_t)(m.table_ids + own_ids)))) return e;
    if (m.table_ids) PA_HIP_TRY(hipMemcpyAsync(t.ids.get(), gs_ids.get(), m.table_ids * 4, hipMemcpyDeviceToDevice, s));
    m.sets = t.ids.get();
    m.out = t.ids.get();
    GN_LAUNCH(gn_intersect_lane<true>, n_mol, s, m);
    if (m.n_long) GN_LAUNCH(gn_intersect_wave<true>, (uint64_t)m.n_long * 64, s, m);
    GN_LAUNCH(gn_mol_finish, n_mol, s, m, flags);
    PA_HIP_TRY(hipStreamSynchronize(s));   // (the table's upload and the stage's scratch leave scope)
    return PA_OK;
}

}  // namespace
