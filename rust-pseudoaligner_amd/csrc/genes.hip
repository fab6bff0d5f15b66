// Cells x genes from BUS records (pa_genes, include/pseudoaligner_amd.h).
//
// Molecule stage (molecule_stage.hpp, shared with bus_umi.hip): run heads over (barcode, UMI); every molecule's gene set = the
// intersection of its records' G(e) (one record: G(e) itself by reference into the table; up to GN_LANE_RECORDS records: a lane; more: a
// wave), counted, scanned and written behind the table in one id buffer. Kept molecules get their cell number; the single-gene ones become (cell, gene) keys, sorted and run-length
// encoded into u_g; the multi-gene ones become (cell, content hash) keys, sorted, collapsed into rows (every member compared with the
// row's first) and laid out per cell: rows -> slots (the (cell, gene) pairs of E, ascending) and the transposed incidence.
// EM: all iterations of a cell inside one launch. alpha[|E|] and q[rows] of the cell live in LDS (a wave per cell for small cells, a
// block per cell above, HBM scratch beyond the LDS cap); E pass a lane per row, M pass a lane per gene, every sum in the layout's
// order. No floating-point atomics, no block waits on another.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <memory>
#include <new>
#include <vector>

#include "bus_host.hpp"
#include "device_prims.hpp"
#include "genes_host.hpp"
#include "genes_state.hpp"
#include "hip_buffer.hpp"
#include "kernel_utils.hpp"
#include "molecule_stage.hpp"
#include "pa_common.hpp"

using namespace pa;

namespace {

enum : uint32_t { GS_MATCHED = PA_GENES_STATS, GS_ERR, GS_WORDS };   // extra device counters behind the stats

// kept molecule j (= molecule kept_idx[j]): the head of a cell when its barcode differs from the kept molecule before it
__global__ __launch_bounds__(B) void gn_cell_heads(const pa_bus_record* __restrict__ rec, const uint32_t* __restrict__ mol_start, const uint32_t* __restrict__ kept_idx,
                                                   uint32_t n_kept, uint32_t* __restrict__ heads) {
    const uint32_t j = blockIdx.x * B + threadIdx.x;
    if (j >= n_kept) return;
    heads[j] = (j == 0 || rec[mol_start[kept_idx[j]]].barcode != rec[mol_start[kept_idx[j - 1]]].barcode) ? 1u : 0u;
}
// cell of kept molecule j = cpos[j] - 1; barcodes of the cells; flags of the single-gene and of the multi-gene molecules
__global__ __launch_bounds__(B) void gn_cells(const pa_bus_record* __restrict__ rec, const uint32_t* __restrict__ mol_start, const uint32_t* __restrict__ kept_idx,
                                              const uint32_t* __restrict__ heads, const uint32_t* __restrict__ cpos, const uint32_t* __restrict__ mol_len, uint32_t n_kept,
                                              ull* __restrict__ barcode, uint32_t* __restrict__ single, uint32_t* __restrict__ multi) {
    const uint32_t j = blockIdx.x * B + threadIdx.x;
    if (j >= n_kept) return;
    const uint32_t i = kept_idx[j];
    if (heads[j]) barcode[cpos[j] - 1] = rec[mol_start[i]].barcode;
    single[j] = mol_len[i] == 1 ? 1u : 0u;
    multi[j] = mol_len[i] > 1 ? 1u : 0u;
}
__global__ __launch_bounds__(B) void gn_single_keys(const uint32_t* __restrict__ sel, uint32_t n_sel, const uint32_t* __restrict__ kept_idx, const uint32_t* __restrict__ cpos,
                                                    const ull* __restrict__ mol_off, const uint32_t* __restrict__ ids, ull* __restrict__ keys) {
    const uint32_t s = blockIdx.x * B + threadIdx.x;
    if (s >= n_sel) return;
    const uint32_t j = sel[s];
    keys[s] = ((ull)(cpos[j] - 1) << 32) | ids[mol_off[kept_idx[j]]];
}
__global__ __launch_bounds__(B) void gn_multi_keys(const uint32_t* __restrict__ sel, uint32_t n_sel, const uint32_t* __restrict__ kept_idx, const uint32_t* __restrict__ cpos,
                                                   const ull* __restrict__ mol_hash, u128* __restrict__ keys, uint32_t* __restrict__ vals) {
    const uint32_t s = blockIdx.x * B + threadIdx.x;
    if (s >= n_sel) return;
    const uint32_t j = sel[s], i = kept_idx[j];
    keys[s] = ((u128)(cpos[j] - 1) << 64) | mol_hash[i];
    vals[s] = i;
}
__global__ __launch_bounds__(B) void gn_counts_f64(const uint32_t* __restrict__ cnt, uint32_t n, double* __restrict__ out, uint32_t* __restrict__ zero) {
    const uint32_t i = blockIdx.x * B + threadIdx.x;
    if (i < n) { out[i] = (double)cnt[i]; zero[i] = 0u; }
}

// ---- rows ----
// every multi-gene molecule against the first of its row (equal hash means the same set only after the contents were compared)
__global__ __launch_bounds__(B) void gn_verify_rows(const u128* __restrict__ keys, const uint32_t* __restrict__ vals, const uint32_t* __restrict__ pos,
                                                    const uint32_t* __restrict__ start, uint32_t n, const ull* __restrict__ mol_off, const uint32_t* __restrict__ mol_len,
                                                    const uint32_t* __restrict__ ids, ull* __restrict__ err) {
    const uint32_t s = blockIdx.x * B + threadIdx.x;
    if (s >= n) return;
    const uint32_t first = start[pos[s] - 1];
    if (first == s) return;
    const uint32_t i = vals[s], f = vals[first];
    bool same = mol_len[i] == mol_len[f];
    if (same && mol_off[i] != mol_off[f])
        for (uint32_t j = 0; j < mol_len[i]; ++j)
            if (ids[mol_off[i] + j] != ids[mol_off[f] + j]) { same = false; break; }
    if (!same) *err = (ull)keys[s] | 1ull;
}
// row r: its cell (as cell << 32), where its ids lie, its length (len[rows] = 0 for the scan), n_S; the longest row
__global__ __launch_bounds__(B) void gn_rows(const u128* __restrict__ unique, const uint32_t* __restrict__ start, const uint32_t* __restrict__ vals, uint32_t rows,
                                             const ull* __restrict__ mol_off, const uint32_t* __restrict__ mol_len, ull* __restrict__ row_key, ull* __restrict__ row_src,
                                             uint32_t* __restrict__ row_len, uint32_t* __restrict__ row_n, ull* __restrict__ stats) {
    const uint32_t r = blockIdx.x * B + threadIdx.x;
    if (r > rows) return;
    if (r == rows) { row_len[r] = 0; return; }
    const uint32_t i = vals[start[r]];
    row_key[r] = (ull)(unique[r] >> 64) << 32;
    row_src[r] = mol_off[i];
    row_len[r] = mol_len[i];
    row_n[r] = start[r + 1] - start[r];
    atomicMax(stats + 9, (ull)mol_len[i]);
}
// sorted keys: out[c] = number of keys whose high part (key >> shift) is below c, c = 0 .. n_cells
template <class K>
__global__ __launch_bounds__(B) void gn_cell_bounds(const K* __restrict__ keys, uint32_t n, uint32_t n_cells, uint32_t* __restrict__ out) {
    const uint32_t c = blockIdx.x * B + threadIdx.x;
    if (c > n_cells) return;
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if ((uint32_t)(keys[mid] >> 32) < c) lo = mid + 1; else hi = mid;
    }
    out[c] = lo;
}
__device__ __forceinline__ uint32_t row_of(const ull* __restrict__ row_ptr, uint32_t rows, ull p) {   // row_ptr[r] <= p < row_ptr[r + 1]
    uint32_t lo = 0, hi = rows;
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (row_ptr[mid] <= p) lo = mid; else hi = mid;
    }
    return lo;
}
// entry p of the incidence -> (cell << 32 | gene, p)
__global__ __launch_bounds__(B) void gn_expand(const ull* __restrict__ row_ptr, uint32_t rows, uint32_t nnz, const ull* __restrict__ row_key, const ull* __restrict__ row_src,
                                               const uint32_t* __restrict__ ids, ull* __restrict__ keys, uint32_t* __restrict__ vals) {
    const uint32_t p = blockIdx.x * B + threadIdx.x;
    if (p >= nnz) return;
    const uint32_t r = row_of(row_ptr, rows, p);
    keys[p] = row_key[r] | ids[row_src[r] + (p - row_ptr[r])];
    vals[p] = p;
}
// entries sorted by (cell, gene), stable: entry j is entry p = vals[j] of the row CSR and lies in slot pos[j] - 1
__global__ __launch_bounds__(B) void gn_transpose(const uint32_t* __restrict__ vals, const uint32_t* __restrict__ pos, uint32_t nnz, const ull* __restrict__ row_ptr, uint32_t rows,
                                                  uint32_t* __restrict__ row_slot, uint32_t* __restrict__ t_row) {
    const uint32_t j = blockIdx.x * B + threadIdx.x;
    if (j >= nnz) return;
    const uint32_t p = vals[j];
    row_slot[p] = pos[j] - 1;
    t_row[j] = row_of(row_ptr, rows, p);
}
// u of every slot from the singleton rows (0 when the gene has none); the largest degree
__global__ __launch_bounds__(B) void gn_slot_u(const ull* __restrict__ slot_key, const uint32_t* __restrict__ slot_start, uint32_t slots, const ull* __restrict__ su_key,
                                               const double* __restrict__ su_val, uint32_t n_su, uint32_t* __restrict__ su_in_e, double* __restrict__ u, ull* __restrict__ stats) {
    const uint32_t s = blockIdx.x * B + threadIdx.x;
    if (s >= slots) return;
    const ull k = slot_key[s];
    uint32_t lo = 0, hi = n_su;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (su_key[mid] < k) lo = mid + 1; else hi = mid;
    }
    double v = 0.0;
    if (lo < n_su && su_key[lo] == k) {
        v = su_val[lo];
        su_in_e[lo] = 1u;
        atomicAdd(stats + GS_MATCHED, 1ull);
    }
    u[s] = v;
    atomicMax(stats + 10, (ull)(slot_start[s + 1] - slot_start[s]));
}
// per cell: |E| + rows (0 for a cell without multi rows), M; flag of the cells with multi rows
__global__ __launch_bounds__(B) void gn_cell_sizes(const uint32_t* __restrict__ cell_row, const uint32_t* __restrict__ cell_slot, const uint32_t* __restrict__ row_n,
                                                   uint32_t n_cells, uint32_t* __restrict__ size, uint32_t* __restrict__ cell_id, double* __restrict__ cell_m,
                                                   uint32_t* __restrict__ flags) {
    const uint32_t c = blockIdx.x * B + threadIdx.x;
    if (c >= n_cells) return;
    const uint32_t r0 = cell_row[c], r1 = cell_row[c + 1];
    ull m = 0;
    for (uint32_t r = r0; r < r1; ++r) m += row_n[r];
    size[c] = r1 > r0 ? (r1 - r0) + (cell_slot[c + 1] - cell_slot[c]) : 0u;
    cell_id[c] = c;
    cell_m[c] = (double)m;
    flags[c] = r1 > r0 ? 1u : 0u;
}
__global__ __launch_bounds__(B) void gn_start(const ull* __restrict__ slot_key, const uint32_t* __restrict__ cell_slot, const double* __restrict__ cell_m,
                                              const double* __restrict__ u, uint32_t slots, int em, double* __restrict__ alpha) {
    const uint32_t s = blockIdx.x * B + threadIdx.x;
    if (s >= slots) return;
    const uint32_t c = (uint32_t)(slot_key[s] >> 32);
    alpha[s] = em ? u[s] + cell_m[c] / (double)(cell_slot[c + 1] - cell_slot[c]) : u[s];
}
// sizes sorted in descending order: out[0] = cells above GN_LDS_CAP, out[1] = cells above GN_WAVE_MAX
__global__ void gn_bin_bounds(const uint32_t* __restrict__ sizes, uint32_t n, uint32_t* __restrict__ out) {
    const uint32_t k = threadIdx.x;
    if (k >= 2) return;
    const uint32_t above = k == 0 ? GN_LDS_CAP : GN_WAVE_MAX;
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (sizes[mid] > above) lo = mid + 1; else hi = mid;
    }
    out[k] = lo;
}

// ---- EM ----
struct EmArgs {
    const uint32_t* order;       // the cells of this launch: order[first .. first + count)
    uint32_t first, count;
    const uint32_t* cell_slot;
    const uint32_t* cell_row;
    const ull* row_ptr;
    const uint32_t* row_slot;
    const uint32_t* row_n;
    const uint32_t* slot_start;
    const uint32_t* t_row;
    const double* u;
    double* alpha;
    double* scratch;             // HBM variant: alpha and q of cell order[first + j] at scratch + scratch_off[j]
    const ull* scratch_off;
    uint32_t* iters;
    uint32_t* notconv;
    uint32_t n_iters;            // stop == 0: exactly this many
    int stop;
    uint32_t min_iters, max_iters, check_every;
    double change_limit, change;
};

// what the G lanes of a cell wrote to a / q is seen by all of them afterwards
template <int G>
__device__ __forceinline__ void group_sync() {
    if (G == 64) {   // one wave: its LDS accesses are served in order; the compiler must not move them across this point
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    } else __syncthreads();
}
template <int G>
__device__ __forceinline__ bool group_any(int x) {
    if (G == 64) {
        group_sync<64>();
        return __ballot(x != 0) != 0;
    }
    return __syncthreads_or(x) != 0;
}

// all iterations of cell c by G lanes; a[|E|] and q[rows] are the cell's working arrays
template <int G>
__device__ __forceinline__ void em_cell(const EmArgs& p, uint32_t c, uint32_t lane, double* a, double* q) {
    const uint32_t s0 = p.cell_slot[c], nE = p.cell_slot[c + 1] - s0, r0 = p.cell_row[c], nR = p.cell_row[c + 1] - r0;
    for (uint32_t g = lane; g < nE; g += G) a[g] = p.alpha[s0 + g];
    group_sync<G>();
    const uint32_t limit = p.stop ? p.max_iters : p.n_iters;
    uint32_t done = 0;
    bool conv = false;
    while (done < limit && !conv) {
        const uint32_t i = done + 1;
        const bool check = p.stop && ((i >= p.min_iters && i % p.check_every == 0) || i == p.max_iters);
        for (uint32_t r = lane; r < nR; r += G) {   // E pass: a row's genes in the row's order
            const ull e = p.row_ptr[r0 + r + 1];
            double d = 0.0;
            for (ull j = p.row_ptr[r0 + r]; j < e; ++j) d += a[p.row_slot[j] - s0];
            q[r] = d > 0.0 ? (double)p.row_n[r0 + r] / d : 0.0;
        }
        group_sync<G>();
        int changed = 0;
        for (uint32_t g = lane; g < nE; g += G) {   // M pass: a gene's rows ascending
            const uint32_t e = p.slot_start[s0 + g + 1];
            double s = 0.0;
            for (uint32_t j = p.slot_start[s0 + g]; j < e; ++j) s += q[p.t_row[j] - r0];
            const double old = a[g], next = p.u[s0 + g] + old * s;
            a[g] = next;
            if (check) changed |= (next > p.change_limit && fabs(next - old) / next > p.change) ? 1 : 0;
        }
        done = i;
        if (check) conv = !group_any<G>(changed) && i >= p.min_iters;
        else group_sync<G>();
    }
    for (uint32_t g = lane; g < nE; g += G) p.alpha[s0 + g] = a[g];
    if (lane == 0) {
        p.iters[c] += done;
        if (p.stop) p.notconv[c] = conv ? 0u : 1u;
    }
}

// a block per cell; HBM: the working arrays in the scratch, else in LDS
template <bool HBM>
__global__ __launch_bounds__(B) void gn_em_block(const EmArgs p) {
    __shared__ double lds[HBM ? 1 : GN_LDS_CAP];
    const uint32_t c = p.order[p.first + blockIdx.x];
    const uint32_t nE = p.cell_slot[c + 1] - p.cell_slot[c];
    double* a = HBM ? p.scratch + p.scratch_off[blockIdx.x] : lds;
    em_cell<256>(p, c, threadIdx.x, a, a + nE);
}
// a wave per cell, GN_WAVE_CELLS cells per block, no block barrier
__global__ __launch_bounds__(B) void gn_em_wave(const EmArgs p) {
    __shared__ double lds[GN_WAVE_CELLS][GN_WAVE_MAX];
    const uint32_t w = threadIdx.x / 64, j = blockIdx.x * GN_WAVE_CELLS + w;
    if (j >= p.count) return;
    const uint32_t c = p.order[p.first + j];
    const uint32_t nE = p.cell_slot[c + 1] - p.cell_slot[c];
    em_cell<64>(p, c, threadIdx.x & 63, lds[w], lds[w] + nE);
}

// ---- after the run ----
__global__ __launch_bounds__(B) void gn_truncate(double* __restrict__ v, uint32_t n, double below, const uint32_t* __restrict__ skip, ull* __restrict__ entries) {
    const uint32_t i = blockIdx.x * B + threadIdx.x;
    bool entry = false;
    if (i < n) {
        if (v[i] < below) v[i] = 0.0;
        entry = v[i] != 0.0 && !(skip && skip[i]);
    }
    const ull m = __ballot(entry);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(entries, (ull)__popcll(m));
}
__global__ __launch_bounds__(B) void gn_run_stats(const uint32_t* __restrict__ iters, const uint32_t* __restrict__ notconv, uint32_t n_cells, ull* __restrict__ stats) {
    const uint32_t c = blockIdx.x * B + threadIdx.x;
    if (c >= n_cells) return;
    if (iters[c]) atomicMax(stats + 12, (ull)iters[c]);
    if (notconv[c]) atomicAdd(stats + 13, 1ull);
}

// everything up to the start point; d_rec: the n records in HBM (read during this call only)
int setup(pa_genes* g, const pa_bus_record* d_rec, uint32_t n, const genes::GeneSets& gs) {
    hipStream_t s = g->stream;
    DeviceBuffer<uint8_t> tmp;
    DeviceBuffer<uint32_t> d_n;
    int e;
    if ((e = g->d_stats.alloc(GS_WORDS)) || (e = d_n.alloc(4))) return e;
    PA_HIP_TRY(hipMemsetAsync(g->d_stats.get(), 0, GS_WORDS * 8, s));
    g->stats[0] = n;
    if (n == 0) return PA_OK;
    // 1. + 2. molecules and their gene sets (molecule_stage.hpp)
    DeviceBuffer<uint32_t> flags;
    MolTable mt;
    if ((e = flags.alloc(n)) || (e = molecule_table(s, tmp, d_n.get(), d_rec, n, gs, flags.get(), flags.get(), mt))) return e;
    const uint32_t n_mol = mt.n_mol;
    DeviceBuffer<uint32_t>&mol_start = mt.mol_start, &mol_len = mt.mol_len, &ids = mt.ids;
    DeviceBuffer<ull>&mol_off = mt.mol_off, &mol_hash = mt.mol_hash;
    g->stats[1] = n_mol;
    // 3. kept molecules, their cells
    DeviceBuffer<uint32_t> kept_idx;
    uint32_t n_kept = 0;
    if ((e = kept_idx.alloc(n_mol))) return e;
    if ((e = select_flagged_indices(s, tmp, (const uint32_t*)flags.get(), (size_t)n_mol, kept_idx.get(), d_n.get())) || (e = fetch_u32(d_n.get(), s, n_kept))) return e;
    g->stats[2] = n_mol - n_kept;
    if (n_kept == 0) return PA_OK;
    DeviceBuffer<uint32_t> cheads, cpos, single, multi, sel;
    if ((e = cheads.alloc(n_kept)) || (e = cpos.alloc(n_kept)) || (e = single.alloc(n_kept)) || (e = multi.alloc(n_kept)) || (e = sel.alloc(n_kept))) return e;
    GN_LAUNCH(gn_cell_heads, n_kept, s, d_rec, (const uint32_t*)mol_start.get(), (const uint32_t*)kept_idx.get(), n_kept, cheads.get());
    if ((e = scan_inclusive_total(s, tmp, (const uint32_t*)cheads.get(), cpos.get(), (size_t)n_kept, g->n_cells))) return e;
    const uint32_t n_cells = g->n_cells;
    g->stats[5] = n_cells;
    const uint32_t cell_bits = std::max(1u, bits_for(n_cells - 1));
    if ((e = g->d_barcode.alloc(n_cells)) || (e = g->d_iters.alloc(n_cells)) || (e = g->d_notconv.alloc(n_cells))) return e;
    PA_HIP_TRY(hipMemsetAsync(g->d_iters.get(), 0, n_cells * 4ull, s));
    PA_HIP_TRY(hipMemsetAsync(g->d_notconv.get(), 0, n_cells * 4ull, s));
    GN_LAUNCH(gn_cells, n_kept, s, d_rec, (const uint32_t*)mol_start.get(), (const uint32_t*)kept_idx.get(), (const uint32_t*)cheads.get(), (const uint32_t*)cpos.get(),
              (const uint32_t*)mol_len.get(), n_kept, g->d_barcode.get(), single.get(), multi.get());
    // 4. single-gene molecules -> u
    uint32_t n_single = 0, n_multi = 0;
    if ((e = select_flagged_indices(s, tmp, (const uint32_t*)single.get(), (size_t)n_kept, sel.get(), d_n.get())) || (e = fetch_u32(d_n.get(), s, n_single))) return e;
    g->stats[3] = n_single;
    g->stats[4] = n_kept - n_single;
    if (n_single) {
        DeviceBuffer<ull> k0, k1;
        DeviceBuffer<uint32_t> cnt;
        if ((e = k0.alloc(n_single)) || (e = k1.alloc(n_single)) || (e = cnt.alloc(n_single)) || (e = g->d_su_key.alloc(n_single))) return e;
        GN_LAUNCH(gn_single_keys, n_single, s, (const uint32_t*)sel.get(), n_single, (const uint32_t*)kept_idx.get(), (const uint32_t*)cpos.get(), (const ull*)mol_off.get(),
                  (const uint32_t*)ids.get(), k0.get());
        if ((e = sort_keys(s, tmp, (const ull*)k0.get(), k1.get(), (size_t)n_single, 0, 32 + cell_bits))) return e;
        if ((e = run_length_encode(s, tmp, (const ull*)k1.get(), (size_t)n_single, g->d_su_key.get(), cnt.get(), d_n.get())) || (e = fetch_u32(d_n.get(), s, g->n_su))) return e;
        if ((e = g->d_su_val.alloc(g->n_su)) || (e = g->d_su_in_e.alloc(g->n_su))) return e;
        GN_LAUNCH(gn_counts_f64, g->n_su, s, (const uint32_t*)cnt.get(), g->n_su, g->d_su_val.get(), g->d_su_in_e.get());
        PA_HIP_TRY(hipStreamSynchronize(s));   // (k0, k1 and cnt leave scope)
    }
    g->n_values = g->n_su;
    // 5. multi-gene molecules -> rows -> the per-cell layout
    if ((e = select_flagged_indices(s, tmp, (const uint32_t*)multi.get(), (size_t)n_kept, sel.get(), d_n.get())) || (e = fetch_u32(d_n.get(), s, n_multi))) return e;
    if (n_multi == 0) return PA_OK;
    DeviceBuffer<u128> mk0, mk1, mku;
    DeviceBuffer<uint32_t> mv0, mv1, mheads, mpos, mstart, row_len;
    DeviceBuffer<ull> row_src, row_key;
    if ((e = mk0.alloc(n_multi)) || (e = mk1.alloc(n_multi)) || (e = mku.alloc(n_multi)) || (e = mv0.alloc(n_multi)) || (e = mv1.alloc(n_multi)) ||
        (e = mheads.alloc(n_multi)) || (e = mpos.alloc(n_multi)) || (e = mstart.alloc((size_t)n_multi + 1)))
        return e;
    GN_LAUNCH(gn_multi_keys, n_multi, s, (const uint32_t*)sel.get(), n_multi, (const uint32_t*)kept_idx.get(), (const uint32_t*)cpos.get(), (const ull*)mol_hash.get(), mk0.get(),
              mv0.get());
    if ((e = sort_pairs(s, tmp, (const u128*)mk0.get(), mk1.get(), (const uint32_t*)mv0.get(), mv1.get(), (size_t)n_multi, 0, 64 + cell_bits))) return e;
    uint32_t rows = 0;
    if ((e = collapse_runs(s, tmp, KeyArray<u128>{mk1.get()}, n_multi, mheads.get(), mpos.get(), mku.get(), mstart.get(), rows))) return e;
    GN_LAUNCH(gn_verify_rows, n_multi, s, (const u128*)mk1.get(), (const uint32_t*)mv1.get(), (const uint32_t*)mpos.get(), (const uint32_t*)mstart.get(), n_multi,
              (const ull*)mol_off.get(), (const uint32_t*)mol_len.get(), (const uint32_t*)ids.get(), g->d_stats.get() + GS_ERR);
    g->n_rows = rows;
    g->stats[7] = rows;
    if ((e = row_key.alloc(rows)) || (e = row_src.alloc(rows)) || (e = row_len.alloc((size_t)rows + 1)) || (e = g->d_row_n.alloc(rows)) ||
        (e = g->d_row_ptr.alloc((size_t)rows + 1)) || (e = g->d_cell_row.alloc((size_t)n_cells + 1)) || (e = g->d_cell_slot.alloc((size_t)n_cells + 1)))
        return e;
    GN_LAUNCH(gn_rows, (uint64_t)rows + 1, s, (const u128*)mku.get(), (const uint32_t*)mstart.get(), (const uint32_t*)mv1.get(), rows, (const ull*)mol_off.get(),
              (const uint32_t*)mol_len.get(), row_key.get(), row_src.get(), row_len.get(), g->d_row_n.get(), g->d_stats.get());
    if ((e = scan_exclusive(s, tmp, (const uint32_t*)row_len.get(), g->d_row_ptr.get(), (size_t)rows + 1))) return e;
    ull nnz = 0, err = 0;
    PA_HIP_TRY(hipMemcpyAsync(&nnz, g->d_row_ptr.get() + rows, 8, hipMemcpyDeviceToHost, s));
    PA_HIP_TRY(hipMemcpyAsync(&err, g->d_stats.get() + GS_ERR, 8, hipMemcpyDeviceToHost, s));
    PA_HIP_TRY(hipStreamSynchronize(s));
    if (err) return fail(PA_ERR_INTERNAL, "two different gene sets of one cell share the content hash %016llx", err & ~1ull);
    if (nnz > 0x7FFFFFFFull) return fail(PA_ERR_UNSUPPORTED, "multi rows of more than 2^31-1 ids");
    g->nnz = nnz;
    g->stats[8] = nnz;
    GN_LAUNCH(gn_cell_bounds<ull>, (uint64_t)n_cells + 1, s, (const ull*)row_key.get(), rows, n_cells, g->d_cell_row.get());
    // entries -> (cell, gene) keys, sorted (stable: a gene's rows stay ascending) -> slots and the transposed incidence
    const uint32_t n_e = (uint32_t)nnz;
    DeviceBuffer<ull> ek0, ek1;
    DeviceBuffer<uint32_t> ev0, ev1, eheads, epos;
    if ((e = ek0.alloc(n_e)) || (e = ek1.alloc(n_e)) || (e = ev0.alloc(n_e)) || (e = ev1.alloc(n_e)) || (e = eheads.alloc(n_e)) || (e = epos.alloc(n_e)) ||
        (e = g->d_slot_key.alloc(n_e)) || (e = g->d_slot_start.alloc((size_t)n_e + 1)) || (e = g->d_row_slot.alloc(n_e)) || (e = g->d_t_row.alloc(n_e)))
        return e;
    GN_LAUNCH(gn_expand, n_e, s, (const ull*)g->d_row_ptr.get(), rows, n_e, (const ull*)row_key.get(), (const ull*)row_src.get(), (const uint32_t*)ids.get(), ek0.get(), ev0.get());
    if ((e = sort_pairs(s, tmp, (const ull*)ek0.get(), ek1.get(), (const uint32_t*)ev0.get(), ev1.get(), (size_t)n_e, 0, 32 + cell_bits))) return e;
    uint32_t slots = 0;
    if ((e = collapse_runs(s, tmp, KeyArray<ull>{ek1.get()}, n_e, eheads.get(), epos.get(), g->d_slot_key.get(), g->d_slot_start.get(), slots))) return e;
    g->n_slots = slots;
    GN_LAUNCH(gn_transpose, n_e, s, (const uint32_t*)ev1.get(), (const uint32_t*)epos.get(), n_e, (const ull*)g->d_row_ptr.get(), rows, g->d_row_slot.get(), g->d_t_row.get());
    GN_LAUNCH(gn_cell_bounds<ull>, (uint64_t)n_cells + 1, s, (const ull*)g->d_slot_key.get(), slots, n_cells, g->d_cell_slot.get());
    if ((e = g->d_u.alloc(slots)) || (e = g->d_alpha.alloc(slots))) return e;
    GN_LAUNCH(gn_slot_u, slots, s, (const ull*)g->d_slot_key.get(), (const uint32_t*)g->d_slot_start.get(), slots, (const ull*)g->d_su_key.get(),
              (const double*)g->d_su_val.get(), g->n_su, g->d_su_in_e.get(), g->d_u.get(), g->d_stats.get());
    // the cells with multi rows, largest first, and the three bins
    DeviceBuffer<uint32_t> size, cell_id, size_s, mc_idx, mc_size, bounds;
    DeviceBuffer<double> cell_m;
    if ((e = size.alloc(n_cells)) || (e = cell_id.alloc(n_cells)) || (e = size_s.alloc(n_cells)) || (e = g->d_order.alloc(n_cells)) || (e = cell_m.alloc(n_cells)) ||
        (e = bounds.alloc(2)) || (e = flags.reserve(n_cells, n_cells)))
        return e;
    GN_LAUNCH(gn_cell_sizes, n_cells, s, (const uint32_t*)g->d_cell_row.get(), (const uint32_t*)g->d_cell_slot.get(), (const uint32_t*)g->d_row_n.get(), n_cells, size.get(),
              cell_id.get(), cell_m.get(), flags.get());
    GN_LAUNCH(gn_start, slots, s, (const ull*)g->d_slot_key.get(), (const uint32_t*)g->d_cell_slot.get(), (const double*)cell_m.get(), (const double*)g->d_u.get(), slots,
              g->par.mode == PA_GENES_EM ? 1 : 0, g->d_alpha.get());
    // (a stable descending sort: cells of equal size keep barcode order; the cells without multi rows, size 0, come last)
    if ((e = sort_pairs_desc(s, tmp, (const uint32_t*)size.get(), size_s.get(), (const uint32_t*)cell_id.get(), g->d_order.get(), (size_t)n_cells, 0, 32))) return e;
    if ((e = select_flagged_indices(s, tmp, (const uint32_t*)flags.get(), (size_t)n_cells, cell_id.get(), d_n.get())) || (e = fetch_u32(d_n.get(), s, g->n_multi_cells))) return e;
    hipLaunchKernelGGL(gn_bin_bounds, dim3(1), dim3(64), 0, s, (const uint32_t*)size_s.get(), g->n_multi_cells, bounds.get());
    PA_HIP_TRY(hipGetLastError());
    uint32_t hb[2] = {0, 0}, largest = 0;
    PA_HIP_TRY(hipMemcpyAsync(hb, bounds.get(), 8, hipMemcpyDeviceToHost, s));
    if ((e = fetch_u32(size_s.get(), s, largest))) return e;
    g->n_hbm = hb[0];
    g->n_block = hb[1] - hb[0];
    g->stats[6] = g->n_multi_cells;
    g->stats[11] = largest;
    if (g->n_hbm) {   // the HBM variant's working arrays, one stretch per cell
        ull last = 0;
        uint32_t last_size = 0;
        if ((e = g->d_scratch_off.alloc(g->n_hbm)) || (e = scan_exclusive(s, tmp, (const uint32_t*)size_s.get(), g->d_scratch_off.get(), (size_t)g->n_hbm))) return e;
        PA_HIP_TRY(hipMemcpyAsync(&last, g->d_scratch_off.get() + (g->n_hbm - 1), 8, hipMemcpyDeviceToHost, s));
        if ((e = fetch_u32(size_s.get() + (g->n_hbm - 1), s, last_size)) || (e = g->d_scratch.alloc((size_t)(last + last_size)))) return e;
    }
    ull d[GS_WORDS];
    PA_HIP_TRY(hipMemcpyAsync(d, g->d_stats.get(), sizeof d, hipMemcpyDeviceToHost, s));
    PA_HIP_TRY(hipStreamSynchronize(s));
    g->stats[9] = d[9];
    g->stats[10] = d[10];
    g->n_values = (uint64_t)g->n_su + slots - d[GS_MATCHED];
    return PA_OK;
}

}  // namespace

namespace {

int launch_em(pa_genes* g, uint32_t n_iters, bool stop) {
    if (g->n_multi_cells == 0 || g->par.mode != PA_GENES_EM) return PA_OK;
    EmArgs p{};
    p.order = g->d_order.get(); p.cell_slot = g->d_cell_slot.get(); p.cell_row = g->d_cell_row.get(); p.row_ptr = g->d_row_ptr.get(); p.row_slot = g->d_row_slot.get();
    p.row_n = g->d_row_n.get(); p.slot_start = g->d_slot_start.get(); p.t_row = g->d_t_row.get(); p.u = g->d_u.get(); p.alpha = g->d_alpha.get();
    p.scratch = g->d_scratch.get(); p.scratch_off = g->d_scratch_off.get(); p.iters = g->d_iters.get(); p.notconv = g->d_notconv.get();
    p.n_iters = n_iters; p.stop = stop ? 1 : 0; p.min_iters = g->par.min_iters; p.max_iters = g->par.max_iters; p.check_every = g->par.check_every;
    p.change_limit = g->par.alpha_change_limit; p.change = g->par.alpha_change;
    // the largest cells first: the HBM variant, the block bin, the wave bin
    const uint32_t n_wave = g->n_multi_cells - g->n_hbm - g->n_block;
    if (g->n_hbm) {
        p.first = 0; p.count = g->n_hbm;
        hipLaunchKernelGGL(gn_em_block<true>, dim3(p.count), dim3(B), 0, g->stream, p);
    }
    if (g->n_block) {
        p.first = g->n_hbm; p.count = g->n_block;
        hipLaunchKernelGGL(gn_em_block<false>, dim3(p.count), dim3(B), 0, g->stream, p);
    }
    if (n_wave) {
        p.first = g->n_hbm + g->n_block; p.count = n_wave;
        hipLaunchKernelGGL(gn_em_wave, dim3((n_wave + GN_WAVE_CELLS - 1) / GN_WAVE_CELLS), dim3(B), 0, g->stream, p);
    }
    PA_HIP_TRY(hipGetLastError());
    return PA_OK;
}

struct Creating {
    std::unique_ptr<pa_genes, void (*)(pa_genes*)> g{nullptr, pa_genes_destroy};
    int open(int device, const pa_genes_params& par, uint32_t bc_len, uint32_t umi_len, uint32_t num_genes) {
        PA_HIP_TRY(hipSetDevice(device));
        g.reset(new (std::nothrow) pa_genes());
        if (!g) return fail(PA_ERR_OOM, "out of host memory");
        g->device = device; g->par = par; g->bc_len = bc_len; g->umi_len = umi_len; g->num_genes = num_genes;
        PA_HIP_TRY(hipStreamCreateWithFlags(&g->stream, hipStreamNonBlocking));
        return PA_OK;
    }
};

int resolve_params(const pa_genes_params* p, pa_genes_params& par) {
    pa_genes_default_params(&par);
    if (p) par = *p;
    return genes::check_params(par);
}

// the (cell, gene, value) triples of every row: the slots of E merged with the singleton rows outside E, in (cell, gene) order
int merged_values(const pa_genes* g, bool drop_zeros, std::vector<uint32_t>& cell, std::vector<uint32_t>& gene, std::vector<double>& value) {
    std::vector<ull> sk(g->n_slots), uk(g->n_su);
    std::vector<double> sv(g->n_slots), uv(g->n_su);
    std::vector<uint32_t> in_e(g->n_su);
    PA_HIP_TRY(hipSetDevice(g->device));
    if (g->n_slots) {
        PA_HIP_TRY(hipMemcpyAsync(sk.data(), g->d_slot_key.get(), g->n_slots * 8ull, hipMemcpyDeviceToHost, g->stream));
        PA_HIP_TRY(hipMemcpyAsync(sv.data(), g->d_alpha.get(), g->n_slots * 8ull, hipMemcpyDeviceToHost, g->stream));
    }
    if (g->n_su) {
        PA_HIP_TRY(hipMemcpyAsync(uk.data(), g->d_su_key.get(), g->n_su * 8ull, hipMemcpyDeviceToHost, g->stream));
        PA_HIP_TRY(hipMemcpyAsync(uv.data(), g->d_su_val.get(), g->n_su * 8ull, hipMemcpyDeviceToHost, g->stream));
        PA_HIP_TRY(hipMemcpyAsync(in_e.data(), g->d_su_in_e.get(), g->n_su * 4ull, hipMemcpyDeviceToHost, g->stream));
    }
    PA_HIP_TRY(hipStreamSynchronize(g->stream));
    cell.clear(); gene.clear(); value.clear();
    size_t a = 0, b = 0;
    auto put = [&](ull k, double v) {
        if (drop_zeros && v == 0.0) return;
        cell.push_back((uint32_t)(k >> 32)); gene.push_back((uint32_t)k); value.push_back(v);
    };
    while (a < sk.size() || b < uk.size()) {
        if (b < uk.size() && in_e[b]) { ++b; continue; }   // (that gene's u is part of its slot)
        if (b >= uk.size() || (a < sk.size() && sk[a] < uk[b])) { put(sk[a], sv[a]); ++a; }
        else { put(uk[b], uv[b]); ++b; }
    }
    return PA_OK;
}

}  // namespace

extern "C" {

void pa_genes_default_params(pa_genes_params* p) {
    if (!p) return;
    pa_quant_params q;
    pa_quant_default_params(&q);
    p->alpha_limit = q.alpha_limit; p->alpha_change_limit = q.alpha_change_limit; p->alpha_change = q.alpha_change;
    p->min_iters = q.min_iters; p->max_iters = q.max_iters; p->check_every = q.check_every;
    p->mode = PA_GENES_EM; p->reserved = 0;
}

int pa_genes_create(pa_index* idx, const pa_bus_record* records, uint64_t n, const uint64_t* ec_offsets, const uint32_t* ec_ids, uint32_t n_ecs, uint32_t num_tx,
                    const uint32_t* tx_gene, uint32_t num_genes, uint32_t bc_len, uint32_t umi_len, const pa_genes_params* p, pa_genes** out) {
    if (out) *out = nullptr;
    if (!out) return fail(PA_ERR_INVALID_ARG, "null argument");
    pa_genes_params par;
    int e;
    if ((e = resolve_params(p, par)) || (e = genes::check_lengths(bc_len, umi_len)) || (e = genes::check_tables(ec_offsets, ec_ids, n_ecs, num_tx, tx_gene, num_genes))) return e;
    if (n > 0x7FFFFFFFull) return fail(PA_ERR_UNSUPPORTED, "more than 2^31-1 records");
    if ((e = genes::check_records(records, n, n_ecs))) return e;
    if ((e = have_device())) return e;
    if (!idx) return fail(PA_ERR_INVALID_ARG, "null argument");
    const uint32_t *h_ec = nullptr, *h_ref = nullptr;
    int device = 0;
    index_host_classes(idx, &h_ec, &h_ref, &device);
    genes::GeneSets gs;
    genes::gene_sets(ec_offsets, ec_ids, n_ecs, tx_gene, gs);
    Creating c;
    if ((e = c.open(device, par, bc_len, umi_len, num_genes))) return e;
    DeviceBuffer<pa_bus_record> d_rec;
    if ((e = upload(d_rec, records, (size_t)n)) || (e = setup(c.g.get(), d_rec.get(), (uint32_t)n, gs))) return e;
    *out = c.g.release();
    return PA_OK;
}

int pa_genes_create_from_bus(const pa_bus* finished, const uint32_t* tx_gene, uint32_t num_genes, const pa_genes_params* p, pa_genes** out) {
    if (out) *out = nullptr;
    if (!finished || !out) return fail(PA_ERR_INVALID_ARG, "null argument");
    pa_genes_params par;
    int e;
    if ((e = resolve_params(p, par))) return e;
    int device = 0;
    const pa_bus_record* d_rec = nullptr;
    uint64_t n = 0;
    const bus::EcTable* table = nullptr;
    uint32_t bc_len = 0, umi_len = 0, num_tx = 0;
    if ((e = bus_finished_view(finished, &device, &d_rec, &n, &table, &bc_len, &umi_len, &num_tx))) return e;
    const uint32_t n_ecs = (uint32_t)table->n_ecs();
    if ((e = genes::check_lengths(bc_len, umi_len)) || (e = genes::check_tables(table->offsets.data(), table->ids.data(), n_ecs, num_tx, tx_gene, num_genes))) return e;
    if (n > 0x7FFFFFFFull) return fail(PA_ERR_UNSUPPORTED, "more than 2^31-1 records");
    genes::GeneSets gs;
    genes::gene_sets(table->offsets.data(), table->ids.data(), n_ecs, tx_gene, gs);
    Creating c;
    if ((e = c.open(device, par, bc_len, umi_len, num_genes)) || (e = setup(c.g.get(), d_rec, (uint32_t)n, gs))) return e;
    *out = c.g.release();
    return PA_OK;
}

int pa_genes_step(pa_genes* g, uint32_t n_iters) {
    if (!g) return fail(PA_ERR_INVALID_ARG, "null argument");
    if (g->ran) return fail(PA_ERR_INVALID_ARG, "the run is over: no steps after pa_genes_run");
    if (n_iters == 0) return PA_OK;
    PA_HIP_TRY(hipSetDevice(g->device));
    const int e = launch_em(g, n_iters, false);
    if (e != PA_OK) return e;
    PA_HIP_TRY(hipStreamSynchronize(g->stream));
    return PA_OK;
}

int pa_genes_run(pa_genes* g, uint32_t* max_iters_run, uint64_t* cells_not_converged) {
    if (max_iters_run) *max_iters_run = 0;
    if (cells_not_converged) *cells_not_converged = 0;
    if (!g) return fail(PA_ERR_INVALID_ARG, "null argument");
    if (!g->ran) {
        PA_HIP_TRY(hipSetDevice(g->device));
        hipStream_t s = g->stream;
        int e = launch_em(g, 0, true);
        if (e != PA_OK) return e;
        ull* entries = g->d_stats.get() + 14;
        if (g->n_slots) GN_LAUNCH(gn_truncate, g->n_slots, s, g->d_alpha.get(), g->n_slots, g->par.alpha_limit, (const uint32_t*)nullptr, entries);
        if (g->n_su) GN_LAUNCH(gn_truncate, g->n_su, s, g->d_su_val.get(), g->n_su, g->par.alpha_limit, (const uint32_t*)g->d_su_in_e.get(), entries);
        if (g->n_cells) GN_LAUNCH(gn_run_stats, g->n_cells, s, (const uint32_t*)g->d_iters.get(), (const uint32_t*)g->d_notconv.get(), g->n_cells, g->d_stats.get());
        ull d[GS_WORDS];
        PA_HIP_TRY(hipMemcpyAsync(d, g->d_stats.get(), sizeof d, hipMemcpyDeviceToHost, s));
        PA_HIP_TRY(hipStreamSynchronize(s));
        g->stats[12] = d[12]; g->stats[13] = d[13]; g->stats[14] = d[14];
        g->stats[15] = g->par.mode == PA_GENES_EM ? g->n_hbm : 0;
        g->ran = true;
    }
    if (max_iters_run) *max_iters_run = (uint32_t)g->stats[12];
    if (cells_not_converged) *cells_not_converged = g->stats[13];
    return PA_OK;
}

int pa_genes_layout(const pa_genes* g, uint64_t* n_cells, uint64_t* n_values) {
    if (!g) return fail(PA_ERR_INVALID_ARG, "null argument");
    if (n_cells) *n_cells = g->n_cells;
    if (n_values) *n_values = g->n_values;
    return PA_OK;
}

int pa_genes_values(const pa_genes* g, uint64_t* barcode, uint32_t* cell, uint32_t* gene, double* alpha, uint64_t cap) {
    if (!g) return fail(PA_ERR_INVALID_ARG, "null argument");
    if (barcode && g->n_cells) {
        PA_HIP_TRY(hipSetDevice(g->device));
        PA_HIP_TRY(hipMemcpy(barcode, g->d_barcode.get(), g->n_cells * 8ull, hipMemcpyDeviceToHost));
    }
    if (!cell && !gene && !alpha) return PA_OK;
    if (cap < g->n_values) return fail(PA_ERR_BUFFER_TOO_SMALL, "%llu values, room for %llu", (ull)g->n_values, (ull)cap);
    std::vector<uint32_t> c, ge;
    std::vector<double> v;
    const int e = merged_values(g, false, c, ge, v);
    if (e != PA_OK) return e;
    if (v.size() != g->n_values) return fail(PA_ERR_INTERNAL, "%zu values merged, %llu laid out", v.size(), (ull)g->n_values);
    if (cell) std::copy(c.begin(), c.end(), cell);
    if (gene) std::copy(ge.begin(), ge.end(), gene);
    if (alpha) std::copy(v.begin(), v.end(), alpha);
    return PA_OK;
}

int pa_genes_cell_iters(const pa_genes* g, uint32_t* iters) {
    if (!g || !iters) return fail(PA_ERR_INVALID_ARG, "null argument");
    if (g->n_cells) {
        PA_HIP_TRY(hipSetDevice(g->device));
        PA_HIP_TRY(hipMemcpy(iters, g->d_iters.get(), g->n_cells * 4ull, hipMemcpyDeviceToHost));
    }
    return PA_OK;
}

int pa_genes_matrix(const pa_genes* g, uint32_t* cell, uint32_t* gene, double* value, uint64_t cap, uint64_t* n_entries) {
    if (!g) return fail(PA_ERR_INVALID_ARG, "null argument");
    if (!g->ran) return fail(PA_ERR_INVALID_ARG, "the matrix exists after pa_genes_run");
    if (n_entries) *n_entries = g->stats[14];
    if (!cell && !gene && !value) return PA_OK;
    if (cap < g->stats[14]) return fail(PA_ERR_BUFFER_TOO_SMALL, "%llu entries, room for %llu", (ull)g->stats[14], (ull)cap);
    std::vector<uint32_t> c, ge;
    std::vector<double> v;
    const int e = merged_values(g, true, c, ge, v);
    if (e != PA_OK) return e;
    if (v.size() != g->stats[14]) return fail(PA_ERR_INTERNAL, "%zu entries merged, %llu counted", v.size(), (ull)g->stats[14]);
    if (cell) std::copy(c.begin(), c.end(), cell);
    if (gene) std::copy(ge.begin(), ge.end(), gene);
    if (value) std::copy(v.begin(), v.end(), value);
    return PA_OK;
}

int pa_genes_stats(const pa_genes* g, uint64_t stats[PA_GENES_STATS]) {
    if (!g || !stats) return fail(PA_ERR_INVALID_ARG, "null argument");
    for (int j = 0; j < PA_GENES_STATS; ++j) stats[j] = g->stats[j];
    return PA_OK;
}

int pa_genes_write(const pa_genes* g, const pa_host_index* h, const char* out_dir) {
    if (!g || !h || !out_dir) return fail(PA_ERR_INVALID_ARG, "null argument");
    if (!g->ran) return fail(PA_ERR_INVALID_ARG, "the files are written after pa_genes_run");
    std::string features;
    int e = genes::features_text(h->h.tx_genes, g->num_genes, features);
    if (e != PA_OK) return e;
    std::vector<uint32_t> c, ge;
    std::vector<double> v;
    if ((e = merged_values(g, true, c, ge, v)) != PA_OK) return e;
    std::vector<uint64_t> bc(g->n_cells);
    if (g->n_cells) PA_HIP_TRY(hipMemcpy(bc.data(), g->d_barcode.get(), g->n_cells * 8ull, hipMemcpyDeviceToHost));
    return genes::write_files(out_dir, genes::matrix_text(g->num_genes, g->n_cells, c.data(), ge.data(), v.data(), v.size()),
                              genes::barcodes_text(bc.data(), g->n_cells, g->bc_len), features);
}

void pa_genes_destroy(pa_genes* g) {
    if (!g) return;
    (void)hipSetDevice(g->device);
    if (g->stream) {
        (void)hipStreamSynchronize(g->stream);
        (void)hipStreamDestroy(g->stream);
    }
    delete g;
}

}  // extern "C"
