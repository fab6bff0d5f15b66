// Bootstrap replicates of the abundance EM (pa_quant_bootstrap_*; the rules are in the header, section "bootstrap
// replicates"). A batch of n <= 64 replicates shares the incidence of csrc/quant.hip (row -> ids, transcript -> rows); what differs
// per replicate (counts n, quotients q, alpha, w) lies replicate-innermost with a stride of 4 .. 64, so that the gather of one id is
// one contiguous run of doubles and the ids and offsets of a row are read once for the lanes of all replicates.
//   draw   a lane takes Philox4x32-10 blocks (two draws each), finds the row of a pick by binary search in the cumulative counts
//          (first ten steps in an LDS copy of every step-th entry) and counts it in an LDS hash table of its block; the table goes
//          to n[row][b] with integer atomics at the end of the block, a pick that finds no slot goes there at once
//   E, M   rows (transcripts) of at most 16 entries: one lane per (row, replicate), the entries summed as a binary tree over 16 / 8 / 4
//          slots; longer ones: 64 lanes x 4 replicates per block, a lane's strided partial sum, then a tree over the 64 lanes through LDS.
// The order of every sum depends on the row's length (the transcript's degree) alone, so a replicate's bits do not depend on its batch.
// No floating-point atomics, no block waits on another, plain launches on the object's own stream.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "device_prims.hpp"
#include "hip_buffer.hpp"
#include "pa_common.hpp"
#include "quant_state.hpp"

using namespace pa;

namespace {

constexpr uint32_t BOOT_MAX = PA_QUANT_BOOT_MAX_BATCH;
constexpr uint32_t LONG_REPS = 4;            // replicates of a block on the long path
constexpr uint32_t LONG_LANES = QB / LONG_REPS;
constexpr int BBIN = 4;                      // long (the first two bins of the layout), then its bins of at most 16 / 8 / 4 entries

// ---------------------------------------------------------------- resampler ----------------------------------------------------------------
constexpr uint32_t DRAW_BLOCKS_PER_LANE = 32;                       // Philox blocks of a lane
constexpr uint32_t DRAW_CHUNK = QB * DRAW_BLOCKS_PER_LANE;          // Philox blocks of a workgroup
constexpr uint32_t HT_SLOTS = 4096, HT_EMPTY = 0xFFFFFFFFu, HT_PROBES = 4;
constexpr uint32_t COARSE = 1024;

struct U4 { uint32_t x, y, z, w; };

__device__ __forceinline__ U4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return U4{c0, c1, c2, c3};
}

struct DrawArgs {
    const unsigned long long* cum;   // [rows + 1]
    const uint32_t* cand_row;        // [rows]
    uint32_t rows, step;             // step = ceil(rows / COARSE)
    unsigned long long N;
    uint32_t k0, k1, first, stride;
    uint32_t* n;                     // [rows][stride]
};

__device__ __forceinline__ void draw_pick(const DrawArgs& a, unsigned long long x, uint32_t b, const unsigned long long* coarse, uint32_t* keys, uint32_t* cnts) {
    const unsigned long long p = __umul64hi(x, a.N);
    uint32_t lo = 0, hi = COARSE;    // coarse[lo] <= p < coarse[hi]
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (coarse[mid] <= p) lo = mid; else hi = mid;
    }
    uint32_t glo = lo * a.step, ghi = min((lo + 1) * a.step, a.rows);   // cum[glo] <= p < cum[ghi]
    while (ghi - glo > 1) {
        const uint32_t mid = glo + ((ghi - glo) >> 1);
        if (a.cum[mid] <= p) glo = mid; else ghi = mid;
    }
    const uint32_t row = a.cand_row[glo];
    const uint32_t h = (row * 2654435761u) >> 20;
    for (uint32_t i = 0; i < HT_PROBES; ++i) {
        const uint32_t s = (h + i) & (HT_SLOTS - 1);
        uint32_t k = keys[s];
        if (k == HT_EMPTY) k = atomicCAS(&keys[s], HT_EMPTY, row);
        if (k == HT_EMPTY || k == row) {
            atomicAdd(&cnts[s], 1u);
            return;
        }
    }
    atomicAdd(&a.n[(size_t)row * a.stride + b], 1u);
}

__global__ __launch_bounds__(QB) void boot_draw(const DrawArgs a) {
    __shared__ unsigned long long coarse[COARSE + 1];
    __shared__ uint32_t keys[HT_SLOTS], cnts[HT_SLOTS];
    const uint32_t b = blockIdx.y;
    for (uint32_t i = threadIdx.x; i <= COARSE; i += QB) coarse[i] = a.cum[min((unsigned long long)i * a.step, (unsigned long long)a.rows)];
    for (uint32_t i = threadIdx.x; i < HT_SLOTS; i += QB) { keys[i] = HT_EMPTY; cnts[i] = 0; }
    __syncthreads();
    const unsigned long long blocks = (a.N + 1) >> 1, base = (unsigned long long)blockIdx.x * DRAW_CHUNK;
    for (uint32_t it = 0; it < DRAW_BLOCKS_PER_LANE; ++it) {
        const unsigned long long i = base + (unsigned long long)it * QB + threadIdx.x;
        if (i >= blocks) break;
        const U4 o = philox4x32_10((uint32_t)i, (uint32_t)(i >> 32), a.first + b, 0u, a.k0, a.k1);
        draw_pick(a, (unsigned long long)o.x | ((unsigned long long)o.y << 32), b, coarse, keys, cnts);
        if (2 * i + 1 < a.N) draw_pick(a, (unsigned long long)o.z | ((unsigned long long)o.w << 32), b, coarse, keys, cnts);
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < HT_SLOTS; i += QB)
        if (keys[i] != HT_EMPTY && cnts[i]) atomicAdd(&a.n[(size_t)keys[i] * a.stride + b], cnts[i]);
}

__global__ void boot_iota(uint32_t n, uint32_t* out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = i;
}

// counts of the rows in candidate order, one zero behind them (the exclusive scan of rows + 1 entries then ends in N)
__global__ void boot_cand_counts(uint32_t rows, const uint32_t* cand_row, const double* row_cnt, unsigned long long* out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i > rows) return;
    out[i] = i < rows ? (unsigned long long)row_cnt[cand_row[i]] : 0ull;
}

__global__ void boot_column(uint32_t rows, uint32_t stride, uint32_t k, const uint32_t* n, uint32_t* out) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r < rows) out[r] = n[(size_t)r * stride + k];
}

__global__ void boot_start(uint32_t num_tx, uint32_t stride, uint32_t n, const uint32_t* tx_off, const double* eff, double a0, double* alpha, double* w) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (uint64_t)num_tx * stride) return;
    const uint32_t t = (uint32_t)(i / stride), b = (uint32_t)(i % stride);
    const double a = b < n && tx_off[t + 1] > tx_off[t] ? a0 : 0.0;
    alpha[i] = a;
    w[i] = a / eff[t];
}

__global__ void boot_truncate(uint64_t count, double below, double* alpha, double* w) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    if (alpha[i] < below) { alpha[i] = 0.0; w[i] = 0.0; }
}

// ---------------------------------------------------------------- the batched passes ----------------------------------------------------------------
struct BootGrid {
    uint32_t begin[BBIN + 1];   // entities [begin[k], begin[k + 1]) are bin k
    uint32_t blk[BBIN + 1];     // blocks [blk[k], blk[k + 1]) serve bin k
};

BootGrid boot_grid(const Layout& l, uint32_t stride) {
    BootGrid g;
    g.begin[0] = 0;
    for (int k = 1; k <= BBIN; ++k) g.begin[k] = l.begin[k + 1];
    g.blk[0] = 0;
    g.blk[1] = (g.begin[1] - g.begin[0]) * (stride / LONG_REPS);
    for (int k = 1; k < BBIN; ++k) {
        const uint32_t per = QB / stride, ents = g.begin[k + 1] - g.begin[k];
        g.blk[k + 1] = g.blk[k] + (ents + per - 1) / per;
    }
    return g;
}

__device__ __forceinline__ int boot_bin(const BootGrid& g) {
    int k = 0;
#pragma unroll
    for (int i = 1; i < BBIN; ++i) k += blockIdx.x >= g.blk[i] ? 1 : 0;
    return k;
}

// at most S entries: slot u holds entry u (or 0), the slots are added as a binary tree
template <int S>
__device__ __forceinline__ double small_sum(const double* __restrict__ val, const uint32_t* __restrict__ idx, uint32_t beg, uint32_t end, uint32_t stride, uint32_t b) {
    double s[S];
#pragma unroll
    for (int u = 0; u < S; ++u) s[u] = beg + u < end ? val[(size_t)idx[beg + u] * stride + b] : 0.0;
#pragma unroll
    for (int o = S / 2; o > 0; o >>= 1) {
#pragma unroll
        for (int u = 0; u < o; ++u) s[u] += s[u + o];
    }
    return s[0];
}

// the long path: lane v of 64 sums entries v, v + 64, ..; then s[v] += s[v + o] for o = 32, 16, .. 1. Thread = v * 4 + replicate. The sum is in
// lds[threadIdx.x] of the threads with v = 0. Every thread of the block comes here.
__device__ __forceinline__ void long_sum(const double* __restrict__ val, const uint32_t* __restrict__ idx, uint32_t beg, uint32_t end, uint32_t stride, uint32_t b,
                                         bool act, double* lds) {
    const uint32_t v = threadIdx.x / LONG_REPS;
    double s = 0.0;
    if (act)
        for (uint32_t j = beg + v; j < end; j += LONG_LANES) s += val[(size_t)idx[j] * stride + b];
    lds[threadIdx.x] = s;
    for (uint32_t o = LONG_LANES / 2; o > 0; o >>= 1) {
        __syncthreads();
        if (v < o) lds[threadIdx.x] += lds[threadIdx.x + o * LONG_REPS];
    }
}

struct BootE {
    BootGrid g;
    uint32_t stride;
    const uint32_t* mask;      // [64] replicates that take part
    const uint32_t* row_off;
    const uint32_t* row_ids;
    const uint32_t* n;         // [rows][stride]
    const double* w;           // [T][stride]
    double* q;                 // [rows][stride]
};

template <int S>
__device__ __forceinline__ void boot_e_small(const BootE& a, int k) {
    const uint32_t row = a.g.begin[k] + (blockIdx.x - a.g.blk[k]) * (QB / a.stride) + threadIdx.x / a.stride, b = threadIdx.x % a.stride;
    if (row >= a.g.begin[k + 1] || !a.mask[b]) return;
    const double d = small_sum<S>(a.w, a.row_ids, a.row_off[row], a.row_off[row + 1], a.stride, b);
    const size_t o = (size_t)row * a.stride + b;
    a.q[o] = d > 0.0 ? (double)a.n[o] / d : 0.0;
}

__global__ __launch_bounds__(QB) void boot_e_pass(const BootE a) {
    __shared__ double lds[QB];
    switch (boot_bin(a.g)) {
        case 0: {
            const uint32_t per = a.stride / LONG_REPS, local = blockIdx.x - a.g.blk[0];
            const uint32_t row = a.g.begin[0] + local / per, b0 = (local % per) * LONG_REPS, b = b0 + threadIdx.x % LONG_REPS;
            if (!(a.mask[b0] | a.mask[b0 + 1] | a.mask[b0 + 2] | a.mask[b0 + 3])) return;   // (the same for the whole block)
            const bool act = a.mask[b] != 0;
            long_sum(a.w, a.row_ids, a.row_off[row], a.row_off[row + 1], a.stride, b, act, lds);
            if (act && threadIdx.x < LONG_REPS) {
                const double d = lds[threadIdx.x];
                const size_t o = (size_t)row * a.stride + b;
                a.q[o] = d > 0.0 ? (double)a.n[o] / d : 0.0;
            }
            break;
        }
        case 1: boot_e_small<16>(a, 1); break;
        case 2: boot_e_small<8>(a, 2); break;
        default: boot_e_small<4>(a, 3); break;
    }
}

struct BootM {
    BootGrid g;                // over transcript slots
    uint32_t stride;
    const uint32_t* mask;
    const uint32_t* tx_order;
    const uint32_t* tx_off;
    const uint32_t* tx_rows;
    const double* q;           // [rows][stride]
    const double* eff;         // [T]
    double* alpha;             // [T][stride]
    double* w;                 // [T][stride]
    uint32_t* flag;            // [64]
    double change_limit, change;
    int check;
};

__device__ __forceinline__ void boot_m_update(const BootM& a, uint32_t t, uint32_t b, double s) {
    const size_t o = (size_t)t * a.stride + b;
    const double old = a.alpha[o], next = a.w[o] * s;
    a.alpha[o] = next;
    a.w[o] = next / a.eff[t];
    // one integer OR per replicate at most from a lane that saw a change, and none once the word is set
    if (a.check && next > a.change_limit && fabs(next - old) / next > a.change && __atomic_load_n(&a.flag[b], __ATOMIC_RELAXED) == 0u) atomicOr(&a.flag[b], 1u);
}

template <int S>
__device__ __forceinline__ void boot_m_small(const BootM& a, int k) {
    const uint32_t slot = a.g.begin[k] + (blockIdx.x - a.g.blk[k]) * (QB / a.stride) + threadIdx.x / a.stride, b = threadIdx.x % a.stride;
    if (slot >= a.g.begin[k + 1] || !a.mask[b]) return;
    const uint32_t t = a.tx_order[slot];
    boot_m_update(a, t, b, small_sum<S>(a.q, a.tx_rows, a.tx_off[t], a.tx_off[t + 1], a.stride, b));
}

__global__ __launch_bounds__(QB) void boot_m_pass(const BootM a) {
    __shared__ double lds[QB];
    switch (boot_bin(a.g)) {
        case 0: {
            const uint32_t per = a.stride / LONG_REPS, local = blockIdx.x - a.g.blk[0];
            const uint32_t slot = a.g.begin[0] + local / per, b0 = (local % per) * LONG_REPS, b = b0 + threadIdx.x % LONG_REPS;
            if (!(a.mask[b0] | a.mask[b0 + 1] | a.mask[b0 + 2] | a.mask[b0 + 3])) return;
            const bool act = a.mask[b] != 0;
            const uint32_t t = a.tx_order[slot];
            long_sum(a.q, a.tx_rows, a.tx_off[t], a.tx_off[t + 1], a.stride, b, act, lds);
            if (act && threadIdx.x < LONG_REPS) boot_m_update(a, t, b, lds[threadIdx.x]);
            break;
        }
        case 1: boot_m_small<16>(a, 1); break;
        case 2: boot_m_small<8>(a, 2); break;
        default: boot_m_small<4>(a, 3); break;
    }
}

// ---------------------------------------------------------------- host ----------------------------------------------------------------
uint32_t stride_for(uint32_t n) {
    uint32_t s = LONG_REPS;
    while (s < n) s <<= 1;
    return s;
}

// the rows in candidate order and their cumulative counts: once per table
int build_tables(pa_quant* q) {
    QuantBoot& bt = q->boot;
    hipStream_t s = q->stream;
    const uint32_t rows = (uint32_t)q->stats[0];
    DeviceBuffer<uint32_t> iota, key_out;
    DeviceBuffer<unsigned long long> cnt;
    DeviceBuffer<uint8_t> tmp;
    int e;
    if ((e = iota.alloc(rows)) || (e = key_out.alloc(rows)) || (e = cnt.alloc((size_t)rows + 1)) || (e = bt.d_cand_row.alloc(rows)) || (e = bt.d_cum.alloc((size_t)rows + 1))) return e;
    bt.row_cand.resize(rows);
    hipLaunchKernelGGL(boot_iota, dim3(grid_for(rows)), dim3(256), 0, s, rows, iota.get());
    if ((e = sort_pairs(s, tmp, q->d_row_cand.get(), key_out.get(), iota.get(), bt.d_cand_row.get(), (size_t)rows, 0, 32))) return e;
    hipLaunchKernelGGL(boot_cand_counts, dim3(grid_for((uint64_t)rows + 1)), dim3(256), 0, s, rows, bt.d_cand_row.get(), q->d_row_cnt.get(), cnt.get());
    if ((e = scan_exclusive(s, tmp, cnt.get(), bt.d_cum.get(), (size_t)rows + 1))) return e;
    PA_HIP_TRY(hipMemcpyAsync(bt.row_cand.data(), q->d_row_cand.get(), 4ull * rows, hipMemcpyDeviceToHost, s));
    PA_HIP_TRY(hipGetLastError());
    PA_HIP_TRY(hipStreamSynchronize(s));
    bt.tables = true;
    return PA_OK;
}

int launch_boot_iteration(pa_quant* q, const uint32_t* mask, bool check) {
    QuantBoot& bt = q->boot;
    BootE e;
    e.g = boot_grid(q->rows, bt.stride); e.stride = bt.stride; e.mask = mask; e.row_off = q->d_row_off.get(); e.row_ids = q->d_row_ids.get();
    e.n = bt.d_n.get(); e.w = bt.d_w.get(); e.q = bt.d_q.get();
    BootM m;
    m.g = boot_grid(q->slots, bt.stride); m.stride = bt.stride; m.mask = mask; m.tx_order = q->d_tx_order.get(); m.tx_off = q->d_tx_off.get();
    m.tx_rows = q->d_tx_rows.get(); m.q = bt.d_q.get(); m.eff = q->d_eff.get(); m.alpha = bt.d_alpha.get(); m.w = bt.d_w.get(); m.flag = bt.d_flag.get();
    m.change_limit = q->par.alpha_change_limit; m.change = q->par.alpha_change; m.check = check ? 1 : 0;
    hipLaunchKernelGGL(boot_e_pass, dim3(e.g.blk[BBIN]), dim3(QB), 0, q->stream, e);
    hipLaunchKernelGGL(boot_m_pass, dim3(m.g.blk[BBIN]), dim3(QB), 0, q->stream, m);
    PA_HIP_TRY(hipGetLastError());
    return PA_OK;
}

int no_batch() { return fail(PA_ERR_INVALID_ARG, "no bootstrap batch drawn"); }

}  // namespace

extern "C" {

int pa_quant_bootstrap_draw(pa_quant* q, uint64_t seed, uint32_t first, uint32_t n) {
    if (!q) return fail(PA_ERR_INVALID_ARG, "null argument");
    if (n == 0 || n > BOOT_MAX) return fail(PA_ERR_INVALID_ARG, "a bootstrap batch of %u replicates: 1 .. %u", n, BOOT_MAX);
    if ((uint64_t)first + n > (1ull << 32)) return fail(PA_ERR_INVALID_ARG, "replicates %u .. %llu: replicate numbers have 32 bits", first, (unsigned long long)first + n - 1);
    const uint64_t N = q->stats[5];
    if (N >> 32) return fail(PA_ERR_UNSUPPORTED, "%llu reads: the bootstrap draws from fewer than 2^32", (unsigned long long)N);
    QuantBoot& bt = q->boot;
    const uint32_t stride = stride_for(n);
    if (!q->ready) {
        if (N) return fail(PA_ERR_INVALID_ARG, "the last pa_quant_set_counts failed: there is no table to draw from");
        bt.n = n; bt.stride = stride;   // no reads: every count and every output of the batch is 0
        return PA_OK;
    }
    PA_HIP_TRY(hipSetDevice(q->device));
    bt.n = 0;
    int e;
    if (!bt.tables && (e = build_tables(q))) return e;
    const uint32_t rows = (uint32_t)q->stats[0], T = q->num_tx;
    const size_t rn = (size_t)rows * stride, tn = (size_t)T * stride;
    if (((bt.d_n.size() != rn || bt.d_q.size() != rn) && ((e = bt.d_n.alloc(rn)) || (e = bt.d_q.alloc(rn)))) ||
        ((bt.d_alpha.size() != tn || bt.d_w.size() != tn) && ((e = bt.d_alpha.alloc(tn)) || (e = bt.d_w.alloc(tn)))) ||
        (e = bt.d_col.reserve(rows, rows)) || (e = bt.d_mask.reserve(2 * BOOT_MAX, 2 * BOOT_MAX)) || (e = bt.d_flag.reserve(BOOT_MAX, BOOT_MAX)) ||
        (e = bt.h_flag.reserve(BOOT_MAX, BOOT_MAX)) || (e = bt.h_mask.reserve(2 * BOOT_MAX, 2 * BOOT_MAX)))
        return e;
    hipStream_t s = q->stream;
    for (uint32_t b = 0; b < BOOT_MAX; ++b) bt.h_mask.get()[b] = bt.h_mask.get()[BOOT_MAX + b] = b < n ? 1u : 0u;
    PA_HIP_TRY(hipMemcpyAsync(bt.d_mask.get(), bt.h_mask.get(), 2 * BOOT_MAX * 4, hipMemcpyHostToDevice, s));
    PA_HIP_TRY(hipMemsetAsync(bt.d_n.get(), 0, rn * 4, s));
    PA_HIP_TRY(hipMemsetAsync(bt.d_q.get(), 0, rn * 8, s));
    DrawArgs a;
    a.cum = bt.d_cum.get(); a.cand_row = bt.d_cand_row.get(); a.rows = rows; a.step = (rows + COARSE - 1) / COARSE; a.N = N;
    a.k0 = (uint32_t)seed; a.k1 = (uint32_t)(seed >> 32); a.first = first; a.stride = stride; a.n = bt.d_n.get();
    const uint64_t blocks = (N + 1) / 2;
    hipLaunchKernelGGL(boot_draw, dim3((uint32_t)((blocks + DRAW_CHUNK - 1) / DRAW_CHUNK), n), dim3(QB), 0, s, a);
    hipLaunchKernelGGL(boot_start, dim3(grid_for(tn)), dim3(256), 0, s, T, stride, n, q->d_tx_off.get(), q->d_eff.get(), (double)N / (double)T, bt.d_alpha.get(), bt.d_w.get());
    PA_HIP_TRY(hipGetLastError());
    PA_HIP_TRY(hipStreamSynchronize(s));
    bt.n = n; bt.stride = stride;
    return PA_OK;
}

int pa_quant_bootstrap_counts(const pa_quant* q, uint32_t k, uint64_t* class_counts, uint64_t counts_len, uint64_t* overflow_counts, uint64_t n_records) {
    if (!q || !class_counts) return fail(PA_ERR_INVALID_ARG, "null argument");
    const QuantBoot& bt = q->boot;
    if (bt.n == 0) return no_batch();
    if (k >= bt.n) return fail(PA_ERR_INVALID_ARG, "replicate %u of a batch of %u", k, bt.n);
    const uint32_t C = q->num_classes;
    if (counts_len != (uint64_t)C + 3) return fail(PA_ERR_INVALID_ARG, "count table of %llu entries: the index has %u classes + 3 tail slots", (unsigned long long)counts_len, C);
    if (n_records != q->n_records) return fail(PA_ERR_INVALID_ARG, "%llu overflow counts: the table was set with %u records", (unsigned long long)n_records, q->n_records);
    if (n_records && !overflow_counts) return fail(PA_ERR_INVALID_ARG, "null overflow counts");
    std::vector<uint32_t> col;
    if (q->ready) {
        const uint32_t rows = (uint32_t)q->stats[0];
        col.resize(rows);
        PA_HIP_TRY(hipSetDevice(q->device));
        hipLaunchKernelGGL(boot_column, dim3(grid_for(rows)), dim3(256), 0, q->stream, rows, bt.stride, k, bt.d_n.get(), bt.d_col.get());
        PA_HIP_TRY(hipGetLastError());
        PA_HIP_TRY(hipMemcpyAsync(col.data(), bt.d_col.get(), 4ull * rows, hipMemcpyDeviceToHost, q->stream));
        PA_HIP_TRY(hipStreamSynchronize(q->stream));
    }
    std::fill(class_counts, class_counts + counts_len, 0ull);
    for (uint64_t r = 0; r < n_records; ++r) overflow_counts[r] = 0;
    for (size_t r = 0; r < col.size(); ++r) {
        const uint32_t c = bt.row_cand[r];
        if (c < C) class_counts[c] = col[r];
        else { overflow_counts[c - C] = col[r]; class_counts[C] += col[r]; }
    }
    return PA_OK;
}

int pa_quant_bootstrap_step(pa_quant* q, uint32_t n_iters) {
    if (!q) return fail(PA_ERR_INVALID_ARG, "null argument");
    if (q->boot.n == 0) return no_batch();
    if (!q->ready || n_iters == 0) return PA_OK;
    PA_HIP_TRY(hipSetDevice(q->device));
    for (uint32_t i = 0; i < n_iters; ++i) {
        const int e = launch_boot_iteration(q, q->boot.d_mask.get(), false);
        if (e != PA_OK) return e;
    }
    PA_HIP_TRY(hipStreamSynchronize(q->stream));
    return PA_OK;
}

int pa_quant_bootstrap_run(pa_quant* q, uint32_t* iters, int* converged) {
    if (!q) return fail(PA_ERR_INVALID_ARG, "null argument");
    QuantBoot& bt = q->boot;
    if (bt.n == 0) return no_batch();
    const uint32_t n = bt.n;
    if (!q->ready) {   // no reads: nothing to iterate
        for (uint32_t b = 0; b < n; ++b) {
            if (iters) iters[b] = 0;
            if (converged) converged[b] = 1;
        }
        return PA_OK;
    }
    PA_HIP_TRY(hipSetDevice(q->device));
    const pa_quant_params& p = q->par;
    hipStream_t s = q->stream;
    uint32_t* run_mask = bt.h_mask.get() + BOOT_MAX;
    uint32_t it_of[BOOT_MAX] = {}, left = n, done = 0;
    int conv_of[BOOT_MAX] = {};
    for (uint32_t b = 0; b < BOOT_MAX; ++b) run_mask[b] = b < n ? 1u : 0u;
    PA_HIP_TRY(hipMemcpyAsync(bt.d_mask.get() + BOOT_MAX, run_mask, BOOT_MAX * 4, hipMemcpyHostToDevice, s));
    while (done < p.max_iters && left) {
        const uint32_t i = done + 1;
        const bool check = (i >= p.min_iters && i % p.check_every == 0) || i == p.max_iters;
        if (check) PA_HIP_TRY(hipMemsetAsync(bt.d_flag.get(), 0, BOOT_MAX * 4, s));
        const int e = launch_boot_iteration(q, bt.d_mask.get() + BOOT_MAX, check);
        if (e != PA_OK) return e;
        done = i;
        if (!check) continue;
        PA_HIP_TRY(hipMemcpyAsync(bt.h_flag.get(), bt.d_flag.get(), BOOT_MAX * 4, hipMemcpyDeviceToHost, s));   // every replicate's flag in one copy
        PA_HIP_TRY(hipStreamSynchronize(s));
        bool froze = false;
        for (uint32_t b = 0; b < n; ++b) {
            if (!run_mask[b]) continue;
            const bool conv = bt.h_flag.get()[b] == 0 && i >= p.min_iters;
            if (!conv && i != p.max_iters) continue;
            run_mask[b] = 0;   // frozen from here on
            it_of[b] = i;
            conv_of[b] = conv ? 1 : 0;
            --left;
            froze = true;
        }
        if (froze && left) PA_HIP_TRY(hipMemcpyAsync(bt.d_mask.get() + BOOT_MAX, run_mask, BOOT_MAX * 4, hipMemcpyHostToDevice, s));
    }
    for (uint32_t b = 0; b < n; ++b)
        if (run_mask[b]) it_of[b] = done;   // (max_iters = 0)
    const uint64_t tn = (uint64_t)q->num_tx * bt.stride;
    hipLaunchKernelGGL(boot_truncate, dim3(grid_for(tn)), dim3(256), 0, s, tn, p.alpha_limit / 10.0, bt.d_alpha.get(), bt.d_w.get());
    PA_HIP_TRY(hipGetLastError());
    PA_HIP_TRY(hipStreamSynchronize(s));
    for (uint32_t b = 0; b < n; ++b) {
        if (iters) iters[b] = it_of[b];
        if (converged) converged[b] = conv_of[b];
    }
    return PA_OK;
}

int pa_quant_bootstrap_fetch(const pa_quant* q, double* est_counts, double* tpm) {
    if (!q) return fail(PA_ERR_INVALID_ARG, "null argument");
    const QuantBoot& bt = q->boot;
    if (bt.n == 0) return no_batch();
    if (!est_counts && !tpm) return PA_OK;
    const uint32_t T = q->num_tx, n = bt.n;
    std::vector<double> all, alpha(T);
    if (q->ready) {
        all.resize((size_t)T * bt.stride);
        PA_HIP_TRY(hipSetDevice(q->device));
        PA_HIP_TRY(hipMemcpyAsync(all.data(), bt.d_alpha.get(), all.size() * 8, hipMemcpyDeviceToHost, q->stream));
        PA_HIP_TRY(hipStreamSynchronize(q->stream));
    }
    for (uint32_t b = 0; b < n; ++b) {
        for (uint32_t t = 0; t < T; ++t) alpha[t] = q->ready ? all[(size_t)t * bt.stride + b] : 0.0;
        if (est_counts) std::copy(alpha.begin(), alpha.end(), est_counts + (size_t)b * T);
        if (tpm) {   // the rule of pa_quant_fetch: the denominator summed in transcript order
            double den = 0.0;
            for (uint32_t t = 0; t < T; ++t) den += alpha[t] / q->eff[t];
            for (uint32_t t = 0; t < T; ++t) tpm[(size_t)b * T + t] = den > 0.0 ? 1e6 * (alpha[t] / q->eff[t]) / den : 0.0;
        }
    }
    return PA_OK;
}

}  // extern "C"
