// Transcript abundances by EM over the class-count table (pa_quant_*).
//
// The reduced problem is a sparse 0/1 incidence: rows = the counted index classes + the overflow records, columns = transcripts.
// One iteration is two gather-only passes over it in f64:
//   E   q_r  = n_r / sum_{t in r} w_t                           (row CSR:        row -> transcript ids)
//   M   a'_t = w_t * sum_{r with t} q_r,  w'_t = a'_t / eff_t   (transposed CSR: transcript -> rows)
// Rows (and transcripts) are ordered by length (degree), longest first, and cut into five bins; one launch serves all bins: a block
// of 256 threads takes one row of more than 1024 entries, or 4 rows of 17..1024 (a wave each), or 16 / 32 / 64 rows of at most
// 16 / 8 / 4 entries (sub-wave groups). Every sum has a fixed order (a lane's strided partial sum, then a xor tree, then the four
// wave sums in order), so two runs on one input give the same bits. No floating-point atomics, no block waits on another.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <charconv>
#include <cmath>
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "device_prims.hpp"
#include "hip_buffer.hpp"
#include "pa_common.hpp"
#include "quant_state.hpp"

using namespace pa;

namespace {

void finish_layout(Layout& l) {
    l.blk[0] = 0;
    for (int k = 0; k < NBIN; ++k) {
        const uint32_t per = QB / bin_group(k), rows = l.begin[k + 1] - l.begin[k];
        l.blk[k + 1] = l.blk[k] + (rows + per - 1) / per;
    }
}

// sum of val[idx[j]] over j in [beg, end) by the G lanes of a group (G = 256: the block). Every lane of the group returns the sum.
template <int G>
__device__ __forceinline__ double group_sum(const double* __restrict__ val, const uint32_t* __restrict__ idx, uint32_t beg, uint32_t end,
                                            uint32_t lane, double* lds) {
    double s = 0.0;
    for (uint32_t j = beg + lane; j < end; j += G) s += val[idx[j]];
    constexpr int W = G < 64 ? G : 64;
#pragma unroll
    for (int o = W / 2; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (G == 256) {   // (the bin is the same for the whole block: every thread comes here)
        if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = s;
        __syncthreads();
        s = ((lds[0] + lds[1]) + lds[2]) + lds[3];
    }
    return s;
}

__device__ __forceinline__ int block_bin(const Layout& l) {
    int k = 0;
#pragma unroll
    for (int i = 1; i < NBIN; ++i) k += blockIdx.x >= l.blk[i] ? 1 : 0;
    return k;
}

struct EArgs {
    Layout lay;
    const uint32_t* row_off;   // [rows + 1]
    const uint32_t* row_ids;   // [nnz] transcript ids
    const double* row_cnt;     // [rows] n_r
    const double* w;           // [T]
    double* q;                 // [rows]
};

template <int G>
__device__ __forceinline__ void e_body(const EArgs& a, int k, double* lds) {
    const uint32_t row = a.lay.begin[k] + (blockIdx.x - a.lay.blk[k]) * (QB / G) + threadIdx.x / G, lane = threadIdx.x % G;
    const bool valid = row < a.lay.begin[k + 1];
    const uint32_t beg = valid ? a.row_off[row] : 0u, end = valid ? a.row_off[row + 1] : 0u;
    const double d = group_sum<G>(a.w, a.row_ids, beg, end, lane, lds);
    if (valid && lane == 0) a.q[row] = d > 0.0 ? a.row_cnt[row] / d : 0.0;
}

__global__ __launch_bounds__(QB) void quant_e_pass(const EArgs a) {
    __shared__ double lds[4];
    switch (block_bin(a.lay)) {
        case 0: e_body<256>(a, 0, lds); break;
        case 1: e_body<64>(a, 1, lds); break;
        case 2: e_body<16>(a, 2, lds); break;
        case 3: e_body<8>(a, 3, lds); break;
        default: e_body<4>(a, 4, lds); break;
    }
}

struct MArgs {
    Layout lay;                // over transcript SLOTS (transcripts by degree, largest first)
    const uint32_t* tx_order;  // [T] transcript of a slot
    const uint32_t* tx_off;    // [T + 1]
    const uint32_t* tx_rows;   // [nnz] rows of a transcript, ascending
    const double* q;           // [rows]
    const double* eff;         // [T]
    double* alpha;             // [T]
    double* w;                 // [T]
    unsigned int* flag;
    double change_limit, change;
    int check;
};

template <int G>
__device__ __forceinline__ int m_body(const MArgs& a, int k, double* lds) {
    const uint32_t slot = a.lay.begin[k] + (blockIdx.x - a.lay.blk[k]) * (QB / G) + threadIdx.x / G, lane = threadIdx.x % G;
    const bool valid = slot < a.lay.begin[k + 1];
    const uint32_t t = valid ? a.tx_order[slot] : 0u;
    const uint32_t beg = valid ? a.tx_off[t] : 0u, end = valid ? a.tx_off[t + 1] : 0u;
    const double s = group_sum<G>(a.q, a.tx_rows, beg, end, lane, lds);
    int changed = 0;
    if (valid && lane == 0) {
        const double old = a.alpha[t], next = a.w[t] * s;
        a.alpha[t] = next;
        a.w[t] = next / a.eff[t];
        changed = next > a.change_limit && fabs(next - old) / next > a.change;
    }
    return changed;
}

__global__ __launch_bounds__(QB) void quant_m_pass(const MArgs a) {
    __shared__ double lds[4];
    int changed;
    switch (block_bin(a.lay)) {
        case 0: changed = m_body<256>(a, 0, lds); break;
        case 1: changed = m_body<64>(a, 1, lds); break;
        case 2: changed = m_body<16>(a, 2, lds); break;
        case 3: changed = m_body<8>(a, 3, lds); break;
        default: changed = m_body<4>(a, 4, lds); break;
    }
    if (a.check) {   // one integer OR per block that saw a change
        const int any = __syncthreads_or(changed);
        if (threadIdx.x == 0 && any) atomicOr(a.flag, 1u);
    }
}

// ---- setup kernels (once per pa_quant_set_counts) ----
// candidate rows: the index classes, then the overflow records; key = entries of the row, 0 for a candidate without reads
__global__ void quant_candidates(uint32_t num_classes, uint32_t n_ovf, const unsigned long long* counts, const unsigned long long* ec_off,
                                 const uint32_t* ovf_len, const unsigned long long* ovf_cnt, uint32_t* key, uint32_t* val) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= num_classes + n_ovf) return;
    uint32_t len;
    if (i < num_classes) len = counts[i] ? (uint32_t)(ec_off[i + 1] - ec_off[i]) : 0u;
    else len = ovf_cnt[i - num_classes] ? ovf_len[i - num_classes] : 0u;
    key[i] = len;
    val[i] = i;
}

// keys sorted in descending order: out[k + 1] = number of keys >= bin_min_len(k); out[0] = 0
__global__ void quant_bounds(const uint32_t* keys, uint32_t n, uint32_t* out) {
    const int k = threadIdx.x;
    if (k == 0) out[0] = 0;
    if (k >= NBIN) return;
    const uint32_t m = bin_min_len(k);
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (keys[mid] >= m) lo = mid + 1; else hi = mid;
    }
    out[k + 1] = lo;
}

struct GatherArgs {
    uint32_t nnz, rows, num_classes;
    const uint32_t* row_off;    // [rows + 1]
    const uint32_t* row_cand;   // [rows] candidate of a row
    const unsigned long long* ec_off;
    const uint32_t* ec_ids;
    const uint32_t* ovf_src;    // word index of a record's first id
    const uint32_t* words;
    uint32_t* row_ids;          // [nnz]
    uint32_t* pair_key;         // [nnz] transcript
    uint32_t* pair_val;         // [nnz] row
};

__global__ void quant_gather(const GatherArgs a) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= a.nnz) return;
    uint32_t lo = 0, hi = a.rows;   // the row r with row_off[r] <= p < row_off[r + 1]
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (a.row_off[mid] <= p) lo = mid; else hi = mid;
    }
    const uint32_t r = lo, j = p - a.row_off[r], c = a.row_cand[r];
    const uint32_t id = c < a.num_classes ? a.ec_ids[a.ec_off[c] + j] : a.words[a.ovf_src[c - a.num_classes] + j];
    a.row_ids[p] = id;
    a.pair_key[p] = id;
    a.pair_val[p] = r;
}

__global__ void quant_row_counts(uint32_t rows, uint32_t num_classes, const uint32_t* row_cand, const unsigned long long* counts,
                                 const unsigned long long* ovf_cnt, double* row_cnt) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= rows) return;
    const uint32_t c = row_cand[r];
    row_cnt[r] = (double)(c < num_classes ? counts[c] : ovf_cnt[c - num_classes]);   // exact: every count is below 2^53
}

// keys ascending: tx_off[t] = number of keys below t, t = 0 .. T
__global__ void quant_tx_offsets(uint32_t num_tx, const uint32_t* keys, uint32_t nnz, uint32_t* tx_off) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t > num_tx) return;
    uint32_t lo = 0, hi = nnz;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (keys[mid] < t) lo = mid + 1; else hi = mid;
    }
    tx_off[t] = lo;
}

__global__ void quant_degrees(uint32_t num_tx, const uint32_t* tx_off, uint32_t* key, uint32_t* val) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= num_tx) return;
    key[t] = tx_off[t + 1] - tx_off[t];
    val[t] = t;
}

__global__ void quant_start(uint32_t num_tx, const uint32_t* tx_off, const double* eff, double a0, double* alpha, double* w) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= num_tx) return;
    const double a = tx_off[t + 1] > tx_off[t] ? a0 : 0.0;
    alpha[t] = a;
    w[t] = a / eff[t];
}

__global__ void quant_truncate(uint32_t num_tx, double below, double* alpha, double* w) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= num_tx) return;
    if (alpha[t] < below) { alpha[t] = 0.0; w[t] = 0.0; }
}

// an f64 as pa_write_mappability_tsv prints it: shortest digits that read back as the same double, fixed notation
std::string tsv_f64(double v) {
    if (v != v) return "NaN";
    char buf[400];
    const auto r = std::to_chars(buf, buf + sizeof buf, v, std::chars_format::fixed);
    return std::string(buf, r.ptr);
}

bool params_ok(const pa_quant_params& p) {
    const double d[4] = {p.mean_read_len, p.alpha_limit, p.alpha_change_limit, p.alpha_change};
    for (double x : d)
        if (!(x == x) || std::isinf(x)) return false;
    return p.alpha_limit >= 0.0 && p.alpha_change_limit >= 0.0 && p.alpha_change >= 0.0 && p.check_every >= 1;
}

}  // namespace

namespace {

struct OverflowRows {
    std::vector<uint32_t> src, len;         // word index of a record's first id, its ids
    std::vector<unsigned long long> cnt;
};

int launch_iteration(pa_quant* q, bool check) {
    EArgs e;
    e.lay = q->rows; e.row_off = q->d_row_off.get(); e.row_ids = q->d_row_ids.get(); e.row_cnt = q->d_row_cnt.get(); e.w = q->d_w.get(); e.q = q->d_q.get();
    MArgs m;
    m.lay = q->slots; m.tx_order = q->d_tx_order.get(); m.tx_off = q->d_tx_off.get(); m.tx_rows = q->d_tx_rows.get(); m.q = q->d_q.get();
    m.eff = q->d_eff.get(); m.alpha = q->d_alpha.get(); m.w = q->d_w.get(); m.flag = q->d_flag.get();
    m.change_limit = q->par.alpha_change_limit; m.change = q->par.alpha_change; m.check = check ? 1 : 0;
    hipLaunchKernelGGL(quant_e_pass, dim3(q->rows.blk[NBIN]), dim3(QB), 0, q->stream, e);
    hipLaunchKernelGGL(quant_m_pass, dim3(q->slots.blk[NBIN]), dim3(QB), 0, q->stream, m);
    PA_HIP_TRY(hipGetLastError());
    return PA_OK;
}

// builds both CSRs on the device; n_rows >= 1, nnz >= 1 (the host counted them)
int setup_device(pa_quant* q, const uint64_t* class_counts, const OverflowRows& ovf, const uint32_t* words, uint64_t n_words, uint32_t n_rows, uint32_t nnz, double a0) {
    hipStream_t s = q->stream;
    const uint32_t C = q->num_classes, T = q->num_tx, n_ovf = (uint32_t)ovf.cnt.size(), NC = C + n_ovf;
    DeviceBuffer<unsigned long long> d_counts, d_ovf_cnt;
    DeviceBuffer<uint32_t> d_ovf_src, d_ovf_len, d_words, key_a, key_b, val_a, val_b, d_bounds;
    DeviceBuffer<uint8_t> tmp;
    const size_t pairs = std::max<size_t>(std::max<size_t>(NC, nnz), T) + 1;
    int e;
    if ((e = d_counts.alloc(C ? C : 1)) || (e = d_ovf_cnt.alloc(n_ovf ? n_ovf : 1)) || (e = d_ovf_src.alloc(n_ovf ? n_ovf : 1)) ||
        (e = d_ovf_len.alloc(n_ovf ? n_ovf : 1)) || (e = d_words.alloc(n_words ? n_words : 1)) || (e = key_a.alloc(pairs)) || (e = key_b.alloc(pairs)) ||
        (e = val_a.alloc(pairs)) || (e = val_b.alloc(pairs)) || (e = d_bounds.alloc(NBIN + 1)) || (e = q->d_row_cand.alloc(n_rows)) ||
        (e = q->d_row_off.alloc((size_t)n_rows + 1)) || (e = q->d_row_ids.alloc(nnz)) || (e = q->d_row_cnt.alloc(n_rows)) || (e = q->d_q.alloc(n_rows)) ||
        (e = q->d_tx_off.alloc((size_t)T + 1)) || (e = q->d_tx_rows.alloc(nnz)) || (e = q->d_tx_order.alloc(T)))
        return e;
    if (C) PA_HIP_TRY(hipMemcpyAsync(d_counts.get(), class_counts, C * 8ull, hipMemcpyHostToDevice, s));
    if (n_ovf) {
        PA_HIP_TRY(hipMemcpyAsync(d_ovf_cnt.get(), ovf.cnt.data(), n_ovf * 8ull, hipMemcpyHostToDevice, s));
        PA_HIP_TRY(hipMemcpyAsync(d_ovf_src.get(), ovf.src.data(), n_ovf * 4ull, hipMemcpyHostToDevice, s));
        PA_HIP_TRY(hipMemcpyAsync(d_ovf_len.get(), ovf.len.data(), n_ovf * 4ull, hipMemcpyHostToDevice, s));
        PA_HIP_TRY(hipMemcpyAsync(d_words.get(), words, n_words * 4ull, hipMemcpyHostToDevice, s));
    }
    PA_HIP_TRY(hipMemsetAsync(key_b.get(), 0, pairs * 4, s));
    // rows: the candidates with entries, longest first (a stable sort: equal lengths keep class order, overflow records after the classes)
    hipLaunchKernelGGL(quant_candidates, dim3(grid_for(NC)), dim3(256), 0, s, C, n_ovf, d_counts.get(), q->d_ec_off.get(), d_ovf_len.get(), d_ovf_cnt.get(),
                       key_a.get(), val_a.get());
    if ((e = sort_pairs_desc(s, tmp, key_a.get(), key_b.get(), val_a.get(), val_b.get(), (size_t)NC, 0, 32))) return e;
    uint32_t bounds[NBIN + 1] = {}, longest = 0, max_degree = 0;
    hipLaunchKernelGGL(quant_bounds, dim3(1), dim3(64), 0, s, key_b.get(), NC, d_bounds.get());
    PA_HIP_TRY(hipMemcpyAsync(bounds, d_bounds.get(), sizeof bounds, hipMemcpyDeviceToHost, s));
    PA_HIP_TRY(hipMemcpyAsync(&longest, key_b.get(), 4, hipMemcpyDeviceToHost, s));
    PA_HIP_TRY(hipStreamSynchronize(s));
    if (bounds[NBIN] != n_rows) return fail(PA_ERR_INTERNAL, "the device found %u rows, the host %u", bounds[NBIN], n_rows);
    for (int k = 0; k <= NBIN; ++k) q->rows.begin[k] = bounds[k];
    finish_layout(q->rows);
    // row offsets (key_b holds an entry beyond NC: the scan reads n_rows + 1 lengths and its last output is nnz)
    if ((e = scan_exclusive(s, tmp, key_b.get(), q->d_row_off.get(), (size_t)n_rows + 1))) return e;
    PA_HIP_TRY(hipMemcpyAsync(q->d_row_cand.get(), val_b.get(), 4ull * n_rows, hipMemcpyDeviceToDevice, s));
    hipLaunchKernelGGL(quant_row_counts, dim3(grid_for(n_rows)), dim3(256), 0, s, n_rows, C, q->d_row_cand.get(), d_counts.get(), d_ovf_cnt.get(), q->d_row_cnt.get());
    GatherArgs g;
    g.nnz = nnz; g.rows = n_rows; g.num_classes = C; g.row_off = q->d_row_off.get(); g.row_cand = q->d_row_cand.get(); g.ec_off = q->d_ec_off.get();
    g.ec_ids = q->d_ec_ids.get(); g.ovf_src = d_ovf_src.get(); g.words = d_words.get(); g.row_ids = q->d_row_ids.get(); g.pair_key = key_a.get(); g.pair_val = val_a.get();
    hipLaunchKernelGGL(quant_gather, dim3(grid_for(nnz)), dim3(256), 0, s, g);
    // transposed CSR: (transcript, row) pairs sorted by transcript; the sort is stable, so a transcript's rows stay ascending
    if ((e = sort_pairs(s, tmp, key_a.get(), key_b.get(), val_a.get(), q->d_tx_rows.get(), (size_t)nnz, 0, std::max(1u, bits_for(T - 1))))) return e;
    hipLaunchKernelGGL(quant_tx_offsets, dim3(grid_for((uint64_t)T + 1)), dim3(256), 0, s, T, key_b.get(), nnz, q->d_tx_off.get());
    // transcripts by degree, largest first
    hipLaunchKernelGGL(quant_degrees, dim3(grid_for(T)), dim3(256), 0, s, T, q->d_tx_off.get(), key_a.get(), val_a.get());
    if ((e = sort_pairs_desc(s, tmp, key_a.get(), key_b.get(), val_a.get(), q->d_tx_order.get(), (size_t)T, 0, 32))) return e;
    hipLaunchKernelGGL(quant_bounds, dim3(1), dim3(64), 0, s, key_b.get(), T, d_bounds.get());
    PA_HIP_TRY(hipMemcpyAsync(bounds, d_bounds.get(), sizeof bounds, hipMemcpyDeviceToHost, s));
    PA_HIP_TRY(hipMemcpyAsync(&max_degree, key_b.get(), 4, hipMemcpyDeviceToHost, s));
    hipLaunchKernelGGL(quant_start, dim3(grid_for(T)), dim3(256), 0, s, T, q->d_tx_off.get(), q->d_eff.get(), a0, q->d_alpha.get(), q->d_w.get());
    PA_HIP_TRY(hipGetLastError());
    PA_HIP_TRY(hipStreamSynchronize(s));
    for (int k = 0; k <= NBIN; ++k) q->slots.begin[k] = bounds[k];
    finish_layout(q->slots);
    q->stats[2] = bounds[NBIN];
    q->stats[3] = longest;
    q->stats[4] = max_degree;
    return PA_OK;
}

int alpha_to_host(const pa_quant* q, double* out) {
    if (!q->ready) {
        for (uint32_t t = 0; t < q->num_tx; ++t) out[t] = 0.0;
        return PA_OK;
    }
    PA_HIP_TRY(hipSetDevice(q->device));
    PA_HIP_TRY(hipMemcpyAsync(out, q->d_alpha.get(), q->num_tx * 8ull, hipMemcpyDeviceToHost, q->stream));
    PA_HIP_TRY(hipStreamSynchronize(q->stream));
    return PA_OK;
}

// tpm of alpha: the denominator summed in transcript order
void tpm_of(const pa_quant* q, const double* alpha, double* tpm) {
    double den = 0.0;
    for (uint32_t t = 0; t < q->num_tx; ++t) den += alpha[t] / q->eff[t];
    for (uint32_t t = 0; t < q->num_tx; ++t) tpm[t] = den > 0.0 ? 1e6 * (alpha[t] / q->eff[t]) / den : 0.0;
}

}  // namespace

extern "C" {

void pa_quant_default_params(pa_quant_params* p) {
    if (!p) return;
    p->mean_read_len = 0.0;
    p->alpha_limit = 1e-7;
    p->alpha_change_limit = 1e-2;
    p->alpha_change = 1e-2;
    p->min_iters = 50;
    p->max_iters = 10000;
    p->check_every = 10;
    p->reserved = 0;
}

int pa_quant_create(pa_index* idx, const pa_host_index* h, const pa_quant_params* p, pa_quant** out) {
    if (out) *out = nullptr;
    if (!h || !out) return fail(PA_ERR_INVALID_ARG, "null argument");
    pa_quant_params par;
    pa_quant_default_params(&par);
    if (p) par = *p;
    if (!params_ok(par)) return fail(PA_ERR_INVALID_ARG, "quantification parameters: limits must be finite and not negative, check_every at least 1");
    const HostIndex& hi = h->h;
    const uint32_t T = hi.num_transcripts;
    const uint32_t C = hi.ec_offset.empty() ? 0 : (uint32_t)(hi.ec_offset.size() - 1);
    if (T < 1 || hi.tx_start.size() != (size_t)T + 1) return fail(PA_ERR_INVALID_ARG, "the host index has no transcripts");
    const uint64_t ids = C ? hi.ec_offset[C] : 0;
    if (ids > 0x7FFFFFFFull) return fail(PA_ERR_UNSUPPORTED, "class lists of more than 2^31-1 ids");
    for (uint64_t j = 0; j < ids; ++j)
        if (hi.ec_ids[j] >= T) return fail(PA_ERR_INVALID_ARG, "class id %u is no transcript of the host index", hi.ec_ids[j]);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(PA_ERR_NO_DEVICE, "no HIP device available; this library has no CPU fallback");
    if (!idx) return fail(PA_ERR_INVALID_ARG, "null argument");
    pa_index_stats ist{};
    int e = pa_index_get_stats(idx, &ist);
    if (e != PA_OK) return e;
    if (ist.num_classes != C || ist.k != hi.k || ist.num_nodes != hi.node_len.size())
        return fail(PA_ERR_INVALID_ARG, "host index (k %u, %zu nodes, %u classes) is not the one the device index (k %u, %u nodes, %u classes) was made from", hi.k,
                    hi.node_len.size(), C, ist.k, ist.num_nodes, ist.num_classes);
    const uint32_t *h_ec = nullptr, *h_ref = nullptr;
    int device = 0;
    index_host_classes(idx, &h_ec, &h_ref, &device);
    PA_HIP_TRY(hipSetDevice(device));
    std::unique_ptr<pa_quant, void (*)(pa_quant*)> q(new (std::nothrow) pa_quant(), pa_quant_destroy);
    if (!q) return fail(PA_ERR_OOM, "out of host memory");
    q->device = device;
    q->par = par;
    q->num_tx = T;
    q->num_classes = C;
    q->eff.resize(T);
    q->len.resize(T);
    for (uint32_t t = 0; t < T; ++t) {
        const uint64_t len = hi.tx_start[t + 1] - hi.tx_start[t];
        q->len[t] = len;
        q->eff[t] = std::max(par.mean_read_len > 0.0 ? (double)len - par.mean_read_len + 1.0 : (double)len, 1.0);
    }
    q->class_len.resize(C);
    for (uint32_t c = 0; c < C; ++c) q->class_len[c] = (uint32_t)(hi.ec_offset[c + 1] - hi.ec_offset[c]);
    q->tx_gene.resize(T);
    if ((e = pa_host_index_genes(h, q->tx_gene.data(), &q->num_genes)) != PA_OK) return e;
    q->names = hi.tx_names;
    q->names.resize(T);
    PA_HIP_TRY(hipStreamCreateWithFlags(&q->stream, hipStreamNonBlocking));
    if ((e = q->d_ec_off.alloc((size_t)C + 1)) || (e = q->d_ec_ids.alloc(ids ? ids : 1)) || (e = q->d_eff.alloc(T)) || (e = q->d_alpha.alloc(T)) ||
        (e = q->d_w.alloc(T)) || (e = q->d_flag.alloc(1)) || (e = q->h_flag.alloc(1)))
        return e;
    if (C) PA_HIP_TRY(hipMemcpy(q->d_ec_off.get(), hi.ec_offset.data(), ((size_t)C + 1) * 8, hipMemcpyHostToDevice));
    else PA_HIP_TRY(hipMemset(q->d_ec_off.get(), 0, 8));
    if (ids) PA_HIP_TRY(hipMemcpy(q->d_ec_ids.get(), hi.ec_ids.data(), ids * 4, hipMemcpyHostToDevice));
    PA_HIP_TRY(hipMemcpy(q->d_eff.get(), q->eff.data(), T * 8ull, hipMemcpyHostToDevice));
    *out = q.release();
    return PA_OK;
}

int pa_quant_set_counts(pa_quant* q, const uint64_t* class_counts, uint64_t counts_len, const uint32_t* overflow_words, uint64_t n_words) {
    if (!q || !class_counts) return fail(PA_ERR_INVALID_ARG, "null argument");
    const uint32_t C = q->num_classes, T = q->num_tx;
    if (counts_len != (uint64_t)C + 3) return fail(PA_ERR_INVALID_ARG, "count table of %llu entries: the index has %u classes + 3 tail slots", (unsigned long long)counts_len, C);
    if (!overflow_words && n_words) return fail(PA_ERR_INVALID_ARG, "null overflow words");
    uint64_t n_rows = 0, nnz = 0, reads = 0;
    for (uint32_t c = 0; c < C; ++c) {
        if (class_counts[c] >> 53) return fail(PA_ERR_UNSUPPORTED, "class %u has %llu reads: counts of 2^53 and more are not exact in f64", c, (unsigned long long)class_counts[c]);
        if (class_counts[c] && q->class_len[c]) { ++n_rows; nnz += q->class_len[c]; reads += class_counts[c]; }
    }
    OverflowRows ovf;
    uint64_t novel_left_out = class_counts[C];
    if (overflow_words) {
        if (n_words < 2 || overflow_words[1] != n_words || n_words > 0xFFFFFFFFull)
            return fail(PA_ERR_INVALID_ARG, "overflow table: %llu words given, the header says %u", (unsigned long long)n_words, n_words >= 2 ? overflow_words[1] : 0u);
        const uint32_t records = overflow_words[0];
        uint64_t p = 2, total = 0;
        for (uint32_t r = 0; r < records; ++r) {
            if (p + 3 > n_words || p + 3 + overflow_words[p] > n_words) return fail(PA_ERR_INVALID_ARG, "overflow table: record %u ends beyond its %llu words", r, (unsigned long long)n_words);
            const uint32_t len = overflow_words[p];
            const unsigned long long cnt = (unsigned long long)overflow_words[p + 1] | ((unsigned long long)overflow_words[p + 2] << 32);
            if (cnt >> 53) return fail(PA_ERR_UNSUPPORTED, "overflow record %u has %llu reads: counts of 2^53 and more are not exact in f64", r, cnt);
            for (uint32_t j = 0; j < len; ++j) {
                const uint32_t id = overflow_words[p + 3 + j];
                if (id >= T) return fail(PA_ERR_INVALID_ARG, "overflow record %u: id %u is no transcript (the index has %u)", r, id, T);
                if (j && id <= overflow_words[p + 2 + j]) return fail(PA_ERR_INVALID_ARG, "overflow record %u: its ids are not sorted", r);
            }
            ovf.src.push_back((uint32_t)(p + 3));
            ovf.len.push_back(len);
            ovf.cnt.push_back(cnt);
            total += cnt;
            if (cnt && len) { ++n_rows; nnz += len; reads += cnt; }
            p += 3 + (uint64_t)len;
        }
        if (p != n_words) return fail(PA_ERR_INVALID_ARG, "overflow table: its records end at word %llu of %llu", (unsigned long long)p, (unsigned long long)n_words);
        if (total != class_counts[C])
            return fail(PA_ERR_INVALID_ARG, "overflow records hold %llu reads, the novel slot of the table %llu", (unsigned long long)total, (unsigned long long)class_counts[C]);
        novel_left_out = 0;
    }
    if (nnz > 0x7FFFFFFFull || (uint64_t)C + ovf.cnt.size() > 0x7FFFFFFFull) return fail(PA_ERR_UNSUPPORTED, "an incidence of more than 2^31-1 ids");
    if (reads >> 53) return fail(PA_ERR_UNSUPPORTED, "%llu reads: counts of 2^53 and more are not exact in f64", (unsigned long long)reads);
    // every argument is checked: from here on the state changes
    q->ready = false;
    q->boot.drop();   // a bootstrap batch belongs to the table it was drawn from
    q->n_records = (uint32_t)ovf.cnt.size();
    for (uint64_t& x : q->stats) x = 0;
    q->stats[0] = n_rows;
    q->stats[1] = nnz;
    q->stats[5] = reads;
    q->stats[6] = novel_left_out;
    if (reads == 0) return PA_OK;   // every output is 0
    PA_HIP_TRY(hipSetDevice(q->device));
    const int e = setup_device(q, class_counts, ovf, overflow_words, overflow_words ? n_words : 0, (uint32_t)n_rows, (uint32_t)nnz, (double)reads / (double)T);
    if (e != PA_OK) return e;
    q->ready = true;
    return PA_OK;
}

int pa_quant_step(pa_quant* q, uint32_t n_iters) {
    if (!q) return fail(PA_ERR_INVALID_ARG, "null argument");
    if (!q->ready || n_iters == 0) return PA_OK;
    PA_HIP_TRY(hipSetDevice(q->device));
    for (uint32_t i = 0; i < n_iters; ++i) {
        const int e = launch_iteration(q, false);
        if (e != PA_OK) return e;
    }
    PA_HIP_TRY(hipStreamSynchronize(q->stream));
    q->stats[7] += n_iters;
    return PA_OK;
}

int pa_quant_run(pa_quant* q, uint32_t* iters, int* converged) {
    if (iters) *iters = 0;
    if (converged) *converged = 0;
    if (!q) return fail(PA_ERR_INVALID_ARG, "null argument");
    if (!q->ready) {   // no reads: nothing to iterate
        if (converged) *converged = 1;
        return PA_OK;
    }
    PA_HIP_TRY(hipSetDevice(q->device));
    const pa_quant_params& p = q->par;
    uint32_t done = 0;
    bool conv = false;
    while (done < p.max_iters && !conv) {
        const uint32_t i = done + 1;
        const bool check = (i >= p.min_iters && i % p.check_every == 0) || i == p.max_iters;
        if (check) PA_HIP_TRY(hipMemsetAsync(q->d_flag.get(), 0, 4, q->stream));
        const int e = launch_iteration(q, check);
        if (e != PA_OK) return e;
        done = i;
        if (check) {   // the flag comes back on the launches' own stream
            PA_HIP_TRY(hipMemcpyAsync(q->h_flag.get(), q->d_flag.get(), 4, hipMemcpyDeviceToHost, q->stream));
            PA_HIP_TRY(hipStreamSynchronize(q->stream));
            conv = *q->h_flag.get() == 0 && i >= p.min_iters;
        }
    }
    hipLaunchKernelGGL(quant_truncate, dim3(grid_for(q->num_tx)), dim3(256), 0, q->stream, q->num_tx, p.alpha_limit / 10.0, q->d_alpha.get(), q->d_w.get());
    PA_HIP_TRY(hipGetLastError());
    PA_HIP_TRY(hipStreamSynchronize(q->stream));
    q->stats[7] += done;
    if (iters) *iters = done;
    if (converged) *converged = conv ? 1 : 0;
    return PA_OK;
}

int pa_quant_alpha(const pa_quant* q, double* alpha) {
    if (!q || !alpha) return fail(PA_ERR_INVALID_ARG, "null argument");
    return alpha_to_host(q, alpha);
}

int pa_quant_fetch(const pa_quant* q, double* est_counts, double* tpm, double* eff_len) {
    if (!q) return fail(PA_ERR_INVALID_ARG, "null argument");
    if (eff_len) std::copy(q->eff.begin(), q->eff.end(), eff_len);
    if (!est_counts && !tpm) return PA_OK;
    std::vector<double> alpha(q->num_tx);
    const int e = alpha_to_host(q, alpha.data());
    if (e != PA_OK) return e;
    if (tpm) tpm_of(q, alpha.data(), tpm);
    if (est_counts) std::copy(alpha.begin(), alpha.end(), est_counts);
    return PA_OK;
}

int pa_quant_fetch_genes(const pa_quant* q, double* est_counts, double* tpm) {
    if (!q) return fail(PA_ERR_INVALID_ARG, "null argument");
    if (q->num_genes == 0) return PA_OK;   // an index without gene names: nothing to sum into
    std::vector<double> alpha(q->num_tx), t(q->num_tx);
    const int e = alpha_to_host(q, alpha.data());
    if (e != PA_OK) return e;
    tpm_of(q, alpha.data(), t.data());
    for (uint32_t g = 0; g < q->num_genes; ++g) {
        if (est_counts) est_counts[g] = 0.0;
        if (tpm) tpm[g] = 0.0;
    }
    for (uint32_t i = 0; i < q->num_tx; ++i) {   // transcript order
        if (q->tx_gene[i] >= q->num_genes) continue;
        if (est_counts) est_counts[q->tx_gene[i]] += alpha[i];
        if (tpm) tpm[q->tx_gene[i]] += t[i];
    }
    return PA_OK;
}

int pa_quant_stats(const pa_quant* q, uint64_t stats[PA_QUANT_STATS]) {
    if (!q || !stats) return fail(PA_ERR_INVALID_ARG, "null argument");
    for (int j = 0; j < PA_QUANT_STATS; ++j) stats[j] = q->stats[j];
    return PA_OK;
}

int pa_write_abundance_tsv(const pa_quant* q, const char* path) {
    if (!q || !path) return fail(PA_ERR_INVALID_ARG, "null argument");
    std::vector<double> alpha(q->num_tx), tpm(q->num_tx);
    const int e = alpha_to_host(q, alpha.data());
    if (e != PA_OK) return e;
    tpm_of(q, alpha.data(), tpm.data());
    FILE* f = fopen(path, "w");
    if (!f) return fail(PA_ERR_IO, "cannot write %s", path);
    fputs("target_id\tlength\teff_length\test_counts\ttpm\n", f);
    for (uint32_t t = 0; t < q->num_tx; ++t)
        fprintf(f, "%s\t%llu\t%s\t%s\t%s\n", q->names[t].c_str(), (unsigned long long)q->len[t], tsv_f64(q->eff[t]).c_str(), tsv_f64(alpha[t]).c_str(),
                tsv_f64(tpm[t]).c_str());
    if (fclose(f) != 0) return fail(PA_ERR_IO, "cannot write %s", path);
    return PA_OK;
}

void pa_quant_destroy(pa_quant* q) {
    if (!q) return;
    (void)hipSetDevice(q->device);
    if (q->stream) {
        (void)hipStreamSynchronize(q->stream);
        (void)hipStreamDestroy(q->stream);
    }
    delete q;
}

}  // extern "C"
