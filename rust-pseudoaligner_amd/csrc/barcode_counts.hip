// Two single-cell counters, both a radix sort of one 64-bit key per read followed by run-length encodes.
//
// 1. Per-barcode class counts (pa::barcode_counts) — SURVEY.md §8f.3, the use the reference was written for (README.md:3: a
//    pseudo-alignment tool for single-cell RNA-seq): every read carries the index of its cell barcode, and what downstream
//    wants is the SPARSE matrix (barcode, equivalence class) -> reads. The key is barcode << 32 | column, the columns being
//    those of the dense count table (class id, or novel / empty / unmapped); the result is the sorted unique keys with their
//    counts, ready for a CSR / triplet matrix on the host.
// 2. The UMI count matrix from barcode + UMI reads (pa_cell_counter, second half of the file): (cell, gene) -> molecules.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <memory>
#include <new>
#include <vector>

#include "device_prims.hpp"
#include "hip_buffer.hpp"
#include "kernel_utils.hpp"
#include "kernels.hpp"
#include "pa_common.hpp"

using namespace pa;

namespace {

__global__ __launch_bounds__(256) void pa_barcode_keys_kernel(const pa_read_result* __restrict__ results, const uint32_t* __restrict__ arena,
                                                              const uint32_t* __restrict__ barcode, uint64_t n_reads, const DevIndexView ix,
                                                              const uint32_t* __restrict__ class_table, uint64_t class_table_size,
                                                              unsigned long long* __restrict__ keys) {
    const uint32_t num_classes = ix.num_classes;
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_reads) return;
    const pa_read_result r = results[i];
    uint32_t col;
    if (!(r.mismatches & PA_MAPPED_BIT)) col = num_classes + 2;
    else if (r.class_len == 0) col = num_classes + 1;
    else {
        uint32_t c = (r.class_off & PA_CLASS_REF) ? (r.class_off & ~PA_CLASS_REF) : class_of_list(arena + r.class_off, r.class_len, ix, class_table, class_table_size);
        col = c == 0xFFFFFFFFu ? num_classes : c;
    }
    keys[i] = ((unsigned long long)barcode[i] << 32) | col;
}

}  // namespace

namespace pa {

// pa_counts_by_barcode_device (device_index.hip) hands over the pieces of the index this needs
int barcode_counts(const DevIndexView& ix, const uint32_t* class_table, uint64_t class_table_size, const pa_read_result* d_results,
                   const uint32_t* d_arena, const uint32_t* d_barcode, uint64_t n, uint32_t barcode_bits, uint64_t* d_keys, uint32_t* d_vals,
                   uint64_t* n_entries, hipStream_t stream) {
    *n_entries = 0;
    if (n == 0) return PA_OK;
    if (n > 0x7FFFFFFFull) return fail(PA_ERR_UNSUPPORTED, "at most 2^31-1 reads per call");
    DeviceBuffer<unsigned long long> keys_in, keys_sorted;
    DeviceBuffer<uint32_t> d_runs;
    DeviceBuffer<uint8_t> tmp;
    int e;
    if ((e = keys_in.alloc(n)) || (e = keys_sorted.alloc(n)) || (e = d_runs.alloc(1))) return e;
    hipLaunchKernelGGL(pa_barcode_keys_kernel, dim3(grid_for(n)), dim3(256), 0, stream, d_results, d_arena, d_barcode, n, ix, class_table, class_table_size,
                       keys_in.get());
    PA_HIP_TRY(hipGetLastError());
    // the column's 32 bits and the barcode's bits that can differ are sorted (the count as an int: 32-bit indexing, n < 2^31)
    const uint32_t end_bit = 32 + (barcode_bits ? (barcode_bits > 32 ? 32 : barcode_bits) : 32);
    uint32_t runs = 0;
    if ((e = sort_keys(stream, tmp, keys_in.get(), keys_sorted.get(), (int)n, 0, end_bit)) ||
        (e = run_length_encode(stream, tmp, keys_sorted.get(), n, (unsigned long long*)d_keys, d_vals, d_runs.get())) || (e = fetch_u32(d_runs.get(), stream, runs)))
        return e;
    *n_entries = runs;
    return PA_OK;
}

}  // namespace pa

// ---------------------------------------------------------------------------------------------------------------------------------
// Single-cell UMI count matrix (pa_cell_counter, include/pseudoaligner_amd.h). Every read becomes one 64-bit molecule key
// cell | gene | UMI (a sentinel above every valid key when it drops); a batch is radix-sorted over the key's used bits and
// run-length encoded into (key, reads) entries that are appended to an accumulator in HBM. finish() sorts and reduces the
// accumulator, corrects UMIs inside every (cell, gene) segment (a wave per segment: all pairs of up to 64 UMIs through lane
// shuffles; larger segments binary-search the 3 L neighbours of each UMI), re-keys as (cell, UMI, gene) to settle gene conflicts
// and re-keys as (cell, gene) for the count. DESIGN.md "Single-cell UMI counts".
// ---------------------------------------------------------------------------------------------------------------------------------
namespace {

constexpr uint32_t CELL_NONE = 0xFFFFFFFFu;         // no whitelist barcode / no gene
constexpr uint32_t CELL_GENE_MULTI = 0xFFFFFFFEu;    // a class whose transcripts span several genes
constexpr uint32_t CELL_BLOCK = 256;                 // 4 waves
constexpr uint32_t CELL_SMALL_SEGMENT = 64;          // UMIs of a (cell, gene) segment that one wave compares pairwise in registers
enum : uint32_t { ST_READS = 0, ST_EXACT, ST_CORRECTED, ST_BC_INVALID, ST_UMI_INVALID, ST_UNMAPPED, ST_COUNTED, ST_MOVED, ST_CONFLICT, ST_UMIS };

__host__ __device__ inline unsigned long long shl64(unsigned long long x, uint32_t s) { return s >= 64 ? 0ull : x << s; }
__host__ __device__ inline unsigned long long shr64(unsigned long long x, uint32_t s) { return s >= 64 ? 0ull : x >> s; }
__device__ inline uint32_t cell_base(uint8_t c) { return c == 'A' ? 0u : c == 'C' ? 1u : c == 'G' ? 2u : c == 'T' ? 3u : 4u; }
// two 2-bit codes words at Hamming distance 1: exactly one base differs
__device__ inline bool hamming1(uint32_t x) { return __popc((x | (x >> 1)) & 0x55555555u) == 1; }

// whitelist table: open addressing, linear probing from pa_mix64(barcode), slot = barcode << 32 | line, empty = ~0 (a line is < 2^31)
__device__ inline uint32_t wl_probe(const unsigned long long* __restrict__ slots, uint64_t mask, uint32_t bc) {
    for (uint64_t j = pa_mix64(bc) & mask;; j = (j + 1) & mask) {
        const unsigned long long s = slots[j];
        if (s == ~0ull) return CELL_NONE;
        if ((uint32_t)(s >> 32) == bc) return (uint32_t)s;
    }
}

struct CellKeyParams {
    const pa_read_result* results;
    const uint32_t* arena;
    const uint8_t* r1;
    const uint64_t* r1_off;
    uint64_t n;
    const unsigned long long* wl;
    uint64_t wl_mask;
    const uint32_t* class_gene;   // [num_classes]: gene of an index class, CELL_NONE (empty) or CELL_GENE_MULTI
    uint32_t num_classes;
    const uint32_t* tx_gene;
    uint32_t num_tx;
    uint32_t bc_len, umi_len, cell_shift;   // key = cell << cell_shift | gene << 2 umi_len | UMI
    unsigned long long sentinel;
    unsigned long long* keys;
    unsigned long long* stats;
};

// the gene of a mapped read: CELL_NONE when unmapped or empty, CELL_GENE_MULTI when its class spans several genes
__device__ inline uint32_t read_gene(const CellKeyParams& p, const pa_read_result r) {
    if (!(r.mismatches & PA_MAPPED_BIT) || r.class_len == 0) return CELL_NONE;
    if (r.class_off & PA_CLASS_REF) {
        const uint32_t c = r.class_off & ~PA_CLASS_REF;
        return c < p.num_classes ? p.class_gene[c] : CELL_GENE_MULTI;
    }
    const uint32_t* ids = p.arena + r.class_off;
    uint32_t g = CELL_NONE;
    for (uint32_t j = 0; j < r.class_len; ++j) {
        const uint32_t t = ids[j];
        const uint32_t gj = t < p.num_tx ? p.tx_gene[t] : CELL_GENE_MULTI;
        if (j == 0) g = gj;
        else if (gj != g) return CELL_GENE_MULTI;
    }
    return g;
}

// one lane per read: barcode correction against the whitelist table, UMI, gene -> molecule key; fate counts summed per wave
__global__ __launch_bounds__(CELL_BLOCK) void pa_cell_keys_kernel(const CellKeyParams p) {
    const uint64_t i = (uint64_t)blockIdx.x * CELL_BLOCK + threadIdx.x;
    bool exact = false, corrected = false, bc_invalid = false, umi_invalid = false, unmapped = false, counted = false;
    if (i < p.n) {
        const uint64_t off = p.r1_off[i];
        const uint64_t len = p.r1_off[i + 1] - off;
        unsigned long long key = p.sentinel;
        uint32_t cell = CELL_NONE;
        if (len >= (uint64_t)p.bc_len + p.umi_len) {
            uint32_t bc = 0, n_count = 0, n_pos = 0;
            for (uint32_t j = 0; j < p.bc_len; ++j) {
                uint32_t b = cell_base(p.r1[off + j]);
                if (b > 3) { ++n_count; n_pos = j; b = 0; }
                bc = (bc << 2) | b;
            }
            if (n_count == 0) cell = wl_probe(p.wl, p.wl_mask, bc);
            if (cell != CELL_NONE) exact = true;
            else if (n_count <= 1) {   // the unique whitelisted single substitution (any position; or the N's position)
                uint32_t hits = 0, hit = CELL_NONE;
                const uint32_t first = n_count ? n_pos : 0, last = n_count ? n_pos + 1 : p.bc_len;
                for (uint32_t pos = first; pos < last && hits < 2; ++pos) {
                    const uint32_t sh = 2 * (p.bc_len - 1 - pos);
                    const uint32_t cur = (bc >> sh) & 3u;
                    for (uint32_t b = 0; b < 4 && hits < 2; ++b) {
                        if (n_count == 0 && b == cur) continue;
                        const uint32_t c = wl_probe(p.wl, p.wl_mask, (bc & ~(3u << sh)) | (b << sh));
                        if (c != CELL_NONE) { ++hits; hit = c; }
                    }
                }
                if (hits == 1) { cell = hit; corrected = true; }
            }
        }
        if (cell == CELL_NONE) bc_invalid = true;
        else {
            uint32_t umi = 0, bad = 0;
            for (uint32_t j = 0; j < p.umi_len; ++j) {
                const uint32_t b = cell_base(p.r1[off + p.bc_len + j]);
                bad |= b >> 2;
                umi = (umi << 2) | (b & 3u);
            }
            if (bad) umi_invalid = true;
            else {
                const uint32_t g = read_gene(p, p.results[i]);
                if (g >= CELL_GENE_MULTI) unmapped = true;
                else {
                    counted = true;
                    key = shl64(cell, p.cell_shift) | ((unsigned long long)g << (2 * p.umi_len)) | umi;
                }
            }
        }
        p.keys[i] = key;
    }
    // one atomic per wave and fate (wave64: 64-bit ballots)
    const bool fates[7] = {i < p.n, exact, corrected, bc_invalid, umi_invalid, unmapped, counted};
    for (int f = 0; f < 7; ++f) {
        const unsigned long long m = __ballot(fates[f]);
        if ((threadIdx.x & 63) == 0 && m) atomicAdd(p.stats + f, (unsigned long long)__popcll(m));
    }
}

// the (cell, gene) part of a key
__global__ __launch_bounds__(CELL_BLOCK) void pa_cell_segment_kernel(const unsigned long long* __restrict__ keys, uint64_t n, uint32_t umi_bits,
                                                                      unsigned long long* __restrict__ seg) {
    const uint64_t i = (uint64_t)blockIdx.x * CELL_BLOCK + threadIdx.x;
    if (i < n) seg[i] = keys[i] >> umi_bits;
}

// UMI correction, one wave per (cell, gene) segment: every UMI u moves to the greatest of {u} and its Hamming-1 neighbours in the
// segment under (reads, UMI value). Writes the re-keyed molecule cell | corrected UMI | gene.
__global__ __launch_bounds__(CELL_BLOCK) void pa_cell_umi_correct_kernel(const unsigned long long* __restrict__ keys, const uint32_t* __restrict__ reads,
                                                                          const uint32_t* __restrict__ seg_start, uint32_t n_segs, uint32_t umi_len,
                                                                          uint32_t gene_bits, uint32_t cell_shift, unsigned long long* __restrict__ key2,
                                                                          unsigned long long* __restrict__ stats) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t nwaves = gridDim.x * (CELL_BLOCK / 64);
    const uint32_t umi_bits = 2 * umi_len;
    const uint32_t umask = (uint32_t)low_mask(umi_bits);
    const unsigned long long gmask = low_mask(gene_bits);
    uint32_t moved = 0;
    auto rekey = [&](unsigned long long k, uint32_t tgt) {
        return shl64(shr64(k, cell_shift), cell_shift) | ((unsigned long long)tgt << gene_bits) | ((k >> umi_bits) & gmask);
    };
    for (uint32_t s = (blockIdx.x * CELL_BLOCK + threadIdx.x) >> 6; s < n_segs; s += nwaves) {   // (uniform per wave)
        const uint32_t a = seg_start[s], b = seg_start[s + 1];
        const uint32_t size = b - a;
        if (size <= CELL_SMALL_SEGMENT) {
            const bool have = lane < size;
            const unsigned long long k = have ? keys[a + lane] : 0ull;
            const uint32_t u = (uint32_t)k & umask;
            const uint32_t n = have ? reads[a + lane] : 0u;
            uint32_t bu = u, bn = n;
            for (uint32_t j = 0; j < size; ++j) {
                const uint32_t uj = (uint32_t)__shfl((int)u, (int)j, 64);
                const uint32_t nj = (uint32_t)__shfl((int)n, (int)j, 64);
                if (hamming1(u ^ uj) && (nj > bn || (nj == bn && uj > bu))) { bu = uj; bn = nj; }
            }
            if (have) {
                key2[a + lane] = rekey(k, bu);
                moved += bu != u;
            }
        } else {   // large segment: the 3 L neighbours of each UMI by binary search in the sorted segment
            for (uint32_t i = a + lane; i < b; i += 64) {
                const unsigned long long k = keys[i];
                const uint32_t u = (uint32_t)k & umask;
                const unsigned long long prefix = k & ~(unsigned long long)umask;
                uint32_t bu = u, bn = reads[i];
                for (uint32_t pos = 0; pos < umi_len; ++pos) {
                    const uint32_t sh = 2 * pos;
                    const uint32_t cur = (u >> sh) & 3u;
                    for (uint32_t base = 0; base < 4; ++base) {
                        if (base == cur) continue;
                        const uint32_t v = (u & ~(3u << sh)) | (base << sh);
                        const unsigned long long want = prefix | v;
                        uint32_t lo = a, hi = b;
                        while (lo < hi) {
                            const uint32_t mid = lo + (hi - lo) / 2;
                            if (keys[mid] < want) lo = mid + 1;
                            else hi = mid;
                        }
                        if (lo < b && keys[lo] == want) {
                            const uint32_t nj = reads[lo];
                            if (nj > bn || (nj == bn && v > bu)) { bu = v; bn = nj; }
                        }
                    }
                }
                key2[i] = rekey(k, bu);
                moved += bu != u;
            }
        }
    }
    // one atomic per wave
    for (int o = 32; o > 0; o >>= 1) moved += (uint32_t)__shfl_xor((int)moved, o, 64);
    if (lane == 0 && moved) atomicAdd(stats + ST_MOVED, (unsigned long long)moved);
}

// gene conflicts over (cell, UMI, gene) molecules sorted by that key: a molecule survives when its reads strictly exceed those of
// every other gene of its (cell, UMI); survivors are re-keyed as cell | gene, the others get the sentinel
__global__ __launch_bounds__(CELL_BLOCK) void pa_cell_conflict_kernel(const unsigned long long* __restrict__ key2, const uint32_t* __restrict__ reads,
                                                                       uint64_t n, uint32_t gene_bits, uint32_t cell_shift, unsigned long long sentinel,
                                                                       unsigned long long* __restrict__ key3, unsigned long long* __restrict__ stats) {
    const uint64_t i = (uint64_t)blockIdx.x * CELL_BLOCK + threadIdx.x;
    bool lost = false;
    if (i < n) {
        const unsigned long long k = key2[i];
        const unsigned long long seg = k >> gene_bits;
        const uint32_t r = reads[i];
        uint32_t other = 0;
        for (uint64_t j = i; j > 0 && (key2[j - 1] >> gene_bits) == seg; --j) other = max(other, reads[j - 1]);
        for (uint64_t j = i + 1; j < n && (key2[j] >> gene_bits) == seg; ++j) other = max(other, reads[j]);
        lost = r <= other;
        key3[i] = lost ? sentinel : (shl64(shr64(k, cell_shift), gene_bits) | (k & low_mask(gene_bits)));
    }
    const unsigned long long m = __ballot(lost);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(stats + ST_CONFLICT, (unsigned long long)__popcll(m));
}

}  // namespace

struct pa_cell_counter {
    int device = 0;
    uint32_t bc_len = 0, umi_len = 0, num_genes = 0, num_classes = 0, num_tx = 0;
    uint32_t cell_bits = 0, gene_bits = 0;
    uint64_t n_whitelist = 0, wl_mask = 0;
    DeviceBuffer<unsigned long long> d_wl;
    DeviceBuffer<uint32_t> d_class_gene, d_tx_gene;
    DeviceBuffer<unsigned long long> d_stats;
    // (key, reads) entries of every batch so far, unsorted across batches
    DeviceBuffer<unsigned long long> acc_keys;
    DeviceBuffer<uint32_t> acc_reads;
    uint64_t acc_n = 0;
    bool finished = false;
    uint64_t stats[PA_CELL_STATS] = {};
    std::vector<uint32_t> m_cell, m_gene, m_umis;   // the matrix after finish
    uint32_t key_bits() const { return cell_bits + gene_bits + 2 * umi_len; }
};

namespace {

int fetch_stats(pa_cell_counter* c, hipStream_t stream) {
    unsigned long long d[PA_CELL_STATS];
    PA_HIP_TRY(hipMemcpyAsync(d, c->d_stats.get(), sizeof d, hipMemcpyDeviceToHost, stream));
    PA_HIP_TRY(hipStreamSynchronize(stream));
    for (int j = 0; j < ST_UMIS; ++j) c->stats[j] = d[j];
    return PA_OK;
}

}  // namespace

extern "C" {

int pa_cell_counter_create(pa_index* idx, const pa_host_index* h, const uint32_t* tx_gene, uint32_t num_genes, const char* whitelist,
                           uint64_t n_whitelist, uint32_t bc_len, uint32_t umi_len, pa_cell_counter** out) {
    if (out) *out = nullptr;
    if (!idx || !h || !tx_gene || !whitelist || !out) return fail(PA_ERR_INVALID_ARG, "null argument");
    if (bc_len < 1 || bc_len > 16 || umi_len < 1 || umi_len > 16) return fail(PA_ERR_INVALID_ARG, "barcode length %u / UMI length %u: both must be 1..16", bc_len, umi_len);
    if (num_genes < 1 || num_genes >= CELL_GENE_MULTI) return fail(PA_ERR_INVALID_ARG, "num_genes %u out of range", num_genes);
    if (n_whitelist < 1 || n_whitelist > 0x7FFFFFFFull) return fail(PA_ERR_INVALID_ARG, "whitelist of %llu barcodes: 1 .. 2^31-1", (unsigned long long)n_whitelist);
    const HostIndex& hi = h->h;
    const uint32_t num_tx = hi.num_transcripts;
    const uint32_t num_classes = hi.ec_offset.empty() ? 0 : (uint32_t)(hi.ec_offset.size() - 1);
    for (uint32_t t = 0; t < num_tx; ++t)
        if (tx_gene[t] >= num_genes) return fail(PA_ERR_INVALID_ARG, "tx_gene[%u] = %u is not below num_genes %u", t, tx_gene[t], num_genes);
    const uint32_t cell_bits = bits_for(n_whitelist - 1), gene_bits = bits_for(num_genes - 1);
    if (cell_bits + gene_bits + 2 * umi_len > 64)
        return fail(PA_ERR_UNSUPPORTED, "molecule key of %u cell + %u gene + %u UMI bits exceeds 64", cell_bits, gene_bits, 2 * umi_len);
    // the whitelist table (host build), capacity a power of two at load <= 0.5
    uint64_t cap = 2;
    while (cap < 2 * n_whitelist) cap <<= 1;
    std::vector<unsigned long long> wl(cap, ~0ull);
    for (uint64_t line = 0; line < n_whitelist; ++line) {
        uint32_t bc = 0;
        for (uint32_t j = 0; j < bc_len; ++j) {
            const char ch = whitelist[line * bc_len + j];
            const uint32_t b = ch == 'A' ? 0u : ch == 'C' ? 1u : ch == 'G' ? 2u : ch == 'T' ? 3u : 4u;
            if (b > 3) return fail(PA_ERR_INVALID_ARG, "whitelist barcode %llu: byte %u is not A, C, G or T", (unsigned long long)line, j);
            bc = (bc << 2) | b;
        }
        uint64_t j = pa_mix64(bc) & (cap - 1);
        while (wl[j] != ~0ull) {
            if ((uint32_t)(wl[j] >> 32) == bc) return fail(PA_ERR_INVALID_ARG, "whitelist barcode %llu repeats barcode %u", (unsigned long long)line, (uint32_t)wl[j]);
            j = (j + 1) & (cap - 1);
        }
        wl[j] = ((unsigned long long)bc << 32) | line;
    }
    // the gene of every index class (one gene, empty, or several)
    std::vector<uint32_t> class_gene(num_classes ? num_classes : 1, CELL_NONE);
    for (uint32_t c = 0; c < num_classes; ++c) {
        uint32_t g = CELL_NONE;
        for (uint64_t j = hi.ec_offset[c]; j < hi.ec_offset[c + 1]; ++j) {
            const uint32_t t = hi.ec_ids[j];
            const uint32_t gj = t < num_tx ? tx_gene[t] : CELL_GENE_MULTI;
            if (j == hi.ec_offset[c]) g = gj;
            else if (gj != g) { g = CELL_GENE_MULTI; break; }
        }
        class_gene[c] = g;
    }
    // the device side (the index's device)
    pa_index_stats ist{};
    int e = pa_index_get_stats(idx, &ist);
    if (e != PA_OK) return e;
    if (ist.num_classes != num_classes) return fail(PA_ERR_INVALID_ARG, "host index has %u classes, the device index %u: not the index it was made from", num_classes, ist.num_classes);
    const uint32_t *h_ec = nullptr, *h_ref = nullptr;
    int device = 0;
    index_host_classes(idx, &h_ec, &h_ref, &device);
    PA_HIP_TRY(hipSetDevice(device));
    std::unique_ptr<pa_cell_counter> c(new (std::nothrow) pa_cell_counter());
    if (!c) return fail(PA_ERR_OOM, "out of host memory");
    c->device = device;
    c->bc_len = bc_len; c->umi_len = umi_len; c->num_genes = num_genes; c->num_classes = num_classes; c->num_tx = num_tx;
    c->cell_bits = cell_bits; c->gene_bits = gene_bits; c->n_whitelist = n_whitelist; c->wl_mask = cap - 1;
    if ((e = c->d_wl.alloc(cap)) || (e = c->d_class_gene.alloc(class_gene.size())) || (e = c->d_tx_gene.alloc(num_tx ? num_tx : 1)) ||
        (e = c->d_stats.alloc(PA_CELL_STATS)))
        return e;
    PA_HIP_TRY(hipMemcpy(c->d_wl.get(), wl.data(), cap * 8, hipMemcpyHostToDevice));
    PA_HIP_TRY(hipMemcpy(c->d_class_gene.get(), class_gene.data(), class_gene.size() * 4, hipMemcpyHostToDevice));
    if (num_tx) PA_HIP_TRY(hipMemcpy(c->d_tx_gene.get(), tx_gene, num_tx * 4ull, hipMemcpyHostToDevice));
    PA_HIP_TRY(hipMemset(c->d_stats.get(), 0, PA_CELL_STATS * 8));
    *out = c.release();
    return PA_OK;
}

int pa_cell_counter_add_device(pa_cell_counter* c, const pa_read_result* d_results, const uint32_t* d_arena, const uint8_t* d_r1,
                               const uint64_t* d_r1_offsets, uint64_t n_reads, void* stream) {
    if (!c || (n_reads && (!d_results || !d_arena || !d_r1 || !d_r1_offsets))) return fail(PA_ERR_INVALID_ARG, "null argument");
    if (c->finished) return fail(PA_ERR_INVALID_ARG, "the counter is finished: no batches after pa_cell_counter_finish");
    if (n_reads > 0x7FFFFFFFull) return fail(PA_ERR_UNSUPPORTED, "at most 2^31-1 reads per batch");
    if (n_reads == 0) return PA_OK;
    PA_HIP_TRY(hipSetDevice(c->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    DeviceBuffer<unsigned long long> keys, sorted;
    DeviceBuffer<uint32_t> d_runs;
    DeviceBuffer<uint8_t> tmp;
    int e;
    if ((e = keys.alloc(n_reads)) || (e = sorted.alloc(n_reads)) || (e = d_runs.alloc(1))) return e;
    const uint32_t end_bit = std::max(1u, c->key_bits());
    CellKeyParams p;
    p.results = d_results; p.arena = d_arena; p.r1 = d_r1; p.r1_off = d_r1_offsets; p.n = n_reads;
    p.wl = c->d_wl.get(); p.wl_mask = c->wl_mask;
    p.class_gene = c->d_class_gene.get(); p.num_classes = c->num_classes; p.tx_gene = c->d_tx_gene.get(); p.num_tx = c->num_tx;
    p.bc_len = c->bc_len; p.umi_len = c->umi_len; p.cell_shift = c->gene_bits + 2 * c->umi_len;
    p.sentinel = low_mask(end_bit);   // >= every valid key: the dropped reads sort behind the counted ones
    p.keys = keys.get(); p.stats = c->d_stats.get();
    const uint64_t counted_before = c->stats[ST_COUNTED];
    hipLaunchKernelGGL(pa_cell_keys_kernel, dim3(grid_for(n_reads, CELL_BLOCK)), dim3(CELL_BLOCK), 0, s, p);
    PA_HIP_TRY(hipGetLastError());
    if ((e = fetch_stats(c, s)) != PA_OK) return e;
    const uint64_t counted = c->stats[ST_COUNTED] - counted_before;
    if (counted == 0) return PA_OK;
    if (c->acc_n + counted > 0x7FFFFFFFull) return fail(PA_ERR_UNSUPPORTED, "more than 2^31-1 distinct molecule entries");
    if (c->acc_n + counted > c->acc_keys.size()) {   // grow the accumulator (doubling), keeping what it holds
        const uint64_t want = std::max<uint64_t>(c->acc_n + counted, 2 * c->acc_keys.size());
        DeviceBuffer<unsigned long long> nk;
        DeviceBuffer<uint32_t> nr;
        if ((e = nk.alloc(want)) || (e = nr.alloc(want))) return e;
        if (c->acc_n) {
            PA_HIP_TRY(hipMemcpyAsync(nk.get(), c->acc_keys.get(), c->acc_n * 8, hipMemcpyDeviceToDevice, s));
            PA_HIP_TRY(hipMemcpyAsync(nr.get(), c->acc_reads.get(), c->acc_n * 4, hipMemcpyDeviceToDevice, s));
        }
        c->acc_keys = std::move(nk);
        c->acc_reads = std::move(nr);
    }
    // only the key's used bits are sorted; the counted reads are the first `counted` sorted keys
    uint32_t runs = 0;
    if ((e = sort_keys(s, tmp, keys.get(), sorted.get(), (int)n_reads, 0, end_bit)) ||
        (e = run_length_encode(s, tmp, sorted.get(), counted, c->acc_keys.get() + c->acc_n, c->acc_reads.get() + c->acc_n, d_runs.get())) ||
        (e = fetch_u32(d_runs.get(), s, runs)))
        return e;
    c->acc_n += runs;
    return PA_OK;
}

int pa_cell_counter_finish(pa_cell_counter* c, uint64_t* n_entries) {
    if (!c || !n_entries) return fail(PA_ERR_INVALID_ARG, "null argument");
    if (c->finished) { *n_entries = c->m_cell.size(); return PA_OK; }
    *n_entries = 0;
    PA_HIP_TRY(hipSetDevice(c->device));
    hipStream_t s = nullptr;
    const uint64_t M0 = c->acc_n;
    const uint32_t umi_bits = 2 * c->umi_len, cell_shift = c->gene_bits + umi_bits;
    const uint32_t end_bit = std::max(1u, c->key_bits());
    const uint32_t end_bit3 = std::max(1u, c->cell_bits + c->gene_bits);
    int e = PA_OK;
    if (M0) {
        DeviceBuffer<unsigned long long> k1, k2, seg, seg_u;
        DeviceBuffer<uint32_t> r1, r2, seg_n, seg_start;
        DeviceBuffer<uint32_t> d_cnt;
        DeviceBuffer<uint8_t> tmp;
        if ((e = k1.alloc(M0)) || (e = k2.alloc(M0)) || (e = r1.alloc(M0)) || (e = r2.alloc(M0)) || (e = d_cnt.alloc(1))) return e;
        uint32_t cnt = 0;
        // 1. every batch's entries together: sort by key, sum the reads of equal keys -> (k2, r2)[M]   (sort counts as int: 32-bit indexing)
        if ((e = sort_pairs(s, tmp, c->acc_keys.get(), k1.get(), c->acc_reads.get(), r1.get(), (int)M0, 0, end_bit)) ||
            (e = reduce_by_key_sum(s, tmp, k1.get(), r1.get(), M0, k2.get(), r2.get(), d_cnt.get())) || (e = fetch_u32(d_cnt.get(), s, cnt)))
            return e;
        const uint64_t M = cnt;
        c->acc_keys.release();
        c->acc_reads.release();
        // 2. (cell, gene) segments: their sizes, then their starts seg_start[0 .. segs]
        if ((e = seg.alloc(M)) || (e = seg_u.alloc(M)) || (e = seg_n.alloc(M)) || (e = seg_start.alloc(M + 1))) return e;
        hipLaunchKernelGGL(pa_cell_segment_kernel, dim3(grid_for(M, CELL_BLOCK)), dim3(CELL_BLOCK), 0, s, k2.get(), M, umi_bits, seg.get());
        PA_HIP_TRY(hipGetLastError());
        if ((e = run_length_encode(s, tmp, seg.get(), M, seg_u.get(), seg_n.get(), d_cnt.get())) || (e = fetch_u32(d_cnt.get(), s, cnt))) return e;
        const uint32_t segs = cnt;
        PA_HIP_TRY(hipMemsetAsync(seg_start.get(), 0, 4, s));
        if ((e = scan_inclusive(s, tmp, seg_n.get(), seg_start.get() + 1, segs))) return e;
        seg.release(); seg_u.release(); seg_n.release();
        // 3. UMI correction -> (cell, corrected UMI, gene) molecules in k1 (reads r2)
        {
            int cus = 0;
            PA_HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->device));
            const uint32_t blocks = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((segs + 3) / 4, (uint64_t)std::max(cus, 1) * 32));
            hipLaunchKernelGGL(pa_cell_umi_correct_kernel, dim3(blocks), dim3(CELL_BLOCK), 0, s, k2.get(), r2.get(), seg_start.get(), segs, c->umi_len,
                               c->gene_bits, cell_shift, k1.get(), c->d_stats.get());
            PA_HIP_TRY(hipGetLastError());
        }
        seg_start.release();
        // 4. molecules that moved onto one UMI join: sort, sum -> (k1, r1)[M2]
        if ((e = sort_pairs(s, tmp, k1.get(), k2.get(), r2.get(), r1.get(), (int)M, 0, end_bit)) ||
            (e = reduce_by_key_sum(s, tmp, k2.get(), r1.get(), M, k1.get(), r2.get(), d_cnt.get())) || (e = fetch_u32(d_cnt.get(), s, cnt)))
            return e;
        const uint64_t M2 = cnt;
        // 5. gene conflicts per (cell, UMI): survivors re-keyed cell | gene in k2, the rest get the sentinel
        const unsigned long long sentinel3 = low_mask(end_bit3);
        const uint64_t lost_before = c->stats[ST_CONFLICT];
        hipLaunchKernelGGL(pa_cell_conflict_kernel, dim3(grid_for(M2, CELL_BLOCK)), dim3(CELL_BLOCK), 0, s, k1.get(), r2.get(), M2, c->gene_bits, cell_shift, sentinel3,
                           k2.get(), c->d_stats.get());
        PA_HIP_TRY(hipGetLastError());
        if ((e = fetch_stats(c, s)) != PA_OK) return e;
        const uint64_t kept = M2 - (c->stats[ST_CONFLICT] - lost_before);
        // 6. UMIs per (cell, gene): sort the survivors, run-length encode
        if (kept) {
            if ((e = sort_keys(s, tmp, k2.get(), k1.get(), (int)M2, 0, end_bit3)) || (e = run_length_encode(s, tmp, k1.get(), kept, k2.get(), r1.get(), d_cnt.get())) ||
                (e = fetch_u32(d_cnt.get(), s, cnt)))
                return e;
            const uint64_t entries = cnt;
            std::vector<unsigned long long> hk(entries);
            c->m_umis.resize(entries);
            PA_HIP_TRY(hipMemcpyAsync(hk.data(), k2.get(), entries * 8, hipMemcpyDeviceToHost, s));
            PA_HIP_TRY(hipMemcpyAsync(c->m_umis.data(), r1.get(), entries * 4, hipMemcpyDeviceToHost, s));
            PA_HIP_TRY(hipStreamSynchronize(s));
            c->m_cell.resize(entries);
            c->m_gene.resize(entries);
            const unsigned long long gmask = low_mask(c->gene_bits);
            for (uint64_t i = 0; i < entries; ++i) {
                c->m_cell[i] = (uint32_t)shr64(hk[i], c->gene_bits);
                c->m_gene[i] = (uint32_t)(hk[i] & gmask);
            }
        }
    }
    uint64_t umis = 0;
    for (const uint32_t u : c->m_umis) umis += u;
    c->stats[ST_UMIS] = umis;
    c->finished = true;
    *n_entries = c->m_cell.size();
    return PA_OK;
}

int pa_cell_counter_matrix(const pa_cell_counter* c, uint32_t* cell, uint32_t* gene, uint32_t* umis, uint64_t cap) {
    if (!c) return fail(PA_ERR_INVALID_ARG, "null argument");
    if (!c->finished) return fail(PA_ERR_INVALID_ARG, "the matrix exists after pa_cell_counter_finish");
    const uint64_t n = c->m_cell.size();
    if (cap < n) return fail(PA_ERR_BUFFER_TOO_SMALL, "the matrix has %llu entries, room for %llu", (unsigned long long)n, (unsigned long long)cap);
    if (n && (!cell || !gene || !umis)) return fail(PA_ERR_INVALID_ARG, "null argument");
    if (n) {
        memcpy(cell, c->m_cell.data(), n * 4);
        memcpy(gene, c->m_gene.data(), n * 4);
        memcpy(umis, c->m_umis.data(), n * 4);
    }
    return PA_OK;
}

int pa_cell_counter_stats(const pa_cell_counter* c, uint64_t stats[PA_CELL_STATS]) {
    if (!c || !stats) return fail(PA_ERR_INVALID_ARG, "null argument");
    memcpy(stats, c->stats, sizeof c->stats);
    return PA_OK;
}

void pa_cell_counter_destroy(pa_cell_counter* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    delete c;
}

}  // extern "C"
