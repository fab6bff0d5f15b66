// The abundance object (pa_quant) and the row / slot layout that csrc/quant.hip builds and csrc/quant_boot.hip reads.
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "hip_buffer.hpp"
#include "pa_common.hpp"

namespace pa {

constexpr int QB = 256;     // threads of a block
constexpr int NBIN = 5;
// bin k holds the rows of at least bin_min_len(k) entries that are in no earlier bin; a row of bin k is summed by bin_group(k) lanes
__host__ __device__ constexpr uint32_t bin_min_len(int k) { return k == 0 ? 1025u : k == 1 ? 17u : k == 2 ? 9u : k == 3 ? 5u : 1u; }
constexpr uint32_t bin_group(int k) { return k == 0 ? 256u : k == 1 ? 64u : k == 2 ? 16u : k == 3 ? 8u : 4u; }

struct Layout {
    uint32_t begin[NBIN + 1];   // rows [begin[k], begin[k + 1]) are bin k; begin[NBIN] = rows with at least one entry
    uint32_t blk[NBIN + 1];     // blocks [blk[k], blk[k + 1]) serve bin k
};

// The bootstrap batch of a pa_quant (csrc/quant_boot.hip): extra buffers only. The candidate-order tables are made on the first draw after
// a pa_quant_set_counts and serve every batch of that table; the per-replicate arrays are replicate-innermost with a stride of
// `stride` (the batch size rounded up to a power of two, at least 4).
struct QuantBoot {
    bool tables = false;                      // cum / cand_row hold the current table
    uint32_t n = 0, stride = 0;               // n = 0: no batch drawn
    DeviceBuffer<unsigned long long> d_cum;   // [rows + 1] reads before the i-th row in candidate order; d_cum[rows] = N
    DeviceBuffer<uint32_t> d_cand_row;        // [rows] the i-th row in candidate order
    DeviceBuffer<uint32_t> d_n;               // [rows][stride] resampled counts
    DeviceBuffer<double> d_q, d_alpha, d_w;   // [rows][stride], [T][stride], [T][stride]
    DeviceBuffer<uint32_t> d_mask;            // [2][64]: replicate b < n, replicate still iterating (pa_quant_bootstrap_run)
    DeviceBuffer<uint32_t> d_flag, d_col;     // [64] change flags of a checked iteration; [rows] one replicate's counts
    PinnedBuffer<uint32_t> h_flag, h_mask;    // [64], [2][64]
    std::vector<uint32_t> row_cand;           // host copy of d_row_cand (pa_quant_bootstrap_counts)
    void drop() {
        tables = false;
        n = 0;
        d_cum.release(); d_cand_row.release(); d_n.release(); d_q.release(); d_alpha.release(); d_w.release(); d_col.release();
        row_cand.clear();
    }
};

}  // namespace pa

struct pa_quant {
    int device = 0;
    hipStream_t stream = nullptr;
    pa_quant_params par{};
    uint32_t num_tx = 0, num_classes = 0, num_genes = 0;
    std::vector<double> eff;
    std::vector<uint64_t> len;
    std::vector<uint32_t> class_len, tx_gene;
    std::vector<std::string> names;
    // the index classes and the effective lengths, uploaded once
    pa::DeviceBuffer<unsigned long long> d_ec_off;
    pa::DeviceBuffer<uint32_t> d_ec_ids;
    pa::DeviceBuffer<double> d_eff;
    // the reduced problem of the last set_counts (ready: there is one, with at least one read)
    bool ready = false;
    pa::Layout rows{}, slots{};
    pa::DeviceBuffer<uint32_t> d_row_off, d_row_ids, d_tx_off, d_tx_rows, d_tx_order;
    pa::DeviceBuffer<uint32_t> d_row_cand;    // [rows] candidate of a row: class c, or num_classes + overflow record
    uint32_t n_records = 0;                   // overflow records of the last set_counts
    pa::DeviceBuffer<double> d_row_cnt, d_q, d_alpha, d_w;
    pa::DeviceBuffer<unsigned int> d_flag;
    pa::PinnedBuffer<unsigned int> h_flag;
    uint64_t stats[PA_QUANT_STATS] = {};
    pa::QuantBoot boot;
};
