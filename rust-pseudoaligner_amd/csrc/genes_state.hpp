// The gene counter (pa_genes) as csrc/genes.hip builds it: the thresholds of its kernels and the per-cell layout in HBM.
// (GN_BLOCK and GN_LANE_RECORDS are the molecule stage's, csrc/molecule_stage.hpp, which csrc/bus_umi.hip runs too.)
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

#include "hip_buffer.hpp"
#include "pa_common.hpp"

namespace pa {

constexpr uint32_t GN_BLOCK = 256;          // threads of a block (4 waves)
constexpr uint32_t GN_LANE_RECORDS = 4;     // a molecule of up to this many records is intersected by one lane, a longer one by a wave
constexpr uint32_t GN_WAVE_CELLS = 4;       // cells of the wave bin that share a block
constexpr uint32_t GN_WAVE_MAX = 512;       // a cell of |E| + rows up to this: one wave, alpha and q in the block's LDS (4 x 4 KiB)
constexpr uint32_t GN_LDS_CAP = 8192;       // a cell of |E| + rows up to this: one block, alpha and q in LDS (64 KiB: two blocks share a CU's 160 KiB); above: in HBM

}  // namespace pa

struct pa_genes {
    typedef unsigned long long ull;
    int device = 0;
    hipStream_t stream = nullptr;
    pa_genes_params par{};
    uint32_t bc_len = 0, umi_len = 0, num_genes = 0;
    uint64_t stats[PA_GENES_STATS] = {};
    bool ran = false;
    // sizes (the counts the host reads back)
    uint32_t n_cells = 0, n_su = 0, n_rows = 0, n_slots = 0, n_multi_cells = 0, n_hbm = 0, n_block = 0;
    uint64_t nnz = 0, n_values = 0;
    // cells
    pa::DeviceBuffer<ull> d_barcode;                  // [n_cells]
    pa::DeviceBuffer<uint32_t> d_iters, d_notconv;    // [n_cells]
    // singleton rows: distinct (cell << 32 | gene) ascending, their molecule counts as f64, 1 where the gene is also in E
    pa::DeviceBuffer<ull> d_su_key;
    pa::DeviceBuffer<double> d_su_val;
    pa::DeviceBuffer<uint32_t> d_su_in_e;
    // multi rows, numbered over all cells (a cell's rows are consecutive, ordered by content hash)
    pa::DeviceBuffer<uint32_t> d_cell_row;            // [n_cells + 1]
    pa::DeviceBuffer<ull> d_row_ptr;                  // [n_rows + 1] into d_row_slot
    pa::DeviceBuffer<uint32_t> d_row_slot;            // [nnz] the slot (global gene number) of every entry
    pa::DeviceBuffer<uint32_t> d_row_n;               // [n_rows] n_S
    // slots: the (cell, gene) pairs of E over all cells, ascending; transposed incidence
    pa::DeviceBuffer<uint32_t> d_cell_slot;           // [n_cells + 1]
    pa::DeviceBuffer<ull> d_slot_key;                 // [n_slots] cell << 32 | gene
    pa::DeviceBuffer<uint32_t> d_slot_start;          // [n_slots + 1] into d_t_row
    pa::DeviceBuffer<uint32_t> d_t_row;               // [nnz] a slot's rows, ascending
    pa::DeviceBuffer<double> d_u, d_alpha;            // [n_slots]
    // the cells with multi rows, largest |E| + rows first: [0, n_hbm) HBM variant, [n_hbm, n_hbm + n_block) block bin, the rest wave bin
    pa::DeviceBuffer<uint32_t> d_order;
    pa::DeviceBuffer<ull> d_scratch_off;              // [n_hbm]
    pa::DeviceBuffer<double> d_scratch;
    pa::DeviceBuffer<ull> d_stats;                    // [PA_GENES_STATS]
};
