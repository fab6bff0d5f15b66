// Host half of the cell calling on BUS records (pa_bus_knee, pa_bus_keep; include/pseudoaligner_amd.h): the checks of the params, of the
// records and of a barcode list with their messages, the three threshold rules over the curve (v, R), the barcode_ranks.tsv writer.
// Free of HIP: bus_knee.hip calls it, and tests/knee/knee_host_check.cpp drives it as a plain g++ program under the sanitizers.
#pragma once
#include <cstdint>
#include <vector>

#include "pa_common.hpp"

namespace pa {
namespace knee {

constexpr uint32_t EXPECTED_PERCENTILE = 100;   // PA_KNEE_EXPECTED: the row at rank expected_cells / 100 ...
constexpr uint32_t EXPECTED_DIVISOR = 10;       // ... and a tenth of its molecules, rounded up

// p as the caller gave it (NULL: the defaults) -> out; lower, divisor, min_umis or expected_cells 0 or an unknown mode: PA_ERR_INVALID_ARG
int take_params(const pa_knee_params* p, pa_knee_params& out);

// bc_len / umi_len as pa_bus_create takes them (PA_ERR_UNSUPPORTED), then bus_records_host's walk over the records: strictly ascending
// by (barcode, UMI, ec), every barcode < 4^bc_len, every UMI < 4^umi_len, else PA_ERR_INVALID_ARG naming the first offending record
int check_records(const pa_bus_record* records, uint64_t n, uint32_t bc_len, uint32_t umi_len);

// strictly ascending, every value < 4^bc_len: else PA_ERR_INVALID_ARG naming the first offending entry. n = 0 is valid
int check_list(const uint64_t* barcodes, uint64_t n, uint32_t bc_len);

// the curve: v[D] strictly descending (the distinct umis values), R[D] = the barcodes with umis >= v[j] (so R[D - 1] = B). -> the
// threshold t >= 1; *L = the values >= lower under PA_KNEE_CURVE, else 0. p has passed take_params
uint64_t threshold(const pa_knee_params& p, const uint32_t* v, const uint64_t* R, uint64_t D, uint64_t* L);

// PA_KNEE_CURVE's k over the first L points (L >= 1): the knee's index
uint64_t curve_knee(const uint32_t* v, const uint64_t* R, uint64_t L);

int write_ranks_tsv(const pa_bus_barcode_row* rows, uint64_t n, uint32_t bc_len, const char* path);

}  // namespace knee
}  // namespace pa

// bus_knee.hip: pa_bus_knee with the outputs as vectors, for the file-level calls (one run of the kernels, no second call for the sizes)
int pa_bus_knee_vectors(const pa_bus* finished, const pa_knee_params* p, std::vector<pa_bus_barcode_row>& rows, std::vector<uint64_t>& called, uint64_t* stats);
