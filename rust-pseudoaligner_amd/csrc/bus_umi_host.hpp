// Host half of the UMI correction on BUS records (pa_bus_umi_correct, include/pseudoaligner_amd.h): the checks of the arguments
// with their messages, in the order the header states, and the names of the stats. Free of HIP: bus_umi.hip calls it, and
// tests/umi/umi_host_check.cpp drives it as a plain g++ program under the sanitizers.
#pragma once
#include <cstdint>

#include "pa_common.hpp"

namespace pa {
namespace umi {

// PA_UMI_GREATEST or PA_UMI_DIRECTIONAL, else PA_ERR_INVALID_ARG
int check_mode(uint32_t mode);

// strictly ascending by (barcode, UMI, ec), every barcode < 4^bc_len, every UMI < 4^umi_len (pa_bus_correct_records' messages), every ec in
// [0, n_ecs) (pa_genes_create's message): else PA_ERR_INVALID_ARG naming the first offending record
int check_records(const pa_bus_record* records, uint64_t n, uint32_t n_ecs, uint32_t bc_len, uint32_t umi_len);

// every host argument of pa_bus_umi_correct_records, pa_genes_create's checks in pa_genes_create's order: the mode (where the gene counter checks its
// params), the lengths, the ec table and tx_gene, the record count (more than 2^31 - 1: PA_ERR_UNSUPPORTED), the records
int check_call(const pa_bus_record* records, uint64_t n, const uint64_t* ec_offsets, const uint32_t* ec_ids, uint32_t n_ecs, uint32_t num_tx, const uint32_t* tx_gene,
               uint32_t num_genes, uint32_t bc_len, uint32_t umi_len, uint32_t mode);

// the name of stats[j], j < PA_BUS_UMI_STATS (nullptr beyond)
const char* stat_name(uint32_t j);

}  // namespace umi
}  // namespace pa
