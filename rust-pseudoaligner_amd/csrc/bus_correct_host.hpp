// Host half of the BUS barcode correction (pa_bus_correct, include/pseudoaligner_amd.h): packing a whitelist, the checks of the whitelist and
// of the records with their messages, the capacity rule of the whitelist table. Free of HIP: bus_correct.hip calls it, and
// tests/correct/correct_host_check.cpp drives it as a plain g++ program under the sanitizers.
#pragma once
#include <cstdint>

#include "pa_common.hpp"

namespace pa {
namespace correct {

// bc_len / umi_len as pa_bus_create takes them, else PA_ERR_UNSUPPORTED
int check_lengths(uint32_t bc_len, uint32_t umi_len);

// n * bc_len bytes, no separators -> packed[n]: 2 bits per base, A=0 C=1 G=2 T=3, first base most significant. A byte that is none of
// A, C, G, T: PA_ERR_INVALID_ARG naming the entry and the byte
int pack_whitelist(const char* whitelist, uint64_t n, uint32_t bc_len, uint64_t* packed);

// 1 <= n <= 2^31 - 1, every value < 4^bc_len, no value twice: else PA_ERR_INVALID_ARG naming the entry (of a duplicate: the smaller index;
// of several offending entries: the smallest named index)
int check_whitelist(const uint64_t* whitelist, uint64_t n, uint32_t bc_len);

// strictly ascending by (barcode, UMI, ec), every barcode < 4^bc_len, every UMI < 4^umi_len: else PA_ERR_INVALID_ARG naming the first
// offending record
int check_records(const pa_bus_record* records, uint64_t n, uint32_t bc_len, uint32_t umi_len);

// slots of the whitelist table: the power of two >= 2 * n_whitelist
uint64_t table_capacity(uint64_t n_whitelist);

}  // namespace correct
}  // namespace pa
