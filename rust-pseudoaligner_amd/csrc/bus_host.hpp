// Host half of the BUS writer (pa_bus, include/pseudoaligner_amd.h): the numbering of equivalence classes and the three output files.
// Free of HIP: bus.hip calls it, and tests/bus/bus_host_check.cpp drives it as a plain g++ program under the sanitizers.
#pragma once
#include <cstdint>
#include <functional>
#include <string>
#include <vector>

#include "pa_common.hpp"

namespace pa {
namespace bus {

constexpr uint32_t CLASS_EC_NONE = 0xFFFFFFFFu;   // an index class without ids (or with an id that is no transcript): no ec

// every ec of a run as a CSR: ec e = ids[offsets[e] .. offsets[e + 1]), ascending. T singletons, M index classes of two ids or more,
// R novel lists.
struct EcTable {
    uint32_t T = 0, M = 0, R = 0;
    std::vector<uint64_t> offsets;
    std::vector<uint32_t> ids;
    uint64_t n_ecs() const { return (uint64_t)T + M + R; }
};

// class_ec[c]: t for an index class {t}, T + j for the j-th class of two ids or more (class-id order), CLASS_EC_NONE otherwise; *M = their
// number. PA_ERR_UNSUPPORTED when T + M exceeds 2^31 - 1.
int class_ecs(uint32_t T, const uint64_t* ec_offset, const uint32_t* ec_ids, uint32_t num_classes, std::vector<uint32_t>& class_ec, uint32_t* M);

// The ec of every recorded arena list of two ids or more (list l = list_ids[list_off[l] .. list_off[l + 1]), strictly ascending; the same
// content may come several times): the ec of the index class of equal content, else T + M + its rank among the distinct remaining
// lists in lexicographic order. Fills list_ec[n_lists] and the table of all ecs. PA_ERR_UNSUPPORTED beyond 2^31 - 1 ecs.
int assign_ecs(uint32_t T, const uint64_t* ec_offset, const uint32_t* ec_ids, uint32_t num_classes, const uint64_t* list_off, const uint32_t* list_ids,
               uint64_t n_lists, EcTable& table, std::vector<int32_t>& list_ec);

// the bytes of the three files
std::string bus_header(uint32_t bc_len, uint32_t umi_len);                     // "BUS\0", version 1, bclen, umilen, tlen = 0
std::string matrix_ec_text(const EcTable& table);                              // "ec\tid,id,...\n" for every ec
std::string transcripts_text(const std::vector<std::string>& names);           // one name per line

// the records of a run a piece at a time, in file order: *records / *n = the next piece (valid until the next call), *n = 0 at the end;
// returns a pa_status
typedef std::function<int(const pa_bus_record** records, uint64_t* n)> RecordSource;

// out_dir/output.bus, matrix.ec, transcripts.txt (PA_ERR_IO naming the file that could not be written)
int write_files(const char* out_dir, uint32_t bc_len, uint32_t umi_len, const RecordSource& next, const EcTable& table, const std::vector<std::string>& names);
// ... with the records in one array
int write_files(const char* out_dir, uint32_t bc_len, uint32_t umi_len, const pa_bus_record* records, uint64_t n_records, const EcTable& table,
                const std::vector<std::string>& names);

}  // namespace bus

// bus.hip: what a finished writer holds, for the gene counter (genes.hip): its device, the records in HBM, the ec table, the lengths and the
// index's transcripts. PA_ERR_INVALID_ARG before pa_bus_finish
int bus_finished_view(const pa_bus* b, int* device, const pa_bus_record** d_records, uint64_t* n_records, const bus::EcTable** table, uint32_t* bc_len, uint32_t* umi_len,
                      uint32_t* num_tx);

}  // namespace pa
