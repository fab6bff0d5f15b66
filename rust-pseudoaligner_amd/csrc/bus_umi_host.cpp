// Host half of the UMI correction on BUS records: see bus_umi_host.hpp. No HIP in this file.
#include "bus_umi_host.hpp"

#include "bus_records_host.hpp"
#include "genes_host.hpp"

namespace pa {
namespace umi {

typedef unsigned long long ull;

int check_mode(uint32_t mode) {
    if (mode != PA_UMI_GREATEST && mode != PA_UMI_DIRECTIONAL) return fail(PA_ERR_INVALID_ARG, "UMI correction mode %u: PA_UMI_GREATEST or PA_UMI_DIRECTIONAL", mode);
    return PA_OK;
}

int check_records(const pa_bus_record* records, uint64_t n, uint32_t n_ecs, uint32_t bc_len, uint32_t umi_len) {
    const uint64_t bc_limit = bus_records::value_limit(bc_len), umi_limit = bus_records::value_limit(umi_len);
    return bus_records::walk(records, n, [&](const pa_bus_record& r) { return r.barcode >= bc_limit || r.umi >= umi_limit || r.ec < 0 || (uint32_t)r.ec >= n_ecs; },
                             [&](uint64_t i, const pa_bus_record& r) {
        if (r.barcode >= bc_limit) return fail(PA_ERR_INVALID_ARG, "record %llu: barcode %llu is no barcode of %u bases", (ull)i, (ull)r.barcode, bc_len);
        if (r.umi >= umi_limit) return fail(PA_ERR_INVALID_ARG, "record %llu: UMI %llu is no UMI of %u bases", (ull)i, (ull)r.umi, umi_len);
        return fail(PA_ERR_INVALID_ARG, "record %llu: ec %d is outside [0, %u)", (ull)i, r.ec, n_ecs);
    });
}

int check_call(const pa_bus_record* records, uint64_t n, const uint64_t* ec_offsets, const uint32_t* ec_ids, uint32_t n_ecs, uint32_t num_tx, const uint32_t* tx_gene,
               uint32_t num_genes, uint32_t bc_len, uint32_t umi_len, uint32_t mode) {
    int e;
    if ((e = check_mode(mode)) || (e = genes::check_lengths(bc_len, umi_len)) || (e = genes::check_tables(ec_offsets, ec_ids, n_ecs, num_tx, tx_gene, num_genes))) return e;
    if (n > 0x7FFFFFFFull) return fail(PA_ERR_UNSUPPORTED, "more than 2^31-1 records");
    return check_records(records, n, n_ecs, bc_len, umi_len);
}

const char* stat_name(uint32_t j) {
    static const char* const names[PA_BUS_UMI_STATS] = {"records_in", "reads_in", "molecules_in", "barcodes", "molecules_inert", "molecules_with_hamming1", "molecules_with_neighbour",
                                                        "molecules_moved", "molecules_moved_onto_moved", "records_rewritten", "reads_moved", "records_out", "molecules_out",
                                                        "largest_barcode", "barcodes_hbm"};
    return j < PA_BUS_UMI_STATS ? names[j] : nullptr;
}

}  // namespace umi
}  // namespace pa
