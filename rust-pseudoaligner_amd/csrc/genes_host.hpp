// Host half of the gene counter (pa_genes, include/pseudoaligner_amd.h): the ec -> gene-set table, the argument checks,
// barcode decoding and the three output files. Free of HIP: genes.hip calls it, and tests/genes/genes_host_check.cpp drives it as a
// plain g++ program under the sanitizers.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "pa_common.hpp"

namespace pa {
namespace genes {

// G(e) of every ec as a CSR (ascending distinct genes) and the content hash of each set (the function of kernel_utils.hpp's
// list_hash_dev: a set that a kernel builds and one of this table hash alike when their contents are equal)
struct GeneSets {
    std::vector<uint64_t> off;    // [n_ecs + 1]
    std::vector<uint32_t> ids;
    std::vector<uint64_t> hash;   // [n_ecs]
};

uint64_t set_hash(const uint32_t* v, uint32_t n);

// params, lengths, the ec table (offsets ascending from 0, ids ascending and < num_tx) and tx_gene (< num_genes): PA_ERR_INVALID_ARG
int check_params(const pa_genes_params& p);
int check_lengths(uint32_t bc_len, uint32_t umi_len);
int check_tables(const uint64_t* ec_offsets, const uint32_t* ec_ids, uint32_t n_ecs, uint32_t num_tx, const uint32_t* tx_gene, uint32_t num_genes);
// strictly ascending by (barcode, UMI, ec), every ec in [0, n_ecs): the message names the first offending record
int check_records(const pa_bus_record* records, uint64_t n, uint32_t n_ecs);

void gene_sets(const uint64_t* ec_offsets, const uint32_t* ec_ids, uint32_t n_ecs, const uint32_t* tx_gene, GeneSets& out);

// 2 bits per base, first base most significant
std::string decode_barcode(uint64_t barcode, uint32_t bc_len);
// an f64 as pa_write_abundance_tsv prints it
std::string f64_text(double v);

// the bytes of the three files: the matrix is genes x cells, 1-based, entries in (cell, gene) order
std::string matrix_text(uint32_t num_genes, uint64_t n_cells, const uint32_t* cell, const uint32_t* gene, const double* value, uint64_t n);
std::string barcodes_text(const uint64_t* barcodes, uint64_t n_cells, uint32_t bc_len);
// gene names numbered as pa_host_index_genes numbers them; PA_ERR_INVALID_ARG when their number is not num_genes
int features_text(const std::vector<std::string>& tx_genes, uint32_t num_genes, std::string& out);
// out_dir/matrix.mtx, barcodes.tsv, features.tsv (PA_ERR_IO naming the file that could not be written)
int write_files(const char* out_dir, const std::string& matrix, const std::string& barcodes, const std::string& features);

}  // namespace genes
}  // namespace pa
