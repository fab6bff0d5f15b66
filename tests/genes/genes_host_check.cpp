// Stand-alone driver of csrc/genes_host.cpp (the host half of the gene counter: the ec -> gene-set table, the argument checks, barcode
// decoding and the three file writers) for tests/test_genes_host.py, built with g++ under AddressSanitizer + UndefinedBehaviorSanitizer
// and run as a program. It reads one case from the file named on the command line (whitespace-separated tokens):
//   T num_genes bc_len umi_len | tx_gene[T] | C, then C ecs "len id ..." | R, then R records "barcode umi ec count" |
//   cells, then their barcodes | E, then E entries "cell gene value" (value as a C99 hex float) | T gene names | the output directory |
//   a directory that does not exist
// prints "tables rc", "records rc [message]", "lengths rc", "set e g ...", "hash e h", writes the three files, prints "unwritable rc" and
// ends with "OK".
#include <cinttypes>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "genes_host.hpp"

// the two symbols of the host runtime the header needs (the product has them in host_index.cpp)
namespace pa {
std::string& last_error_ref() {
    static thread_local std::string s;
    return s;
}
int fail(int code, const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    last_error_ref() = buf;
    return code;
}
}  // namespace pa

using namespace pa;

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    std::ifstream in(argv[1]);
    uint32_t T = 0, num_genes = 0, bc_len = 0, umi_len = 0;
    in >> T >> num_genes >> bc_len >> umi_len;
    std::vector<uint32_t> tx_gene(T);
    for (uint32_t& g : tx_gene) in >> g;
    uint64_t C = 0;
    in >> C;
    std::vector<uint64_t> off(1, 0);
    std::vector<uint32_t> ids;
    for (uint64_t e = 0; e < C; ++e) {
        uint64_t len = 0;
        in >> len;
        for (uint64_t j = 0; j < len; ++j) { uint32_t t = 0; in >> t; ids.push_back(t); }
        off.push_back(ids.size());
    }
    uint64_t R = 0;
    in >> R;
    std::vector<pa_bus_record> rec(R);
    for (pa_bus_record& r : rec) { r = pa_bus_record(); in >> r.barcode >> r.umi >> r.ec >> r.count; }
    uint64_t n_cells = 0, E = 0;
    in >> n_cells;
    std::vector<uint64_t> barcodes(n_cells);
    for (uint64_t& b : barcodes) in >> b;
    in >> E;
    std::vector<uint32_t> cell(E), gene(E);
    std::vector<double> value(E);
    for (uint64_t i = 0; i < E; ++i) {
        std::string v;
        in >> cell[i] >> gene[i] >> v;
        value[i] = strtod(v.c_str(), nullptr);
    }
    std::vector<std::string> names(T);
    for (std::string& s : names) in >> s;
    std::string out_dir, no_dir;
    in >> out_dir >> no_dir;
    if (!in) return 3;

    int rc = genes::check_tables(off.data(), ids.data(), (uint32_t)C, T, tx_gene.data(), num_genes);
    printf("tables %d\n", rc);
    if (rc != PA_OK) { printf("OK\n"); return 0; }
    rc = genes::check_records(rec.data(), R, (uint32_t)C);
    printf("records %d %s\n", rc, rc ? last_error_ref().c_str() : "");
    printf("lengths %d\n", genes::check_lengths(bc_len, umi_len));
    genes::GeneSets gs;
    genes::gene_sets(off.data(), ids.data(), (uint32_t)C, tx_gene.data(), gs);
    for (uint64_t e = 0; e < C; ++e) {
        printf("set %" PRIu64, e);
        for (uint64_t j = gs.off[e]; j < gs.off[e + 1]; ++j) printf(" %u", gs.ids[j]);
        printf("\nhash %" PRIu64 " %" PRIu64 "\n", e, gs.hash[e]);
        if (gs.hash[e] != genes::set_hash(gs.ids.data() + gs.off[e], (uint32_t)(gs.off[e + 1] - gs.off[e]))) printf("MISS hash %" PRIu64 "\n", e);
    }
    std::string features;
    rc = genes::features_text(names, num_genes, features);
    printf("features %d\n", rc);
    const std::string matrix = genes::matrix_text(num_genes, n_cells, cell.data(), gene.data(), value.data(), E);
    const std::string bcs = genes::barcodes_text(barcodes.data(), n_cells, bc_len);
    printf("write %d\n", genes::write_files(out_dir.c_str(), matrix, bcs, features));
    printf("unwritable %d\n", genes::write_files(no_dir.c_str(), matrix, bcs, features));
    printf("OK\n");
    return 0;
}
