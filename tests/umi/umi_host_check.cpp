// Stand-alone driver of csrc/bus_umi_host.cpp (the host half of the UMI correction: the checks of the arguments in their order, the stat names) for
// tests/test_umi_host.py, built with g++ under AddressSanitizer + UndefinedBehaviorSanitizer and run as a program. It reads one case from the file
// named on the command line (whitespace-separated tokens):
//   bc_len umi_len mode num_tx num_genes | num_tx values of tx_gene | E, then E + 1 offsets | I, then I ec ids | R, then R records "barcode umi ec count"
// and prints "mode <status>", "records <status> [message]", "call <status> [message]", "sets <the genes of every ec, ';' between ecs>" (when the call
// is valid), "names <the stat names>", then "OK". The arrays are heap blocks of exactly the stated size, so a read past either end is caught.
#include <cinttypes>
#include <cstdarg>
#include <cstdio>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "bus_umi_host.hpp"
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
    if (argc < 2) return 2;
    std::ifstream in(argv[1]);
    uint32_t bc_len = 0, umi_len = 0, mode = 0, num_tx = 0, num_genes = 0;
    uint64_t E = 0, I = 0, R = 0;
    in >> bc_len >> umi_len >> mode >> num_tx >> num_genes;
    std::vector<uint32_t> tx_gene(num_tx);
    for (uint32_t& g : tx_gene) in >> g;
    in >> E;
    std::vector<uint64_t> off(E + 1);
    for (uint64_t& o : off) in >> o;
    in >> I;
    std::vector<uint32_t> ids(I);
    for (uint32_t& t : ids) in >> t;
    in >> R;
    std::vector<pa_bus_record> rec(R);
    for (pa_bus_record& r : rec) {
        in >> r.barcode >> r.umi >> r.ec >> r.count;
        r.flags = r.pad = 0;
    }
    if (!in) { printf("MISS the case file is short\n"); return 1; }

    printf("mode %d\n", umi::check_mode(mode));
    {
        const int e = umi::check_records(rec.data(), R, (uint32_t)E, bc_len, umi_len);
        printf("records %d %s\n", e, e == PA_OK ? "" : last_error_ref().c_str());
    }
    const int e = umi::check_call(rec.data(), R, off.data(), ids.data(), (uint32_t)E, num_tx, tx_gene.data(), num_genes, bc_len, umi_len, mode);
    printf("call %d %s\n", e, e == PA_OK ? "" : last_error_ref().c_str());
    if (e == PA_OK) {
        genes::GeneSets gs;
        genes::gene_sets(off.data(), ids.data(), (uint32_t)E, tx_gene.data(), gs);
        printf("sets");
        for (uint64_t k = 0; k < E; ++k) {
            for (uint64_t j = gs.off[k]; j < gs.off[k + 1]; ++j) printf(" %u", gs.ids[j]);
            printf(" ;");
        }
        printf("\n");
    }
    printf("names");
    for (uint32_t j = 0; umi::stat_name(j); ++j) printf(" %s", umi::stat_name(j));
    printf("\n");
    if (umi::stat_name(PA_BUS_UMI_STATS) != nullptr) printf("MISS a name beyond the stats\n");
    printf("OK\n");
    return 0;
}
