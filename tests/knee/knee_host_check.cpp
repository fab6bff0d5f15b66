// Stand-alone driver of csrc/bus_knee_host.cpp (the host half of the cell calling on BUS records: the checks of the params, of the records and of
// a barcode list, the three threshold rules, the barcode_ranks.tsv writer) for tests/test_knee_host.py, built with g++ under AddressSanitizer +
// UndefinedBehaviorSanitizer and run as a program. It reads one case from the file named first on the command line (whitespace-separated tokens):
//   bc_len umi_len | mode lower divisor expected_cells min_umis | D, then D pairs "v R" | K, then K list values | R, then R records
//   "barcode umi ec count" | N, then N rows "barcode reads records umis rank called"
// and prints "defaults ...", "params <status> [message]", "threshold <t> <L>" (valid params only), "records <status> [message]",
// "list <status> [message]", "tsv <status> [message]" (the rows written to the file named second), then "OK". The arrays are heap blocks of
// exactly the stated size, so a read past either end is caught.
#include <cinttypes>
#include <cstdarg>
#include <cstdio>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "bus_knee_host.hpp"

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
    if (argc < 3) return 2;
    std::ifstream in(argv[1]);
    uint32_t bc_len = 0, umi_len = 0;
    pa_knee_params p{};
    uint64_t D = 0, K = 0, R = 0, N = 0;
    in >> bc_len >> umi_len >> p.mode >> p.lower >> p.divisor >> p.expected_cells >> p.min_umis >> D;
    std::vector<uint32_t> v(D);
    std::vector<uint64_t> atleast(D);
    for (uint64_t j = 0; j < D; ++j) in >> v[j] >> atleast[j];
    in >> K;
    std::vector<uint64_t> list(K);
    for (uint64_t& x : list) in >> x;
    in >> R;
    std::vector<pa_bus_record> rec(R);
    for (pa_bus_record& r : rec) {
        in >> r.barcode >> r.umi >> r.ec >> r.count;
        r.flags = r.pad = 0;
    }
    in >> N;
    std::vector<pa_bus_barcode_row> rows(N);
    for (pa_bus_barcode_row& r : rows) in >> r.barcode >> r.reads >> r.records >> r.umis >> r.rank >> r.called;
    if (!in) { printf("MISS the case file is short\n"); return 1; }

    {
        pa_knee_params d{};
        d.mode = 99;
        pa_knee_params taken{};
        const int e = knee::take_params(nullptr, taken);   // NULL: the defaults
        pa_knee_default_params(&d);
        printf("defaults %d %u %u %u %u %u %u\n", e, d.mode, d.lower, d.divisor, d.expected_cells, d.min_umis, (unsigned)(taken.lower == d.lower && taken.mode == d.mode));
    }
    pa_knee_params checked{};
    const int pe = knee::take_params(&p, checked);
    printf("params %d %s\n", pe, pe == PA_OK ? "" : last_error_ref().c_str());
    if (pe == PA_OK) {
        uint64_t L = 99;
        const uint64_t t = knee::threshold(checked, v.data(), atleast.data(), D, &L);
        printf("threshold %" PRIu64 " %" PRIu64 "\n", t, L);
    }
    {
        const int e = knee::check_records(rec.data(), R, bc_len, umi_len);
        printf("records %d %s\n", e, e == PA_OK ? "" : last_error_ref().c_str());
    }
    {
        const int e = knee::check_list(list.data(), K, bc_len);
        printf("list %d %s\n", e, e == PA_OK ? "" : last_error_ref().c_str());
    }
    {
        const int e = pa_write_barcode_ranks_tsv(rows.data(), N, bc_len, argv[2]);
        printf("tsv %d %s\n", e, e == PA_OK ? "" : last_error_ref().c_str());
    }
    printf("OK\n");
    return 0;
}
