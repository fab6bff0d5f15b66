// Stand-alone driver of csrc/bus_host.cpp (the host half of the BUS writer: ec numbering and the three file writers) for
// tests/test_bus_host.py, built with g++ under AddressSanitizer + UndefinedBehaviorSanitizer and run as a program. It reads one case
// from the file named on the command line (whitespace-separated tokens):
//   T | bc_len umi_len | C, then C classes "len id ..." | L, then L lists "len id ..." | R, then R records "barcode umi ec count" |
//   N, then N names | the output directory
// prints "class_ec ...", "list_ec ...", "table T M R ids", writes the three files there and ends with "OK".
#include <cinttypes>
#include <cstdarg>
#include <cstdio>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "bus_host.hpp"

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

static void read_csr(std::istream& in, std::vector<uint64_t>& off, std::vector<uint32_t>& ids) {
    uint64_t n = 0;
    in >> n;
    off.assign(1, 0);
    for (uint64_t i = 0; i < n; ++i) {
        uint64_t len = 0;
        in >> len;
        for (uint64_t j = 0; j < len; ++j) {
            uint32_t t = 0;
            in >> t;
            ids.push_back(t);
        }
        off.push_back(ids.size());
    }
}

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: bus_host_check CASE\n"); return 2; }
    std::ifstream in(argv[1]);
    if (!in) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    uint32_t T = 0, bc_len = 0, umi_len = 0;
    in >> T >> bc_len >> umi_len;
    std::vector<uint64_t> ec_offset, list_off;
    std::vector<uint32_t> ec_ids, list_ids;
    read_csr(in, ec_offset, ec_ids);
    read_csr(in, list_off, list_ids);
    uint64_t n_records = 0, n_names = 0;
    in >> n_records;
    std::vector<pa_bus_record> records(n_records);
    for (pa_bus_record& r : records) {
        in >> r.barcode >> r.umi >> r.ec >> r.count;
        r.flags = r.pad = 0;
    }
    in >> n_names;
    std::vector<std::string> names(n_names);
    for (std::string& s : names) in >> s;
    std::string dir;
    in >> dir;
    if (!in) { fprintf(stderr, "malformed case\n"); return 2; }
    const uint32_t num_classes = (uint32_t)(ec_offset.size() - 1);

    std::vector<uint32_t> class_ec;
    uint32_t M = 0;
    int e = bus::class_ecs(T, ec_offset.data(), ec_ids.data(), num_classes, class_ec, &M);
    if (e != PA_OK) { printf("MISS class_ecs %d %s\n", e, last_error_ref().c_str()); return 1; }
    printf("class_ec");
    for (const uint32_t x : class_ec) printf(" %" PRId64, x == bus::CLASS_EC_NONE ? (int64_t)-1 : (int64_t)x);
    printf("\n");

    bus::EcTable table;
    std::vector<int32_t> list_ec;
    e = bus::assign_ecs(T, ec_offset.data(), ec_ids.data(), num_classes, list_off.data(), list_ids.data(), list_off.size() - 1, table, list_ec);
    if (e != PA_OK) { printf("MISS assign_ecs %d %s\n", e, last_error_ref().c_str()); return 1; }
    printf("list_ec");
    for (const int32_t x : list_ec) printf(" %d", x);
    printf("\n");
    printf("table %u %u %u %zu\n", table.T, table.M, table.R, table.ids.size());
    if (table.M != M || table.offsets.size() != table.n_ecs() + 1 || table.offsets.back() != table.ids.size()) { printf("MISS table shape\n"); return 1; }

    e = bus::write_files(dir.c_str(), bc_len, umi_len, records.data(), records.size(), table, names);
    if (e != PA_OK) { printf("MISS write_files %d %s\n", e, last_error_ref().c_str()); return 1; }
    // a directory that does not exist: PA_ERR_IO, nothing written
    e = bus::write_files((dir + "/no/such/dir").c_str(), bc_len, umi_len, records.data(), records.size(), table, names);
    if (e != PA_ERR_IO) { printf("MISS missing directory gave %d\n", e); return 1; }
    // no records, no lists: a header alone and T + M lines
    bus::EcTable empty;
    std::vector<int32_t> none;
    e = bus::assign_ecs(T, ec_offset.data(), ec_ids.data(), num_classes, list_off.data(), list_ids.data(), 0, empty, none);
    if (e != PA_OK || empty.R != 0 || empty.n_ecs() != (uint64_t)T + M || bus::bus_header(bc_len, umi_len).size() != 20) { printf("MISS empty run\n"); return 1; }
    printf("OK\n");
    return 0;
}
