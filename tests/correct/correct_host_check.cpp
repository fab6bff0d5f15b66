// Stand-alone driver of csrc/bus_correct_host.cpp (the host half of the BUS barcode correction: packing, the checks of the whitelist and of
// the records, the capacity rule) for tests/test_correct_host.py, built with g++ under AddressSanitizer + UndefinedBehaviorSanitizer and
// run as a program. It reads one case from the file named on the command line (whitespace-separated tokens):
//   bc_len umi_len | W, then W barcode strings of bc_len bytes | V, then V packed whitelist values | R, then R records "barcode umi ec count"
// and prints "lengths <status>", "pack <status> [values | message]", "whitelist <status> [message]", "records <status> [message]",
// "capacity <n> <slots>" for a few n, then "OK". The arrays are heap blocks of exactly the stated size, so a read past either end is caught.
#include <cinttypes>
#include <cstdarg>
#include <cstdio>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "bus_correct_host.hpp"

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
    uint32_t bc_len = 0, umi_len = 0;
    uint64_t W = 0, V = 0, R = 0;
    in >> bc_len >> umi_len >> W;
    std::string text;
    for (uint64_t i = 0; i < W; ++i) {
        std::string s;
        in >> s;
        text += s;
    }
    in >> V;
    std::vector<uint64_t> values(V);
    for (uint64_t& v : values) in >> v;
    in >> R;
    std::vector<pa_bus_record> rec(R);
    for (pa_bus_record& r : rec) {
        in >> r.barcode >> r.umi >> r.ec >> r.count;
        r.flags = r.pad = 0;
    }
    if (!in) { printf("MISS the case file is short\n"); return 1; }

    printf("lengths %d\n", correct::check_lengths(bc_len, umi_len));
    {
        std::vector<char> bytes(text.begin(), text.end());   // (no terminator: exactly W * bc_len bytes)
        std::vector<uint64_t> packed(W);
        const int e = correct::pack_whitelist(bytes.data(), W, bc_len, packed.data());
        printf("pack %d", e);
        if (e == PA_OK) for (uint64_t v : packed) printf(" %" PRIu64, v);
        else printf(" %s", last_error_ref().c_str());
        printf("\n");
    }
    {
        const int e = correct::check_whitelist(values.data(), V, bc_len);
        printf("whitelist %d %s\n", e, e == PA_OK ? "" : last_error_ref().c_str());
    }
    {
        const int e = correct::check_records(rec.data(), R, bc_len, umi_len);
        printf("records %d %s\n", e, e == PA_OK ? "" : last_error_ref().c_str());
    }
    for (uint64_t n : {1ull, 2ull, 3ull, 1024ull, 1025ull, 6800000ull, 0x7FFFFFFFull}) printf("capacity %" PRIu64 " %" PRIu64 "\n", n, correct::table_capacity(n));
    printf("OK\n");
    return 0;
}
