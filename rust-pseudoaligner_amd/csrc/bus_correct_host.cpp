// Host half of the BUS barcode correction: see bus_correct_host.hpp. No HIP in this file.
#include "bus_correct_host.hpp"

#include <algorithm>
#include <numeric>
#include <vector>

#include "bus_records_host.hpp"

namespace pa {
namespace correct {

typedef unsigned long long ull;

int check_lengths(uint32_t bc_len, uint32_t umi_len) { return bus_records::check_lengths(bc_len, umi_len, PA_ERR_UNSUPPORTED, " (one 64-bit word)"); }

int pack_whitelist(const char* whitelist, uint64_t n, uint32_t bc_len, uint64_t* packed) {
    if ((n && !whitelist) || (n && !packed)) return fail(PA_ERR_INVALID_ARG, "null argument");
    if (bc_len < 1 || bc_len > 31) return fail(PA_ERR_UNSUPPORTED, "barcode length %u: 1..31 bases", bc_len);
    for (uint64_t i = 0; i < n; ++i) {
        uint64_t v = 0;
        for (uint32_t j = 0; j < bc_len; ++j) {
            const char c = whitelist[i * bc_len + j];
            const uint32_t b = c == 'A' ? 0u : c == 'C' ? 1u : c == 'G' ? 2u : c == 'T' ? 3u : 4u;
            if (b > 3) return fail(PA_ERR_INVALID_ARG, "whitelist entry %llu: byte %u is not A, C, G or T", (ull)i, j + 1);
            v = (v << 2) | b;
        }
        packed[i] = v;
    }
    return PA_OK;
}

int check_whitelist(const uint64_t* whitelist, uint64_t n, uint32_t bc_len) {
    if (!whitelist) return fail(PA_ERR_INVALID_ARG, "null argument");
    if (n < 1 || n > 0x7FFFFFFFull) return fail(PA_ERR_INVALID_ARG, "a whitelist of %llu barcodes: 1 .. 2^31-1", (ull)n);
    const uint64_t limit = bus_records::value_limit(bc_len);
    for (uint64_t i = 0; i < n; ++i)
        if (whitelist[i] >= limit) return fail(PA_ERR_INVALID_ARG, "whitelist entry %llu: %llu is no barcode of %u bases", (ull)i, (ull)whitelist[i], bc_len);
    // duplicates: the entries ordered by (value, index); of all pairs of equal neighbours the one whose first index is smallest
    std::vector<uint32_t> order((size_t)n);
    std::iota(order.begin(), order.end(), 0u);
    std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return whitelist[a] != whitelist[b] ? whitelist[a] < whitelist[b] : a < b; });
    uint64_t first = n, second = n;
    for (uint64_t i = 1; i < n; ++i)
        if (whitelist[order[i]] == whitelist[order[i - 1]] && order[i - 1] < first) { first = order[i - 1]; second = order[i]; }
    if (first < n) return fail(PA_ERR_INVALID_ARG, "whitelist entry %llu: entry %llu holds the same barcode", (ull)first, (ull)second);
    return PA_OK;
}

int check_records(const pa_bus_record* records, uint64_t n, uint32_t bc_len, uint32_t umi_len) { return bus_records::check_records(records, n, bc_len, umi_len); }

uint64_t table_capacity(uint64_t n_whitelist) {
    uint64_t cap = 2;
    while (cap < 2 * n_whitelist) cap <<= 1;
    return cap;
}

}  // namespace correct
}  // namespace pa
