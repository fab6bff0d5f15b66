// Host half of the BUS barcode correction: see bus_correct_host.hpp. No HIP in this file.
#include "bus_correct_host.hpp"

#include <algorithm>
#include <numeric>
#include <vector>

namespace pa {
namespace correct {

typedef unsigned long long ull;

static uint64_t value_limit(uint32_t bases) { return bases >= 32 ? ~0ull : (1ull << (2 * bases)); }   // 4^bases (bases <= 31 here)

int check_lengths(uint32_t bc_len, uint32_t umi_len) {
    if (bc_len < 1 || umi_len < 1 || (uint64_t)bc_len + umi_len > 32)
        return fail(PA_ERR_UNSUPPORTED, "barcode length %u / UMI length %u: both at least 1, together at most 32 bases (one 64-bit word)", bc_len, umi_len);
    return PA_OK;
}

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
    const uint64_t limit = value_limit(bc_len);
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

int check_records(const pa_bus_record* records, uint64_t n, uint32_t bc_len, uint32_t umi_len) {
    if (n && !records) return fail(PA_ERR_INVALID_ARG, "null argument");
    const uint64_t bc_limit = value_limit(bc_len), umi_limit = value_limit(umi_len);
    for (uint64_t i = 0; i < n; ++i) {
        const pa_bus_record& r = records[i];
        if (r.barcode >= bc_limit) return fail(PA_ERR_INVALID_ARG, "record %llu: barcode %llu is no barcode of %u bases", (ull)i, (ull)r.barcode, bc_len);
        if (r.umi >= umi_limit) return fail(PA_ERR_INVALID_ARG, "record %llu: UMI %llu is no UMI of %u bases", (ull)i, (ull)r.umi, umi_len);
        if (i == 0) continue;
        const pa_bus_record& q = records[i - 1];
        const bool ascending = q.barcode != r.barcode ? q.barcode < r.barcode : q.umi != r.umi ? q.umi < r.umi : q.ec < r.ec;
        if (!ascending) return fail(PA_ERR_INVALID_ARG, "record %llu: not above record %llu by (barcode, UMI, ec)", (ull)i, (ull)i - 1);
    }
    return PA_OK;
}

uint64_t table_capacity(uint64_t n_whitelist) {
    uint64_t cap = 2;
    while (cap < 2 * n_whitelist) cap <<= 1;
    return cap;
}

}  // namespace correct
}  // namespace pa
