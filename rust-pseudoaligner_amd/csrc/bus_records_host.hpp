// The checks that every stage over BUS records (correction, cell calling, the gene counter) makes of host arrays of them, with their
// messages. Free of HIP and header-only, so that a program which links one stage's host half needs no further source: the stages' host
// halves call it, and the stand-alone programs under tests/correct, tests/knee and tests/genes drive it through them under the sanitizers.
#pragma once
#include <cstdint>

#include "pa_common.hpp"

namespace pa {
namespace bus_records {

// 4^bases: the values of `bases` bases lie below it (bases <= 31)
inline uint64_t value_limit(uint32_t bases) { return bases >= 32 ? ~0ull : (1ull << (2 * bases)); }

// bc_len / umi_len as pa_bus_create takes them: both at least 1, together at most 32 bases. Else `status`, the message ending in `tail`
inline int check_lengths(uint32_t bc_len, uint32_t umi_len, int status, const char* tail) {
    if (bc_len < 1 || umi_len < 1 || (uint64_t)bc_len + umi_len > 32)
        return fail(status, "barcode length %u / UMI length %u: both at least 1, together at most 32 bases%s", bc_len, umi_len, tail);
    return PA_OK;
}

// q before r by (barcode, UMI, ec), strictly
inline bool ascending(const pa_bus_record& q, const pa_bus_record& r) {
    return q.barcode != r.barcode ? q.barcode < r.barcode : q.umi != r.umi ? q.umi < r.umi : q.ec < r.ec;
}

// Every record against the stage's own test, bad(r) -> refuse(i, r) is the status returned, then against the record before it: strictly
// ascending by (barcode, UMI, ec), else PA_ERR_INVALID_ARG. The first offending record is the one named. (The test is a plain predicate so
// that the loop over some ten million records holds no call)
template <class Bad, class Refuse>
int walk(const pa_bus_record* records, uint64_t n, Bad&& bad, Refuse&& refuse) {
    typedef unsigned long long ull;
    if (n && !records) return fail(PA_ERR_INVALID_ARG, "null argument");
    for (uint64_t i = 0; i < n; ++i) {
        const pa_bus_record& r = records[i];
        if (bad(r)) return refuse(i, r);
        if (i == 0) continue;
        if (!ascending(records[i - 1], r)) return fail(PA_ERR_INVALID_ARG, "record %llu: not above record %llu by (barcode, UMI, ec)", (ull)i, (ull)i - 1);
    }
    return PA_OK;
}

// the walk with every barcode < 4^bc_len and every UMI < 4^umi_len
inline int check_records(const pa_bus_record* records, uint64_t n, uint32_t bc_len, uint32_t umi_len) {
    typedef unsigned long long ull;
    const uint64_t bc_limit = value_limit(bc_len), umi_limit = value_limit(umi_len);
    return walk(records, n, [&](const pa_bus_record& r) { return r.barcode >= bc_limit || r.umi >= umi_limit; }, [&](uint64_t i, const pa_bus_record& r) {
        if (r.barcode >= bc_limit) return fail(PA_ERR_INVALID_ARG, "record %llu: barcode %llu is no barcode of %u bases", (ull)i, (ull)r.barcode, bc_len);
        return fail(PA_ERR_INVALID_ARG, "record %llu: UMI %llu is no UMI of %u bases", (ull)i, (ull)r.umi, umi_len);
    });
}

}  // namespace bus_records
}  // namespace pa
