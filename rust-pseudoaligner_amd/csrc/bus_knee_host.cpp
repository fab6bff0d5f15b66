// Host half of the cell calling on BUS records: see bus_knee_host.hpp. No HIP in this file.
#include "bus_knee_host.hpp"

#include <cmath>
#include <string>

#include "bus_records_host.hpp"

namespace pa {
namespace knee {

typedef unsigned long long ull;

int take_params(const pa_knee_params* p, pa_knee_params& out) {
    if (!p) { pa_knee_default_params(&out); return PA_OK; }
    out = *p;
    if (out.mode != PA_KNEE_CURVE && out.mode != PA_KNEE_EXPECTED && out.mode != PA_KNEE_MIN) return fail(PA_ERR_INVALID_ARG, "knee params: unknown mode %u", out.mode);
    if (out.lower == 0) return fail(PA_ERR_INVALID_ARG, "knee params: lower is 0 (a threshold is at least 1)");
    if (out.divisor == 0) return fail(PA_ERR_INVALID_ARG, "knee params: divisor is 0");
    if (out.expected_cells == 0) return fail(PA_ERR_INVALID_ARG, "knee params: expected_cells is 0");
    if (out.min_umis == 0) return fail(PA_ERR_INVALID_ARG, "knee params: min_umis is 0 (a threshold is at least 1)");
    return PA_OK;
}

int check_records(const pa_bus_record* records, uint64_t n, uint32_t bc_len, uint32_t umi_len) {
    const int e = bus_records::check_lengths(bc_len, umi_len, PA_ERR_UNSUPPORTED, " (one 64-bit word)");
    return e != PA_OK ? e : bus_records::check_records(records, n, bc_len, umi_len);
}

int check_list(const uint64_t* barcodes, uint64_t n, uint32_t bc_len) {
    if (n && !barcodes) return fail(PA_ERR_INVALID_ARG, "null argument");
    const uint64_t limit = bus_records::value_limit(bc_len);
    for (uint64_t i = 0; i < n; ++i) {
        if (barcodes[i] >= limit) return fail(PA_ERR_INVALID_ARG, "barcode list entry %llu: %llu is no barcode of %u bases", (ull)i, (ull)barcodes[i], bc_len);
        if (i && barcodes[i - 1] >= barcodes[i]) return fail(PA_ERR_INVALID_ARG, "barcode list entry %llu: not above entry %llu", (ull)i, (ull)i - 1);
    }
    return PA_OK;
}

// every product and difference below is one rounded f64 operation: no fused multiply-add may take the place of two of them
#if defined(__clang__)
#pragma clang fp contract(off)
#endif   // (a g++ build of this file is given -ffp-contract=off: tests/knee/build.py)
uint64_t curve_knee(const uint32_t* v, const uint64_t* R, uint64_t L) {
    if (L <= 2) return L - 1;
    const double x0 = log10((double)R[0]), y0 = log10((double)v[0]);
    const double dx = log10((double)R[L - 1]) - x0, dy = log10((double)v[L - 1]) - y0;
    uint64_t best = 0;
    double best_s = 0.0;
    bool have = false;
    for (uint64_t j = 0; j < L; ++j) {
        const double x = log10((double)R[j]), y = log10((double)v[j]);
        const double a = (y - y0) * dx, b = (x - x0) * dy;
        const double s = a - b;
        if (!have || s > best_s) { best = j; best_s = s; have = true; }
    }
    return best_s > 0.0 ? best : L - 1;
}

uint64_t threshold(const pa_knee_params& p, const uint32_t* v, const uint64_t* R, uint64_t D, uint64_t* L_out) {
    if (L_out) *L_out = 0;
    if (p.mode == PA_KNEE_MIN) return p.min_umis;
    if (p.mode == PA_KNEE_EXPECTED) {
        if (D == 0) return 1;
        const uint64_t B = R[D - 1];
        uint64_t r = p.expected_cells / EXPECTED_PERCENTILE;
        if (r > B - 1) r = B - 1;
        uint64_t j = 0;
        while (j + 1 < D && R[j] <= r) ++j;   // (R[D - 1] = B > r: the walk ends inside the curve)
        return ((uint64_t)v[j] + EXPECTED_DIVISOR - 1) / EXPECTED_DIVISOR;
    }
    uint64_t L = 0;
    while (L < D && v[L] >= p.lower) ++L;   // (v descends)
    if (L_out) *L_out = L;
    if (L == 0) return p.lower;
    const uint64_t k = curve_knee(v, R, L);
    const uint64_t t = ((uint64_t)v[k] + p.divisor - 1) / p.divisor;
    return t > p.lower ? t : p.lower;
}

int write_ranks_tsv(const pa_bus_barcode_row* rows, uint64_t n, uint32_t bc_len, const char* path) {
    if (!path || (n && !rows)) return fail(PA_ERR_INVALID_ARG, "null argument");
    if (bc_len < 1 || bc_len > 31) return fail(PA_ERR_UNSUPPORTED, "barcode length %u: 1..31 bases", bc_len);
    FILE* f = fopen(path, "wb");
    if (!f) return fail(PA_ERR_IO, "cannot write %s", path);
    std::string s = "barcode\trecords\tumis\treads\trank\tcalled\n";
    char line[160];
    for (uint64_t i = 0; i < n; ++i) {
        const pa_bus_barcode_row& r = rows[i];
        for (uint32_t j = 0; j < bc_len; ++j) line[j] = "ACGT"[(r.barcode >> (2 * (bc_len - 1 - j))) & 3u];
        const int m = snprintf(line + bc_len, sizeof line - bc_len, "\t%u\t%u\t%llu\t%u\t%u\n", r.records, r.umis, (ull)r.reads, r.rank, r.called);
        s.append(line, bc_len + (size_t)m);
        if (s.size() >= (1u << 20) || i + 1 == n) {
            if (fwrite(s.data(), 1, s.size(), f) != s.size()) { fclose(f); return fail(PA_ERR_IO, "cannot write %s", path); }
            s.clear();
        }
    }
    if (!s.empty() && fwrite(s.data(), 1, s.size(), f) != s.size()) { fclose(f); return fail(PA_ERR_IO, "cannot write %s", path); }
    if (fclose(f) != 0) return fail(PA_ERR_IO, "cannot write %s", path);
    return PA_OK;
}

}  // namespace knee
}  // namespace pa

extern "C" void pa_knee_default_params(pa_knee_params* p) {
    if (!p) return;
    *p = pa_knee_params{};
    p->mode = PA_KNEE_CURVE;
    p->lower = 10;
    p->divisor = 10;
    p->expected_cells = 3000;
    p->min_umis = 1;
}

extern "C" int pa_write_barcode_ranks_tsv(const pa_bus_barcode_row* rows, uint64_t n, uint32_t bc_len, const char* path) {
    return pa::knee::write_ranks_tsv(rows, n, bc_len, path);
}
