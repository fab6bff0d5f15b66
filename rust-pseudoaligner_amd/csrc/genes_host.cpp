// Host half of the gene counter: see genes_host.hpp. No HIP in this file.
#include "genes_host.hpp"

#include <sys/stat.h>

#include <algorithm>
#include <cerrno>
#include <charconv>
#include <cmath>
#include <unordered_set>

#include "bus_records_host.hpp"

namespace pa {
namespace genes {

typedef unsigned long long ull;

uint64_t set_hash(const uint32_t* v, uint32_t n) {
    uint64_t h = 0x243f6a8885a308d3ull ^ n;
    for (uint32_t i = 0; i < n; ++i) h = mix64(h ^ v[i]) + 0x9e3779b97f4a7c15ull;
    return h;
}

int check_params(const pa_genes_params& p) {
    const double d[3] = {p.alpha_limit, p.alpha_change_limit, p.alpha_change};
    for (double x : d)
        if (!(x == x) || std::isinf(x) || x < 0.0) return fail(PA_ERR_INVALID_ARG, "gene counter parameters: limits must be finite and not negative");
    if (p.check_every < 1) return fail(PA_ERR_INVALID_ARG, "gene counter parameters: check_every at least 1");
    if (p.mode != PA_GENES_EM && p.mode != PA_GENES_UNIQUE) return fail(PA_ERR_INVALID_ARG, "gene counter mode %u: PA_GENES_EM or PA_GENES_UNIQUE", p.mode);
    return PA_OK;
}

int check_lengths(uint32_t bc_len, uint32_t umi_len) { return bus_records::check_lengths(bc_len, umi_len, PA_ERR_INVALID_ARG, ""); }

int check_tables(const uint64_t* ec_offsets, const uint32_t* ec_ids, uint32_t n_ecs, uint32_t num_tx, const uint32_t* tx_gene, uint32_t num_genes) {
    if (!ec_offsets || (num_tx && !tx_gene)) return fail(PA_ERR_INVALID_ARG, "null argument");
    if (n_ecs > 0x7FFFFFFFu) return fail(PA_ERR_INVALID_ARG, "%u ecs: at most 2^31-1", n_ecs);
    if (ec_offsets[0] != 0) return fail(PA_ERR_INVALID_ARG, "ec table: offsets[0] is %llu, not 0", (ull)ec_offsets[0]);
    for (uint32_t t = 0; t < num_tx; ++t)
        if (tx_gene[t] >= num_genes) return fail(PA_ERR_INVALID_ARG, "tx_gene[%u] = %u is no gene (there are %u)", t, tx_gene[t], num_genes);
    for (uint32_t e = 0; e < n_ecs; ++e) {
        if (ec_offsets[e + 1] < ec_offsets[e]) return fail(PA_ERR_INVALID_ARG, "ec table: offsets descend at ec %u", e);
        if (ec_offsets[e + 1] > ec_offsets[e] && !ec_ids) return fail(PA_ERR_INVALID_ARG, "null argument");
        for (uint64_t j = ec_offsets[e]; j < ec_offsets[e + 1]; ++j) {
            if (ec_ids[j] >= num_tx) return fail(PA_ERR_INVALID_ARG, "ec %u: id %u is no transcript (there are %u)", e, ec_ids[j], num_tx);
            if (j > ec_offsets[e] && ec_ids[j] <= ec_ids[j - 1]) return fail(PA_ERR_INVALID_ARG, "ec %u: its ids are not ascending", e);
        }
    }
    if (ec_offsets[n_ecs] > 0x7FFFFFFFull) return fail(PA_ERR_UNSUPPORTED, "an ec table of more than 2^31-1 ids");
    return PA_OK;
}

int check_records(const pa_bus_record* records, uint64_t n, uint32_t n_ecs) {
    return bus_records::walk(records, n, [&](const pa_bus_record& r) { return r.ec < 0 || (uint32_t)r.ec >= n_ecs; },
                             [&](uint64_t i, const pa_bus_record& r) { return fail(PA_ERR_INVALID_ARG, "record %llu: ec %d is outside [0, %u)", (ull)i, r.ec, n_ecs); });
}

void gene_sets(const uint64_t* ec_offsets, const uint32_t* ec_ids, uint32_t n_ecs, const uint32_t* tx_gene, GeneSets& out) {
    out.off.assign((size_t)n_ecs + 1, 0);
    out.ids.clear();
    out.hash.assign(n_ecs, 0);
    std::vector<uint32_t> g;
    for (uint32_t e = 0; e < n_ecs; ++e) {
        g.clear();
        for (uint64_t j = ec_offsets[e]; j < ec_offsets[e + 1]; ++j) g.push_back(tx_gene[ec_ids[j]]);
        std::sort(g.begin(), g.end());
        g.erase(std::unique(g.begin(), g.end()), g.end());
        out.hash[e] = set_hash(g.data(), (uint32_t)g.size());
        out.ids.insert(out.ids.end(), g.begin(), g.end());
        out.off[e + 1] = out.ids.size();
    }
}

std::string decode_barcode(uint64_t barcode, uint32_t bc_len) {
    std::string s(bc_len, 'A');
    for (uint32_t j = 0; j < bc_len; ++j) s[j] = "ACGT"[(barcode >> (2 * (bc_len - 1 - j))) & 3u];
    return s;
}

std::string f64_text(double v) {
    if (v != v) return "NaN";
    char buf[400];
    const auto r = std::to_chars(buf, buf + sizeof buf, v, std::chars_format::fixed);
    return std::string(buf, r.ptr);
}

std::string matrix_text(uint32_t num_genes, uint64_t n_cells, const uint32_t* cell, const uint32_t* gene, const double* value, uint64_t n) {
    std::string s = "%%MatrixMarket matrix coordinate real general\n";
    s += std::to_string(num_genes) + " " + std::to_string(n_cells) + " " + std::to_string(n) + "\n";
    for (uint64_t i = 0; i < n; ++i) {
        s += std::to_string(gene[i] + 1);
        s += ' ';
        s += std::to_string(cell[i] + 1);
        s += ' ';
        s += f64_text(value[i]);
        s += '\n';
    }
    return s;
}

std::string barcodes_text(const uint64_t* barcodes, uint64_t n_cells, uint32_t bc_len) {
    std::string s;
    s.reserve((size_t)n_cells * (bc_len + 1));
    for (uint64_t c = 0; c < n_cells; ++c) {
        s += decode_barcode(barcodes[c], bc_len);
        s += '\n';
    }
    return s;
}

int features_text(const std::vector<std::string>& tx_genes, uint32_t num_genes, std::string& out) {
    out.clear();
    std::unordered_set<std::string> seen;
    for (const std::string& g : tx_genes) {
        if (!seen.insert(g).second) continue;
        out += g;
        out += '\t';
        out += g;
        out += "\tGene Expression\n";
    }
    if (seen.size() != num_genes) return fail(PA_ERR_INVALID_ARG, "the host index names %zu genes, the counter has %u", seen.size(), num_genes);
    return PA_OK;
}

static int write_text(const std::string& path, const std::string& text) {
    FILE* f = fopen(path.c_str(), "wb");
    if (!f) return fail(PA_ERR_IO, "cannot create %s: %s", path.c_str(), strerror(errno));
    const bool ok = fwrite(text.data(), 1, text.size(), f) == text.size();
    if (fclose(f) != 0 || !ok) return fail(PA_ERR_IO, "cannot write %s", path.c_str());
    return PA_OK;
}

int write_files(const char* out_dir, const std::string& matrix, const std::string& barcodes, const std::string& features) {
    struct stat sd;
    if (stat(out_dir, &sd) != 0 || !S_ISDIR(sd.st_mode)) return fail(PA_ERR_IO, "%s is no directory", out_dir);
    const std::string dir(out_dir);
    int e;
    if ((e = write_text(dir + "/matrix.mtx", matrix)) != PA_OK || (e = write_text(dir + "/barcodes.tsv", barcodes)) != PA_OK ||
        (e = write_text(dir + "/features.tsv", features)) != PA_OK)
        return e;
    return PA_OK;
}

}  // namespace genes
}  // namespace pa
