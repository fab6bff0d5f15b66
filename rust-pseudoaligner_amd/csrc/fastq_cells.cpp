// The barcoded drivers over PAIRED FASTQ files: R1 is a prefix of barcode + UMI bytes that is never encoded or mapped, R2 is mapped. pa_count_cells -> the
// cells x genes UMI matrix (pa_cell_counter), pa_write_bus -> sorted (barcode, UMI, class) records (pa_bus), pa_count_cells_em -> those records shared out
// over genes by a per-cell EM (pa_genes); with the barcode whitelist's reader. Reader,
// batches, loop and call frame are pair_reader.hpp's; a mapping that ran out of arena goes through map_finish_regrow (hip_buffer.hpp).
#include <hip/hip_runtime.h>
#include <sys/stat.h>
#include <zlib.h>

#include <algorithm>
#include <cerrno>
#include <cstdio>
#include <memory>
#include <string>
#include <unordered_set>

#include "bus_knee_host.hpp"
#include "bus_umi_host.hpp"
#include "pair_reader.hpp"

using namespace pa;
using namespace pa::ingest;

// ---- the barcode whitelist ----

extern "C" int pa_whitelist_load(const char* path, uint32_t bc_len, char* out, uint64_t cap, uint64_t* n) {
    if (!path || !n) return fail(PA_ERR_INVALID_ARG, "null argument");
    if (bc_len < 1 || bc_len > 16) return fail(PA_ERR_INVALID_ARG, "barcode length %u: must be 1..16", bc_len);
    *n = 0;
    gzFile g = gzopen(path, "rb");   // (plain text reads through as it is)
    if (!g) return fail(PA_ERR_IO, "cannot open %s: %s", path, strerror(errno));
    std::vector<char> text;
    {
        char buf[1 << 16];
        for (;;) {
            const int got = gzread(g, buf, sizeof buf);
            if (got < 0) { int e = 0; const char* why = gzerror(g, &e); const int rc = fail(PA_ERR_FORMAT, "%s: corrupt gzip stream: %s", path, why); gzclose(g); return rc; }
            if (got == 0) break;
            text.insert(text.end(), buf, buf + got);
        }
    }
    gzclose(g);
    std::vector<uint32_t> seen;   // packed barcodes (first base most significant) of the lines so far, for the duplicate check
    uint64_t count = 0, line = 0;
    for (size_t p = 0; p < text.size();) {
        const char* nl = (const char*)memchr(text.data() + p, '\n', text.size() - p);
        size_t e = nl ? (size_t)(nl - text.data()) : text.size();
        const size_t next = nl ? e + 1 : text.size();
        if (e > p && text[e - 1] == '\r') --e;
        ++line;
        if (e - p != bc_len) return fail(PA_ERR_FORMAT, "%s: line %llu has %zu bytes, a barcode has %u", path, (unsigned long long)line, e - p, bc_len);
        uint32_t bc = 0;
        for (size_t j = p; j < e; ++j) {
            const char c = text[j];
            const uint32_t b = c == 'A' ? 0u : c == 'C' ? 1u : c == 'G' ? 2u : c == 'T' ? 3u : 4u;
            if (b > 3) return fail(PA_ERR_FORMAT, "%s: line %llu: byte %zu is not A, C, G or T", path, (unsigned long long)line, j - p + 1);
            bc = (bc << 2) | b;
        }
        if (out && count < cap) memcpy(out + count * bc_len, text.data() + p, bc_len);
        seen.push_back(bc);
        ++count;
        p = next;
    }
    std::vector<uint64_t> order(seen.size());
    for (uint64_t i = 0; i < order.size(); ++i) order[i] = i;
    std::sort(order.begin(), order.end(), [&](uint64_t a, uint64_t b) { return seen[a] != seen[b] ? seen[a] < seen[b] : a < b; });
    for (uint64_t i = 1; i < order.size(); ++i)
        if (seen[order[i]] == seen[order[i - 1]])
            return fail(PA_ERR_FORMAT, "%s: line %llu repeats the barcode of line %llu", path, (unsigned long long)order[i] + 1, (unsigned long long)order[i - 1] + 1);
    *n = count;
    if (out && cap < count) return fail(PA_ERR_BUFFER_TOO_SMALL, "%s holds %llu barcodes, room for %llu", path, (unsigned long long)count, (unsigned long long)cap);
    return PA_OK;
}

namespace {

// the batch's GPU leg up to the mapping: copies, encode, map (asynchronous on s)
int cell_batch_map(pa_index* idx, MateBatch& b, hipStream_t s) {
    Mate& r2 = b.mate[1];
    int e = PA_OK;
    if ((e = r2.encode(idx, b.n, 0, s)) != PA_OK || (e = b.mate[0].to_device(b.n, s)) != PA_OK) return e;
    return r2.map(idx, r2.d_tiles.get(), b.n, PA_DEFAULT_ALLOWED_MISMATCHES, s);
}

// waits for the mapping (regrowing the arena as pa_map_finish asks), then hands the batch to consume(r1, r2, n): the counter's or the BUS stage's add
template <class Consume>
int cell_batch_finish(pa_index* idx, MateBatch& b, hipStream_t s, double* st, Consume&& consume) {
    double t0 = now();
    Mate &r1 = b.mate[0], &r2 = b.mate[1];
    uint64_t used = 0;
    int e = map_finish_regrow(idx, s, r2.d_arena, &used, [&] { return r2.map(idx, r2.d_tiles.get(), b.n, PA_DEFAULT_ALLOWED_MISMATCHES, s); });
    st[ST_WAIT] += now() - t0;
    if (e != PA_OK) return e;
    t0 = now();
    e = consume(r1, r2, b.n);
    st[ST_TALLY] += now() - t0;
    return e;
}

// both drivers' batches: mapped on the call's one stream, finished into `consume`
template <class Consume>
int run_cell_batches(pa_index* idx, PairedCall& call, MateBatch (&batches)[2], Consume&& consume) {
    hipStream_t s = call.s[0];
    return run_batches(*call.rd, batches, [&](MateBatch& b) { return cell_batch_map(idx, b, s); }, [&](MateBatch& b) { return cell_batch_finish(idx, b, s, call.st, consume); });
}

int write_text(const std::string& path, const std::string& text) {
    FILE* f = fopen(path.c_str(), "wb");
    if (!f) return fail(PA_ERR_IO, "cannot create %s: %s", path.c_str(), strerror(errno));
    const bool ok = fwrite(text.data(), 1, text.size(), f) == text.size();
    if (fclose(f) != 0 || !ok) return fail(PA_ERR_IO, "cannot write %s", path.c_str());
    return PA_OK;
}

int count_cells_impl(pa_index* idx, const pa_host_index* h, const char* r1_path, const char* r2_path, const char* whitelist_path, uint32_t bc_len,
                     uint32_t umi_len, const char* out_dir, int num_threads, uint64_t* stats) {
    std::unique_ptr<pa_cell_counter, void (*)(pa_cell_counter*)> own(nullptr, pa_cell_counter_destroy);   // (in front of the frame: destroyed behind its streams)
    PairedCall call(num_threads);
    double* const st = call.st;
    if (!idx || !h || !r1_path || !r2_path || !whitelist_path || !out_dir) return fail(PA_ERR_INVALID_ARG, "null argument");
    if (bc_len < 1 || bc_len > 16 || umi_len < 1 || umi_len > 16) return fail(PA_ERR_INVALID_ARG, "barcode length %u / UMI length %u: both must be 1..16", bc_len, umi_len);
    struct stat sd;
    if (stat(out_dir, &sd) != 0 || !S_ISDIR(sd.st_mode)) return fail(PA_ERR_IO, "%s is no directory", out_dir);
    uint64_t n_wl = 0;
    int rc = pa_whitelist_load(whitelist_path, bc_len, nullptr, 0, &n_wl);
    if (rc != PA_OK) return rc;
    std::vector<char> wl((size_t)n_wl * bc_len + 1);
    if ((rc = pa_whitelist_load(whitelist_path, bc_len, wl.data(), n_wl, &n_wl)) != PA_OK) return rc;
    const uint32_t ntx = pa_host_index_num_transcripts(h);
    std::vector<uint32_t> tx_gene(ntx ? ntx : 1);
    uint32_t num_genes = 0;
    if ((rc = pa_host_index_genes(h, tx_gene.data(), &num_genes)) != PA_OK) return rc;
    pa_cell_counter* counter = nullptr;
    if ((rc = pa_cell_counter_create(idx, h, tx_gene.data(), num_genes, wl.data(), n_wl, bc_len, umi_len, &counter)) != PA_OK) return rc;
    own.reset(counter);
    const uint32_t prefix = bc_len + umi_len;

    if ((rc = call.open(idx, r1_path, r2_path, prefix, 1, 1)) != PA_OK) return rc;
    Pool& pool = *call.pool;
    hipStream_t s = call.s[0];
    MateBatch batches[2];
    rc = run_cell_batches(idx, call, batches, [&](Mate& r1, Mate& r2, uint64_t n) {
        return pa_cell_counter_add_device(counter, r2.d_results.get(), r2.d_arena.get(), r1.d_bytes.get(), r1.d_off.get(), n, s);
    });
    if (rc != PA_OK) return rc;
    double t0 = now();
    uint64_t entries = 0;
    if ((rc = pa_cell_counter_finish(counter, &entries)) != PA_OK) return rc;
    st[ST_TALLY] += now() - t0;
    t0 = now();
    std::vector<uint32_t> cell(entries), gene(entries), umis(entries);
    if ((rc = pa_cell_counter_matrix(counter, cell.data(), gene.data(), umis.data(), entries)) != PA_OK) return rc;
    // columns: the cells with at least one UMI, in whitelist order (the matrix is sorted by cell)
    std::string bc_text, mtx;
    std::vector<uint32_t> column(entries);
    uint32_t cols = 0;
    for (uint64_t i = 0; i < entries; ++i) {
        if (i == 0 || cell[i] != cell[i - 1]) {
            bc_text.append(wl.data() + (size_t)cell[i] * bc_len, bc_len);
            bc_text.push_back('\n');
            ++cols;
        }
        column[i] = cols;
    }
    char head[96];
    snprintf(head, sizeof head, "%%%%MatrixMarket matrix coordinate integer general\n%u %u %llu\n", num_genes, cols, (unsigned long long)entries);
    // "gene cell umis" lines, rendered in pieces on the pool (a matrix has millions of entries; one formatted print per line cost
    // most of the call)
    auto put_u32 = [](char* p, uint32_t v) {   // decimal digits of v at p; returns the end
        char tmp[10];
        int n = 0;
        do { tmp[n++] = (char)('0' + v % 10); v /= 10; } while (v);
        while (n) *p++ = tmp[--n];
        return p;
    };
    const int pieces = std::max(1, std::min<int>(pool.size() * 4, (int)(entries / 4096) + 1));
    std::vector<std::string> piece((size_t)pieces);
    pool.run(pieces, [&](int t) {
        const uint64_t a = entries * (uint64_t)t / pieces, b = entries * (uint64_t)(t + 1) / pieces;
        std::string& o = piece[(size_t)t];
        o.resize((size_t)(b - a) * 33);
        char* p = &o[0];
        for (uint64_t i = a; i < b; ++i) {
            p = put_u32(p, gene[i] + 1); *p++ = ' ';
            p = put_u32(p, column[i]); *p++ = ' ';
            p = put_u32(p, umis[i]); *p++ = '\n';
        }
        o.resize((size_t)(p - o.data()));
    });
    mtx = head;
    size_t mtx_len = mtx.size();
    for (const std::string& x : piece) mtx_len += x.size();
    mtx.reserve(mtx_len);
    for (const std::string& x : piece) mtx += x;
    // gene names numbered as pa_host_index_genes numbers them (first appearance in transcript order), built once: the name lookup
    // of the C ABI rebuilds that table on every call
    std::string features;
    {
        std::unordered_set<std::string> seen;
        for (const std::string& g : h->h.tx_genes) {
            if (!seen.insert(g).second) continue;
            features += g;
            features += '\t';
            features += g;
            features += "\tGene Expression\n";
        }
        if (seen.size() != num_genes) return fail(PA_ERR_INTERNAL, "%zu gene names for %u genes", seen.size(), num_genes);
    }
    const std::string dir(out_dir);
    if ((rc = write_text(dir + "/matrix.mtx", mtx)) != PA_OK || (rc = write_text(dir + "/barcodes.tsv", bc_text)) != PA_OK ||
        (rc = write_text(dir + "/features.tsv", features)) != PA_OK)
        return rc;
    st[ST_WRITE] = now() - t0;
    if (stats) (void)pa_cell_counter_stats(counter, stats);
    call.done();
    return PA_OK;
}

// ---- pa_write_bus / pa_count_cells_em: the same two files -> sorted (barcode, UMI, ec) records in HBM, then `after(bus, st)`: the writer's three files, or
// the gene stage and its three files (after() adds its own seconds to st[ST_TALLY] / st[ST_WRITE]). With a whitelist file (the *_corrected calls) the
// barcodes of the finished records are corrected against it in HBM before `after` sees them (pa_bus_correct; its seconds go to st[ST_TALLY]); with a knee (the
// *_called calls) cells are called there too (pa_bus_knee, then pa_bus_correct or pa_bus_keep; st[ST_TALLY], the table's file st[ST_WRITE]); the *_umi calls take
// both as options and correct the UMIs behind them (pa_bus_umi_correct; st[ST_TALLY]) ----
struct BusWhitelist {
    const char* path = nullptr;   // nullptr: no correction
    uint64_t* stats = nullptr;    // [PA_BUS_CORRECT_STATS], may be nullptr
};

// Cell calling (the *_called calls; pa_bus_knee): without a whitelist file the called barcodes ARE the whitelist of the correction; with one the
// corrected records are ranked and the uncalled barcodes filtered out (pa_bus_keep). Either way out_dir/barcode_ranks.tsv holds the knee's table
struct BusKnee {
    bool on = false;
    const pa_knee_params* params = nullptr;   // nullptr: the defaults
    uint64_t* stats = nullptr;                // [PA_KNEE_STATS], may be nullptr
};

// UMI correction (the *_umi calls; pa_bus_umi_correct with the host index's genes): always the last of the record steps, behind correction and cell calling
struct BusUmi {
    bool on = false;
    uint32_t mode = PA_UMI_GREATEST;
    uint64_t* stats = nullptr;                // [PA_BUS_UMI_STATS], may be nullptr
};

// after pa_bus_finish: correction and cell calling in the order the two inputs ask for; the seconds of the table's file go to *write_seconds
int bus_call_cells(pa_bus* bus, const BusWhitelist& wl, const std::vector<uint64_t>& packed, const BusKnee& knee, uint32_t bc_len, const char* out_dir, double* write_seconds) {
    int rc = PA_OK;
    if (wl.path && (rc = pa_bus_correct(bus, packed.data(), packed.size(), wl.stats)) != PA_OK) return rc;
    if (!knee.on) return PA_OK;
    std::vector<pa_bus_barcode_row> rows;
    std::vector<uint64_t> called;
    uint64_t ks[PA_KNEE_STATS] = {};
    if ((rc = pa_bus_knee_vectors(bus, knee.params, rows, called, ks)) != PA_OK) return rc;
    if (knee.stats) memcpy(knee.stats, ks, sizeof ks);
    if (called.empty()) return fail(PA_ERR_FORMAT, "no barcode reaches the threshold of %llu molecules", (unsigned long long)ks[6]);
    // listed barcodes are only filtered (a second correction would move listed, uncalled barcodes into called neighbours); unlisted ones are corrected against the called
    rc = wl.path ? pa_bus_keep(bus, called.data(), called.size(), nullptr) : pa_bus_correct(bus, called.data(), called.size(), wl.stats);
    if (rc != PA_OK) return rc;
    const double t0 = now();
    if ((rc = pa_write_barcode_ranks_tsv(rows.data(), rows.size(), bc_len, (std::string(out_dir) + "/barcode_ranks.tsv").c_str())) != PA_OK) return rc;
    *write_seconds = now() - t0;
    return PA_OK;
}

template <class After>
int bus_run(pa_index* idx, const pa_host_index* h, const char* r1_path, const char* r2_path, const BusWhitelist& wl, const BusKnee& knee, const BusUmi& umi, uint32_t bc_len,
            uint32_t umi_len, const char* out_dir, int num_threads, After&& after) {
    std::unique_ptr<pa_bus, void (*)(pa_bus*)> own(nullptr, pa_bus_destroy);   // (in front of the frame: destroyed behind its streams)
    PairedCall call(num_threads);
    double* const st = call.st;
    if (!idx || !h || !r1_path || !r2_path || !out_dir) return fail(PA_ERR_INVALID_ARG, "null argument");
    struct stat sd;
    if (stat(out_dir, &sd) != 0 || !S_ISDIR(sd.st_mode)) return fail(PA_ERR_IO, "%s is no directory", out_dir);
    int rc = PA_OK;
    pa_knee_params knee_checked;
    if (knee.on && (rc = pa::knee::take_params(knee.params, knee_checked)) != PA_OK) return rc;   // refused before a read is mapped, like the whitelist
    if (umi.on && (rc = pa::umi::check_mode(umi.mode)) != PA_OK) return rc;
    std::vector<uint64_t> packed;
    if (wl.path) {   // the whitelist first: a file that cannot be used is refused before a read is mapped
        if (bc_len > 16) return fail(PA_ERR_UNSUPPORTED, "barcode length %u: a whitelist file holds barcodes of at most 16 bases", bc_len);
        uint64_t n_wl = 0;
        if ((rc = pa_whitelist_load(wl.path, bc_len, nullptr, 0, &n_wl)) != PA_OK) return rc;
        std::vector<char> text((size_t)n_wl * bc_len + 1);
        packed.resize((size_t)n_wl + 1);
        if ((rc = pa_whitelist_load(wl.path, bc_len, text.data(), n_wl, &n_wl)) != PA_OK || (rc = pa_bus_whitelist_pack(text.data(), n_wl, bc_len, packed.data())) != PA_OK)
            return rc;
        packed.resize((size_t)n_wl);
        if (packed.empty()) return fail(PA_ERR_INVALID_ARG, "%s holds no barcode", wl.path);
    }
    pa_bus* bus = nullptr;
    if ((rc = pa_bus_create(idx, h, bc_len, umi_len, &bus)) != PA_OK) return rc;
    own.reset(bus);

    if ((rc = call.open(idx, r1_path, r2_path, bc_len + umi_len, 1, 1)) != PA_OK) return rc;
    hipStream_t s = call.s[0];
    MateBatch batches[2];
    rc = run_cell_batches(idx, call, batches, [&](Mate& r1, Mate& r2, uint64_t n) {
        return pa_bus_add_device(bus, r2.d_results.get(), r2.d_arena.get(), r2.d_arena.size(), r1.d_bytes.get(), r1.d_off.get(), n, s);
    });
    if (rc != PA_OK) return rc;
    double t0 = now();
    uint64_t n_records = 0;
    uint32_t n_ecs = 0;
    if ((rc = pa_bus_finish(bus, &n_records, &n_ecs)) != PA_OK) return rc;
    double ranks_seconds = 0.0;
    if ((rc = bus_call_cells(bus, wl, packed, knee, bc_len, out_dir, &ranks_seconds)) != PA_OK) return rc;
    if (umi.on) {
        const uint32_t ntx = pa_host_index_num_transcripts(h);
        std::vector<uint32_t> tx_gene(ntx ? ntx : 1);
        uint32_t num_genes = 0;
        if ((rc = pa_host_index_genes(h, tx_gene.data(), &num_genes)) != PA_OK || (rc = pa_bus_umi_correct(bus, tx_gene.data(), num_genes, umi.mode, umi.stats)) != PA_OK) return rc;
    }
    st[ST_TALLY] += now() - t0 - ranks_seconds;
    if ((rc = after(bus, st)) != PA_OK) return rc;
    st[ST_WRITE] += ranks_seconds;
    call.done();
    return PA_OK;
}

int write_bus_impl(pa_index* idx, const pa_host_index* h, const char* r1_path, const char* r2_path, const BusWhitelist& wl, const BusKnee& knee, const BusUmi& umi,
                   uint32_t bc_len, uint32_t umi_len, const char* out_dir, int num_threads, uint64_t* stats) {
    return bus_run(idx, h, r1_path, r2_path, wl, knee, umi, bc_len, umi_len, out_dir, num_threads, [&](pa_bus* bus, double* st) {
        const double t0 = now();
        const int rc = pa_bus_write(bus, out_dir);
        if (rc != PA_OK) return rc;
        st[ST_WRITE] = now() - t0;
        if (stats) (void)pa_bus_stats(bus, stats);
        return (int)PA_OK;
    });
}

int count_cells_em_impl(pa_index* idx, const pa_host_index* h, const char* r1_path, const char* r2_path, const BusWhitelist& wl, const BusKnee& knee, const BusUmi& umi,
                        uint32_t bc_len, uint32_t umi_len, const pa_genes_params* p, const char* out_dir, int num_threads, uint64_t* stats) {
    return bus_run(idx, h, r1_path, r2_path, wl, knee, umi, bc_len, umi_len, out_dir, num_threads, [&](pa_bus* bus, double* st) {
        double t0 = now();
        const uint32_t ntx = pa_host_index_num_transcripts(h);
        std::vector<uint32_t> tx_gene(ntx ? ntx : 1);
        uint32_t num_genes = 0;
        int rc = pa_host_index_genes(h, tx_gene.data(), &num_genes);
        if (rc != PA_OK) return rc;
        pa_genes* g = nullptr;
        if ((rc = pa_genes_create_from_bus(bus, tx_gene.data(), num_genes, p, &g)) != PA_OK) return rc;
        std::unique_ptr<pa_genes, void (*)(pa_genes*)> own(g, pa_genes_destroy);
        if ((rc = pa_genes_run(g, nullptr, nullptr)) != PA_OK) return rc;
        st[ST_TALLY] += now() - t0;
        t0 = now();
        if ((rc = pa_genes_write(g, h, out_dir)) != PA_OK) return rc;
        st[ST_WRITE] = now() - t0;
        if (stats) (void)pa_genes_stats(g, stats);
        return (int)PA_OK;
    });
}

}  // namespace

extern "C" int pa_count_cells(pa_index* idx, const pa_host_index* h, const char* r1_path, const char* r2_path, const char* whitelist_path, uint32_t bc_len,
                              uint32_t umi_len, const char* out_dir, int num_threads, uint64_t stats[PA_CELL_STATS]) {
    return no_throw("pa_count_cells", [&] { return count_cells_impl(idx, h, r1_path, r2_path, whitelist_path, bc_len, umi_len, out_dir, num_threads, stats); });
}

extern "C" int pa_write_bus(pa_index* idx, const pa_host_index* h, const char* r1_path, const char* r2_path, uint32_t bc_len, uint32_t umi_len, const char* out_dir,
                            int num_threads, uint64_t stats[PA_BUS_STATS]) {
    return no_throw("pa_write_bus", [&] { return write_bus_impl(idx, h, r1_path, r2_path, BusWhitelist{}, BusKnee{}, BusUmi{}, bc_len, umi_len, out_dir, num_threads, stats); });
}

extern "C" int pa_count_cells_em(pa_index* idx, const pa_host_index* h, const char* r1_path, const char* r2_path, uint32_t bc_len, uint32_t umi_len, const pa_genes_params* p,
                                 const char* out_dir, int num_threads, uint64_t stats[PA_GENES_STATS]) {
    return no_throw("pa_count_cells_em", [&] { return count_cells_em_impl(idx, h, r1_path, r2_path, BusWhitelist{}, BusKnee{}, BusUmi{}, bc_len, umi_len, p, out_dir, num_threads, stats); });
}

extern "C" int pa_write_bus_corrected(pa_index* idx, const pa_host_index* h, const char* r1_path, const char* r2_path, const char* whitelist_path, uint32_t bc_len,
                                      uint32_t umi_len, const char* out_dir, int num_threads, uint64_t bus_stats[PA_BUS_STATS], uint64_t correct_stats[PA_BUS_CORRECT_STATS]) {
    return no_throw("pa_write_bus_corrected", [&] {
        if (!whitelist_path) return fail(PA_ERR_INVALID_ARG, "null argument");
        return write_bus_impl(idx, h, r1_path, r2_path, BusWhitelist{whitelist_path, correct_stats}, BusKnee{}, BusUmi{}, bc_len, umi_len, out_dir, num_threads, bus_stats);
    });
}

extern "C" int pa_count_cells_em_corrected(pa_index* idx, const pa_host_index* h, const char* r1_path, const char* r2_path, const char* whitelist_path, uint32_t bc_len,
                                           uint32_t umi_len, const pa_genes_params* p, const char* out_dir, int num_threads, uint64_t genes_stats[PA_GENES_STATS],
                                           uint64_t correct_stats[PA_BUS_CORRECT_STATS]) {
    return no_throw("pa_count_cells_em_corrected", [&] {
        if (!whitelist_path) return fail(PA_ERR_INVALID_ARG, "null argument");
        return count_cells_em_impl(idx, h, r1_path, r2_path, BusWhitelist{whitelist_path, correct_stats}, BusKnee{}, BusUmi{}, bc_len, umi_len, p, out_dir, num_threads, genes_stats);
    });
}

extern "C" int pa_write_bus_called(pa_index* idx, const pa_host_index* h, const char* r1_path, const char* r2_path, const char* whitelist_path, uint32_t bc_len,
                                   uint32_t umi_len, const pa_knee_params* kp, const char* out_dir, int num_threads, uint64_t bus_stats[PA_BUS_STATS],
                                   uint64_t correct_stats[PA_BUS_CORRECT_STATS], uint64_t knee_stats[PA_KNEE_STATS]) {
    return no_throw("pa_write_bus_called", [&] {
        return write_bus_impl(idx, h, r1_path, r2_path, BusWhitelist{whitelist_path, correct_stats}, BusKnee{true, kp, knee_stats}, BusUmi{}, bc_len, umi_len, out_dir, num_threads, bus_stats);
    });
}

extern "C" int pa_count_cells_em_called(pa_index* idx, const pa_host_index* h, const char* r1_path, const char* r2_path, const char* whitelist_path, uint32_t bc_len,
                                        uint32_t umi_len, const pa_knee_params* kp, const pa_genes_params* p, const char* out_dir, int num_threads,
                                        uint64_t genes_stats[PA_GENES_STATS], uint64_t correct_stats[PA_BUS_CORRECT_STATS], uint64_t knee_stats[PA_KNEE_STATS]) {
    return no_throw("pa_count_cells_em_called", [&] {
        return count_cells_em_impl(idx, h, r1_path, r2_path, BusWhitelist{whitelist_path, correct_stats}, BusKnee{true, kp, knee_stats}, BusUmi{}, bc_len, umi_len, p, out_dir, num_threads,
                                   genes_stats);
    });
}

extern "C" int pa_write_bus_umi(pa_index* idx, const pa_host_index* h, const char* r1_path, const char* r2_path, const char* whitelist_path, uint32_t bc_len, uint32_t umi_len,
                                int call_cells, const pa_knee_params* kp, uint32_t umi_mode, const char* out_dir, int num_threads, uint64_t bus_stats[PA_BUS_STATS],
                                uint64_t correct_stats[PA_BUS_CORRECT_STATS], uint64_t knee_stats[PA_KNEE_STATS], uint64_t umi_stats[PA_BUS_UMI_STATS]) {
    return no_throw("pa_write_bus_umi", [&] {
        return write_bus_impl(idx, h, r1_path, r2_path, BusWhitelist{whitelist_path, correct_stats}, BusKnee{call_cells != 0, kp, knee_stats}, BusUmi{true, umi_mode, umi_stats},
                              bc_len, umi_len, out_dir, num_threads, bus_stats);
    });
}

extern "C" int pa_count_cells_em_umi(pa_index* idx, const pa_host_index* h, const char* r1_path, const char* r2_path, const char* whitelist_path, uint32_t bc_len, uint32_t umi_len,
                                     int call_cells, const pa_knee_params* kp, uint32_t umi_mode, const pa_genes_params* p, const char* out_dir, int num_threads,
                                     uint64_t genes_stats[PA_GENES_STATS], uint64_t correct_stats[PA_BUS_CORRECT_STATS], uint64_t knee_stats[PA_KNEE_STATS],
                                     uint64_t umi_stats[PA_BUS_UMI_STATS]) {
    return no_throw("pa_count_cells_em_umi", [&] {
        return count_cells_em_impl(idx, h, r1_path, r2_path, BusWhitelist{whitelist_path, correct_stats}, BusKnee{call_cells != 0, kp, knee_stats},
                                   BusUmi{true, umi_mode, umi_stats}, bc_len, umi_len, p, out_dir, num_threads, genes_stats);
    });
}
