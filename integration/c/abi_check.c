/* A plain-C client of include/pseudoaligner_amd.h that calls EVERY entry point of the header once, with the argument types a
 * foreign binding (integration/rust/src/amd_ffi.rs, rust-pseudoaligner_amd/_ffi.py) assumes. Compiled by __graft_entry__.build()
 * with gcc -Wall -Werror against the header, so a drifting prototype is a build error, not a run-time surprise; run by the
 * tests: without a GPU the host half runs and every device entry point must fail with PA_ERR_NO_DEVICE (no CPU fallback),
 * with a GPU the whole sequence runs on a toy transcriptome.
 *   usage: abi_check <fasta> <fastq> <scratch dir>          exit code 0 = every call behaved
 */
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "pseudoaligner_amd.h"

static int failures = 0;
#define EXPECT(cond)                                                                      \
    do {                                                                                  \
        if (!(cond)) { fprintf(stderr, "abi_check: %s:%d: %s (last error: %s)\n", __FILE__, __LINE__, #cond, pa_last_error()); ++failures; } \
    } while (0)

int main(int argc, char** argv) {
    if (argc < 4) { fprintf(stderr, "usage: %s <fasta> <fastq> <scratch dir>\n", argv[0]); return 2; }
    const char *fasta = argv[1], *fastq = argv[2], *dir = argv[3];
    char path[1024], report[256];

    /* the struct layouts as THIS compiler sees them, for the test that checks the #[repr(C)] structs of integration/rust/src/amd_ffi.rs
     * against them (tests/test_abi.py): "layout <struct> sizeof <n>" and "layout <struct>.<field> <offset>" */
#define LAYOUT_STRUCT(T) printf("layout %s sizeof %zu\n", #T, sizeof(T))
#define LAYOUT_FIELD(T, f) printf("layout %s.%s %zu\n", #T, #f, offsetof(T, f))
    LAYOUT_STRUCT(pa_flat_index);
    LAYOUT_FIELD(pa_flat_index, k); LAYOUT_FIELD(pa_flat_index, num_nodes); LAYOUT_FIELD(pa_flat_index, num_classes); LAYOUT_FIELD(pa_flat_index, num_transcripts);
    LAYOUT_FIELD(pa_flat_index, seq_bases); LAYOUT_FIELD(pa_flat_index, node_seq); LAYOUT_FIELD(pa_flat_index, node_start); LAYOUT_FIELD(pa_flat_index, node_len);
    LAYOUT_FIELD(pa_flat_index, node_exts); LAYOUT_FIELD(pa_flat_index, node_colour); LAYOUT_FIELD(pa_flat_index, ec_offset); LAYOUT_FIELD(pa_flat_index, ec_ids);
    LAYOUT_FIELD(pa_flat_index, node_redge); LAYOUT_FIELD(pa_flat_index, node_ledge);
    LAYOUT_STRUCT(pa_read_result);
    LAYOUT_FIELD(pa_read_result, coverage); LAYOUT_FIELD(pa_read_result, mismatches); LAYOUT_FIELD(pa_read_result, class_off); LAYOUT_FIELD(pa_read_result, class_len);
    LAYOUT_STRUCT(pa_index_stats);
    LAYOUT_FIELD(pa_index_stats, num_kmers); LAYOUT_FIELD(pa_index_stats, table_slots); LAYOUT_FIELD(pa_index_stats, bytes_table); LAYOUT_FIELD(pa_index_stats, bytes_graph);
    LAYOUT_FIELD(pa_index_stats, bytes_classes); LAYOUT_FIELD(pa_index_stats, bytes_total); LAYOUT_FIELD(pa_index_stats, num_nodes); LAYOUT_FIELD(pa_index_stats, num_classes);
    LAYOUT_FIELD(pa_index_stats, k); LAYOUT_FIELD(pa_index_stats, max_class_len);
    LAYOUT_STRUCT(pa_bus_record);   /* = the 32-byte record of a BUS file */
    LAYOUT_FIELD(pa_bus_record, barcode); LAYOUT_FIELD(pa_bus_record, umi); LAYOUT_FIELD(pa_bus_record, ec); LAYOUT_FIELD(pa_bus_record, count);
    LAYOUT_FIELD(pa_bus_record, flags); LAYOUT_FIELD(pa_bus_record, pad);
    EXPECT(sizeof(pa_bus_record) == 32 && offsetof(pa_bus_record, ec) == 16 && offsetof(pa_bus_record, pad) == 28);

    /* ---- host half ---- */
    EXPECT(pa_abi_version() == PA_ABI_VERSION);
    EXPECT(pa_last_error() != NULL);
    const int ndev = pa_device_count();
    pa_host_index *h = NULL, *h2 = NULL, *h3 = NULL, *h4 = NULL;
    EXPECT(pa_host_index_build_fasta(fasta, 20, 2, &h) == PA_OK && h);
    if (!h) return 1;
    pa_flat_index flat;
    EXPECT(pa_host_index_view(h, &flat) == PA_OK && flat.k == 20 && flat.num_nodes > 0);
    EXPECT(pa_host_index_from_flat(&flat, &h2) == PA_OK);
    EXPECT(pa_host_index_compare(h, h2, 1u << 20, report, sizeof report) == 0);
    snprintf(path, sizeof path, "%s/abi_check.idx", dir);
    EXPECT(pa_host_index_save(h, path) == PA_OK);
    EXPECT(pa_host_index_load(path, &h3) == PA_OK);
    const uint32_t ntx = pa_host_index_num_transcripts(h);
    EXPECT(ntx == flat.num_transcripts && pa_host_index_tx_name(h, 0) != NULL && pa_host_index_tx_gene(h, 0) != NULL);
    uint32_t ngenes = 0;
    uint32_t* tx_gene = (uint32_t*)calloc(ntx ? ntx : 1, 4);
    EXPECT(pa_host_index_genes(h, tx_gene, &ngenes) == PA_OK && ngenes >= 1 && pa_host_index_gene_name(h, 0) != NULL);
    const uint64_t counts_len = (uint64_t)flat.num_classes + 3;
    uint64_t* counts = (uint64_t*)calloc(counts_len, 8);
    uint64_t* gene_counts = (uint64_t*)calloc(ngenes + 1, 8);
    counts[0] = 5;
    EXPECT(pa_counts_collapse_genes(h, counts, counts_len, gene_counts) == PA_OK);
    uint64_t* mult = (uint64_t*)calloc((size_t)ntx * PA_MAPPABILITY_COUNTS_LEN, 8);
    EXPECT(pa_host_index_mappability(h, mult, NULL) == PA_OK);
    snprintf(path, sizeof path, "%s/abi_check_mappability.tsv", dir);
    EXPECT(pa_write_mappability_tsv(h, path) == PA_OK);
    const uint64_t *packed = NULL, *tx_start = NULL;
    uint32_t ntx2 = 0;
    EXPECT(pa_host_index_transcripts(h, &packed, &tx_start, &ntx2) == PA_OK && ntx2 == ntx);
    EXPECT(pa_host_index_build_packed(packed, tx_start, ntx2, 20, 1, &h4) == PA_OK);
    EXPECT(pa_host_index_compare(h, h4, 1u << 20, report, sizeof report) == 0);

    const uint8_t ascii[] = "ACGTACGTACGTTTGACCAGTNNAC";
    const uint64_t offsets[3] = {0, 12, 25};
    const uint32_t wpr = pa_words_per_read(13);
    EXPECT(wpr == 1 && pa_tiles_words(2, wpr) == 64);
    uint64_t tiles[64];
    uint32_t lens[2];
    EXPECT(pa_encode_reads_host(ascii, offsets, 2, wpr, tiles, lens) == PA_OK && lens[0] == 12 && lens[1] == 13);
    {   /* the scan stage of process_reads, no GPU needed */
        uint64_t nrec = 0, starts[4];
        uint32_t hdr[4], sq[4];
        int kind = -1;
        EXPECT(pa_fastq_scan_host(fastq, 2, &nrec, starts, hdr, sq, 4, &kind) == PA_OK && nrec > 4 && kind == 0 && starts[0] == 0 && sq[0] > 0 &&
               starts[1] > starts[0] + hdr[0] + sq[0]);
    }

    {   /* single-cell counting, host side: the whitelist file and argument checks that come before any device call */
        uint64_t nwl = 0;
        char wlb[4 * 4];
        FILE* f;
        snprintf(path, sizeof path, "%s/abi_check_whitelist.txt", dir);
        f = fopen(path, "w");
        if (f) { fputs("ACGT\r\nTTTT\nGGCA\n", f); fclose(f); }
        EXPECT(pa_whitelist_load(path, 4, NULL, 0, &nwl) == PA_OK && nwl == 3);
        EXPECT(pa_whitelist_load(path, 4, wlb, 4, &nwl) == PA_OK && memcmp(wlb, "ACGTTTTTGGCA", 12) == 0);
        EXPECT(pa_whitelist_load(path, 5, NULL, 0, &nwl) == PA_ERR_FORMAT);
        pa_cell_counter* cc = NULL;
        uint64_t cst[PA_CELL_STATS], nent = 0;
        EXPECT(pa_cell_counter_create(NULL, h, tx_gene, ngenes, "ACGT", 1, 4, 4, &cc) == PA_ERR_INVALID_ARG && cc == NULL);
        EXPECT(pa_cell_counter_create(NULL, h, tx_gene, ngenes, "ACGT", 1, 0, 4, &cc) == PA_ERR_INVALID_ARG);
        EXPECT(pa_cell_counter_add_device(NULL, NULL, NULL, NULL, NULL, 0, NULL) == PA_ERR_INVALID_ARG);
        EXPECT(pa_cell_counter_finish(NULL, &nent) == PA_ERR_INVALID_ARG);
        EXPECT(pa_cell_counter_matrix(NULL, NULL, NULL, NULL, 0) == PA_ERR_INVALID_ARG);
        EXPECT(pa_cell_counter_stats(NULL, cst) == PA_ERR_INVALID_ARG);
        pa_cell_counter_destroy(NULL);
        EXPECT(pa_count_cells(NULL, h, fastq, fastq, path, 4, 4, dir, 1, cst) == PA_ERR_INVALID_ARG);
        /* BUS output: every entry point refuses a null handle before any device call */
        pa_bus* bus = NULL;
        uint64_t bst[PA_BUS_STATS], nrec = 0, nids = 0;
        uint32_t necs = 0;
        EXPECT(pa_bus_create(NULL, h, 16, 12, &bus) == PA_ERR_INVALID_ARG && bus == NULL);
        EXPECT(pa_bus_add_device(NULL, NULL, NULL, 0, NULL, NULL, 0, NULL) == PA_ERR_INVALID_ARG);
        EXPECT(pa_bus_finish(NULL, &nrec, &necs) == PA_ERR_INVALID_ARG);
        EXPECT(pa_bus_records(NULL, NULL, 0) == PA_ERR_INVALID_ARG);
        EXPECT(pa_bus_ecs(NULL, NULL, NULL, 0, &nids) == PA_ERR_INVALID_ARG);
        EXPECT(pa_bus_stats(NULL, bst) == PA_ERR_INVALID_ARG);
        EXPECT(pa_bus_write(NULL, dir) == PA_ERR_INVALID_ARG);
        pa_bus_destroy(NULL);
        EXPECT(pa_write_bus(NULL, h, fastq, fastq, 4, 4, dir, 1, bst) == PA_ERR_INVALID_ARG);
    }

    {   /* transcript abundances, host side: the defaults, the struct as this compiler lays it out, and the checks that come before any device call */
        pa_quant_params qp;
        pa_quant* qq = NULL;
        uint64_t qst[PA_QUANT_STATS];
        uint32_t qit = 1;
        int qconv = 1;
        double qd[1];
        printf("layout pa_quant_params sizeof %zu\n", sizeof(pa_quant_params));
        LAYOUT_FIELD(pa_quant_params, mean_read_len); LAYOUT_FIELD(pa_quant_params, alpha_limit); LAYOUT_FIELD(pa_quant_params, alpha_change_limit);
        LAYOUT_FIELD(pa_quant_params, alpha_change); LAYOUT_FIELD(pa_quant_params, min_iters); LAYOUT_FIELD(pa_quant_params, max_iters);
        LAYOUT_FIELD(pa_quant_params, check_every); LAYOUT_FIELD(pa_quant_params, reserved);
        pa_quant_default_params(NULL);
        pa_quant_default_params(&qp);
        EXPECT(qp.min_iters == 50 && qp.max_iters == 10000 && qp.check_every == 10 && qp.alpha_limit == 1e-7 && qp.alpha_change == 1e-2 && qp.mean_read_len == 0.0);
        EXPECT(pa_quant_create(NULL, NULL, &qp, &qq) == PA_ERR_INVALID_ARG && qq == NULL);
        qp.check_every = 0;
        EXPECT(pa_quant_create(NULL, h, &qp, &qq) == PA_ERR_INVALID_ARG && qq == NULL);
        EXPECT(pa_quant_create(NULL, h, NULL, &qq) == (ndev < 1 ? PA_ERR_NO_DEVICE : PA_ERR_INVALID_ARG) && qq == NULL);
        EXPECT(pa_quant_set_counts(NULL, counts, counts_len, NULL, 0) == PA_ERR_INVALID_ARG);
        EXPECT(pa_quant_step(NULL, 1) == PA_ERR_INVALID_ARG && pa_quant_run(NULL, &qit, &qconv) == PA_ERR_INVALID_ARG && qit == 0 && qconv == 0);
        EXPECT(pa_quant_alpha(NULL, qd) == PA_ERR_INVALID_ARG && pa_quant_fetch(NULL, qd, NULL, NULL) == PA_ERR_INVALID_ARG);
        EXPECT(pa_quant_fetch_genes(NULL, qd, NULL) == PA_ERR_INVALID_ARG && pa_quant_stats(NULL, qst) == PA_ERR_INVALID_ARG);
        EXPECT(pa_write_abundance_tsv(NULL, path) == PA_ERR_INVALID_ARG);
        EXPECT(pa_quant_bootstrap_draw(NULL, 1, 0, 1) == PA_ERR_INVALID_ARG && pa_quant_bootstrap_counts(NULL, 0, counts, counts_len, NULL, 0) == PA_ERR_INVALID_ARG);
        EXPECT(pa_quant_bootstrap_step(NULL, 1) == PA_ERR_INVALID_ARG && pa_quant_bootstrap_run(NULL, &qit, &qconv) == PA_ERR_INVALID_ARG);
        EXPECT(pa_quant_bootstrap_fetch(NULL, qd, NULL) == PA_ERR_INVALID_ARG && PA_QUANT_BOOT_MAX_BATCH == 64);
        pa_quant_destroy(NULL);
    }

    {   /* cells x genes from BUS records, host side: the defaults, the struct's layout, and the refusals that come before any device call, on a two-cell hand-made input */
        pa_genes_params gp;
        pa_genes* gg = NULL;
        uint64_t gst[PA_GENES_STATS], gnc = 0, gnv = 0;
        uint32_t git = 1;
        /* cell 1: a molecule of gene 0, one of genes {0, 1}; cell 2: one molecule of two records whose genes meet in gene 1 */
        const pa_bus_record two_cells[4] = {{1, 0, 0, 1, 0, 0}, {1, 1, 2, 3, 0, 0}, {2, 0, 2, 1, 0, 0}, {2, 0, 3, 1, 0, 0}};
        pa_bus_record bad[4];
        const uint64_t goff[5] = {0, 1, 2, 4, 6};
        const uint32_t gids[6] = {0, 1, 0, 1, 1, 2}, gtx[3] = {0, 1, 2}, gtx_bad[3] = {0, 1, 3};
        LAYOUT_STRUCT(pa_genes_params);
        LAYOUT_FIELD(pa_genes_params, alpha_limit); LAYOUT_FIELD(pa_genes_params, alpha_change_limit); LAYOUT_FIELD(pa_genes_params, alpha_change);
        LAYOUT_FIELD(pa_genes_params, min_iters); LAYOUT_FIELD(pa_genes_params, max_iters); LAYOUT_FIELD(pa_genes_params, check_every);
        LAYOUT_FIELD(pa_genes_params, mode); LAYOUT_FIELD(pa_genes_params, reserved);
        pa_genes_default_params(NULL);
        pa_genes_default_params(&gp);
        EXPECT(gp.min_iters == 50 && gp.max_iters == 10000 && gp.check_every == 10 && gp.alpha_limit == 1e-7 && gp.alpha_change == 1e-2 && gp.mode == PA_GENES_EM);
        EXPECT(pa_genes_create(NULL, two_cells, 4, goff, gids, 4, 3, gtx, 3, 4, 4, &gp, NULL) == PA_ERR_INVALID_ARG);
        EXPECT(pa_genes_create(NULL, two_cells, 4, goff, gids, 4, 3, gtx, 3, 17, 16, &gp, &gg) == PA_ERR_INVALID_ARG && gg == NULL);
        EXPECT(pa_genes_create(NULL, two_cells, 4, goff, gids, 4, 3, gtx_bad, 3, 4, 4, &gp, &gg) == PA_ERR_INVALID_ARG && strstr(pa_last_error(), "tx_gene[2]"));
        EXPECT(pa_genes_create(NULL, two_cells, 4, goff, gids, 3, 3, gtx, 3, 4, 4, &gp, &gg) == PA_ERR_INVALID_ARG && strstr(pa_last_error(), "record 3"));
        memcpy(bad, two_cells, sizeof bad);
        bad[2].barcode = 1; bad[2].umi = 1;   /* equal to the record before it */
        EXPECT(pa_genes_create(NULL, bad, 4, goff, gids, 4, 3, gtx, 3, 4, 4, &gp, &gg) == PA_ERR_INVALID_ARG && strstr(pa_last_error(), "record 2"));
        gp.mode = 7;
        EXPECT(pa_genes_create(NULL, two_cells, 4, goff, gids, 4, 3, gtx, 3, 4, 4, &gp, &gg) == PA_ERR_INVALID_ARG);
        EXPECT(pa_genes_create(NULL, two_cells, 4, goff, gids, 4, 3, gtx, 3, 4, 4, NULL, &gg) == (ndev < 1 ? PA_ERR_NO_DEVICE : PA_ERR_INVALID_ARG) && gg == NULL);
        EXPECT(pa_genes_create_from_bus(NULL, gtx, 3, NULL, &gg) == PA_ERR_INVALID_ARG && gg == NULL);
        EXPECT(pa_genes_step(NULL, 1) == PA_ERR_INVALID_ARG && pa_genes_run(NULL, &git, &gnc) == PA_ERR_INVALID_ARG && git == 0);
        EXPECT(pa_genes_layout(NULL, &gnc, &gnv) == PA_ERR_INVALID_ARG && pa_genes_values(NULL, NULL, NULL, NULL, NULL, 0) == PA_ERR_INVALID_ARG);
        EXPECT(pa_genes_cell_iters(NULL, &git) == PA_ERR_INVALID_ARG && pa_genes_matrix(NULL, NULL, NULL, NULL, 0, &gnv) == PA_ERR_INVALID_ARG);
        EXPECT(pa_genes_stats(NULL, gst) == PA_ERR_INVALID_ARG && pa_genes_write(NULL, h, dir) == PA_ERR_INVALID_ARG);
        pa_genes_destroy(NULL);
        EXPECT(pa_count_cells_em(NULL, h, fastq, fastq, 4, 4, NULL, dir, 1, gst) == PA_ERR_INVALID_ARG);
    }

    {   /* BUS barcode correction, host side: the packer, and every refusal that comes before a device call */
        uint64_t wlp[3] = {0, 0, 0}, cst13[PA_BUS_CORRECT_STATS], cn = 7;
        float cms[PA_BUS_CORRECT_PHASES];
        const uint64_t cwl[3] = {27, 255, 164}, cwl_dup[3] = {27, 255, 27}, cwl_big[3] = {27, 256, 164};   /* ACGT TTTT GGCA */
        const pa_bus_record crec[3] = {{26, 0, 0, 1, 0, 0}, {27, 0, 0, 2, 0, 0}, {27, 1, 0, 1, 0, 0}};
        pa_bus_record cbad[3], cout[3];
        EXPECT(PA_BUS_CORRECT_STATS == 13 && PA_BUS_CORRECT_PHASES == 4);
        EXPECT(pa_bus_whitelist_pack("ACGTTTTTGGCA", 3, 4, wlp) == PA_OK && wlp[0] == 27 && wlp[1] == 255 && wlp[2] == 164);
        EXPECT(pa_bus_whitelist_pack("ACGTTTNTGGCA", 3, 4, wlp) == PA_ERR_INVALID_ARG && strstr(pa_last_error(), "entry 1"));
        EXPECT(pa_bus_whitelist_pack("ACGT", 1, 32, wlp) == PA_ERR_UNSUPPORTED);
        EXPECT(pa_bus_correct_records(NULL, crec, 3, 4, 4, cwl, 3, cout, 3, NULL, cst13) == PA_ERR_INVALID_ARG);
        EXPECT(pa_bus_correct_records(NULL, crec, 3, 17, 16, cwl, 3, cout, 3, &cn, cst13) == PA_ERR_UNSUPPORTED && cn == 0);
        EXPECT(pa_bus_correct_records(NULL, crec, 3, 4, 4, cwl_dup, 3, cout, 3, &cn, cst13) == PA_ERR_INVALID_ARG && strstr(pa_last_error(), "entry 0"));
        EXPECT(pa_bus_correct_records(NULL, crec, 3, 4, 4, cwl_big, 3, cout, 3, &cn, cst13) == PA_ERR_INVALID_ARG && strstr(pa_last_error(), "entry 1"));
        EXPECT(pa_bus_correct_records(NULL, crec, 3, 4, 4, cwl, 0, cout, 3, &cn, cst13) == PA_ERR_INVALID_ARG);
        memcpy(cbad, crec, sizeof cbad);
        cbad[2].umi = 0;   /* equal to the record before it */
        EXPECT(pa_bus_correct_records(NULL, cbad, 3, 4, 4, cwl, 3, cout, 3, &cn, cst13) == PA_ERR_INVALID_ARG && strstr(pa_last_error(), "record 2"));
        cbad[2].umi = 256;   /* no UMI of 4 bases */
        EXPECT(pa_bus_correct_records(NULL, cbad, 3, 4, 4, cwl, 3, cout, 3, &cn, cst13) == PA_ERR_INVALID_ARG && strstr(pa_last_error(), "record 2"));
        EXPECT(pa_bus_correct_records(NULL, crec, 3, 4, 4, cwl, 3, cout, 3, &cn, cst13) == (ndev < 1 ? PA_ERR_NO_DEVICE : PA_ERR_INVALID_ARG) && cn == 0);
        EXPECT(pa_bus_correct(NULL, cwl, 3, cst13) == PA_ERR_INVALID_ARG);
        EXPECT(pa_bus_correct_phase_ms(NULL) == PA_ERR_INVALID_ARG && pa_bus_correct_phase_ms(cms) == PA_OK);
        snprintf(path, sizeof path, "%s/abi_check_whitelist.txt", dir);
        EXPECT(pa_write_bus_corrected(NULL, h, fastq, fastq, path, 4, 4, dir, 1, NULL, cst13) == PA_ERR_INVALID_ARG);
        EXPECT(pa_count_cells_em_corrected(NULL, h, fastq, fastq, path, 4, 4, NULL, dir, 1, NULL, cst13) == PA_ERR_INVALID_ARG);
    }

    {   /* UMI correction on BUS records, host side: every refusal that comes before a device call */
        uint64_t ust[PA_BUS_UMI_STATS], un = 7;
        float ums[PA_BUS_UMI_PHASES];
        const uint64_t uoff[3] = {0, 1, 2};
        const uint32_t uids[2] = {0, 1}, utg[2] = {0, 1}, utg_bad[2] = {0, 2};
        const pa_bus_record urec[3] = {{27, 0, 0, 5, 0, 0}, {27, 1, 0, 1, 0, 0}, {27, 4, 1, 1, 0, 0}};
        pa_bus_record ubad[3], uout[3];
        EXPECT(PA_BUS_UMI_STATS == 15 && PA_BUS_UMI_PHASES == 4 && PA_UMI_GREATEST == 0 && PA_UMI_DIRECTIONAL == 1);
        EXPECT(pa_bus_umi_correct_records(NULL, urec, 3, uoff, uids, 2, 2, utg, 2, 4, 4, PA_UMI_GREATEST, uout, 3, NULL, ust) == PA_ERR_INVALID_ARG);
        EXPECT(pa_bus_umi_correct_records(NULL, urec, 3, uoff, uids, 2, 2, utg, 2, 4, 4, 2, uout, 3, &un, ust) == PA_ERR_INVALID_ARG && un == 0 && strstr(pa_last_error(), "mode 2"));
        EXPECT(pa_bus_umi_correct_records(NULL, urec, 3, uoff, uids, 2, 2, utg, 2, 17, 16, PA_UMI_GREATEST, uout, 3, &un, ust) == PA_ERR_INVALID_ARG);
        EXPECT(pa_bus_umi_correct_records(NULL, urec, 3, uoff, uids, 2, 2, utg_bad, 2, 4, 4, PA_UMI_GREATEST, uout, 3, &un, ust) == PA_ERR_INVALID_ARG && strstr(pa_last_error(), "tx_gene[1]"));
        EXPECT(pa_bus_umi_correct_records(NULL, urec, 1ull << 31, uoff, uids, 2, 2, utg, 2, 4, 4, PA_UMI_DIRECTIONAL, uout, 3, &un, ust) == PA_ERR_UNSUPPORTED);
        memcpy(ubad, urec, sizeof ubad);
        ubad[2].ec = 2;   /* no ec of the table */
        EXPECT(pa_bus_umi_correct_records(NULL, ubad, 3, uoff, uids, 2, 2, utg, 2, 4, 4, PA_UMI_GREATEST, uout, 3, &un, ust) == PA_ERR_INVALID_ARG && strstr(pa_last_error(), "record 2"));
        ubad[2].ec = 1;
        ubad[1].umi = 256;   /* no UMI of 4 bases */
        EXPECT(pa_bus_umi_correct_records(NULL, ubad, 3, uoff, uids, 2, 2, utg, 2, 4, 4, PA_UMI_GREATEST, uout, 3, &un, ust) == PA_ERR_INVALID_ARG && strstr(pa_last_error(), "record 1"));
        EXPECT(pa_bus_umi_correct_records(NULL, urec, 3, uoff, uids, 2, 2, utg, 2, 4, 4, PA_UMI_DIRECTIONAL, uout, 3, &un, ust) == (ndev < 1 ? PA_ERR_NO_DEVICE : PA_ERR_INVALID_ARG) &&
               un == 0);
        EXPECT(pa_bus_umi_correct(NULL, utg, 2, PA_UMI_GREATEST, ust) == PA_ERR_INVALID_ARG);
        EXPECT(pa_bus_umi_correct_phase_ms(NULL) == PA_ERR_INVALID_ARG && pa_bus_umi_correct_phase_ms(ums) == PA_OK);
        EXPECT(pa_write_bus_umi(NULL, h, fastq, fastq, NULL, 4, 4, 0, NULL, PA_UMI_GREATEST, dir, 1, NULL, NULL, NULL, ust) == PA_ERR_INVALID_ARG);
        EXPECT(pa_count_cells_em_umi(NULL, h, fastq, fastq, NULL, 4, 4, 0, NULL, PA_UMI_GREATEST, NULL, dir, 1, NULL, NULL, NULL, ust) == PA_ERR_INVALID_ARG);
    }

    {   /* cell calling on BUS records, host side: the defaults, the TSV writer, and every refusal that comes before a device call */
        pa_knee_params kp, kbad;
        uint64_t kst[PA_KNEE_STATS], pst[PA_BUS_KEEP_STATS], knr = 7, knc = 7, kn = 7;
        float kms[PA_KNEE_PHASES];
        const pa_bus_record krec[3] = {{26, 0, 0, 1, 0, 0}, {27, 0, 0, 2, 0, 0}, {27, 1, 0, 1, 0, 0}};
        const uint64_t klist[2] = {26, 27}, klist_dup[2] = {27, 27}, klist_big[2] = {27, 256};
        const pa_bus_barcode_row krow[1] = {{27, 3, 2, 2, 0, 1}};
        pa_bus_record kbadrec[3];
        EXPECT(PA_KNEE_STATS == 10 && PA_KNEE_PHASES == 3 && PA_BUS_KEEP_STATS == 7 && sizeof(pa_bus_barcode_row) == 32 && sizeof(pa_knee_params) == 32);
        pa_knee_default_params(NULL);
        pa_knee_default_params(&kp);
        EXPECT(kp.mode == PA_KNEE_CURVE && kp.lower == 10 && kp.divisor == 10 && kp.expected_cells == 3000 && kp.min_umis == 1 && kp.reserved[2] == 0);
        EXPECT(pa_bus_knee_records(NULL, krec, 3, 4, 4, &kp, NULL, 0, NULL, NULL, 0, &knc, kst) == PA_ERR_INVALID_ARG);
        kbad = kp;
        kbad.lower = 0;
        EXPECT(pa_bus_knee_records(NULL, krec, 3, 4, 4, &kbad, NULL, 0, &knr, NULL, 0, &knc, kst) == PA_ERR_INVALID_ARG && strstr(pa_last_error(), "lower") && knr == 0);
        kbad = kp;
        kbad.mode = 3;
        EXPECT(pa_bus_knee_records(NULL, krec, 3, 4, 4, &kbad, NULL, 0, &knr, NULL, 0, &knc, kst) == PA_ERR_INVALID_ARG && strstr(pa_last_error(), "mode"));
        EXPECT(pa_bus_knee_records(NULL, krec, 3, 17, 16, &kp, NULL, 0, &knr, NULL, 0, &knc, kst) == PA_ERR_UNSUPPORTED);
        memcpy(kbadrec, krec, sizeof kbadrec);
        kbadrec[2].umi = 0;   /* equal to the record before it */
        EXPECT(pa_bus_knee_records(NULL, kbadrec, 3, 4, 4, NULL, NULL, 0, &knr, NULL, 0, &knc, kst) == PA_ERR_INVALID_ARG && strstr(pa_last_error(), "record 2"));
        EXPECT(pa_bus_knee_records(NULL, krec, 3, 4, 4, NULL, NULL, 0, &knr, NULL, 0, &knc, kst) == (ndev < 1 ? PA_ERR_NO_DEVICE : PA_ERR_INVALID_ARG) && knc == 0);
        EXPECT(pa_bus_knee(NULL, &kp, NULL, 0, &knr, NULL, 0, &knc, kst) == PA_ERR_INVALID_ARG);
        EXPECT(pa_bus_knee_phase_ms(NULL) == PA_ERR_INVALID_ARG && pa_bus_knee_phase_ms(kms) == PA_OK);
        EXPECT(pa_bus_keep_records(NULL, krec, 3, 4, 4, klist, 2, NULL, 0, NULL, pst) == PA_ERR_INVALID_ARG);
        EXPECT(pa_bus_keep_records(NULL, krec, 3, 4, 4, klist_dup, 2, NULL, 0, &kn, pst) == PA_ERR_INVALID_ARG && strstr(pa_last_error(), "entry 1") && kn == 0);
        EXPECT(pa_bus_keep_records(NULL, krec, 3, 4, 4, klist_big, 2, NULL, 0, &kn, pst) == PA_ERR_INVALID_ARG && strstr(pa_last_error(), "entry 1"));
        EXPECT(pa_bus_keep_records(NULL, krec, 3, 4, 4, klist, 2, NULL, 0, &kn, pst) == (ndev < 1 ? PA_ERR_NO_DEVICE : PA_ERR_INVALID_ARG));
        EXPECT(pa_bus_keep(NULL, klist, 2, pst) == PA_ERR_INVALID_ARG);
        snprintf(path, sizeof path, "%s/abi_check_ranks.tsv", dir);
        EXPECT(pa_write_barcode_ranks_tsv(krow, 1, 4, path) == PA_OK && pa_write_barcode_ranks_tsv(krow, 1, 4, NULL) == PA_ERR_INVALID_ARG);
        EXPECT(pa_write_barcode_ranks_tsv(krow, 1, 32, path) == PA_ERR_UNSUPPORTED && remove(path) == 0);
        EXPECT(pa_write_bus_called(NULL, h, fastq, fastq, NULL, 4, 4, &kp, dir, 1, NULL, NULL, kst) == PA_ERR_INVALID_ARG);
        EXPECT(pa_count_cells_em_called(NULL, h, fastq, fastq, NULL, 4, 4, &kp, NULL, dir, 1, NULL, NULL, kst) == PA_ERR_INVALID_ARG);
    }

    {   /* paired-end reads, host side: the checks that come before any device call */
        uint64_t pst[PA_PAIR_STATS], pu = 0, pn = 0, poff[2] = {0, 0};
        pa_read_result pr[1];
        EXPECT(PA_PAIR_FR == 0 && PA_PAIR_RF == 1 && PA_PAIR_FF == 2 && PA_PAIR_STATS == 8);
        EXPECT(pa_revcomp_tiles_device(NULL, NULL, NULL, 0, 1, NULL, NULL) == PA_ERR_INVALID_ARG);
        EXPECT(pa_pairs_scratch_bytes(0) >= 256 && pa_pairs_scratch_bytes(1000) > pa_pairs_scratch_bytes(10));
        EXPECT(pa_pairs_combine_device(NULL, NULL, NULL, NULL, NULL, 0, NULL, NULL, 0, NULL, NULL, 0, NULL) == PA_ERR_INVALID_ARG);
        EXPECT(pa_pairs_finish(NULL, NULL, NULL, pst, &pu, &pn) == PA_ERR_INVALID_ARG);
        EXPECT(pa_map_pairs(NULL, NULL, poff, NULL, poff, 1, PA_PAIR_FR, 2, pr, NULL, NULL) == PA_ERR_INVALID_ARG);
        EXPECT(pa_count_pairs(NULL, fastq, fastq, PA_PAIR_FR, 2, 1, counts, &pn, pst) == PA_ERR_INVALID_ARG);
        /* unstranded libraries: the same checks */
        EXPECT(PA_STRAND_FWD == 0 && PA_STRAND_REV == 1 && PA_STRAND_BOTH == 2 && PA_STRAND_STATS == 8);
        EXPECT(pa_strands_scratch_bytes(0) >= 256 && pa_strands_scratch_bytes(1000) > pa_strands_scratch_bytes(10) && pa_strands_scratch_bytes(1ull << 31) == 0);
        EXPECT(pa_strands_merge_device(NULL, NULL, NULL, NULL, NULL, 0, NULL, NULL, 0, NULL, NULL, 0, NULL) == PA_ERR_INVALID_ARG);
        EXPECT(pa_strands_finish(NULL, NULL, NULL, pst, &pu, &pn) == PA_ERR_INVALID_ARG);
        EXPECT(pa_map_batch_strand(NULL, NULL, poff, 1, PA_STRAND_BOTH, 2, pr, NULL, NULL) == PA_ERR_INVALID_ARG);
        EXPECT(pa_map_pairs_unstranded(NULL, NULL, poff, NULL, poff, 1, 2, pr, NULL, NULL) == PA_ERR_INVALID_ARG);
        EXPECT(pa_count_pairs_unstranded(NULL, fastq, fastq, 2, 1, counts, &pn, pst) == PA_ERR_INVALID_ARG);
        /* the pair scan on the device: its scratch is sized on the host, null outputs are refused before any device call */
        EXPECT(PA_PAIRS_CTL_WORDS == 8 && PA_PAIRS_WHOLE_READ == 0xFFFFFFFFu);
        {
            uint64_t pis[2 * PA_INGEST_INPUT_STATS];
            EXPECT(pa_pairs_input_stats(pis) == PA_OK && pa_pairs_input_stats(NULL) == PA_ERR_INVALID_ARG && (pa_pairs_input_path() == 0 || pa_pairs_input_path() == 1));
        }
        EXPECT(pa_pairs_gather_scratch_bytes(0) >= 256 && pa_pairs_gather_scratch_bytes(1000) > pa_pairs_gather_scratch_bytes(10) && pa_pairs_gather_scratch_bytes(1ull << 31) == 0);
        EXPECT(pa_pairs_gather_device(0, NULL, 0, NULL, NULL, 0, NULL, 0, 0, 0, NULL, 0, NULL, NULL, 0, NULL, NULL, NULL, 0, NULL) == PA_ERR_INVALID_ARG);
    }

    pa_txome *tx = NULL, *tx2 = NULL, *tx3 = NULL;
    EXPECT(pa_txome_synthesize(50, 120, 7, &tx) == PA_OK);
    {   /* the same genes with repeat families and low-complexity tracts in their last exons */
        pa_txome* txr = NULL;
        const pa_synth_repeats rep = {4, 100, 100000, 150000, 1, 30000, 60000, 500000, 3};
        uint32_t ntx_plain = 0, ntx_rep = 0;
        const uint64_t *st_plain = NULL, *st_rep = NULL;
        EXPECT(pa_txome_synthesize_repeats(50, 120, 7, &rep, &txr) == PA_OK);
        EXPECT(pa_txome_view(tx, NULL, &st_plain, &ntx_plain) == PA_OK && pa_txome_view(txr, NULL, &st_rep, &ntx_rep) == PA_OK);
        EXPECT(ntx_plain == ntx_rep && st_rep[ntx_rep] > st_plain[ntx_plain]);
        pa_txome_destroy(txr);
    }
    EXPECT(pa_txome_from_host_index(h, &tx2) == PA_OK);
    EXPECT(pa_txome_from_fasta(fasta, &tx3) == PA_OK);
    EXPECT(pa_txome_view(tx2, &packed, &tx_start, &ntx2) == PA_OK && ntx2 == ntx);
    const uint64_t nsim = 256;
    const uint32_t sim_wpr = pa_words_per_read(60);
    uint64_t* sim_tiles = (uint64_t*)calloc(pa_tiles_words(nsim, sim_wpr), 8);
    uint32_t* sim_lens = (uint32_t*)calloc(nsim, 4);
    EXPECT(pa_simulate_reads_host(tx2, 60, 1, 10000, 0, nsim, sim_wpr, sim_tiles, sim_lens) == PA_OK && sim_lens[0] == 60);

    const uint32_t ovf_a[] = {1, 7, 2, 3, 0, 4, 9}, ovf_b[] = {1, 7, 2, 1, 0, 4, 9};
    const uint32_t* bufs[2] = {ovf_a, ovf_b};
    const uint64_t nwords[2] = {7, 7};
    uint32_t merged[16];
    uint64_t merged_words = 0;
    EXPECT(pa_overflow_merge(bufs, nwords, 2, merged, 16, &merged_words) == PA_OK && merged_words == 7 && merged[3] == 4);

    /* BGZF: the member table of a two-member file (28 bytes of text, then the EOF block), found on the host */
    static const uint8_t bgzf_file[] = {0x1f, 0x8b, 0x08, 0x04, 0x00, 0x00, 0x00, 0x00, 0x00, 0xff, 0x06, 0x00, 0x42, 0x43, 0x02, 0x00, 0x2b, 0x00, 0x73, 0x28, 0x32, 0xe4, 0x72, 0x74, 0x76, 0x0f, 0x81, 0x60, 0x2e, 0x6d, 0x2e, 0x4f, 0x38, 0xe0, 0x02, 0x00, 0x9d, 0x3b, 0x6e, 0x4c, 0x1c, 0x00, 0x00, 0x00, 0x1f, 0x8b, 0x08, 0x04, 0x00, 0x00, 0x00, 0x00, 0x00, 0xff, 0x06, 0x00, 0x42, 0x43, 0x02, 0x00, 0x1b, 0x00, 0x03, 0x00, 0x00, 0x00, 0x00, 0x00, 0x00, 0x00, 0x00, 0x00};
    static const char bgzf_text[] = "@r1\nACGTACGTAC\n+\nIIIIIIIIII\n";
    pa_bgzf_member bgzf_rows[2];
    uint64_t bgzf_n = 0, bgzf_text_bytes = 0;
    EXPECT(pa_bgzf_scan(bgzf_file, sizeof bgzf_file, bgzf_rows, 2, &bgzf_n, &bgzf_text_bytes) == PA_OK && bgzf_n == 2 && bgzf_text_bytes == 28 &&
           bgzf_rows[0].in_off == 18 && bgzf_rows[0].out_len == 28 && bgzf_rows[1].out_off == 28 && bgzf_rows[1].out_len == 0 && bgzf_rows[1].in_len == 2);
    EXPECT(pa_bgzf_scan(bgzf_file, sizeof bgzf_file - 1, NULL, 0, &bgzf_n, NULL) == PA_ERR_NOT_BGZF && bgzf_n == 0);
    EXPECT(strcmp(pa_inflate_status_name(PA_INFLATE_CRC_MISMATCH), "crc mismatch") == 0);
    {
        uint64_t ist[PA_INGEST_INPUT_STATS];
        EXPECT(pa_process_reads_input_stats(ist) == PA_OK && pa_process_reads_input_stats(NULL) == PA_ERR_INVALID_ARG);
    }
    printf("layout pa_bgzf_member sizeof %zu\n", sizeof(pa_bgzf_member));
    LAYOUT_FIELD(pa_bgzf_member, in_off); LAYOUT_FIELD(pa_bgzf_member, out_off); LAYOUT_FIELD(pa_bgzf_member, file_off); LAYOUT_FIELD(pa_bgzf_member, in_len);
    LAYOUT_FIELD(pa_bgzf_member, out_len); LAYOUT_FIELD(pa_bgzf_member, crc32); LAYOUT_FIELD(pa_bgzf_member, reserved);

    /* ---- device half: with a GPU it runs, without one every entry point refuses (there is no CPU fallback) ---- */
    pa_index* idx = NULL;
    int rc = pa_index_create(&flat, 0, &idx);
    if (ndev < 1) {
        void *p = NULL, *ev = NULL;
        pa_overflow* o = NULL;
        pa_txome_device* td = NULL;
        EXPECT(rc == PA_ERR_NO_DEVICE && idx == NULL);
        EXPECT(pa_device_malloc(0, 64, &p) == PA_ERR_NO_DEVICE);
        {
            uint32_t bst[2];
            uint8_t btext[32];
            EXPECT(pa_bgzf_inflate_device(0, bgzf_file, sizeof bgzf_file, bgzf_rows, 2, btext, sizeof btext, bst, NULL) == PA_ERR_NO_DEVICE);
        }
        {
            uint64_t goff[4], gctl[PA_PAIRS_CTL_WORDS];
            void* gscr = (void*)(uintptr_t)256;   /* (never touched: the call refuses before it looks at device memory) */
            EXPECT(pa_pairs_gather_device(0, NULL, 0, NULL, NULL, 0, NULL, 0, 2, 0, NULL, 0, goff, NULL, 0, goff + 2, gctl, gscr, 4096, NULL) == PA_ERR_NO_DEVICE);
        }
        EXPECT(pa_overflow_create(0, 16, 64, &o) == PA_ERR_NO_DEVICE);
        EXPECT(pa_txome_upload(tx2, 60, 0, &td) == PA_ERR_NO_DEVICE);
        EXPECT(pa_event_create(&ev) < 0);
        const int devs0[1] = {0};
        pa_index* multi0[1] = {NULL};
        EXPECT(pa_index_create_multi(&flat, devs0, 1, multi0) == PA_ERR_NO_DEVICE && multi0[0] == NULL);
        pa_host_index* hg = NULL;
        EXPECT(pa_host_index_build_fasta_device(fasta, 20, 0, &hg) == PA_ERR_NO_DEVICE && hg == NULL);
        EXPECT(pa_host_index_build_packed_device(packed, tx_start, ntx2, 20, 0, &hg) == PA_ERR_NO_DEVICE && hg == NULL);
        printf("abi_check: host half ok, no device: %d failures\n", failures);
    } else {
        EXPECT(rc == PA_OK && idx);
        /* one call for the GPUs of a single-process host (here: the one GPU, and a refused duplicate) */
        const int devs[2] = {0, 0};
        pa_index* multi[2] = {NULL, NULL};
        EXPECT(pa_index_create_multi(&flat, devs, 1, multi) == PA_OK && multi[0] != NULL);
        pa_index_stats mst;
        EXPECT(pa_index_get_stats(multi[0], &mst) == PA_OK && mst.num_nodes == flat.num_nodes);
        pa_index_destroy(multi[0]);
        multi[0] = NULL;
        EXPECT(pa_index_create_multi(&flat, devs, 2, multi) == PA_ERR_INVALID_ARG && multi[0] == NULL && multi[1] == NULL);
        /* the graph built on the GPU is the graph the CPU builder gives */
        pa_host_index *hg = NULL, *hg2 = NULL;
        EXPECT(pa_host_index_build_fasta_device(fasta, 20, 0, &hg) == PA_OK && hg);
        EXPECT(pa_host_index_compare(h, hg, 1u << 20, report, sizeof report) == 0);
        EXPECT(pa_host_index_build_packed_device(packed, tx_start, ntx2, 20, 0, &hg2) == PA_OK && hg2);
        EXPECT(pa_host_index_compare(h, hg2, 1u << 20, report, sizeof report) == 0);
        pa_host_index_destroy(hg);
        pa_host_index_destroy(hg2);
        pa_index_stats st;
        EXPECT(pa_index_get_stats(idx, &st) == PA_OK && st.k == 20 && st.num_nodes == flat.num_nodes);
        EXPECT(pa_counts_len(idx) == counts_len);
        {   /* the two members inflated on the GPU */
            void *d_bcomp = NULL, *d_brows = NULL, *d_btext = NULL, *d_bst = NULL;
            uint32_t bst[2] = {99, 99};
            char btext[28];
            EXPECT(pa_device_malloc(0, sizeof bgzf_file, &d_bcomp) == PA_OK && pa_device_malloc(0, sizeof bgzf_rows, &d_brows) == PA_OK &&
                   pa_device_malloc(0, 64, &d_btext) == PA_OK && pa_device_malloc(0, 8, &d_bst) == PA_OK);
            EXPECT(pa_memcpy_h2d(d_bcomp, bgzf_file, sizeof bgzf_file, NULL) == PA_OK && pa_memcpy_h2d(d_brows, bgzf_rows, sizeof bgzf_rows, NULL) == PA_OK);
            EXPECT(pa_bgzf_inflate_device(0, (const uint8_t*)d_bcomp, sizeof bgzf_file, (const pa_bgzf_member*)d_brows, 2, (uint8_t*)d_btext, 28, (uint32_t*)d_bst, NULL) == PA_OK);
            EXPECT(pa_memcpy_d2h(btext, d_btext, 28, NULL) == PA_OK && pa_memcpy_d2h(bst, d_bst, 8, NULL) == PA_OK && pa_stream_synchronize(NULL) == PA_OK);
            EXPECT(bst[0] == PA_INFLATE_OK && bst[1] == PA_INFLATE_OK && memcmp(btext, bgzf_text, 28) == 0);
            pa_device_free(d_bcomp); pa_device_free(d_brows); pa_device_free(d_btext); pa_device_free(d_bst);
        }
        {   /* two pairs matched and gathered on the GPU: "a/1" with "a/2", "b" with "c" (position 1 differs); R1 cut to two bytes */
            static const char gt1[] = "a/1ACGTbGGG", gt2[] = "a/2TTTTTcCA";
            const uint32_t grec1[8] = {0, 3, 3, 4, 7, 1, 8, 3}, grec2[8] = {0, 3, 3, 5, 8, 1, 9, 2};
            const size_t gsb = pa_pairs_gather_scratch_bytes(2);
            void *d_gt1 = NULL, *d_gt2 = NULL, *d_gr1 = NULL, *d_gr2 = NULL, *d_gb1 = NULL, *d_gb2 = NULL, *d_go1 = NULL, *d_go2 = NULL, *d_gctl = NULL, *d_gscr = NULL;
            uint64_t gctl[PA_PAIRS_CTL_WORDS], go1[3], go2[3];
            char gb1[4], gb2[7];
            EXPECT(pa_device_malloc(0, 16, &d_gt1) == PA_OK && pa_device_malloc(0, 16, &d_gt2) == PA_OK && pa_device_malloc(0, 32, &d_gr1) == PA_OK &&
                   pa_device_malloc(0, 32, &d_gr2) == PA_OK && pa_device_malloc(0, 64, &d_gb1) == PA_OK && pa_device_malloc(0, 64, &d_gb2) == PA_OK &&
                   pa_device_malloc(0, 24, &d_go1) == PA_OK && pa_device_malloc(0, 24, &d_go2) == PA_OK && pa_device_malloc(0, sizeof gctl, &d_gctl) == PA_OK &&
                   pa_device_malloc(0, gsb, &d_gscr) == PA_OK);
            EXPECT(pa_memcpy_h2d(d_gt1, gt1, 11, NULL) == PA_OK && pa_memcpy_h2d(d_gt2, gt2, 11, NULL) == PA_OK && pa_memcpy_h2d(d_gr1, grec1, 32, NULL) == PA_OK &&
                   pa_memcpy_h2d(d_gr2, grec2, 32, NULL) == PA_OK && pa_stream_synchronize(NULL) == PA_OK);
            EXPECT(pa_pairs_gather_device(0, (const uint8_t*)d_gt1, 11, (const uint32_t*)d_gr1, (const uint8_t*)d_gt2, 11, (const uint32_t*)d_gr2, 2, 2, 0, (uint8_t*)d_gb1, 64,
                                          (uint64_t*)d_go1, (uint8_t*)d_gb2, 64, (uint64_t*)d_go2, (uint64_t*)d_gctl, d_gscr, gsb, NULL) == PA_OK);
            EXPECT(pa_memcpy_d2h(gctl, d_gctl, sizeof gctl, NULL) == PA_OK && pa_memcpy_d2h(go1, d_go1, 24, NULL) == PA_OK && pa_memcpy_d2h(go2, d_go2, 24, NULL) == PA_OK &&
                   pa_memcpy_d2h(gb1, d_gb1, 4, NULL) == PA_OK && pa_memcpy_d2h(gb2, d_gb2, 7, NULL) == PA_OK && pa_stream_synchronize(NULL) == PA_OK);
            EXPECT(gctl[0] == 1 && gctl[1] == 2 && gctl[2] == 5 && gctl[3] == 4 && gctl[4] == 7 && gctl[5] == ~0ull);
            EXPECT(go1[0] == 0 && go1[1] == 2 && go1[2] == 4 && go2[0] == 0 && go2[1] == 5 && go2[2] == 7);
            EXPECT(memcmp(gb1, "ACGG", 4) == 0 && memcmp(gb2, "TTTTTCA", 7) == 0);
            pa_device_free(d_gt1); pa_device_free(d_gt2); pa_device_free(d_gr1); pa_device_free(d_gr2); pa_device_free(d_gb1); pa_device_free(d_gb2);
            pa_device_free(d_go1); pa_device_free(d_go2); pa_device_free(d_gctl); pa_device_free(d_gscr);
        }
        /* single reads and host batches */
        const char* ex1 = "GGCTGTCAACCAGTCCATAGGCAGGGCCATCAGGCACCAAAGGGATTCTGCCAGCATAGT";
        uint32_t cls[64], ncls = 0, cov = 0, mm = 0, nodes[256], nn = 0;
        rc = pa_map_read(idx, (const uint8_t*)ex1, 60, cls, 64, &ncls, &cov);
        EXPECT(rc == 0 || (rc == 1 && cov <= 60));
        EXPECT(pa_map_read_with_mismatch(idx, (const uint8_t*)ex1, 60, 2, cls, 64, &ncls, &cov, &mm) >= 0);
        EXPECT(pa_map_read_to_nodes(idx, (const uint8_t*)ex1, 60, 2, nodes, 256, &nn, &cov, &mm) >= 0);
        pa_read_result res[2];
        uint64_t coff[3];
        const uint32_t* cids = NULL;
        EXPECT(pa_map_batch(idx, ascii, offsets, 2, 2, res, coff, &cids) == PA_OK);
        /* the same two reads as a DnaString would hold them: 2-bit words (LSB-first: the host encoder's tiles of reads 0 and 1) */
        {
            uint64_t pw[8];
            uint32_t plen[2] = {lens[0], lens[1]};
            uint64_t poff[3] = {0, wpr, 2ull * wpr};
            for (uint32_t w = 0; w < wpr && w < 4; ++w) { pw[w] = tiles[(uint64_t)w * 64]; pw[wpr + w] = tiles[(uint64_t)w * 64 + 1]; }
            pa_read_result pres[2];
            uint64_t pcoff[3];
            const uint32_t* pcids = NULL;
            EXPECT(pa_map_batch_packed(idx, pw, poff, plen, 2, PA_PACKED_LSB_FIRST, 2, pres, pcoff, &pcids) == PA_OK);
            EXPECT(pres[0].coverage == res[0].coverage && pres[1].coverage == res[1].coverage && pcoff[2] == coff[2]);
            uint32_t pcls[64], pn = 0, pcov = 0, pmm = 0;
            EXPECT(pa_map_read_packed(idx, pw, plen[0], PA_PACKED_LSB_FIRST, 2, pcls, 64, &pn, &pcov, &pmm) >= 0 && pcov == res[0].coverage);
        }
        /* process_reads for a caller that holds the reader: push records, pull the tuples */
        {
            pa_record_stream* rs = NULL;
            EXPECT(pa_record_stream_create(idx, 2, 64, &rs) == PA_OK && rs);
            const uint8_t ids2[] = "r0r1";
            const uint64_t ioff[3] = {0, 2, 4};
            EXPECT(pa_records_push(rs, ids2, ioff, ascii, offsets, 2) == PA_OK);
            char text[512];
            size_t nb = 1;
            EXPECT(pa_records_pull(rs, text, sizeof text, &nb) == PA_OK && nb == 0);   /* nothing rendered yet: the batch is still being filled */
            EXPECT(pa_records_flush(rs) == PA_OK);
            EXPECT(pa_records_pull(rs, text, sizeof text, &nb) == PA_OK && nb > 0 && text[nb - 1] == '\n' && text[0] == '(');
            uint64_t rn = 0, rf = 0;
            EXPECT(pa_record_stream_stats(rs, &rn, &rf) == PA_OK && rn == 2);
            { double st[PA_INGEST_STAGES]; EXPECT(pa_record_stream_stage_seconds(rs, st) == PA_OK && st[7] == 2.0 && st[6] >= 0.0);
              EXPECT(pa_process_reads_stage_seconds(st) == PA_OK); }
            pa_record_stream_destroy(rs);
            {   /* the same stream over two lanes of the handle: the same tuples */
                pa_index* two[2]; char text2[4096]; size_t nb2 = 0;
                two[0] = idx; two[1] = idx;
                EXPECT(pa_record_stream_create_multi(two, 2, 2, 64, &rs) == PA_OK && rs);
                EXPECT(pa_records_push(rs, ids2, ioff, ascii, offsets, 2) == PA_OK && pa_records_flush(rs) == PA_OK);
                EXPECT(pa_records_pull(rs, text2, sizeof text2, &nb2) == PA_OK && nb2 == nb && memcmp(text, text2, nb) == 0);
                pa_record_stream_destroy(rs);
            }
        }
        uint32_t nodes_flat[2 * 64], nodes_len[2];
        EXPECT(pa_map_batch_nodes(idx, ascii, offsets, 2, 2, res, nodes_flat, 64, nodes_len) == PA_OK);
        snprintf(path, sizeof path, "%s/abi_check_tuples.txt", dir);
        uint64_t nreads = 0, nflag = 0;
        EXPECT(pa_process_reads(idx, fastq, path, 2, &nreads, &nflag) == PA_OK && nreads > 0);
        { pa_index* two[2]; uint64_t n2 = 0, f2 = 0; two[0] = idx; two[1] = idx;   /* two lanes on one GPU */
          EXPECT(pa_process_reads_multi(two, 2, fastq, path, 2, &n2, &f2) == PA_OK && n2 == nreads && f2 == nflag); }
        /* device-resident batch: simulate on the device, map with the fused count table, overflow table, RCCL world of one */
        pa_txome_device* td = NULL;
        EXPECT(pa_txome_upload(tx2, 60, 0, &td) == PA_OK);
        void *d_tiles = NULL, *d_lens = NULL, *d_res = NULL, *d_arena = NULL, *d_counts = NULL, *d_colour = NULL, *d_ascii = NULL, *d_off = NULL;
        const uint64_t arena_cap = pa_map_arena_hint(idx, nsim);
        EXPECT(pa_device_malloc(0, pa_tiles_words(nsim, sim_wpr) * 8, &d_tiles) == PA_OK);
        EXPECT(pa_device_malloc(0, nsim * 4, &d_lens) == PA_OK && pa_device_malloc(0, nsim * sizeof(pa_read_result), &d_res) == PA_OK);
        EXPECT(pa_device_malloc(0, arena_cap * 4, &d_arena) == PA_OK && pa_device_malloc(0, counts_len * 8, &d_counts) == PA_OK);
        EXPECT(pa_device_malloc(0, nsim * 4, &d_colour) == PA_OK && pa_device_malloc(0, 64, &d_ascii) == PA_OK && pa_device_malloc(0, 64, &d_off) == PA_OK);
        EXPECT(pa_memset_device(d_counts, 0, counts_len * 8, NULL) == PA_OK);
        void *ev0 = NULL, *ev1 = NULL;
        float ms = -1.0f;
        EXPECT(pa_event_create(&ev0) == PA_OK && pa_event_create(&ev1) == PA_OK);
        EXPECT(pa_simulate_reads_device(td, 1, 10000, 0, nsim, sim_wpr, (uint64_t*)d_tiles, (uint32_t*)d_lens, NULL) == PA_OK);
        pa_overflow* ovf = NULL;
        EXPECT(pa_overflow_create(0, 1024, 1 << 16, &ovf) == PA_OK && pa_index_set_overflow(idx, ovf) == PA_OK);
        EXPECT(pa_event_record(ev0, NULL) == PA_OK);
        EXPECT(pa_index_set_timing(idx, 1) == PA_OK);
        EXPECT(pa_map_count_batch_device(idx, (const uint64_t*)d_tiles, (const uint32_t*)d_lens, nsim, sim_wpr, 2, (pa_read_result*)d_res,
                                         (uint32_t*)d_arena, arena_cap, (uint64_t*)d_counts, NULL) == PA_OK);
        EXPECT(pa_event_record(ev1, NULL) == PA_OK);
        uint64_t used = 0, need = 0;
        EXPECT(pa_map_finish(idx, NULL, &used, &need) == PA_OK);
        { float kms = -1.0f, st[3] = {-1.0f, -1.0f, -1.0f}; EXPECT(pa_map_kernel_ms(idx, NULL, &kms) == PA_OK && kms > 0.0f);
          EXPECT(pa_map_stage_ms(idx, NULL, st) == PA_OK && st[0] > 0.0f && st[1] >= 0.0f && st[2] >= 0.0f); EXPECT(pa_index_set_timing(idx, 0) == PA_OK); }
        {   /* the records in their 8-byte form + the packed stream of the classes that are no index classes */
            void *d_compact = NULL, *d_packed = NULL, *d_pw = NULL, *d_scr = NULL;
            const size_t scr = pa_compact_scratch_bytes(nsim);
            uint64_t* hc = (uint64_t*)malloc(nsim * 8);
            pa_read_result* hr = (pa_read_result*)malloc(nsim * sizeof(pa_read_result));
            uint64_t pw = ~0ull;
            EXPECT(pa_device_malloc(0, nsim * 8, &d_compact) == PA_OK && pa_device_malloc(0, (arena_cap + 16) * 4, &d_packed) == PA_OK &&
                   pa_device_malloc(0, 8, &d_pw) == PA_OK && pa_device_malloc(0, scr, &d_scr) == PA_OK);
            EXPECT(pa_results_compact_device(idx, (const pa_read_result*)d_res, (const uint32_t*)d_arena, arena_cap, nsim, (uint64_t*)d_compact, (uint32_t*)d_packed,
                                             arena_cap + 16, (uint64_t*)d_pw, d_scr, scr, NULL) == PA_OK);
            EXPECT(pa_memcpy_d2h(hc, d_compact, nsim * 8, NULL) == PA_OK && pa_memcpy_d2h(&pw, d_pw, 8, NULL) == PA_OK &&
                   pa_memcpy_d2h(hr, d_res, nsim * sizeof(pa_read_result), NULL) == PA_OK && pa_stream_synchronize(NULL) == PA_OK);
            for (uint64_t i = 0; i < nsim; ++i) {
                const uint32_t lo = (uint32_t)hc[i];
                EXPECT((lo & 0x3FFFu) == hr[i].coverage && ((lo >> 14) & 0x3FFFu) == (hr[i].mismatches & 0x3FFFu) &&
                       ((lo & PA_COMPACT_MAPPED) != 0) == ((hr[i].mismatches & PA_MAPPED_BIT) != 0));
                if (lo & PA_COMPACT_BY_REF) EXPECT((uint32_t)(hc[i] >> 32) == (hr[i].class_off & ~PA_CLASS_REF) && (hr[i].class_off & PA_CLASS_REF));
            }
            EXPECT(pw <= arena_cap + 16);
            free(hc); free(hr);
            pa_device_free(d_compact); pa_device_free(d_packed); pa_device_free(d_pw); pa_device_free(d_scr);
        }
        {   /* paired-end reads: the batch against its own reverse complement (FR of a pair whose mate 2 is mate 1 reversed: the same read twice) */
            void *d_rc = NULL, *d_rc2 = NULL, *d_res2 = NULL, *d_arena2 = NULL, *d_pres = NULL, *d_parena = NULL, *d_pscr = NULL;
            const size_t pscr = pa_pairs_scratch_bytes(nsim);
            const size_t tile_bytes = pa_tiles_words(nsim, sim_wpr) * 8;
            uint64_t pst[PA_PAIR_STATS], pu = 0, pn = 0, u2 = 0, n2 = 0;
            uint64_t *back = (uint64_t*)malloc(tile_bytes), *fwd = (uint64_t*)malloc(tile_bytes);
            pa_read_result *hp = (pa_read_result*)malloc(nsim * sizeof(pa_read_result)), *h1 = (pa_read_result*)malloc(nsim * sizeof(pa_read_result));
            EXPECT(pa_device_malloc(0, tile_bytes, &d_rc) == PA_OK && pa_device_malloc(0, tile_bytes, &d_rc2) == PA_OK &&
                   pa_device_malloc(0, nsim * sizeof(pa_read_result), &d_res2) == PA_OK && pa_device_malloc(0, arena_cap * 4, &d_arena2) == PA_OK &&
                   pa_device_malloc(0, nsim * sizeof(pa_read_result), &d_pres) == PA_OK && pa_device_malloc(0, arena_cap * 4, &d_parena) == PA_OK &&
                   pa_device_malloc(0, pscr, &d_pscr) == PA_OK);
            EXPECT(pa_revcomp_tiles_device(idx, (const uint64_t*)d_tiles, (const uint32_t*)d_lens, nsim, sim_wpr, (uint64_t*)d_tiles, NULL) == PA_ERR_INVALID_ARG);   /* not in place */
            EXPECT(pa_revcomp_tiles_device(idx, (const uint64_t*)d_tiles, (const uint32_t*)d_lens, nsim, sim_wpr, (uint64_t*)d_rc, NULL) == PA_OK);
            EXPECT(pa_revcomp_tiles_device(idx, (const uint64_t*)d_rc, (const uint32_t*)d_lens, nsim, sim_wpr, (uint64_t*)d_rc2, NULL) == PA_OK);
            EXPECT(pa_memcpy_d2h(back, d_rc2, tile_bytes, NULL) == PA_OK && pa_memcpy_d2h(fwd, d_tiles, tile_bytes, NULL) == PA_OK && pa_stream_synchronize(NULL) == PA_OK &&
                   memcmp(back, fwd, tile_bytes) == 0);
            EXPECT(pa_map_batch_device(idx, (const uint64_t*)d_rc2, (const uint32_t*)d_lens, nsim, sim_wpr, 2, (pa_read_result*)d_res2, (uint32_t*)d_arena2, arena_cap, NULL,
                                       NULL) == PA_OK && pa_map_finish(idx, NULL, &u2, &n2) == PA_OK);
            EXPECT(pa_pairs_combine_device(idx, (const pa_read_result*)d_res, (const uint32_t*)d_arena, (const pa_read_result*)d_res2, (const uint32_t*)d_arena2, nsim,
                                           (pa_read_result*)d_pres, (uint32_t*)d_parena, arena_cap, NULL, d_pscr, pscr - 1, NULL) == PA_ERR_INVALID_ARG);
            EXPECT(pa_pairs_combine_device(idx, (const pa_read_result*)d_res, (const uint32_t*)d_arena, (const pa_read_result*)d_res2, (const uint32_t*)d_arena2, nsim,
                                           (pa_read_result*)d_pres, (uint32_t*)d_parena, arena_cap, NULL, d_pscr, pscr, NULL) == PA_OK);
            EXPECT(pa_pairs_finish(idx, d_pscr, NULL, pst, &pu, &pn) == PA_OK && pu == pn && pu <= arena_cap);
            EXPECT(pst[0] == nsim && pst[0] == pst[1] + pst[2] + pst[3] + pst[4] && pst[2] == 0 && pst[3] == 0);
            EXPECT(pa_memcpy_d2h(hp, d_pres, nsim * sizeof(pa_read_result), NULL) == PA_OK && pa_memcpy_d2h(h1, d_res, nsim * sizeof(pa_read_result), NULL) == PA_OK &&
                   pa_stream_synchronize(NULL) == PA_OK);
            for (uint64_t i = 0; i < nsim; ++i)   /* a read paired with itself: its class, twice its coverage */
                EXPECT(hp[i].class_len == h1[i].class_len && hp[i].coverage == 2 * h1[i].coverage && (hp[i].mismatches & PA_MAPPED_BIT) == (h1[i].mismatches & PA_MAPPED_BIT));
            {   /* unstranded: the same records as both candidates — every mapped item is a tie of a list with itself: the read's own result */
                uint64_t sst[PA_STRAND_STATS], su = 0, sn = 0;
                EXPECT(pa_strands_scratch_bytes(nsim) <= pscr);
                EXPECT(pa_strands_merge_device(idx, (const pa_read_result*)d_res, (const uint32_t*)d_arena, (const pa_read_result*)d_res2, (const uint32_t*)d_arena2, nsim,
                                               (pa_read_result*)d_pres, (uint32_t*)d_parena, arena_cap, NULL, d_pscr, pscr, NULL) == PA_OK);
                EXPECT(pa_strands_finish(idx, d_pscr, NULL, sst, &su, &sn) == PA_OK && su == sn && su <= arena_cap);
                EXPECT(sst[0] == nsim && sst[0] == sst[1] + sst[2] + sst[3] + sst[4] && sst[2] == 0 && sst[3] == 0 && sst[5] == sst[1]);
                EXPECT(pa_memcpy_d2h(hp, d_pres, nsim * sizeof(pa_read_result), NULL) == PA_OK && pa_stream_synchronize(NULL) == PA_OK);
                for (uint64_t i = 0; i < nsim; ++i)
                    EXPECT(hp[i].class_len == h1[i].class_len && hp[i].coverage == h1[i].coverage && hp[i].mismatches == h1[i].mismatches);
            }
            {   /* ... and through the host-buffer paths: a bad strand is refused, both strands of two reads, an unstranded pair of a read with itself */
                pa_read_result sr[2];
                uint64_t sco[3] = {9, 9, 9};
                const uint32_t* sci = NULL;
                EXPECT(pa_map_batch_strand(idx, ascii, offsets, 2, 3, 2, sr, sco, &sci) == PA_ERR_INVALID_ARG);
                EXPECT(pa_map_batch_strand(idx, ascii, offsets, 2, PA_STRAND_FWD, 2, sr, sco, &sci) == PA_OK && sco[0] == 0 && sr[0].class_len == res[0].class_len &&
                       sr[0].coverage == res[0].coverage);
                EXPECT(pa_map_batch_strand(idx, ascii, offsets, 2, PA_STRAND_BOTH, 2, sr, sco, &sci) == PA_OK && sco[0] == 0 && sco[2] == sco[1] + sr[1].class_len);
                EXPECT(pa_map_pairs_unstranded(idx, ascii, offsets, ascii, offsets, 2, 2, sr, sco, &sci) == PA_OK && sco[0] == 0 && sco[2] == sco[1] + sr[1].class_len);
            }
            {   /* ... and from files: every pair counted once */
                uint64_t* pc = (uint64_t*)calloc(counts_len, 8);
                uint64_t npairs = 0, sst[PA_STRAND_STATS], tot = 0;
                EXPECT(pa_count_pairs_unstranded(idx, fastq, fastq, 2, 2, pc, &npairs, sst) == PA_OK && npairs == nreads && sst[0] == nreads &&
                       sst[0] == sst[1] + sst[2] + sst[3] + sst[4]);
                for (uint64_t i = 0; i < counts_len; ++i) tot += pc[i];
                EXPECT(tot == nreads);
                free(pc);
            }
            {
                pa_read_result pr[2];
                uint64_t pco[3] = {9, 9, 9};
                const uint32_t* pci = NULL;
                EXPECT(pa_map_pairs(idx, ascii, offsets, ascii, offsets, 2, 3, 2, pr, pco, &pci) == PA_ERR_INVALID_ARG);   /* no such orientation */
                EXPECT(pa_map_pairs(idx, ascii, offsets, ascii, offsets, 2, PA_PAIR_FF, 2, pr, pco, &pci) == PA_OK && pco[0] == 0 && pco[2] == pco[1] + pr[1].class_len);
                EXPECT(pr[0].class_len == res[0].class_len && pr[0].coverage == 2 * res[0].coverage);
            }
            {   /* the same file as both mates, both as given: every pair is its read twice */
                uint64_t* pc = (uint64_t*)calloc(counts_len, 8);
                uint64_t npairs = 0, cst2[PA_PAIR_STATS], tot = 0;
                EXPECT(pa_count_pairs(idx, fastq, fastq, 7, 2, 2, pc, &npairs, cst2) == PA_ERR_INVALID_ARG);
                EXPECT(pa_count_pairs(idx, fastq, fastq, PA_PAIR_FF, 2, 2, pc, &npairs, cst2) == PA_OK && npairs == nreads && cst2[0] == nreads && cst2[2] == 0 && cst2[3] == 0);
                for (uint64_t i = 0; i < counts_len; ++i) tot += pc[i];
                EXPECT(tot == nreads);
                free(pc);
            }
            free(back); free(fwd); free(hp); free(h1);
            pa_device_free(d_rc); pa_device_free(d_rc2); pa_device_free(d_res2); pa_device_free(d_arena2); pa_device_free(d_pres); pa_device_free(d_parena); pa_device_free(d_pscr);
        }
        {   /* host to host: the simulated batch from pinned host tiles to compact records + count table, chunks of 64 reads on two streams */
            void *ph_tiles = NULL, *ph_compact = NULL, *ph_packed = NULL, *ph_counts = NULL;
            const uint64_t clen = pa_counts_len(idx);
            uint64_t pwords = ~0ull, total = 0;
            EXPECT(pa_host_alloc_pinned(pa_tiles_words(nsim, sim_wpr) * 8, &ph_tiles) == PA_OK && pa_host_alloc_pinned(nsim * 8, &ph_compact) == PA_OK &&
                   pa_host_alloc_pinned((arena_cap + 16) * 4, &ph_packed) == PA_OK && pa_host_alloc_pinned(clen * 8, &ph_counts) == PA_OK);
            memcpy(ph_tiles, sim_tiles, pa_tiles_words(nsim, sim_wpr) * 8);
            EXPECT(pa_map_tiles_host(idx, (const uint64_t*)ph_tiles, sim_lens, 0, nsim, sim_wpr, 2, (uint64_t*)ph_compact, (uint32_t*)ph_packed, arena_cap + 16, &pwords,
                                     (uint64_t*)ph_counts, 64, 2) == PA_OK);
            for (uint64_t i = 0; i < clen; ++i) total += ((uint64_t*)ph_counts)[i];
            EXPECT(total == nsim && pwords <= arena_cap + 16);
            EXPECT(pa_map_tiles_host(idx, (const uint64_t*)ph_tiles, NULL, 60, nsim, sim_wpr, 2, (uint64_t*)ph_compact, (uint32_t*)ph_packed, arena_cap + 16, &pwords, NULL, 0, 0) == PA_OK);
            EXPECT(pa_host_free_pinned(ph_tiles) == PA_OK && pa_host_free_pinned(ph_compact) == PA_OK && pa_host_free_pinned(ph_packed) == PA_OK && pa_host_free_pinned(ph_counts) == PA_OK);
        }
        {   /* the same batch as a uniform one (the simulator's reads all have 60 bases): the same records without a length array */
            void* d_res2 = NULL;
            pa_read_result *r1 = (pa_read_result*)malloc(nsim * sizeof(pa_read_result)), *r2 = (pa_read_result*)malloc(nsim * sizeof(pa_read_result));
            EXPECT(pa_device_malloc(0, nsim * sizeof(pa_read_result), &d_res2) == PA_OK);
            EXPECT(pa_map_count_batch_uniform_device(idx, (const uint64_t*)d_tiles, 0, nsim, sim_wpr, 2, (pa_read_result*)d_res2, (uint32_t*)d_arena, arena_cap,
                                                     (uint64_t*)d_counts, NULL) == PA_ERR_INVALID_ARG);
            EXPECT(pa_memcpy_d2h(r1, d_res, nsim * sizeof(pa_read_result), NULL) == PA_OK);
            EXPECT(pa_map_count_batch_uniform_device(idx, (const uint64_t*)d_tiles, 60, nsim, sim_wpr, 2, (pa_read_result*)d_res2, (uint32_t*)d_arena, arena_cap,
                                                     (uint64_t*)d_counts, NULL) == PA_OK);
            EXPECT(pa_map_finish(idx, NULL, &used, &need) == PA_OK);
            EXPECT(pa_memcpy_d2h(r2, d_res2, nsim * sizeof(pa_read_result), NULL) == PA_OK && pa_stream_synchronize(NULL) == PA_OK);
            uint64_t same = 0;
            for (uint64_t i = 0; i < nsim; ++i)
                same += r1[i].coverage == r2[i].coverage && r1[i].mismatches == r2[i].mismatches && r1[i].class_len == r2[i].class_len &&
                        ((r1[i].class_off & PA_CLASS_REF) ? r1[i].class_off == r2[i].class_off : !(r2[i].class_off & PA_CLASS_REF));
            EXPECT(same == nsim);
            EXPECT(pa_device_free(d_res2) == PA_OK);
            free(r1); free(r2);
        }
        EXPECT(pa_index_release_stream(idx, NULL) == PA_OK);   /* the null stream's launch context goes; the next launch makes a new one */
        EXPECT(pa_event_elapsed_ms(ev0, ev1, &ms) == PA_OK && ms >= 0.0f);
        EXPECT(pa_map_batch_device(idx, (const uint64_t*)d_tiles, (const uint32_t*)d_lens, nsim, sim_wpr, 2, (pa_read_result*)d_res, (uint32_t*)d_arena,
                                   arena_cap, (uint32_t*)d_colour, NULL) == PA_OK);
        EXPECT(pa_map_finish(idx, NULL, &used, &need) == PA_OK);
        EXPECT(pa_counts_accumulate_device(idx, (const pa_read_result*)d_res, (const uint32_t*)d_arena, (const uint32_t*)d_colour, nsim, (uint64_t*)d_counts, NULL) == PA_OK);
        EXPECT(pa_stream_synchronize(NULL) == PA_OK);
        {   /* per-barcode counts: four cells' worth of barcodes over the same records */
            void *d_bc = NULL, *d_keys = NULL, *d_vals = NULL;
            uint32_t* bc = (uint32_t*)calloc(nsim, 4);
            for (uint64_t i = 0; i < nsim; ++i) bc[i] = (uint32_t)(i & 3);
            uint64_t cells = 0;
            EXPECT(pa_device_malloc(0, nsim * 4, &d_bc) == PA_OK && pa_device_malloc(0, nsim * 8, &d_keys) == PA_OK && pa_device_malloc(0, nsim * 4, &d_vals) == PA_OK);
            EXPECT(pa_memcpy_h2d(d_bc, bc, nsim * 4, NULL) == PA_OK);
            EXPECT(pa_counts_by_barcode_device(idx, (const pa_read_result*)d_res, (const uint32_t*)d_arena, (const uint32_t*)d_bc, nsim, 2, (uint64_t*)d_keys,
                                               (uint32_t*)d_vals, &cells, NULL) == PA_OK && cells >= 4 && cells <= nsim);
            EXPECT(pa_device_free(d_bc) == PA_OK && pa_device_free(d_keys) == PA_OK && pa_device_free(d_vals) == PA_OK);
            free(bc);
        }
        {   /* single-cell UMI counts: the toy reads as R2, R1 = a whitelisted barcode + UMI per read; then the file-level entry (the
               FASTQ as both R1 and R2: its reads' first 8 bases are barcode + UMI, most of them invalid) */
            pa_cell_counter* cc = NULL;
            const char wl[] = "ACGTTGCA";
            uint8_t* r1 = (uint8_t*)malloc(nsim * 8);
            uint64_t* r1o = (uint64_t*)malloc((nsim + 1) * 8);
            void *d_r1 = NULL, *d_r1o = NULL;
            for (uint64_t i = 0; i <= nsim; ++i) r1o[i] = i * 8;
            for (uint64_t i = 0; i < nsim; ++i) { memcpy(r1 + i * 8, (i & 1) ? "ACGT" : "TGCA", 4); memcpy(r1 + i * 8 + 4, "ACGTACGT" + (i % 4), 4); }
            EXPECT(pa_cell_counter_create(idx, h, tx_gene, ngenes, wl, 2, 4, 4, &cc) == PA_OK && cc);
            EXPECT(pa_device_malloc(0, nsim * 8, &d_r1) == PA_OK && pa_device_malloc(0, (nsim + 1) * 8, &d_r1o) == PA_OK);
            EXPECT(pa_memcpy_h2d(d_r1, r1, nsim * 8, NULL) == PA_OK && pa_memcpy_h2d(d_r1o, r1o, (nsim + 1) * 8, NULL) == PA_OK);
            EXPECT(pa_cell_counter_add_device(cc, (const pa_read_result*)d_res, (const uint32_t*)d_arena, (const uint8_t*)d_r1, (const uint64_t*)d_r1o, nsim, NULL) == PA_OK);
            uint64_t nent = 0, cst[PA_CELL_STATS];
            EXPECT(pa_cell_counter_finish(cc, &nent) == PA_OK && nent >= 1);
            uint32_t *mc = (uint32_t*)calloc(nent + 1, 4), *mg = (uint32_t*)calloc(nent + 1, 4), *mu = (uint32_t*)calloc(nent + 1, 4);
            EXPECT(pa_cell_counter_matrix(cc, mc, mg, mu, nent) == PA_OK && mc[0] <= 1 && mu[0] >= 1);
            EXPECT(pa_cell_counter_stats(cc, cst) == PA_OK && cst[0] == nsim && cst[0] == cst[3] + cst[4] + cst[5] + cst[6] && cst[1] == nsim);
            EXPECT(pa_cell_counter_add_device(cc, (const pa_read_result*)d_res, (const uint32_t*)d_arena, (const uint8_t*)d_r1, (const uint64_t*)d_r1o, nsim, NULL) == PA_ERR_INVALID_ARG);
            pa_cell_counter_destroy(cc);
            {   /* BUS records of the same batch (barcode 4 + UMI 4), then the file-level entry on the FASTQ as both R1 and R2 */
                pa_bus* bus = NULL;
                uint64_t nrec = 0, nids = 0, bst[PA_BUS_STATS];
                uint32_t necs = 0;
                EXPECT(pa_bus_create(idx, h, 17, 16, &bus) == PA_ERR_UNSUPPORTED && bus == NULL);
                EXPECT(pa_bus_create(idx, h, 4, 4, &bus) == PA_OK && bus);
                EXPECT(pa_bus_add_device(bus, (const pa_read_result*)d_res, (const uint32_t*)d_arena, arena_cap, (const uint8_t*)d_r1, (const uint64_t*)d_r1o, nsim, NULL) == PA_OK);
                EXPECT(pa_bus_finish(bus, &nrec, &necs) == PA_OK && nrec >= 1 && necs >= ntx);
                pa_bus_record* rec = (pa_bus_record*)calloc(nrec + 1, sizeof(pa_bus_record));
                EXPECT(pa_bus_records(bus, rec, nrec - 1) == PA_ERR_BUFFER_TOO_SMALL);
                EXPECT(pa_bus_records(bus, rec, nrec) == PA_OK && rec[0].count >= 1 && rec[0].flags == 0 && rec[0].ec >= 0 && (uint32_t)rec[0].ec < necs);
                EXPECT(pa_bus_ecs(bus, NULL, NULL, 0, &nids) == PA_OK && nids >= necs);
                uint64_t* eoff = (uint64_t*)calloc((size_t)necs + 1, 8);
                uint32_t* eids = (uint32_t*)calloc(nids + 1, 4);
                EXPECT(pa_bus_ecs(bus, eoff, eids, nids, &nids) == PA_OK && eoff[0] == 0 && eoff[necs] == nids && eids[0] == 0);
                EXPECT(pa_bus_stats(bus, bst) == PA_OK && bst[0] == nsim && bst[0] == bst[1] + bst[2] + bst[3] + bst[4] + bst[5] + bst[6] && bst[7] == nrec);
                EXPECT(pa_bus_write(bus, dir) == PA_OK);
                {   /* corrected in place against every barcode of 4 bases but the first record's: nothing else changes; then the identity */
                    uint64_t* all = (uint64_t*)calloc(256, 8);
                    uint64_t cst13[PA_BUS_CORRECT_STATS], n_all = 0, nrec2 = 0;
                    uint32_t necs2 = 0;
                    for (uint64_t v = 0; v < 256; ++v) if (v != rec[0].barcode) all[n_all++] = v;
                    EXPECT(pa_bus_correct(bus, all, n_all, cst13) == PA_OK && cst13[0] == nrec && cst13[6] == 1 && cst13[4] == 0 && cst13[11] < nrec);
                    EXPECT(pa_bus_finish(bus, &nrec2, &necs2) == PA_OK && nrec2 == cst13[11] && necs2 == necs);
                    EXPECT(pa_bus_correct(bus, all, n_all, cst13) == PA_OK && cst13[0] == nrec2 && cst13[11] == nrec2 && cst13[3] == cst13[2]);
                    EXPECT(pa_bus_stats(bus, bst) == PA_OK && bst[7] == nrec2);
                    nrec = nrec2;
                    free(all);
                }
                {   /* the gene stage on those records where they lie, then on the two-cell hand-made input, then from the files */
                    pa_genes* gg = NULL;
                    uint64_t gst[PA_GENES_STATS], gnc = 0, gnv = 0, gne = 0, gnot = 0, gbc[2];
                    uint32_t git = 0, gcell[4], ggene[4], giter[2];
                    double gval[4];
                    const pa_bus_record two_cells[4] = {{1, 0, 0, 1, 0, 0}, {1, 1, 2, 3, 0, 0}, {2, 0, 2, 1, 0, 0}, {2, 0, 3, 1, 0, 0}};
                    const uint64_t goff[5] = {0, 1, 2, 4, 6};
                    const uint32_t gids[6] = {0, 1, 0, 1, 1, 2}, gtx[3] = {0, 1, 2};
                    EXPECT(pa_genes_create_from_bus(bus, tx_gene, ngenes, NULL, &gg) == PA_OK && gg);
                    EXPECT(pa_genes_run(gg, &git, &gnot) == PA_OK && pa_genes_stats(gg, gst) == PA_OK && gst[0] == nrec && gst[1] == gst[2] + gst[3] + gst[4]);
                    EXPECT(pa_genes_matrix(gg, NULL, NULL, NULL, 0, &gne) == PA_OK && gne == gst[14]);
                    pa_genes_destroy(gg);
                    gg = NULL;
                    EXPECT(pa_genes_create(idx, two_cells, 4, goff, gids, 4, 3, gtx, 3, 4, 4, NULL, &gg) == PA_OK && gg);
                    EXPECT(pa_genes_layout(gg, &gnc, &gnv) == PA_OK && gnc == 2 && gnv == 3);
                    EXPECT(pa_genes_values(gg, gbc, gcell, ggene, gval, 2) == PA_ERR_BUFFER_TOO_SMALL);
                    EXPECT(pa_genes_values(gg, gbc, gcell, ggene, gval, 4) == PA_OK && gbc[0] == 1 && gbc[1] == 2 && gcell[2] == 1 && ggene[2] == 1 && gval[2] == 1.0);
                    EXPECT(gval[0] == 1.5 && gval[1] == 0.5);   /* u = (1, 0), M = 1 over |E| = 2 */
                    EXPECT(pa_genes_matrix(gg, gcell, ggene, gval, 4, &gne) == PA_ERR_INVALID_ARG);
                    EXPECT(pa_genes_step(gg, 1) == PA_OK && pa_genes_cell_iters(gg, giter) == PA_OK && giter[0] == 1 && giter[1] == 0);
                    EXPECT(pa_genes_values(gg, NULL, NULL, NULL, gval, 4) == PA_OK && gval[0] > 1.74 && gval[0] < 1.76 && gval[0] + gval[1] > 1.999 && gval[0] + gval[1] < 2.001);
                    EXPECT(pa_genes_run(gg, &git, &gnot) == PA_OK && git >= 51 && gnot == 0 && pa_genes_step(gg, 1) == PA_ERR_INVALID_ARG);
                    EXPECT(pa_genes_matrix(gg, gcell, ggene, gval, 4, &gne) == PA_OK && gne >= 2 && gne <= 3 && gval[0] > 1.9);
                    EXPECT(pa_genes_stats(gg, gst) == PA_OK && gst[0] == 4 && gst[1] == 3 && gst[5] == 2 && gst[6] == 1 && gst[7] == 1 && gst[14] == gne);
                    EXPECT(pa_genes_write(gg, h, dir) == (ngenes == 3 ? PA_OK : PA_ERR_INVALID_ARG));
                    pa_genes_destroy(gg);
                    EXPECT(pa_count_cells_em(idx, h, fastq, fastq, 4, 4, NULL, dir, 2, gst) == PA_OK && gst[0] >= 1 && gst[1] == gst[2] + gst[3] + gst[4]);
                }
                EXPECT(pa_bus_add_device(bus, (const pa_read_result*)d_res, (const uint32_t*)d_arena, arena_cap, (const uint8_t*)d_r1, (const uint64_t*)d_r1o, nsim, NULL) == PA_ERR_INVALID_ARG);
                pa_bus_destroy(bus);
                free(rec); free(eoff); free(eids);
                EXPECT(pa_write_bus(idx, h, fastq, fastq, 4, 4, dir, 2, bst) == PA_OK && bst[0] == nreads && bst[0] == bst[1] + bst[2] + bst[3] + bst[4] + bst[5] + bst[6]);
                {   /* barcode correction: three hand-made records against ACGT TTTT GGCA, then the file-level entries with the whitelist file */
                    const uint64_t cwl[3] = {27, 255, 164};
                    const pa_bus_record crec[4] = {{26, 0, 0, 1, 0, 0}, {27, 0, 0, 2, 0, 0}, {27, 1, 0, 1, 0, 0}, {90, 0, 0, 5, 0, 0}};   /* ACGG -> ACGT; ACGT; CCGG: none */
                    pa_bus_record cout[4];
                    uint64_t cn = 0, cst13[PA_BUS_CORRECT_STATS], gst[PA_GENES_STATS];
                    float cms[PA_BUS_CORRECT_PHASES];
                    EXPECT(pa_bus_correct_records(idx, crec, 4, 4, 4, cwl, 3, cout, 1, &cn, cst13) == PA_ERR_BUFFER_TOO_SMALL && cn == 2);
                    EXPECT(pa_bus_correct_records(idx, crec, 4, 4, 4, cwl, 3, cout, 4, &cn, cst13) == PA_OK && cn == 2);
                    EXPECT(cout[0].barcode == 27 && cout[0].umi == 0 && cout[0].count == 3 && cout[1].umi == 1 && cout[1].count == 1 && cout[1].flags == 0);
                    EXPECT(cst13[0] == 4 && cst13[1] == 9 && cst13[2] == 3 && cst13[3] == 1 && cst13[4] == 1 && cst13[5] == 1 && cst13[6] == 0 && cst13[9] == 1 && cst13[10] == 5 &&
                           cst13[11] == 2 && cst13[12] == 1);
                    EXPECT(pa_bus_correct_phase_ms(cms) == PA_OK && cms[0] >= 0.0f);
                    snprintf(path, sizeof path, "%s/abi_check_whitelist.txt", dir);
                    EXPECT(pa_write_bus_corrected(idx, h, fastq, fastq, path, 4, 4, dir, 2, bst, cst13) == PA_OK && bst[0] == nreads && cst13[11] == bst[7] &&
                           cst13[2] == cst13[3] + cst13[4] + cst13[5] + cst13[6] && cst13[0] == cst13[7] + cst13[8] + cst13[9]);
                    EXPECT(pa_write_bus_corrected(idx, h, fastq, fastq, path, 17, 4, dir, 2, bst, cst13) == PA_ERR_UNSUPPORTED);
                    EXPECT(pa_count_cells_em_corrected(idx, h, fastq, fastq, path, 4, 4, NULL, dir, 2, gst, cst13) == PA_OK && gst[0] == cst13[11]);
                }
                {   /* cell calling: barcode 27 has two molecules, 26 and 90 one each; min_umis 2 calls 27 alone; then the filter; then the file-level entries */
                    const pa_bus_record krec[5] = {{26, 0, 0, 1, 0, 0}, {27, 0, 0, 2, 0, 0}, {27, 0, 1, 4, 0, 0}, {27, 1, 0, 1, 0, 0}, {90, 0, 0, 5, 0, 0}};
                    const uint64_t klist[2] = {27, 91};
                    pa_knee_params kp;
                    pa_bus_barcode_row krows[3];
                    pa_bus_record kout[5];
                    uint64_t kcalled[3], knr = 0, knc = 0, kn = 0, kst[PA_KNEE_STATS], pst[PA_BUS_KEEP_STATS], cst13[PA_BUS_CORRECT_STATS], gst[PA_GENES_STATS];
                    float kms[PA_KNEE_PHASES];
                    pa_knee_default_params(&kp);
                    kp.mode = PA_KNEE_MIN;
                    kp.min_umis = 2;
                    EXPECT(pa_bus_knee_records(idx, krec, 5, 4, 4, &kp, krows, 2, &knr, kcalled, 3, &knc, kst) == PA_ERR_BUFFER_TOO_SMALL && knr == 3 && knc == 1);
                    EXPECT(pa_bus_knee_records(idx, krec, 5, 4, 4, &kp, NULL, 0, &knr, NULL, 0, &knc, kst) == PA_OK && knr == 3 && knc == 1);
                    EXPECT(pa_bus_knee_records(idx, krec, 5, 4, 4, &kp, krows, 3, &knr, kcalled, 3, &knc, kst) == PA_OK && knr == 3 && knc == 1 && kcalled[0] == 27);
                    EXPECT(krows[1].barcode == 27 && krows[1].records == 3 && krows[1].umis == 2 && krows[1].reads == 7 && krows[1].rank == 0 && krows[1].called == 1);
                    EXPECT(krows[0].rank == 1 && krows[2].rank == 2 && krows[0].called == 0 && krows[2].reads == 5);
                    EXPECT(kst[0] == 5 && kst[1] == 13 && kst[2] == 4 && kst[3] == 3 && kst[4] == 2 && kst[5] == 0 && kst[6] == 2 && kst[7] == 1 && kst[8] == 2 && kst[9] == 7);
                    EXPECT(pa_bus_knee_phase_ms(kms) == PA_OK && kms[0] >= 0.0f);
                    EXPECT(pa_bus_keep_records(idx, krec, 5, 4, 4, klist, 2, kout, 2, &kn, pst) == PA_ERR_BUFFER_TOO_SMALL && kn == 3);
                    EXPECT(pa_bus_keep_records(idx, krec, 5, 4, 4, klist, 2, kout, 5, &kn, pst) == PA_OK && kn == 3 && kout[0].barcode == 27 && kout[2].umi == 1 && kout[1].count == 4);
                    EXPECT(pst[0] == 5 && pst[1] == 13 && pst[2] == 3 && pst[3] == 1 && pst[4] == 3 && pst[5] == 7 && pst[6] == 1);
                    kp.min_umis = 1;
                    EXPECT(pa_write_bus_called(idx, h, fastq, fastq, NULL, 4, 4, &kp, dir, 2, bst, cst13, kst) == PA_OK && bst[0] == nreads && kst[7] == kst[3] &&
                           cst13[3] == cst13[2] && bst[7] == kst[0]);
                    snprintf(path, sizeof path, "%s/abi_check_whitelist.txt", dir);
                    EXPECT(pa_count_cells_em_called(idx, h, fastq, fastq, path, 4, 4, &kp, NULL, dir, 2, gst, cst13, kst) == PA_OK && gst[0] == kst[0] && kst[0] == cst13[11]);
                    kp.min_umis = 1000000;
                    EXPECT(pa_write_bus_called(idx, h, fastq, fastq, NULL, 4, 4, &kp, dir, 2, bst, cst13, kst) == PA_ERR_FORMAT && strstr(pa_last_error(), "threshold of 1000000"));
                    snprintf(path, sizeof path, "%s/barcode_ranks.tsv", dir);
                    EXPECT(remove(path) == 0);   /* (the two calls that went through wrote it) */
                }
                {   /* UMI correction: AAAC joins AAAA (one base apart, one gene), AACA has another gene and stays; then the file-level entries */
                    const uint64_t uoff[3] = {0, 1, 2};
                    const uint32_t uids[2] = {0, 1}, utg[2] = {0, 1};
                    const pa_bus_record urec[3] = {{27, 0, 0, 5, 0, 0}, {27, 1, 0, 1, 0, 0}, {27, 4, 1, 1, 0, 0}};
                    const uint64_t uwant[PA_BUS_UMI_STATS] = {3, 7, 3, 1, 0, 3, 2, 1, 0, 1, 1, 2, 2, 3, 0};
                    pa_bus_record uout[3];
                    pa_knee_params kp;
                    uint64_t un = 0, ust[PA_BUS_UMI_STATS], cst13[PA_BUS_CORRECT_STATS], kst[PA_KNEE_STATS], gst[PA_GENES_STATS];
                    float ums[PA_BUS_UMI_PHASES];
                    EXPECT(pa_bus_umi_correct_records(idx, urec, 3, uoff, uids, 2, 2, utg, 2, 4, 4, PA_UMI_GREATEST, uout, 1, &un, ust) == PA_ERR_BUFFER_TOO_SMALL && un == 2);
                    EXPECT(pa_bus_umi_correct_records(idx, urec, 3, uoff, uids, 2, 2, utg, 2, 4, 4, PA_UMI_GREATEST, uout, 3, &un, ust) == PA_OK && un == 2);
                    EXPECT(uout[0].umi == 0 && uout[0].count == 6 && uout[1].umi == 4 && uout[1].ec == 1 && uout[1].count == 1 && uout[1].flags == 0);
                    EXPECT(memcmp(ust, uwant, sizeof ust) == 0);
                    EXPECT(pa_bus_umi_correct_records(idx, urec, 3, uoff, uids, 2, 2, utg, 2, 4, 4, PA_UMI_DIRECTIONAL, uout, 3, &un, ust) == PA_OK && un == 2 && ust[7] == 1);
                    EXPECT(pa_bus_umi_correct_phase_ms(ums) == PA_OK && ums[1] >= 0.0f);
                    EXPECT(pa_write_bus_umi(idx, h, fastq, fastq, NULL, 4, 4, 0, NULL, PA_UMI_GREATEST, dir, 2, bst, cst13, kst, ust) == PA_OK && bst[0] == nreads && ust[11] == bst[7] &&
                           ust[7] <= ust[6] && ust[6] <= ust[5] && ust[5] <= ust[2] - ust[4]);
                    EXPECT(pa_write_bus_umi(idx, h, fastq, fastq, NULL, 4, 4, 0, NULL, 2, dir, 2, bst, cst13, kst, ust) == PA_ERR_INVALID_ARG);
                    pa_knee_default_params(&kp);
                    kp.mode = PA_KNEE_MIN;
                    snprintf(path, sizeof path, "%s/abi_check_whitelist.txt", dir);
                    EXPECT(pa_count_cells_em_umi(idx, h, fastq, fastq, path, 4, 4, 1, &kp, PA_UMI_DIRECTIONAL, NULL, dir, 2, gst, cst13, kst, ust) == PA_OK && gst[0] == ust[11] &&
                           ust[0] <= kst[0] && kst[0] == cst13[11]);
                    snprintf(path, sizeof path, "%s/barcode_ranks.tsv", dir);
                    EXPECT(remove(path) == 0);
                }
            }
            free(mc); free(mg); free(mu); free(r1); free(r1o);
            EXPECT(pa_device_free(d_r1) == PA_OK && pa_device_free(d_r1o) == PA_OK);
            snprintf(path, sizeof path, "%s/abi_check_whitelist.txt", dir);
            EXPECT(pa_count_cells(idx, h, fastq, fastq, path, 4, 4, dir, 2, cst) == PA_OK && cst[0] == nreads && cst[0] == cst[3] + cst[4] + cst[5] + cst[6]);
        }
        uint64_t* h_counts = (uint64_t*)calloc(counts_len, 8);
        EXPECT(pa_memcpy_d2h(h_counts, d_counts, counts_len * 8, NULL) == PA_OK);
        uint64_t total = 0;
        for (uint64_t i = 0; i < counts_len; ++i) total += h_counts[i];
        EXPECT(total == 3 * nsim);                                   /* counted by the two fused launches (ragged form, uniform form) and once by the count kernel */
        const uint32_t* words = NULL;
        uint64_t nw = 0;
        EXPECT(pa_overflow_fetch(ovf, NULL, &words, &nw) == PA_OK && nw >= 2 && words[1] == nw);
        {   /* transcript abundances from that table (the novel reads left out: the table saw three launches, the overflow two) */
            pa_quant* qq = NULL;
            pa_quant_params qp;
            uint64_t qst[PA_QUANT_STATS];
            uint32_t qit = 0;
            int qconv = 0;
            double *qa = (double*)calloc(ntx, 8), *qe = (double*)calloc(ntx, 8), *qt = (double*)calloc(ntx, 8), *ql = (double*)calloc(ntx, 8);
            double *ge = (double*)calloc(ngenes, 8), *gt = (double*)calloc(ngenes, 8), sum = 0.0, tsum = 0.0;
            pa_quant_default_params(&qp);
            qp.mean_read_len = 60.0;
            EXPECT(pa_quant_create(idx, h, &qp, &qq) == PA_OK && qq);
            EXPECT(pa_quant_set_counts(qq, h_counts, counts_len - 1, NULL, 0) == PA_ERR_INVALID_ARG);
            EXPECT(pa_quant_set_counts(qq, h_counts, counts_len, NULL, 0) == PA_OK);
            EXPECT(pa_quant_step(qq, 2) == PA_OK && pa_quant_alpha(qq, qa) == PA_OK);
            EXPECT(pa_quant_run(qq, &qit, &qconv) == PA_OK && qit >= 1 && qit <= qp.max_iters);
            EXPECT(pa_quant_fetch(qq, qe, qt, ql) == PA_OK && pa_quant_fetch_genes(qq, ge, gt) == PA_OK && pa_quant_stats(qq, qst) == PA_OK);
            for (uint32_t t = 0; t < ntx; ++t) { sum += qe[t]; tsum += qt[t]; }
            EXPECT(qst[5] > 0 && qst[6] == h_counts[flat.num_classes] && qst[7] == 2 + (uint64_t)qit && ql[0] >= 1.0);
            EXPECT(sum > 0.999 * (double)qst[5] && sum < 1.001 * (double)qst[5] && tsum > 999999.0 && tsum < 1000001.0);
            snprintf(path, sizeof path, "%s/abi_check_abundance.tsv", dir);
            EXPECT(pa_write_abundance_tsv(qq, path) == PA_OK);
            {   /* three bootstrap replicates of that table: each a table of its own with the reads of the original, each run to its own stop */
                uint64_t* bc = (uint64_t*)calloc(counts_len, 8);
                double* be = (double*)calloc(3 * (size_t)ntx, 8), *bt = (double*)calloc(3 * (size_t)ntx, 8);
                uint32_t bit[3] = {0, 0, 0};
                int bconv[3] = {0, 0, 0};
                EXPECT(pa_quant_bootstrap_fetch(qq, be, bt) == PA_ERR_INVALID_ARG && pa_quant_bootstrap_step(qq, 1) == PA_ERR_INVALID_ARG);   /* no batch drawn */
                EXPECT(pa_quant_bootstrap_draw(qq, 7, 0, 0) == PA_ERR_INVALID_ARG && pa_quant_bootstrap_draw(qq, 7, 0, PA_QUANT_BOOT_MAX_BATCH + 1) == PA_ERR_INVALID_ARG);
                EXPECT(pa_quant_bootstrap_draw(qq, 7, 0xFFFFFFFEu, 3) == PA_ERR_INVALID_ARG);
                EXPECT(pa_quant_bootstrap_draw(qq, 7, 0, 3) == PA_OK);
                EXPECT(pa_quant_bootstrap_counts(qq, 3, bc, counts_len, NULL, 0) == PA_ERR_INVALID_ARG);
                for (uint32_t k = 0; k < 3; ++k) {
                    uint64_t bsum = 0;
                    EXPECT(pa_quant_bootstrap_counts(qq, k, bc, counts_len, NULL, 0) == PA_OK);
                    for (uint64_t i = 0; i < counts_len; ++i) bsum += bc[i];
                    EXPECT(bsum == qst[5]);
                }
                EXPECT(pa_quant_bootstrap_step(qq, 2) == PA_OK && pa_quant_bootstrap_run(qq, bit, bconv) == PA_OK);
                EXPECT(pa_quant_bootstrap_fetch(qq, be, bt) == PA_OK);
                for (uint32_t k = 0; k < 3; ++k) {
                    double bs = 0.0, bts = 0.0;
                    for (uint32_t t = 0; t < ntx; ++t) { bs += be[(size_t)k * ntx + t]; bts += bt[(size_t)k * ntx + t]; }
                    EXPECT(bit[k] >= 1 && bit[k] <= qp.max_iters && bs > 0.999 * (double)qst[5] && bs < 1.001 * (double)qst[5] && bts > 999999.0 && bts < 1000001.0);
                }
                EXPECT(pa_quant_fetch(qq, qa, NULL, NULL) == PA_OK && memcmp(qa, qe, (size_t)ntx * 8) == 0);   /* the point estimate did not move */
                free(bc); free(be); free(bt);
            }
            pa_quant_destroy(qq);
            free(qa); free(qe); free(qt); free(ql); free(ge); free(gt);
        }
        uint8_t id[128];
        pa_comm* comm = NULL;
        if (pa_comm_unique_id(id) == PA_OK) {                        /* RCCL present: a world of one */
            EXPECT(pa_comm_create(0, 1, 0, id, &comm) == PA_OK && pa_comm_rank(comm) == 0 && pa_comm_size(comm) == 1);
            EXPECT(pa_counts_allreduce(idx, (uint64_t*)d_counts, comm, NULL) == PA_OK);
            EXPECT(pa_overflow_allgather(ovf, comm, NULL, &words, &nw) == PA_OK && words[1] == nw);
            pa_comm_destroy(comm);
        } else {
            EXPECT(pa_counts_allreduce(idx, (uint64_t*)d_counts, NULL, NULL) == PA_OK);
            EXPECT(pa_overflow_allgather(ovf, NULL, NULL, &words, &nw) == PA_OK);
            EXPECT(pa_comm_rank(NULL) == 0 && pa_comm_size(NULL) == 1);
        }
        EXPECT(pa_overflow_reset(ovf, NULL) == PA_OK && pa_index_set_overflow(idx, NULL) == PA_OK);
        pa_overflow_destroy(ovf);
        /* the encode kernel */
        EXPECT(pa_memcpy_h2d(d_ascii, ascii, 25, NULL) == PA_OK && pa_memcpy_h2d(d_off, offsets, 24, NULL) == PA_OK);
        EXPECT(pa_encode_reads_device(idx, (const uint8_t*)d_ascii, (const uint64_t*)d_off, 2, wpr, (uint64_t*)d_tiles, (uint32_t*)d_lens, NULL) == PA_OK);
        uint64_t t2[64];
        EXPECT(pa_memcpy_d2h(t2, d_tiles, sizeof t2, NULL) == PA_OK && memcmp(t2, tiles, sizeof t2) == 0);
        EXPECT(pa_event_destroy(ev0) == PA_OK && pa_event_destroy(ev1) == PA_OK);
        void* bufs_d[] = {d_tiles, d_lens, d_res, d_arena, d_counts, d_colour, d_ascii, d_off};
        for (size_t i = 0; i < sizeof bufs_d / sizeof *bufs_d; ++i) EXPECT(pa_device_free(bufs_d[i]) == PA_OK);
        pa_txome_device_destroy(td);
        pa_index_destroy(idx);
        free(h_counts);
        printf("abi_check: host and device halves ok on %d device(s): %d failures\n", ndev, failures);
    }
    pa_txome_destroy(tx);
    pa_txome_destroy(tx2);
    pa_txome_destroy(tx3);
    pa_host_index_destroy(h);
    pa_host_index_destroy(h2);
    pa_host_index_destroy(h3);
    pa_host_index_destroy(h4);
    free(tx_gene); free(counts); free(gene_counts); free(mult); free(sim_tiles); free(sim_lens);
    return failures ? 1 : 0;
}
