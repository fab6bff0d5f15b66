"""ctypes binding of include/pseudoaligner_amd.h (the same symbols a Rust `extern "C"` block would bind)."""
from __future__ import annotations

import ctypes as C
from pathlib import Path

from . import _build

u8p, u32p, u64p = C.POINTER(C.c_uint8), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
vp = C.c_void_p

PA_OK = 0
PA_ERR_INVALID_ARG = -1
PA_ERR_FORMAT = -3
PA_ERR_NO_DEVICE = -4
PA_ERR_ARENA_FULL = -7
PA_ERR_UNSUPPORTED = -8
PA_ERR_BUFFER_TOO_SMALL = -10
PA_ERR_NOT_BGZF = -11
PA_CELL_STATS = 10
CELL_STAT_NAMES = ("reads", "barcode_exact", "barcode_corrected", "barcode_invalid", "umi_invalid", "not_confidently_mapped", "reads_counted",
                   "umis_corrected", "molecules_lost_to_conflicts", "umis_in_matrix")
PA_BUS_STATS = 8
BUS_STAT_NAMES = ("reads", "r1_short", "barcode_n", "umi_n", "unmapped", "bad_class", "recorded", "records")
PA_BUS_CORRECT_STATS = 13
CORRECT_STAT_NAMES = ("records_in", "reads_in", "barcodes_in", "barcodes_exact", "barcodes_corrected", "barcodes_none", "barcodes_ambiguous", "records_exact",
                      "records_corrected", "records_dropped", "reads_dropped", "records_out", "barcodes_out")
PA_BUS_CORRECT_PHASES = 4
CORRECT_PHASE_NAMES = ("table_ms", "classify_exact_ms", "classify_neighbours_ms", "rewrite_ms")
PA_KNEE_CURVE, PA_KNEE_EXPECTED, PA_KNEE_MIN = 0, 1, 2
KNEE_MODES = {"curve": PA_KNEE_CURVE, "expected": PA_KNEE_EXPECTED, "min": PA_KNEE_MIN}
PA_KNEE_STATS = 10
KNEE_STAT_NAMES = ("records", "reads", "molecules", "barcodes", "distinct_values", "values_above_lower", "threshold", "barcodes_called", "molecules_called", "reads_called")
PA_KNEE_PHASES = 3
KNEE_PHASE_NAMES = ("table_ms", "rank_curve_ms", "called_rows_ms")
PA_BUS_KEEP_STATS = 7
KEEP_STAT_NAMES = ("records_in", "reads_in", "barcodes_in", "barcodes_kept", "records_out", "reads_out", "listed_absent")
PA_UMI_GREATEST, PA_UMI_DIRECTIONAL = 0, 1
UMI_MODES = {"greatest": PA_UMI_GREATEST, "directional": PA_UMI_DIRECTIONAL}
PA_BUS_UMI_STATS = 15
UMI_STAT_NAMES = ("records_in", "reads_in", "molecules_in", "barcodes", "molecules_inert", "molecules_with_hamming1", "molecules_with_neighbour", "molecules_moved",
                  "molecules_moved_onto_moved", "records_rewritten", "reads_moved", "records_out", "molecules_out", "largest_barcode", "barcodes_hbm")
PA_BUS_UMI_PHASES = 4
UMI_PHASE_NAMES = ("molecules_ms", "search_ms", "rewrite_ms", "stats_ms")
PA_MAPPED_BIT = 0x80000000
PA_DEFAULT_ALLOWED_MISMATCHES = 2
PA_READ_COVERAGE_THRESHOLD = 32
PA_MAX_READ_LEN = 1048575


class PaError(RuntimeError):
    def __init__(self, code: int, message: str):
        super().__init__("pseudoaligner_amd error %d: %s" % (code, message))
        self.code = code


class FlatIndex(C.Structure):
    _fields_ = [("k", C.c_uint32), ("num_nodes", C.c_uint32), ("num_classes", C.c_uint32), ("num_transcripts", C.c_uint32),
                ("seq_bases", C.c_uint64), ("node_seq", vp), ("node_start", vp), ("node_len", vp), ("node_exts", vp),
                ("node_colour", vp), ("ec_offset", vp), ("ec_ids", vp), ("node_redge", vp), ("node_ledge", vp)]


class ReadResult(C.Structure):
    _fields_ = [("coverage", C.c_uint32), ("mismatches", C.c_uint32), ("class_off", C.c_uint32), ("class_len", C.c_uint32)]


class SynthRepeats(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("families", "element_len", "div_lo_ppm", "div_hi_ppm", "young_families", "young_div_lo_ppm", "young_div_hi_ppm",
                                          "gene_fraction_ppm", "low_complexity_genes")]


class IndexStats(C.Structure):
    _fields_ = [("num_kmers", C.c_uint64), ("table_slots", C.c_uint64), ("bytes_table", C.c_uint64), ("bytes_graph", C.c_uint64),
                ("bytes_classes", C.c_uint64), ("bytes_total", C.c_uint64), ("num_nodes", C.c_uint32), ("num_classes", C.c_uint32),
                ("k", C.c_uint32), ("max_class_len", C.c_uint32)]


class BusRecord(C.Structure):
    _fields_ = [("barcode", C.c_uint64), ("umi", C.c_uint64), ("ec", C.c_int32), ("count", C.c_uint32), ("flags", C.c_uint32), ("pad", C.c_uint32)]


class QuantParams(C.Structure):
    _fields_ = [("mean_read_len", C.c_double), ("alpha_limit", C.c_double), ("alpha_change_limit", C.c_double), ("alpha_change", C.c_double),
                ("min_iters", C.c_uint32), ("max_iters", C.c_uint32), ("check_every", C.c_uint32), ("reserved", C.c_uint32)]


class GenesParams(C.Structure):
    _fields_ = [("alpha_limit", C.c_double), ("alpha_change_limit", C.c_double), ("alpha_change", C.c_double),
                ("min_iters", C.c_uint32), ("max_iters", C.c_uint32), ("check_every", C.c_uint32), ("mode", C.c_uint32), ("reserved", C.c_uint32)]


class KneeParams(C.Structure):
    _fields_ = [("mode", C.c_uint32), ("lower", C.c_uint32), ("divisor", C.c_uint32), ("expected_cells", C.c_uint32), ("min_umis", C.c_uint32), ("reserved", C.c_uint32 * 3)]


class BgzfMember(C.Structure):
    _fields_ = [("in_off", C.c_uint64), ("out_off", C.c_uint64), ("file_off", C.c_uint64), ("in_len", C.c_uint32), ("out_len", C.c_uint32),
                ("crc32", C.c_uint32), ("reserved", C.c_uint32)]


INFLATE_STATUS_NAMES = ("OK", "BAD_MEMBER", "BAD_BLOCK_TYPE", "STORED_LEN", "TOO_MANY_SYMBOLS", "BAD_CODE_LENGTHS", "BAD_REPEAT", "NO_END_OF_BLOCK", "BAD_SYMBOL",
                        "DISTANCE_TOO_FAR", "INPUT_EXHAUSTED", "TRAILING_INPUT", "OUTPUT_TOO_LONG", "OUTPUT_TOO_SHORT", "CRC_MISMATCH")   # PA_INFLATE_*: the index is the code
PA_QUANT_STATS = 8
PA_GENES_EM, PA_GENES_UNIQUE = 0, 1
GENES_MODES = {"em": PA_GENES_EM, "unique": PA_GENES_UNIQUE}
PA_GENES_STATS = 16
GENES_STAT_NAMES = ("records", "molecules", "molecules_dropped", "unique_gene_molecules", "multi_gene_molecules", "cells", "cells_with_multi_rows", "multi_rows",
                    "multi_row_ids", "longest_multi_row", "largest_degree", "largest_cell", "most_iterations", "cells_not_converged", "matrix_entries", "cells_in_hbm")
PA_PAIR_FR, PA_PAIR_RF, PA_PAIR_FF = 0, 1, 2
PAIR_ORIENTATIONS = {"fr": PA_PAIR_FR, "rf": PA_PAIR_RF, "ff": PA_PAIR_FF}
PA_PAIR_STATS = 8
PAIR_STAT_NAMES = ("pairs", "both_mapped", "mate1_only", "mate2_only", "neither", "both_mapped_empty", "by_reference", "in_arena")
PA_STRAND_FWD, PA_STRAND_REV, PA_STRAND_BOTH = 0, 1, 2
STRANDS = {"fwd": PA_STRAND_FWD, "rev": PA_STRAND_REV, "both": PA_STRAND_BOTH}
PA_STRAND_STATS = 8
STRAND_STAT_NAMES = ("items", "both_mapped", "sense_only", "antisense_only", "neither", "ties", "by_reference", "in_arena")
PA_PAIRS_CTL_WORDS = 8
PAIRS_CTL_NAMES = ("first_bad", "max_len1", "max_len2", "bytes1", "bytes2", "first_outside")
PA_PAIRS_WHOLE_READ = 0xFFFFFFFF
PA_MAX_ARENA_ENTRIES = 0x7FFFFFFF
PA_QUANT_BOOT_MAX_BATCH = 64
QUANT_STAT_NAMES = ("rows", "ids", "transcripts_with_a_row", "longest_row", "largest_degree", "reads_used", "novel_reads_left_out", "iterations")


# name -> (restype, argtypes); every symbol declared in include/pseudoaligner_amd.h
SIGNATURES = {
    "pa_abi_version": (C.c_uint32, []),
    "pa_device_count": (C.c_int, []),
    "pa_last_error": (C.c_char_p, []),
    "pa_host_index_build_fasta": (C.c_int, [C.c_char_p, C.c_uint32, C.c_int, C.POINTER(vp)]),
    "pa_host_index_build_packed": (C.c_int, [vp, vp, C.c_uint32, C.c_uint32, C.c_int, C.POINTER(vp)]),
    "pa_host_index_build_fasta_device": (C.c_int, [C.c_char_p, C.c_uint32, C.c_int, C.POINTER(vp)]),
    "pa_host_index_build_packed_device": (C.c_int, [vp, vp, C.c_uint32, C.c_uint32, C.c_int, C.POINTER(vp)]),
    "pa_host_index_from_flat": (C.c_int, [C.POINTER(FlatIndex), C.POINTER(vp)]),
    "pa_host_index_view": (C.c_int, [vp, C.POINTER(FlatIndex)]),
    "pa_host_index_compare": (C.c_int, [vp, vp, C.c_uint64, C.c_char_p, C.c_size_t]),
    "pa_host_index_save": (C.c_int, [vp, C.c_char_p]),
    "pa_host_index_load": (C.c_int, [C.c_char_p, C.POINTER(vp)]),
    "pa_host_index_num_transcripts": (C.c_uint32, [vp]),
    "pa_host_index_tx_name": (C.c_char_p, [vp, C.c_uint32]),
    "pa_host_index_tx_gene": (C.c_char_p, [vp, C.c_uint32]),
    "pa_host_index_genes": (C.c_int, [vp, vp, u32p]),
    "pa_host_index_gene_name": (C.c_char_p, [vp, C.c_uint32]),
    "pa_counts_collapse_genes": (C.c_int, [vp, vp, C.c_uint64, vp]),
    "pa_host_index_mappability": (C.c_int, [vp, vp, vp]),
    "pa_write_mappability_tsv": (C.c_int, [vp, C.c_char_p]),
    "pa_host_index_transcripts": (C.c_int, [vp, C.POINTER(vp), C.POINTER(vp), u32p]),
    "pa_host_index_destroy": (None, [vp]),
    "pa_index_create": (C.c_int, [C.POINTER(FlatIndex), C.c_int, C.POINTER(vp)]),
    "pa_index_create_multi": (C.c_int, [C.POINTER(FlatIndex), C.POINTER(C.c_int), C.c_int, C.POINTER(vp)]),
    "pa_index_get_stats": (C.c_int, [vp, C.POINTER(IndexStats)]),
    "pa_index_destroy": (None, [vp]),
    "pa_tiles_words": (C.c_size_t, [C.c_uint64, C.c_uint32]),
    "pa_words_per_read": (C.c_uint32, [C.c_uint32]),
    "pa_encode_reads_device": (C.c_int, [vp, vp, vp, C.c_uint64, C.c_uint32, vp, vp, vp]),
    "pa_encode_reads_host": (C.c_int, [vp, vp, C.c_uint64, C.c_uint32, vp, vp]),
    "pa_map_batch_device": (C.c_int, [vp, vp, vp, C.c_uint64, C.c_uint32, C.c_uint32, vp, vp, C.c_uint64, vp, vp]),
    "pa_map_count_batch_device": (C.c_int, [vp, vp, vp, C.c_uint64, C.c_uint32, C.c_uint32, vp, vp, C.c_uint64, vp, vp]),
    "pa_map_count_batch_uniform_device": (C.c_int, [vp, vp, C.c_uint32, C.c_uint64, C.c_uint32, C.c_uint32, vp, vp, C.c_uint64, vp, vp]),
    "pa_map_finish": (C.c_int, [vp, vp, u64p, u64p]),
    "pa_index_release_stream": (C.c_int, [vp, vp]),
    "pa_map_batch_packed": (C.c_int, [vp, vp, vp, vp, C.c_uint64, C.c_int, C.c_uint32, vp, vp, C.POINTER(vp)]),
    "pa_map_read_packed": (C.c_int, [vp, vp, C.c_uint32, C.c_int, C.c_uint32, vp, C.c_uint32, u32p, u32p, u32p]),
    "pa_record_stream_create": (C.c_int, [vp, C.c_int, C.c_uint64, C.POINTER(vp)]),
    "pa_record_stream_create_multi": (C.c_int, [C.POINTER(vp), C.c_int, C.c_int, C.c_uint64, C.POINTER(vp)]),
    "pa_records_push": (C.c_int, [vp, vp, vp, vp, vp, C.c_uint64]),
    "pa_records_pull": (C.c_int, [vp, vp, C.c_size_t, C.POINTER(C.c_size_t)]),
    "pa_records_flush": (C.c_int, [vp]),
    "pa_record_stream_stats": (C.c_int, [vp, u64p, u64p]),
    "pa_record_stream_destroy": (None, [vp]),
    "pa_index_set_timing": (C.c_int, [vp, C.c_int]),
    "pa_map_kernel_ms": (C.c_int, [vp, vp, C.POINTER(C.c_float)]),
    "pa_map_stage_ms": (C.c_int, [vp, vp, C.POINTER(C.c_float)]),
    "pa_process_reads_stage_seconds": (C.c_int, [C.POINTER(C.c_double)]),
    "pa_record_stream_stage_seconds": (C.c_int, [vp, C.POINTER(C.c_double)]),
    "pa_process_reads_input_stats": (C.c_int, [u64p]),
    "pa_map_arena_hint": (C.c_uint64, [vp, C.c_uint64]),
    "pa_map_tiles_host": (C.c_int, [vp, vp, vp, C.c_uint32, C.c_uint64, C.c_uint32, C.c_uint32, vp, vp, C.c_uint64, u64p, vp, C.c_uint64, C.c_int]),
    "pa_host_alloc_pinned": (C.c_int, [C.c_size_t, C.POINTER(vp)]),
    "pa_host_free_pinned": (C.c_int, [vp]),
    "pa_compact_scratch_bytes": (C.c_size_t, [C.c_uint64]),
    "pa_results_compact_device": (C.c_int, [vp, vp, vp, C.c_uint64, C.c_uint64, vp, vp, C.c_uint64, vp, vp, C.c_size_t, vp]),
    "pa_map_batch": (C.c_int, [vp, vp, vp, C.c_uint64, C.c_uint32, vp, vp, C.POINTER(vp)]),
    "pa_map_read": (C.c_int, [vp, C.c_char_p, C.c_uint32, vp, C.c_uint32, u32p, u32p]),
    "pa_map_read_with_mismatch": (C.c_int, [vp, C.c_char_p, C.c_uint32, C.c_uint32, vp, C.c_uint32, u32p, u32p, u32p]),
    "pa_map_read_to_nodes": (C.c_int, [vp, C.c_char_p, C.c_uint32, C.c_uint32, vp, C.c_uint32, u32p, u32p, u32p]),
    "pa_map_batch_nodes": (C.c_int, [vp, vp, vp, C.c_uint64, C.c_uint32, vp, vp, C.c_uint32, vp]),
    "pa_process_reads": (C.c_int, [vp, C.c_char_p, C.c_char_p, C.c_int, u64p, u64p]),
    "pa_process_reads_multi": (C.c_int, [C.POINTER(vp), C.c_int, C.c_char_p, C.c_char_p, C.c_int, u64p, u64p]),
    "pa_fastq_scan_host": (C.c_int, [C.c_char_p, C.c_int, u64p, u64p, u32p, u32p, C.c_uint64, C.POINTER(C.c_int)]),
    "pa_bgzf_scan": (C.c_int, [vp, C.c_uint64, C.POINTER(BgzfMember), C.c_uint64, u64p, u64p]),
    "pa_bgzf_inflate_device": (C.c_int, [C.c_int, vp, C.c_uint64, vp, C.c_uint64, vp, C.c_uint64, vp, vp]),
    "pa_inflate_status_name": (C.c_char_p, [C.c_uint32]),
    "pa_counts_len": (C.c_uint64, [vp]),
    "pa_counts_accumulate_device": (C.c_int, [vp, vp, vp, vp, C.c_uint64, vp, vp]),
    "pa_counts_by_barcode_device": (C.c_int, [vp, vp, vp, vp, C.c_uint64, C.c_uint32, vp, vp, u64p, vp]),
    "pa_cell_counter_create": (C.c_int, [vp, vp, vp, C.c_uint32, C.c_char_p, C.c_uint64, C.c_uint32, C.c_uint32, C.POINTER(vp)]),
    "pa_cell_counter_add_device": (C.c_int, [vp, vp, vp, vp, vp, C.c_uint64, vp]),
    "pa_cell_counter_finish": (C.c_int, [vp, u64p]),
    "pa_cell_counter_matrix": (C.c_int, [vp, vp, vp, vp, C.c_uint64]),
    "pa_cell_counter_stats": (C.c_int, [vp, vp]),
    "pa_cell_counter_destroy": (None, [vp]),
    "pa_whitelist_load": (C.c_int, [C.c_char_p, C.c_uint32, vp, C.c_uint64, u64p]),
    "pa_count_cells": (C.c_int, [vp, vp, C.c_char_p, C.c_char_p, C.c_char_p, C.c_uint32, C.c_uint32, C.c_char_p, C.c_int, vp]),
    "pa_bus_create": (C.c_int, [vp, vp, C.c_uint32, C.c_uint32, C.POINTER(vp)]),
    "pa_bus_add_device": (C.c_int, [vp, vp, vp, C.c_uint64, vp, vp, C.c_uint64, vp]),
    "pa_bus_finish": (C.c_int, [vp, u64p, u32p]),
    "pa_bus_records": (C.c_int, [vp, vp, C.c_uint64]),
    "pa_bus_ecs": (C.c_int, [vp, vp, vp, C.c_uint64, u64p]),
    "pa_bus_stats": (C.c_int, [vp, vp]),
    "pa_bus_write": (C.c_int, [vp, C.c_char_p]),
    "pa_bus_destroy": (None, [vp]),
    "pa_write_bus": (C.c_int, [vp, vp, C.c_char_p, C.c_char_p, C.c_uint32, C.c_uint32, C.c_char_p, C.c_int, vp]),
    "pa_bus_whitelist_pack": (C.c_int, [C.c_char_p, C.c_uint64, C.c_uint32, vp]),
    "pa_bus_correct_records": (C.c_int, [vp, vp, C.c_uint64, C.c_uint32, C.c_uint32, vp, C.c_uint64, vp, C.c_uint64, u64p, vp]),
    "pa_bus_correct": (C.c_int, [vp, vp, C.c_uint64, vp]),
    "pa_bus_correct_phase_ms": (C.c_int, [C.POINTER(C.c_float)]),
    "pa_write_bus_corrected": (C.c_int, [vp, vp, C.c_char_p, C.c_char_p, C.c_char_p, C.c_uint32, C.c_uint32, C.c_char_p, C.c_int, vp, vp]),
    "pa_knee_default_params": (None, [C.POINTER(KneeParams)]),
    "pa_bus_knee_records": (C.c_int, [vp, vp, C.c_uint64, C.c_uint32, C.c_uint32, C.POINTER(KneeParams), vp, C.c_uint64, u64p, vp, C.c_uint64, u64p, vp]),
    "pa_bus_knee": (C.c_int, [vp, C.POINTER(KneeParams), vp, C.c_uint64, u64p, vp, C.c_uint64, u64p, vp]),
    "pa_bus_knee_phase_ms": (C.c_int, [C.POINTER(C.c_float)]),
    "pa_bus_keep_records": (C.c_int, [vp, vp, C.c_uint64, C.c_uint32, C.c_uint32, vp, C.c_uint64, vp, C.c_uint64, u64p, vp]),
    "pa_bus_keep": (C.c_int, [vp, vp, C.c_uint64, vp]),
    "pa_write_barcode_ranks_tsv": (C.c_int, [vp, C.c_uint64, C.c_uint32, C.c_char_p]),
    "pa_write_bus_called": (C.c_int, [vp, vp, C.c_char_p, C.c_char_p, C.c_char_p, C.c_uint32, C.c_uint32, C.POINTER(KneeParams), C.c_char_p, C.c_int, vp, vp, vp]),
    "pa_count_cells_em_called": (C.c_int, [vp, vp, C.c_char_p, C.c_char_p, C.c_char_p, C.c_uint32, C.c_uint32, C.POINTER(KneeParams), C.POINTER(GenesParams), C.c_char_p, C.c_int,
                                           vp, vp, vp]),
    "pa_bus_umi_correct_records": (C.c_int, [vp, vp, C.c_uint64, vp, vp, C.c_uint32, C.c_uint32, vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, vp, C.c_uint64, u64p, vp]),
    "pa_bus_umi_correct": (C.c_int, [vp, vp, C.c_uint32, C.c_uint32, vp]),
    "pa_bus_umi_correct_phase_ms": (C.c_int, [C.POINTER(C.c_float)]),
    "pa_write_bus_umi": (C.c_int, [vp, vp, C.c_char_p, C.c_char_p, C.c_char_p, C.c_uint32, C.c_uint32, C.c_int, C.POINTER(KneeParams), C.c_uint32, C.c_char_p, C.c_int, vp, vp, vp,
                                   vp]),
    "pa_count_cells_em_umi": (C.c_int, [vp, vp, C.c_char_p, C.c_char_p, C.c_char_p, C.c_uint32, C.c_uint32, C.c_int, C.POINTER(KneeParams), C.c_uint32, C.POINTER(GenesParams),
                                        C.c_char_p, C.c_int, vp, vp, vp, vp]),
    "pa_genes_default_params": (None, [C.POINTER(GenesParams)]),
    "pa_genes_create": (C.c_int, [vp, vp, C.c_uint64, vp, vp, C.c_uint32, C.c_uint32, vp, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(GenesParams), C.POINTER(vp)]),
    "pa_genes_create_from_bus": (C.c_int, [vp, vp, C.c_uint32, C.POINTER(GenesParams), C.POINTER(vp)]),
    "pa_genes_step": (C.c_int, [vp, C.c_uint32]),
    "pa_genes_run": (C.c_int, [vp, u32p, u64p]),
    "pa_genes_layout": (C.c_int, [vp, u64p, u64p]),
    "pa_genes_values": (C.c_int, [vp, vp, vp, vp, vp, C.c_uint64]),
    "pa_genes_cell_iters": (C.c_int, [vp, vp]),
    "pa_genes_matrix": (C.c_int, [vp, vp, vp, vp, C.c_uint64, u64p]),
    "pa_genes_stats": (C.c_int, [vp, vp]),
    "pa_genes_write": (C.c_int, [vp, vp, C.c_char_p]),
    "pa_genes_destroy": (None, [vp]),
    "pa_count_cells_em": (C.c_int, [vp, vp, C.c_char_p, C.c_char_p, C.c_uint32, C.c_uint32, C.POINTER(GenesParams), C.c_char_p, C.c_int, vp]),
    "pa_count_cells_em_corrected": (C.c_int, [vp, vp, C.c_char_p, C.c_char_p, C.c_char_p, C.c_uint32, C.c_uint32, C.POINTER(GenesParams), C.c_char_p, C.c_int, vp, vp]),
    "pa_quant_default_params": (None, [C.POINTER(QuantParams)]),
    "pa_quant_create": (C.c_int, [vp, vp, C.POINTER(QuantParams), C.POINTER(vp)]),
    "pa_quant_set_counts": (C.c_int, [vp, vp, C.c_uint64, vp, C.c_uint64]),
    "pa_quant_step": (C.c_int, [vp, C.c_uint32]),
    "pa_quant_run": (C.c_int, [vp, u32p, C.POINTER(C.c_int)]),
    "pa_quant_alpha": (C.c_int, [vp, vp]),
    "pa_quant_fetch": (C.c_int, [vp, vp, vp, vp]),
    "pa_quant_fetch_genes": (C.c_int, [vp, vp, vp]),
    "pa_quant_stats": (C.c_int, [vp, vp]),
    "pa_write_abundance_tsv": (C.c_int, [vp, C.c_char_p]),
    "pa_quant_destroy": (None, [vp]),
    "pa_quant_bootstrap_draw": (C.c_int, [vp, C.c_uint64, C.c_uint32, C.c_uint32]),
    "pa_quant_bootstrap_counts": (C.c_int, [vp, C.c_uint32, vp, C.c_uint64, vp, C.c_uint64]),
    "pa_quant_bootstrap_step": (C.c_int, [vp, C.c_uint32]),
    "pa_quant_bootstrap_run": (C.c_int, [vp, vp, vp]),
    "pa_quant_bootstrap_fetch": (C.c_int, [vp, vp, vp]),
    "pa_revcomp_tiles_device": (C.c_int, [vp, vp, vp, C.c_uint64, C.c_uint32, vp, vp]),
    "pa_pairs_scratch_bytes": (C.c_size_t, [C.c_uint64]),
    "pa_pairs_combine_device": (C.c_int, [vp, vp, vp, vp, vp, C.c_uint64, vp, vp, C.c_uint64, vp, vp, C.c_size_t, vp]),
    "pa_pairs_finish": (C.c_int, [vp, vp, vp, vp, u64p, u64p]),
    "pa_map_pairs": (C.c_int, [vp, vp, vp, vp, vp, C.c_uint64, C.c_int, C.c_uint32, vp, vp, C.POINTER(vp)]),
    "pa_count_pairs": (C.c_int, [vp, C.c_char_p, C.c_char_p, C.c_int, C.c_uint32, C.c_int, vp, u64p, vp]),
    "pa_strands_scratch_bytes": (C.c_size_t, [C.c_uint64]),
    "pa_strands_merge_device": (C.c_int, [vp, vp, vp, vp, vp, C.c_uint64, vp, vp, C.c_uint64, vp, vp, C.c_size_t, vp]),
    "pa_strands_finish": (C.c_int, [vp, vp, vp, vp, u64p, u64p]),
    "pa_map_batch_strand": (C.c_int, [vp, vp, vp, C.c_uint64, C.c_int, C.c_uint32, vp, vp, C.POINTER(vp)]),
    "pa_map_pairs_unstranded": (C.c_int, [vp, vp, vp, vp, vp, C.c_uint64, C.c_uint32, vp, vp, C.POINTER(vp)]),
    "pa_count_pairs_unstranded": (C.c_int, [vp, C.c_char_p, C.c_char_p, C.c_uint32, C.c_int, vp, u64p, vp]),
    "pa_pairs_input_stats": (C.c_int, [u64p]),
    "pa_pairs_input_path": (C.c_int, []),
    "pa_pairs_gather_scratch_bytes": (C.c_size_t, [C.c_uint64]),
    "pa_pairs_gather_device": (C.c_int, [C.c_int, vp, C.c_uint64, vp, vp, C.c_uint64, vp, C.c_uint64, C.c_uint32, C.c_uint64, vp, C.c_uint64, vp, vp, C.c_uint64, vp, vp,
                                         vp, C.c_size_t, vp]),
    "pa_overflow_create": (C.c_int, [C.c_int, C.c_uint64, C.c_uint64, C.POINTER(vp)]),
    "pa_overflow_destroy": (None, [vp]),
    "pa_overflow_reset": (C.c_int, [vp, vp]),
    "pa_index_set_overflow": (C.c_int, [vp, vp]),
    "pa_overflow_fetch": (C.c_int, [vp, vp, C.POINTER(vp), u64p]),
    "pa_overflow_merge": (C.c_int, [vp, vp, C.c_int, vp, C.c_uint64, u64p]),
    "pa_comm_unique_id": (C.c_int, [vp]),
    "pa_comm_create": (C.c_int, [C.c_int, C.c_int, C.c_int, vp, C.POINTER(vp)]),
    "pa_comm_destroy": (None, [vp]),
    "pa_comm_rank": (C.c_int, [vp]),
    "pa_comm_size": (C.c_int, [vp]),
    "pa_counts_allreduce": (C.c_int, [vp, vp, vp, vp]),
    "pa_overflow_allgather": (C.c_int, [vp, vp, vp, C.POINTER(vp), u64p]),
    "pa_txome_synthesize": (C.c_int, [C.c_uint32, C.c_uint32, C.c_uint64, C.POINTER(vp)]),
    "pa_txome_synthesize_repeats": (C.c_int, [C.c_uint32, C.c_uint32, C.c_uint64, C.POINTER(SynthRepeats), C.POINTER(vp)]),
    "pa_txome_from_host_index": (C.c_int, [vp, C.POINTER(vp)]),
    "pa_txome_from_fasta": (C.c_int, [C.c_char_p, C.POINTER(vp)]),
    "pa_txome_view": (C.c_int, [vp, C.POINTER(vp), C.POINTER(vp), u32p]),
    "pa_txome_destroy": (None, [vp]),
    "pa_simulate_reads_host": (C.c_int, [vp, C.c_uint32, C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint32, vp, vp]),
    "pa_txome_upload": (C.c_int, [vp, C.c_uint32, C.c_int, C.POINTER(vp)]),
    "pa_txome_device_destroy": (None, [vp]),
    "pa_simulate_reads_device": (C.c_int, [vp, C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint32, vp, vp, vp]),
    "pa_event_create": (C.c_int, [C.POINTER(vp)]),
    "pa_event_record": (C.c_int, [vp, vp]),
    "pa_event_elapsed_ms": (C.c_int, [vp, vp, C.POINTER(C.c_float)]),
    "pa_event_destroy": (C.c_int, [vp]),
    "pa_device_malloc": (C.c_int, [C.c_int, C.c_size_t, C.POINTER(vp)]),
    "pa_device_free": (C.c_int, [vp]),
    "pa_memcpy_h2d": (C.c_int, [vp, vp, C.c_size_t, vp]),
    "pa_memcpy_d2h": (C.c_int, [vp, vp, C.c_size_t, vp]),
    "pa_memset_device": (C.c_int, [vp, C.c_int, C.c_size_t, vp]),
    "pa_stream_synchronize": (C.c_int, [vp]),
}

_lib = None


def library_path() -> Path:
    """the in-tree product library; PA_PRODUCT_SO (A/B runs of bench.py against an older build, tools/baseline) overrides it"""
    import os
    alt = os.environ.get("PA_PRODUCT_SO")
    return Path(alt) if alt else _build.PRODUCT_SO


def lib() -> C.CDLL:
    """Load libpseudoaligner_amd.so. There is no fallback: a missing library is an error."""
    global _lib
    if _lib is None:
        path = library_path()
        if not path.exists():
            raise ImportError("%s is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                              "(hipcc --offload-arch=gfx950); there is no CPU fallback" % path)
        handle = C.CDLL(str(path))
        for name, (res, args) in SIGNATURES.items():
            if path != _build.PRODUCT_SO and not hasattr(handle, name):
                continue                 # an older build under PA_PRODUCT_SO may lack newer entry points
            fn = getattr(handle, name)   # AttributeError if the library does not export a declared symbol
            fn.restype = res
            fn.argtypes = args
        _lib = handle
    return _lib


def check(rc: int) -> int:
    if rc < 0:
        raise PaError(rc, (lib().pa_last_error() or b"").decode("utf-8", "replace"))
    return rc
