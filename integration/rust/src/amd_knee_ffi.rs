//! `extern "C"` binding of the cell calling on BUS records of include/pseudoaligner_amd.h (pa_bus_knee*, pa_bus_keep*, the barcode_ranks.tsv
//! writer and the two file-level calls that call cells): the barcode table, its rank knee and the filter on the GPU, between the BUS writer
//! and the gene counter. Add `mod amd_knee_ffi;` to src/lib.rs next to `mod amd_bus_ffi;`, `mod amd_genes_ffi;` and `mod amd_correct_ffi;`
//! (`amd::bus_knee`, `amd::write_bus_called` and `amd::count_cells_em_called` use it).
#![allow(non_camel_case_types, dead_code)]
use std::os::raw::{c_char, c_int};

use crate::amd_bus_ffi::{PaBus, PaBusRecord};
use crate::amd_ffi::{PaHostIndex, PaIndex};
use crate::amd_genes_ffi::PaGenesParams;

pub const PA_KNEE_CURVE: u32 = 0;
pub const PA_KNEE_EXPECTED: u32 = 1;
pub const PA_KNEE_MIN: u32 = 2;
pub const PA_KNEE_STATS: usize = 10;
pub const PA_KNEE_PHASES: usize = 3;
pub const PA_BUS_KEEP_STATS: usize = 7;

#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct PaKneeParams {
    pub mode: u32,
    pub lower: u32,
    pub divisor: u32,
    pub expected_cells: u32,
    pub min_umis: u32,
    pub reserved: [u32; 3],
}

#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct PaBusBarcodeRow {
    pub barcode: u64,
    pub reads: u64,
    pub records: u32,
    pub umis: u32,
    pub rank: u32,
    pub called: u32,
}

extern "C" {
    pub fn pa_knee_default_params(p: *mut PaKneeParams);
    pub fn pa_bus_knee_records(idx: *mut PaIndex, records: *const PaBusRecord, n: u64, bc_len: u32, umi_len: u32, p: *const PaKneeParams,
                               rows: *mut PaBusBarcodeRow, rows_cap: u64, n_rows: *mut u64, called: *mut u64, called_cap: u64, n_called: *mut u64,
                               stats: *mut u64) -> c_int;   // u64 stats[PA_KNEE_STATS]
    pub fn pa_bus_knee(finished: *const PaBus, p: *const PaKneeParams, rows: *mut PaBusBarcodeRow, rows_cap: u64, n_rows: *mut u64, called: *mut u64,
                       called_cap: u64, n_called: *mut u64, stats: *mut u64) -> c_int;
    pub fn pa_bus_knee_phase_ms(out: *mut f32) -> c_int;   // f32 out[PA_KNEE_PHASES]
    pub fn pa_bus_keep_records(idx: *mut PaIndex, records: *const PaBusRecord, n: u64, bc_len: u32, umi_len: u32, barcodes: *const u64,
                               n_barcodes: u64, out: *mut PaBusRecord, cap: u64, n_out: *mut u64, stats: *mut u64) -> c_int;   // u64 stats[PA_BUS_KEEP_STATS]
    pub fn pa_bus_keep(finished: *mut PaBus, barcodes: *const u64, n_barcodes: u64, stats: *mut u64) -> c_int;
    pub fn pa_write_barcode_ranks_tsv(rows: *const PaBusBarcodeRow, n: u64, bc_len: u32, path: *const c_char) -> c_int;
    pub fn pa_write_bus_called(idx: *mut PaIndex, h: *const PaHostIndex, r1_path: *const c_char, r2_path: *const c_char,
                               whitelist_path: *const c_char, bc_len: u32, umi_len: u32, p: *const PaKneeParams, out_dir: *const c_char,
                               num_threads: c_int, bus_stats: *mut u64, correct_stats: *mut u64, knee_stats: *mut u64) -> c_int;
    pub fn pa_count_cells_em_called(idx: *mut PaIndex, h: *const PaHostIndex, r1_path: *const c_char, r2_path: *const c_char,
                                    whitelist_path: *const c_char, bc_len: u32, umi_len: u32, kp: *const PaKneeParams, p: *const PaGenesParams,
                                    out_dir: *const c_char, num_threads: c_int, genes_stats: *mut u64, correct_stats: *mut u64,
                                    knee_stats: *mut u64) -> c_int;
}
