//! `extern "C"` binding of the device-batch single-cell counter of include/pseudoaligner_amd.h (pa_cell_counter_*): for a host that
//! maps its own device-resident R2 batches and wants the UMI matrix without the file-level pa_count_cells (amd_ffi.rs). Add
//! `mod amd_cells_ffi;` to src/lib.rs next to `mod amd_ffi;`.
#![allow(non_camel_case_types, dead_code)]
use std::os::raw::{c_char, c_int, c_void};

use crate::amd_ffi::{PaHostIndex, PaIndex, PaReadResult};

#[repr(C)] pub struct PaCellCounter { _private: [u8; 0] }

extern "C" {
    pub fn pa_cell_counter_create(idx: *mut PaIndex, h: *const PaHostIndex, tx_gene: *const u32, num_genes: u32, whitelist: *const c_char,
                                  n_whitelist: u64, bc_len: u32, umi_len: u32, out: *mut *mut PaCellCounter) -> c_int;
    pub fn pa_cell_counter_add_device(c: *mut PaCellCounter, d_results: *const PaReadResult, d_arena: *const u32, d_r1: *const u8,
                                      d_r1_offsets: *const u64, n_reads: u64, stream: *mut c_void) -> c_int;
    pub fn pa_cell_counter_finish(c: *mut PaCellCounter, n_entries: *mut u64) -> c_int;
    pub fn pa_cell_counter_matrix(c: *const PaCellCounter, cell: *mut u32, gene: *mut u32, umis: *mut u32, cap: u64) -> c_int;
    pub fn pa_cell_counter_stats(c: *const PaCellCounter, stats: *mut u64) -> c_int;   // u64 stats[PA_CELL_STATS]
    pub fn pa_cell_counter_destroy(c: *mut PaCellCounter);
}
