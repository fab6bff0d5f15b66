//! `extern "C"` binding of the BUS barcode correction of include/pseudoaligner_amd.h (pa_bus_correct*, pa_bus_whitelist_pack and the two
//! file-level calls with a whitelist): the `bustools correct` + re-sort step on the GPU, between the BUS writer and the gene counter. Add
//! `mod amd_correct_ffi;` to src/lib.rs next to `mod amd_bus_ffi;` and `mod amd_genes_ffi;` (`amd::write_bus_corrected` and
//! `amd::count_cells_em_corrected` use it).
#![allow(non_camel_case_types, dead_code)]
use std::os::raw::{c_char, c_int};

use crate::amd_bus_ffi::{PaBus, PaBusRecord};
use crate::amd_ffi::{PaHostIndex, PaIndex};
use crate::amd_genes_ffi::PaGenesParams;

pub const PA_BUS_CORRECT_STATS: usize = 13;
pub const PA_BUS_CORRECT_PHASES: usize = 4;

extern "C" {
    pub fn pa_bus_whitelist_pack(whitelist: *const c_char, n: u64, bc_len: u32, packed: *mut u64) -> c_int;
    pub fn pa_bus_correct_records(idx: *mut PaIndex, records: *const PaBusRecord, n: u64, bc_len: u32, umi_len: u32, whitelist: *const u64,
                                  n_whitelist: u64, out: *mut PaBusRecord, cap: u64, n_out: *mut u64, stats: *mut u64) -> c_int;   // u64 stats[PA_BUS_CORRECT_STATS]
    pub fn pa_bus_correct(finished: *mut PaBus, whitelist: *const u64, n_whitelist: u64, stats: *mut u64) -> c_int;
    pub fn pa_bus_correct_phase_ms(out: *mut f32) -> c_int;   // f32 out[PA_BUS_CORRECT_PHASES]
    pub fn pa_write_bus_corrected(idx: *mut PaIndex, h: *const PaHostIndex, r1_path: *const c_char, r2_path: *const c_char,
                                  whitelist_path: *const c_char, bc_len: u32, umi_len: u32, out_dir: *const c_char, num_threads: c_int,
                                  bus_stats: *mut u64, correct_stats: *mut u64) -> c_int;
    pub fn pa_count_cells_em_corrected(idx: *mut PaIndex, h: *const PaHostIndex, r1_path: *const c_char, r2_path: *const c_char,
                                       whitelist_path: *const c_char, bc_len: u32, umi_len: u32, p: *const PaGenesParams, out_dir: *const c_char,
                                       num_threads: c_int, genes_stats: *mut u64, correct_stats: *mut u64) -> c_int;
}
