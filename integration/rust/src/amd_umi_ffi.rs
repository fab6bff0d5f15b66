//! `extern "C"` binding of the UMI correction on BUS records of include/pseudoaligner_amd.h (pa_bus_umi_correct* and the two file-level calls
//! that take every record step): a UMI one substitution away from a better-supported UMI of its barcode whose gene set meets its own is joined
//! to it on the GPU, between the barcode steps and the gene counter. Add `mod amd_umi_ffi;` to src/lib.rs next to `mod amd_bus_ffi;`,
//! `mod amd_genes_ffi;`, `mod amd_correct_ffi;` and `mod amd_knee_ffi;` (`amd::bus_umi_correct`, `amd::write_bus_umi` and
//! `amd::count_cells_em_umi` use it).
#![allow(non_camel_case_types, dead_code)]
use std::os::raw::{c_char, c_int};

use crate::amd_bus_ffi::{PaBus, PaBusRecord};
use crate::amd_ffi::{PaHostIndex, PaIndex};
use crate::amd_genes_ffi::PaGenesParams;
use crate::amd_knee_ffi::PaKneeParams;

pub const PA_UMI_GREATEST: u32 = 0;
pub const PA_UMI_DIRECTIONAL: u32 = 1;
pub const PA_BUS_UMI_STATS: usize = 15;
pub const PA_BUS_UMI_PHASES: usize = 4;

extern "C" {
    pub fn pa_bus_umi_correct_records(idx: *mut PaIndex, records: *const PaBusRecord, n: u64, ec_offsets: *const u64, ec_ids: *const u32, n_ecs: u32,
                                      num_tx: u32, tx_gene: *const u32, num_genes: u32, bc_len: u32, umi_len: u32, mode: u32, out: *mut PaBusRecord,
                                      cap: u64, n_out: *mut u64, stats: *mut u64) -> c_int;   // u64 stats[PA_BUS_UMI_STATS]
    pub fn pa_bus_umi_correct(finished: *mut PaBus, tx_gene: *const u32, num_genes: u32, mode: u32, stats: *mut u64) -> c_int;
    pub fn pa_bus_umi_correct_phase_ms(out: *mut f32) -> c_int;   // f32 out[PA_BUS_UMI_PHASES]
    pub fn pa_write_bus_umi(idx: *mut PaIndex, h: *const PaHostIndex, r1_path: *const c_char, r2_path: *const c_char, whitelist_path: *const c_char,
                            bc_len: u32, umi_len: u32, call_cells: c_int, kp: *const PaKneeParams, umi_mode: u32, out_dir: *const c_char,
                            num_threads: c_int, bus_stats: *mut u64, correct_stats: *mut u64, knee_stats: *mut u64, umi_stats: *mut u64) -> c_int;
    pub fn pa_count_cells_em_umi(idx: *mut PaIndex, h: *const PaHostIndex, r1_path: *const c_char, r2_path: *const c_char,
                                 whitelist_path: *const c_char, bc_len: u32, umi_len: u32, call_cells: c_int, kp: *const PaKneeParams, umi_mode: u32,
                                 p: *const PaGenesParams, out_dir: *const c_char, num_threads: c_int, genes_stats: *mut u64,
                                 correct_stats: *mut u64, knee_stats: *mut u64, umi_stats: *mut u64) -> c_int;
}
