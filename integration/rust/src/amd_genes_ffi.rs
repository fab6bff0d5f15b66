//! `extern "C"` binding of the gene counter of include/pseudoaligner_amd.h (pa_genes_*, pa_count_cells_em): cells x genes from BUS
//! records, the molecules whose records span several genes shared out by an EM per cell on the GPU (the `bustools count --genecounts
//! --em` step). Add `mod amd_genes_ffi;` to src/lib.rs next to `mod amd_ffi;` and `mod amd_bus_ffi;` (`amd::count_cells_em` uses it).
#![allow(non_camel_case_types, dead_code)]
use std::os::raw::{c_char, c_int};

use crate::amd_bus_ffi::{PaBus, PaBusRecord};
use crate::amd_ffi::{PaHostIndex, PaIndex};

pub const PA_GENES_EM: u32 = 0;
pub const PA_GENES_UNIQUE: u32 = 1;
pub const PA_GENES_STATS: usize = 16;

#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct PaGenesParams {
    pub alpha_limit: f64,
    pub alpha_change_limit: f64,
    pub alpha_change: f64,
    pub min_iters: u32,
    pub max_iters: u32,
    pub check_every: u32,
    pub mode: u32,
    pub reserved: u32,
}

#[repr(C)] pub struct PaGenes { _private: [u8; 0] }

extern "C" {
    pub fn pa_genes_default_params(p: *mut PaGenesParams);
    pub fn pa_genes_create(idx: *mut PaIndex, records: *const PaBusRecord, n: u64, ec_offsets: *const u64, ec_ids: *const u32, n_ecs: u32,
                           num_tx: u32, tx_gene: *const u32, num_genes: u32, bc_len: u32, umi_len: u32, p: *const PaGenesParams,
                           out: *mut *mut PaGenes) -> c_int;
    pub fn pa_genes_create_from_bus(finished: *const PaBus, tx_gene: *const u32, num_genes: u32, p: *const PaGenesParams,
                                    out: *mut *mut PaGenes) -> c_int;
    pub fn pa_genes_step(g: *mut PaGenes, n_iters: u32) -> c_int;
    pub fn pa_genes_run(g: *mut PaGenes, max_iters_run: *mut u32, cells_not_converged: *mut u64) -> c_int;
    pub fn pa_genes_layout(g: *const PaGenes, n_cells: *mut u64, n_values: *mut u64) -> c_int;
    pub fn pa_genes_values(g: *const PaGenes, barcode: *mut u64, cell: *mut u32, gene: *mut u32, alpha: *mut f64, cap: u64) -> c_int;
    pub fn pa_genes_cell_iters(g: *const PaGenes, iters: *mut u32) -> c_int;
    pub fn pa_genes_matrix(g: *const PaGenes, cell: *mut u32, gene: *mut u32, value: *mut f64, cap: u64, n_entries: *mut u64) -> c_int;
    pub fn pa_genes_stats(g: *const PaGenes, stats: *mut u64) -> c_int;   // u64 stats[PA_GENES_STATS]
    pub fn pa_genes_write(g: *const PaGenes, h: *const PaHostIndex, out_dir: *const c_char) -> c_int;
    pub fn pa_genes_destroy(g: *mut PaGenes);
    pub fn pa_count_cells_em(idx: *mut PaIndex, h: *const PaHostIndex, r1_path: *const c_char, r2_path: *const c_char, bc_len: u32, umi_len: u32,
                             p: *const PaGenesParams, out_dir: *const c_char, num_threads: c_int, stats: *mut u64) -> c_int;
}
