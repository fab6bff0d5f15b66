//! `extern "C"` binding of the transcript-abundance EM of include/pseudoaligner_amd.h (pa_quant_*, pa_write_abundance_tsv): the
//! counterpart of the single-cell matrix for bulk RNA-seq. Add `mod amd_quant_ffi;` to src/lib.rs next to `mod amd_ffi;`.
#![allow(non_camel_case_types, dead_code)]
use std::os::raw::{c_char, c_int};

use crate::amd_ffi::{PaHostIndex, PaIndex};

#[repr(C)] pub struct PaQuant { _private: [u8; 0] }

/// pa_quant_params; fill it with pa_quant_default_params first (kallisto's stop rule: 50, 10 000, 1e-2, 1e-2, 1e-7; check_every 10)
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct PaQuantParams {
    pub mean_read_len: f64, pub alpha_limit: f64, pub alpha_change_limit: f64, pub alpha_change: f64,
    pub min_iters: u32, pub max_iters: u32, pub check_every: u32, pub reserved: u32,
}

pub const PA_QUANT_STATS: usize = 8;
pub const PA_QUANT_BOOT_MAX_BATCH: u32 = 64;

extern "C" {
    pub fn pa_host_index_num_transcripts(h: *const PaHostIndex) -> u32;   // the length of every per-transcript output below
    pub fn pa_quant_default_params(p: *mut PaQuantParams);
    pub fn pa_quant_create(idx: *mut PaIndex, h: *const PaHostIndex, p: *const PaQuantParams, out: *mut *mut PaQuant) -> c_int;
    pub fn pa_quant_set_counts(q: *mut PaQuant, class_counts: *const u64, counts_len: u64, overflow_words: *const u32, n_words: u64) -> c_int;
    pub fn pa_quant_step(q: *mut PaQuant, n_iters: u32) -> c_int;
    pub fn pa_quant_run(q: *mut PaQuant, iters: *mut u32, converged: *mut c_int) -> c_int;
    pub fn pa_quant_alpha(q: *const PaQuant, alpha: *mut f64) -> c_int;
    pub fn pa_quant_fetch(q: *const PaQuant, est_counts: *mut f64, tpm: *mut f64, eff_len: *mut f64) -> c_int;
    pub fn pa_quant_fetch_genes(q: *const PaQuant, est_counts: *mut f64, tpm: *mut f64) -> c_int;
    pub fn pa_quant_stats(q: *const PaQuant, stats: *mut u64) -> c_int;   // u64 stats[PA_QUANT_STATS]
    pub fn pa_write_abundance_tsv(q: *const PaQuant, path: *const c_char) -> c_int;
    pub fn pa_quant_destroy(q: *mut PaQuant);
    // bootstrap replicates: a batch of at most PA_QUANT_BOOT_MAX_BATCH resampled EM runs (the rules are in the header)
    pub fn pa_quant_bootstrap_draw(q: *mut PaQuant, seed: u64, first: u32, n: u32) -> c_int;
    pub fn pa_quant_bootstrap_counts(q: *const PaQuant, k: u32, class_counts: *mut u64, counts_len: u64, overflow_counts: *mut u64, n_records: u64) -> c_int;
    pub fn pa_quant_bootstrap_step(q: *mut PaQuant, n_iters: u32) -> c_int;
    pub fn pa_quant_bootstrap_run(q: *mut PaQuant, iters: *mut u32, converged: *mut c_int) -> c_int;
    pub fn pa_quant_bootstrap_fetch(q: *const PaQuant, est_counts: *mut f64, tpm: *mut f64) -> c_int;
}
