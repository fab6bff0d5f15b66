//! `extern "C"` binding of the unstranded stage of include/pseudoaligner_amd.h (pa_strands_*, pa_map_batch_strand, pa_map_pairs_unstranded,
//! pa_count_pairs_unstranded): both strands mapped, the two answers merged per item. Add `mod amd_strands_ffi;` to src/lib.rs next to
//! `mod amd_ffi;`.
#![allow(non_camel_case_types, dead_code)]
use std::os::raw::{c_char, c_int, c_void};

use crate::amd_ffi::{PaIndex, PaReadResult};

pub const PA_STRAND_FWD: c_int = 0;    // the reads as given
pub const PA_STRAND_REV: c_int = 1;    // their reverse complements
pub const PA_STRAND_BOTH: c_int = 2;   // both, merged
pub const PA_STRAND_STATS: usize = 8;

extern "C" {
    pub fn pa_strands_scratch_bytes(n: u64) -> usize;
    pub fn pa_strands_merge_device(idx: *mut PaIndex, d_resS: *const PaReadResult, d_arenaS: *const u32, d_resR: *const PaReadResult,
                                   d_arenaR: *const u32, n: u64, d_results: *mut PaReadResult, d_arena: *mut u32, arena_cap: u64,
                                   d_counts: *mut u64, d_scratch: *mut c_void, scratch_bytes: usize, stream: *mut c_void) -> c_int;
    pub fn pa_strands_finish(idx: *mut PaIndex, d_scratch: *mut c_void, stream: *mut c_void, stats: *mut u64, arena_used: *mut u64,
                             arena_needed: *mut u64) -> c_int;   // u64 stats[PA_STRAND_STATS]
    pub fn pa_map_batch_strand(idx: *mut PaIndex, ascii: *const u8, offsets: *const u64, n_reads: u64, strand: c_int, allowed_mismatches: u32,
                               results: *mut PaReadResult, class_offsets: *mut u64, class_ids: *mut *const u32) -> c_int;
    pub fn pa_map_pairs_unstranded(idx: *mut PaIndex, ascii1: *const u8, offsets1: *const u64, ascii2: *const u8, offsets2: *const u64,
                                   n_pairs: u64, allowed_mismatches: u32, results: *mut PaReadResult, class_offsets: *mut u64,
                                   class_ids: *mut *const u32) -> c_int;
    pub fn pa_count_pairs_unstranded(idx: *mut PaIndex, r1_path: *const c_char, r2_path: *const c_char, allowed_mismatches: u32, num_threads: c_int,
                                     h_counts: *mut u64, n_pairs: *mut u64, stats: *mut u64) -> c_int;   // u64 stats[PA_STRAND_STATS]
}
