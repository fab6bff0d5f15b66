//! `extern "C"` binding of the paired-end stage of include/pseudoaligner_amd.h (pa_revcomp_tiles_device, pa_pairs_*, pa_map_pairs):
//! mates oriented, mapped by two ordinary launches, their classes intersected per pair. Add `mod amd_pairs_ffi;` to src/lib.rs next to
//! `mod amd_ffi;`.
#![allow(non_camel_case_types, dead_code)]
use std::os::raw::{c_char, c_int, c_void};

use crate::amd_ffi::{PaIndex, PaReadResult};

pub const PA_PAIR_FR: c_int = 0;   // mate 1 as given, mate 2 reverse-complemented
pub const PA_PAIR_RF: c_int = 1;   // mate 1 reverse-complemented, mate 2 as given
pub const PA_PAIR_FF: c_int = 2;   // both as given
pub const PA_PAIR_STATS: usize = 8;

extern "C" {
    pub fn pa_revcomp_tiles_device(idx: *const PaIndex, d_tiles_in: *const u64, d_lens: *const u32, n_reads: u64, words_per_read: u32,
                                   d_tiles_out: *mut u64, stream: *mut c_void) -> c_int;
    pub fn pa_pairs_scratch_bytes(n_pairs: u64) -> usize;
    pub fn pa_pairs_combine_device(idx: *mut PaIndex, d_res1: *const PaReadResult, d_arena1: *const u32, d_res2: *const PaReadResult,
                                   d_arena2: *const u32, n_pairs: u64, d_results: *mut PaReadResult, d_arena: *mut u32, arena_cap: u64,
                                   d_counts: *mut u64, d_scratch: *mut c_void, scratch_bytes: usize, stream: *mut c_void) -> c_int;
    pub fn pa_pairs_finish(idx: *mut PaIndex, d_scratch: *mut c_void, stream: *mut c_void, stats: *mut u64, arena_used: *mut u64,
                           arena_needed: *mut u64) -> c_int;   // u64 stats[PA_PAIR_STATS]
    pub fn pa_map_pairs(idx: *mut PaIndex, ascii1: *const u8, offsets1: *const u64, ascii2: *const u8, offsets2: *const u64, n_pairs: u64,
                        orient: c_int, allowed_mismatches: u32, results: *mut PaReadResult, class_offsets: *mut u64,
                        class_ids: *mut *const u32) -> c_int;
    pub fn pa_count_pairs(idx: *mut PaIndex, r1_path: *const c_char, r2_path: *const c_char, orient: c_int, allowed_mismatches: u32, num_threads: c_int,
                          h_counts: *mut u64, n_pairs: *mut u64, stats: *mut u64) -> c_int;   // u64 stats[PA_PAIR_STATS]
}
