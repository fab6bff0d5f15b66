//! `extern "C"` binding of the pair scan of include/pseudoaligner_amd.h (pa_pairs_gather_scratch_bytes, pa_pairs_gather_device): the ids of
//! record i of two FASTQ texts in HBM compared, R2's sequences and R1's prefixes gathered back to back. Add `mod amd_pairscan_ffi;` to
//! src/lib.rs next to `mod amd_ffi;`.
#![allow(non_camel_case_types, dead_code)]
use std::os::raw::{c_int, c_void};

pub const PA_PAIRS_CTL_WORDS: usize = 8;          // u64 d_ctl[]: first bad, max_len1, max_len2, bytes1, bytes2, first outside, two unused
pub const PA_PAIRS_WHOLE_READ: u32 = 0xFFFFFFFF;  // prefix: all of R1

extern "C" {
    pub fn pa_pairs_input_stats(out: *mut u64) -> c_int;   // u64 out[2 * PA_INGEST_INPUT_STATS]: R1's six entries, then R2's
    pub fn pa_pairs_input_path() -> c_int;                 // 1: the last paired call of this thread took the device path
    pub fn pa_pairs_gather_scratch_bytes(m: u64) -> usize;
    pub fn pa_pairs_gather_device(device: c_int, d_text1: *const u8, text1_bytes: u64, d_rec1: *const u32, d_text2: *const u8, text2_bytes: u64,
                                  d_rec2: *const u32, m: u64, prefix: u32, base: u64, d_bytes1: *mut u8, cap1: u64, d_off1: *mut u64,
                                  d_bytes2: *mut u8, cap2: u64, d_off2: *mut u64, d_ctl: *mut u64, d_scratch: *mut c_void, scratch_bytes: usize,
                                  stream: *mut c_void) -> c_int;
}
