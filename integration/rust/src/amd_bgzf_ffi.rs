//! `extern "C"` binding of the BGZF part of include/pseudoaligner_amd.h (pa_bgzf_scan, pa_bgzf_inflate_device, pa_inflate_status_name): the
//! member table of a blocked gzip file found on the host, the members inflated on the GPU. Add `mod amd_bgzf_ffi;` to src/lib.rs next to
//! `mod amd_ffi;`.
#![allow(non_camel_case_types, dead_code)]
use std::os::raw::{c_char, c_int, c_void};

pub const PA_ERR_NOT_BGZF: c_int = -11;
pub const PA_BGZF_MAX_ISIZE: u32 = 65536;
pub const PA_INGEST_INPUT_STATS: usize = 6;
pub const PA_INFLATE_OK: u32 = 0;
pub const PA_INFLATE_BAD_MEMBER: u32 = 1;
pub const PA_INFLATE_BAD_BLOCK_TYPE: u32 = 2;
pub const PA_INFLATE_STORED_LEN: u32 = 3;
pub const PA_INFLATE_TOO_MANY_SYMBOLS: u32 = 4;
pub const PA_INFLATE_BAD_CODE_LENGTHS: u32 = 5;
pub const PA_INFLATE_BAD_REPEAT: u32 = 6;
pub const PA_INFLATE_NO_END_OF_BLOCK: u32 = 7;
pub const PA_INFLATE_BAD_SYMBOL: u32 = 8;
pub const PA_INFLATE_DISTANCE_TOO_FAR: u32 = 9;
pub const PA_INFLATE_INPUT_EXHAUSTED: u32 = 10;
pub const PA_INFLATE_TRAILING_INPUT: u32 = 11;
pub const PA_INFLATE_OUTPUT_TOO_LONG: u32 = 12;
pub const PA_INFLATE_OUTPUT_TOO_SHORT: u32 = 13;
pub const PA_INFLATE_CRC_MISMATCH: u32 = 14;

/// one row of the member table (`pa_bgzf_member`)
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct PaBgzfMember {
    pub in_off: u64,
    pub out_off: u64,
    pub file_off: u64,
    pub in_len: u32,
    pub out_len: u32,
    pub crc32: u32,
    pub reserved: u32,
}

extern "C" {
    pub fn pa_bgzf_scan(data: *const u8, size: u64, members: *mut PaBgzfMember, cap: u64, n: *mut u64, text_bytes: *mut u64) -> c_int;
    pub fn pa_bgzf_inflate_device(device: c_int, d_comp: *const u8, comp_bytes: u64, d_members: *const PaBgzfMember, n_members: u64,
                                  d_text: *mut u8, text_cap: u64, d_status: *mut u32, stream: *mut c_void) -> c_int;
    pub fn pa_inflate_status_name(status: u32) -> *const c_char;
    pub fn pa_process_reads_input_stats(out: *mut u64) -> c_int;   // u64 out[PA_INGEST_INPUT_STATS]
}
