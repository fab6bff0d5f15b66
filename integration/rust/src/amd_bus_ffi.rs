//! `extern "C"` binding of the BUS output of include/pseudoaligner_amd.h (pa_bus_*, pa_write_bus): sorted, collapsed (barcode, UMI,
//! equivalence class) records for the kallisto | bustools family of tools, built on the GPU from device-resident batches or from a
//! pair of FASTQ files. Add `mod amd_bus_ffi;` to src/lib.rs next to `mod amd_ffi;` (`amd::write_bus` uses it).
#![allow(non_camel_case_types, dead_code)]
use std::os::raw::{c_char, c_int, c_void};

use crate::amd_ffi::{PaHostIndex, PaIndex, PaReadResult};

pub const PA_BUS_STATS: usize = 8;

/// = the 32-byte record of a BUS v1 file (little-endian)
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct PaBusRecord {
    pub barcode: u64,
    pub umi: u64,
    pub ec: i32,
    pub count: u32,
    pub flags: u32,
    pub pad: u32,
}

#[repr(C)] pub struct PaBus { _private: [u8; 0] }

extern "C" {
    pub fn pa_bus_create(idx: *mut PaIndex, h: *const PaHostIndex, bc_len: u32, umi_len: u32, out: *mut *mut PaBus) -> c_int;
    pub fn pa_bus_add_device(b: *mut PaBus, d_results: *const PaReadResult, d_arena: *const u32, arena_len: u64, d_r1: *const u8,
                             d_r1_offsets: *const u64, n_reads: u64, stream: *mut c_void) -> c_int;
    pub fn pa_bus_finish(b: *mut PaBus, n_records: *mut u64, n_ecs: *mut u32) -> c_int;
    pub fn pa_bus_records(b: *const PaBus, out: *mut PaBusRecord, cap: u64) -> c_int;
    pub fn pa_bus_ecs(b: *const PaBus, offsets: *mut u64, ids: *mut u32, ids_cap: u64, n_ids: *mut u64) -> c_int;
    pub fn pa_bus_stats(b: *const PaBus, stats: *mut u64) -> c_int;   // u64 stats[PA_BUS_STATS]
    pub fn pa_bus_write(b: *const PaBus, out_dir: *const c_char) -> c_int;
    pub fn pa_bus_destroy(b: *mut PaBus);
    pub fn pa_write_bus(idx: *mut PaIndex, h: *const PaHostIndex, r1_path: *const c_char, r2_path: *const c_char, bc_len: u32, umi_len: u32,
                        out_dir: *const c_char, num_threads: c_int, stats: *mut u64) -> c_int;
}
