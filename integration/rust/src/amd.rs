//! Exporter + drop-in `process_reads` for the reference crate. Add `mod amd_ffi; mod amd;` to src/lib.rs (and `mod amd_pairs_ffi;` for `map_pairs`, `mod amd_strands_ffi;` for `map_pairs_unstranded`, `mod amd_bgzf_ffi;` for `bgzf_members`, `mod amd_bus_ffi;` for `write_bus`, `mod amd_genes_ffi;` for `count_cells_em`, `mod amd_correct_ffi;` for `write_bus_corrected` / `count_cells_em_corrected`, `mod amd_knee_ffi;` for `bus_knee` / `write_bus_called` / `count_cells_em_called`, `mod amd_umi_ffi;` for `bus_umi_correct` / `write_bus_umi` / `count_cells_em_umi`).
//! The exporter only reads `pub` fields of `Pseudoaligner<K>` (src/pseudoaligner.rs:27-33); `dbg_index` (the boomphf MPHF,
//! :30) is not exported: every hit is verified against the node sequence (:99-107), which makes it an exact dictionary that
//! the library rebuilds. Not compiled in the image of this repository (no rustc): kept in step with
//! include/pseudoaligner_amd.h by integration/c/abi_check.c, which exercises the same calls from C.
use std::collections::HashMap;
use std::ffi::{CStr, CString};
use std::fmt::Debug;
use std::fs::File;
use std::io::{self, Write};
use std::path::Path;
use std::sync::{Arc, Mutex, OnceLock};

use anyhow::{anyhow, Error};                 // the crate's error type (src/pseudoaligner.rs:15)
use bio::io::fastq;
use debruijn::dna_string::DnaString;
use debruijn::{Kmer, Mer, Vmer};
use log::info;

use crate::amd_ffi::*;
use crate::config::DEFAULT_ALLOWED_MISMATCHES;
use crate::pseudoaligner::Pseudoaligner;

fn check(rc: i32) -> Result<i32, Error> {
    if rc >= 0 { return Ok(rc); }
    let msg = unsafe { CStr::from_ptr(pa_last_error()) }.to_string_lossy().into_owned();
    Err(anyhow!("pseudoaligner_amd error {}: {}", rc, msg))
}

/// The arrays of the flat index (include/pseudoaligner_amd.h, pa_flat_index), owned on the Rust side for the duration of a call.
pub struct FlatArrays {
    pub k: u32, pub num_transcripts: u32,
    pub seq: Vec<u64>, pub start: Vec<u64>, pub len: Vec<u32>, pub exts: Vec<u8>, pub colour: Vec<u32>,
    pub ec_off: Vec<u64>, pub ec_ids: Vec<u32>,
}

impl FlatArrays {
    pub fn from_pseudoaligner<K: Kmer>(al: &Pseudoaligner<K>) -> FlatArrays {
        let (mut seq, mut start, mut len, mut exts, mut colour) = (vec![0u64; 1], vec![0u64], vec![], vec![], vec![]);
        let mut pos = 0u64;
        for node in al.dbg.iter_nodes() {                       // debruijn::graph::DebruijnGraph
            let s = node.sequence();
            for i in 0..s.len() {                                // A0 C1 G2 T3, LSB-first 2-bit packing
                if pos % 32 == 0 && pos > 0 { seq.push(0); }
                *seq.last_mut().unwrap() |= (s.get(i) as u64) << (2 * (pos % 32));
                pos += 1;
            }
            start.push(pos); len.push(s.len() as u32); exts.push(node.exts().val); colour.push(*node.data());
        }
        seq.push(0); seq.push(0);                               // pad words: 32-base windows may read past the last base
        let (mut ec_off, mut ec_ids) = (vec![0u64], vec![]);
        for c in &al.eq_classes { ec_ids.extend_from_slice(c); ec_off.push(ec_ids.len() as u64); }
        FlatArrays { k: K::k() as u32, num_transcripts: al.tx_names.len() as u32, seq, start, len, exts, colour, ec_off, ec_ids }
    }

    pub fn view(&self) -> PaFlatIndex {
        PaFlatIndex { k: self.k, num_nodes: self.len.len() as u32, num_classes: (self.ec_off.len() - 1) as u32,
            num_transcripts: self.num_transcripts, seq_bases: *self.start.last().unwrap(), node_seq: self.seq.as_ptr(),
            node_start: self.start.as_ptr(), node_len: self.len.as_ptr(), node_exts: self.exts.as_ptr(),
            node_colour: self.colour.as_ptr(), ec_offset: self.ec_off.as_ptr(), ec_ids: self.ec_ids.as_ptr(),
            node_redge: std::ptr::null(), node_ledge: std::ptr::null() }
    }

    /// Write the index in the library's own container, e.g. to diff it against the index the library builds from the same
    /// FASTA: `pa_host_index_compare` (numbering and unitig break points are free; k-mer -> id-list map must agree).
    pub fn save(&self, path: &str) -> Result<(), Error> {
        let mut h = std::ptr::null_mut();
        check(unsafe { pa_host_index_from_flat(&self.view(), &mut h) })?;
        let p = CString::new(path)?;
        let rc = unsafe { pa_host_index_save(h, p.as_ptr()) };
        unsafe { pa_host_index_destroy(h) };
        check(rc).map(|_| ())
    }

    /// 0 = equivalent to the index the library builds from `fasta` at the same k, 1 = different, 2 = undecided
    pub fn compare_with_fasta(&self, fasta: &str) -> Result<(i32, String), Error> {
        let (mut mine, mut theirs) = (std::ptr::null_mut(), std::ptr::null_mut());
        check(unsafe { pa_host_index_from_flat(&self.view(), &mut mine) })?;
        let p = CString::new(fasta)?;
        check(unsafe { pa_host_index_build_fasta(p.as_ptr(), self.k, 0, &mut theirs) })?;
        let mut report = vec![0u8; 512];
        let rc = unsafe { pa_host_index_compare(mine, theirs, 1 << 28, report.as_mut_ptr() as *mut _, report.len()) };
        unsafe { pa_host_index_destroy(mine); pa_host_index_destroy(theirs); }
        let text = CStr::from_bytes_until_nul(&report).map(|c| c.to_string_lossy().into_owned()).unwrap_or_default();
        check(rc).map(|rc| (rc, text))
    }
}

pub struct AmdIndex { raw: *mut PaIndex, max_class_len: usize }
unsafe impl Send for AmdIndex {}
unsafe impl Sync for AmdIndex {}

impl AmdIndex {
    pub fn from_pseudoaligner<K: Kmer>(al: &Pseudoaligner<K>, device: i32) -> Result<AmdIndex, Error> {
        let flat = FlatArrays::from_pseudoaligner(al);
        let mut raw = std::ptr::null_mut();
        check(unsafe { pa_index_create(&flat.view(), device, &mut raw) })?;   // arrays are only borrowed during the call
        let mut stats = PaIndexStats::default();
        if let Err(e) = check(unsafe { pa_index_get_stats(raw, &mut stats) }) { unsafe { pa_index_destroy(raw) }; return Err(e); }
        Ok(AmdIndex { raw, max_class_len: stats.max_class_len as usize })
    }

    /// map_read_with_mismatch (src/pseudoaligner.rs:361) on the read as the caller holds it: the DnaString's bases go over as
    /// 2-bit words (LSB-first, packed here through `Mer::get`, so nothing depends on the crate's storage order)
    pub fn map_read_with_mismatch(&self, read_seq: &DnaString, allowed_mismatches: usize) -> Result<Option<(Vec<u32>, usize, usize)>, Error> {
        let len = read_seq.len();
        let mut words = vec![0u64; (len + 31) / 32 + 1];
        for i in 0..len { words[i / 32] |= (read_seq.get(i) as u64) << (2 * (i % 32)); }
        // a read's class is an intersection of index classes: never longer than the longest of them
        let mut class = vec![0u32; self.max_class_len.max(1)];
        let (mut n, mut cov, mut mm) = (0u32, 0u32, 0u32);
        let rc = check(unsafe { pa_map_read_packed(self.raw, words.as_ptr(), len as u32, PA_PACKED_LSB_FIRST, allowed_mismatches as u32,
                                                   class.as_mut_ptr(), class.len() as u32, &mut n, &mut cov, &mut mm) })?;
        if rc == 0 { return Ok(None); }
        class.truncate(n as usize);
        Ok(Some((class, cov as usize, mm as usize)))
    }
}
impl Drop for AmdIndex { fn drop(&mut self) { unsafe { pa_index_destroy(self.raw) } } }

/// Orientation of a read pair on the (stranded) index: which mate is reverse-complemented before it is mapped.
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub enum PairOrientation { Fr, Rf, Ff }

/// map_read_with_mismatch for read PAIRS (`pa_map_pairs`): every mate oriented and mapped, the two classes intersected
/// (src/pseudoaligner.rs:389); a pair with one mapped mate takes that mate's result. `None` = neither mate mapped.
pub fn map_pairs(index: &AmdIndex, mates1: &[&[u8]], mates2: &[&[u8]], orient: PairOrientation, allowed_mismatches: usize)
                 -> Result<Vec<Option<(Vec<u32>, usize, usize)>>, Error> {
    use crate::amd_pairs_ffi::*;
    if mates1.len() != mates2.len() { return Err(anyhow!("{} first mates, {} second mates", mates1.len(), mates2.len())); }
    let n = mates1.len();
    let pack = |m: &[&[u8]]| { let mut text = Vec::new(); let mut off = vec![0u64]; for r in m { text.extend_from_slice(r); off.push(text.len() as u64); } (text, off) };
    let ((t1, o1), (t2, o2)) = (pack(mates1), pack(mates2));
    let mut res = vec![PaReadResult::default(); n];
    let mut coff = vec![0u64; n + 1];
    let mut ids: *const u32 = std::ptr::null();
    let o = match orient { PairOrientation::Fr => PA_PAIR_FR, PairOrientation::Rf => PA_PAIR_RF, PairOrientation::Ff => PA_PAIR_FF };
    check(unsafe { pa_map_pairs(index.raw, t1.as_ptr(), o1.as_ptr(), t2.as_ptr(), o2.as_ptr(), n as u64, o, allowed_mismatches as u32, res.as_mut_ptr(), coff.as_mut_ptr(), &mut ids) })?;
    let all = if coff[n] == 0 { &[][..] } else { unsafe { std::slice::from_raw_parts(ids, coff[n] as usize) } };   // library-owned until this thread's next call
    Ok((0..n).map(|i| if res[i].mismatches & PA_MAPPED_BIT == 0 { None } else {
        Some((all[coff[i] as usize..coff[i + 1] as usize].to_vec(), res[i].coverage as usize, (res[i].mismatches & !PA_MAPPED_BIT) as usize))
    }).collect())
}

/// The class-count table of a paired-end run from its two FASTQ files (`pa_count_pairs`): (table of `pa_counts_len` entries, pairs, stats).
/// An overflow table attached to the index receives the novel results; table + overflow are what `quantify` takes.
pub fn count_pairs<P: AsRef<Path>>(index: &AmdIndex, r1_fastq: P, r2_fastq: P, orient: PairOrientation, allowed_mismatches: usize, threads: usize)
                                   -> Result<(Vec<u64>, u64, [u64; 8]), Error> {
    use crate::amd_pairs_ffi::*;
    let p1 = CString::new(r1_fastq.as_ref().to_string_lossy().as_bytes())?;
    let p2 = CString::new(r2_fastq.as_ref().to_string_lossy().as_bytes())?;
    let mut counts = vec![0u64; unsafe { pa_counts_len(index.raw) } as usize];
    let (mut n, mut stats) = (0u64, [0u64; 8]);
    let o = match orient { PairOrientation::Fr => PA_PAIR_FR, PairOrientation::Rf => PA_PAIR_RF, PairOrientation::Ff => PA_PAIR_FF };
    check(unsafe { pa_count_pairs(index.raw, p1.as_ptr(), p2.as_ptr(), o, allowed_mismatches as u32, threads as i32, counts.as_mut_ptr(), &mut n, stats.as_mut_ptr()) })?;
    Ok((counts, n, stats))
}

/// Which strand of a single read is mapped on the (stranded) index; `Both`: an unstranded library, the two answers merged.
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub enum Strand { Fwd, Rev, Both }

fn results_to_options(res: &[PaReadResult], coff: &[u64], ids: *const u32) -> Vec<Option<(Vec<u32>, usize, usize)>> {
    let n = res.len();
    let all = if coff[n] == 0 { &[][..] } else { unsafe { std::slice::from_raw_parts(ids, coff[n] as usize) } };   // library-owned until this thread's next call
    (0..n).map(|i| if res[i].mismatches & PA_MAPPED_BIT == 0 { None } else {
        Some((all[coff[i] as usize..coff[i + 1] as usize].to_vec(), res[i].coverage as usize, (res[i].mismatches & !PA_MAPPED_BIT) as usize))
    }).collect()
}

/// map_read_with_mismatch for a batch of reads on a chosen strand (`pa_map_batch_strand`). `Strand::Both` maps the read and its reverse
/// complement and merges the two answers by the rule of unstranded libraries (include/pseudoaligner_amd.h): the better one, or on a tie
/// the union of the two classes.
pub fn map_reads_strand(index: &AmdIndex, reads: &[&[u8]], strand: Strand, allowed_mismatches: usize) -> Result<Vec<Option<(Vec<u32>, usize, usize)>>, Error> {
    use crate::amd_strands_ffi::*;
    let n = reads.len();
    let (mut text, mut off) = (Vec::new(), vec![0u64]);
    for r in reads { text.extend_from_slice(r); off.push(text.len() as u64); }
    let mut res = vec![PaReadResult::default(); n];
    let mut coff = vec![0u64; n + 1];
    let mut ids: *const u32 = std::ptr::null();
    let s = match strand { Strand::Fwd => PA_STRAND_FWD, Strand::Rev => PA_STRAND_REV, Strand::Both => PA_STRAND_BOTH };
    check(unsafe { pa_map_batch_strand(index.raw, text.as_ptr(), off.as_ptr(), n as u64, s, allowed_mismatches as u32, res.as_mut_ptr(), coff.as_mut_ptr(), &mut ids) })?;
    Ok(results_to_options(&res, &coff, ids))
}

/// `map_pairs` for an UNSTRANDED library (`pa_map_pairs_unstranded`): every pair is mapped as `Fr` and as `Rf` and the two answers are merged.
pub fn map_pairs_unstranded(index: &AmdIndex, mates1: &[&[u8]], mates2: &[&[u8]], allowed_mismatches: usize) -> Result<Vec<Option<(Vec<u32>, usize, usize)>>, Error> {
    use crate::amd_strands_ffi::*;
    if mates1.len() != mates2.len() { return Err(anyhow!("{} first mates, {} second mates", mates1.len(), mates2.len())); }
    let n = mates1.len();
    let pack = |m: &[&[u8]]| { let mut text = Vec::new(); let mut off = vec![0u64]; for r in m { text.extend_from_slice(r); off.push(text.len() as u64); } (text, off) };
    let ((t1, o1), (t2, o2)) = (pack(mates1), pack(mates2));
    let mut res = vec![PaReadResult::default(); n];
    let mut coff = vec![0u64; n + 1];
    let mut ids: *const u32 = std::ptr::null();
    check(unsafe { pa_map_pairs_unstranded(index.raw, t1.as_ptr(), o1.as_ptr(), t2.as_ptr(), o2.as_ptr(), n as u64, allowed_mismatches as u32, res.as_mut_ptr(), coff.as_mut_ptr(), &mut ids) })?;
    Ok(results_to_options(&res, &coff, ids))
}

/// `count_pairs` for an UNSTRANDED library (`pa_count_pairs_unstranded`): (table, pairs, stats). stats: [0] pairs, [1] both candidates mapped,
/// [2] sense only, [3] antisense only, [4] neither, [5] ties, [6] by reference, [7] in the arena; [2] far above [3] (or the reverse) says
/// that the library is stranded after all.
pub fn count_pairs_unstranded<P: AsRef<Path>>(index: &AmdIndex, r1_fastq: P, r2_fastq: P, allowed_mismatches: usize, threads: usize)
                                              -> Result<(Vec<u64>, u64, [u64; 8]), Error> {
    use crate::amd_strands_ffi::*;
    let p1 = CString::new(r1_fastq.as_ref().to_string_lossy().as_bytes())?;
    let p2 = CString::new(r2_fastq.as_ref().to_string_lossy().as_bytes())?;
    let mut counts = vec![0u64; unsafe { pa_counts_len(index.raw) } as usize];
    let (mut n, mut stats) = (0u64, [0u64; 8]);
    check(unsafe { pa_count_pairs_unstranded(index.raw, p1.as_ptr(), p2.as_ptr(), allowed_mismatches as u32, threads as i32, counts.as_mut_ptr(), &mut n, stats.as_mut_ptr()) })?;
    Ok((counts, n, stats))
}

/// The member table of a BGZF file (`pa_bgzf_scan`): one row per member and the bytes of text the file holds; `None` when the bytes are
/// not BGZF from first to last (ordinary gzip, a truncated member). The rows are what `pa_bgzf_inflate_device` takes, copied to the GPU.
pub fn bgzf_members(data: &[u8]) -> Result<Option<(Vec<crate::amd_bgzf_ffi::PaBgzfMember>, u64)>, Error> {
    use crate::amd_bgzf_ffi::*;
    let (mut n, mut text) = (0u64, 0u64);
    let rc = unsafe { pa_bgzf_scan(data.as_ptr(), data.len() as u64, std::ptr::null_mut(), 0, &mut n, &mut text) };
    if rc == PA_ERR_NOT_BGZF { return Ok(None); }
    check(rc)?;
    let mut rows = vec![PaBgzfMember::default(); n as usize];
    check(unsafe { pa_bgzf_scan(data.as_ptr(), data.len() as u64, rows.as_mut_ptr(), n, &mut n, &mut text) })?;
    Ok(Some((rows, text)))
}

/// What this thread's last `process_reads_path` read (`pa_process_reads_input_stats`): [text_kind, members_total, members_gpu, members_host, bytes_h2d, text_bytes_gpu]
pub fn process_reads_input_stats() -> Result<[u64; 6], Error> {
    let mut st = [0u64; 6];
    check(unsafe { crate::amd_bgzf_ffi::pa_process_reads_input_stats(st.as_mut_ptr()) })?;
    Ok(st)
}

/// What this thread's last paired call (`count_pairs_path` and the cells / BUS drivers) read: ([R1's input stats], [R2's], device path taken),
/// the stats in `process_reads_input_stats`' meaning (`pa_pairs_input_stats`, `pa_pairs_input_path`).
pub fn pairs_input_stats() -> Result<([u64; 6], [u64; 6], bool), Error> {
    let mut st = [0u64; 12];
    check(unsafe { crate::amd_pairscan_ffi::pa_pairs_input_stats(st.as_mut_ptr()) })?;
    let (mut r1, mut r2) = ([0u64; 6], [0u64; 6]);
    r1.copy_from_slice(&st[..6]);
    r2.copy_from_slice(&st[6..]);
    Ok((r1, r2, unsafe { crate::amd_pairscan_ffi::pa_pairs_input_path() } == 1))
}

/// Device buffers of one segment of a batch of pairs for `pairs_gather_segment` (`pa_pairs_gather_device`): raw device pointers and sizes, as the header names them.
pub struct PairSegment {
    pub d_text1: *const u8, pub text1_bytes: u64, pub d_rec1: *const u32,
    pub d_text2: *const u8, pub text2_bytes: u64, pub d_rec2: *const u32,
    pub m: u64, pub prefix: u32, pub base: u64,
    pub d_bytes1: *mut u8, pub cap1: u64, pub d_off1: *mut u64,
    pub d_bytes2: *mut u8, pub cap2: u64, pub d_off2: *mut u64,
    pub d_ctl: *mut u64, pub d_scratch: *mut std::ffi::c_void, pub scratch_bytes: usize,
}

/// The ids of `m` pairs compared and their R1 prefixes and R2 sequences gathered on GPU `device`, asynchronous on `stream`; `base == 0` opens a batch.
/// # Safety
/// Every pointer of `seg` is a device pointer that is valid for the sizes the header gives.
pub unsafe fn pairs_gather_segment(device: i32, seg: &PairSegment, stream: *mut std::ffi::c_void) -> Result<(), Error> {
    use crate::amd_pairscan_ffi::pa_pairs_gather_device;
    check(pa_pairs_gather_device(device, seg.d_text1, seg.text1_bytes, seg.d_rec1, seg.d_text2, seg.text2_bytes, seg.d_rec2, seg.m, seg.prefix, seg.base,
                                 seg.d_bytes1, seg.cap1, seg.d_off1, seg.d_bytes2, seg.cap2, seg.d_off2, seg.d_ctl, seg.d_scratch, seg.scratch_bytes, stream))
}

/// One replica of the index per GPU (`pa_index_create_multi`): what `process_reads_path` deals its windows of text to.
pub struct AmdIndexSet { raw: Vec<*mut PaIndex> }
unsafe impl Send for AmdIndexSet {}
unsafe impl Sync for AmdIndexSet {}
impl AmdIndexSet {
    pub fn from_pseudoaligner<K: Kmer>(al: &Pseudoaligner<K>, devices: &[i32]) -> Result<AmdIndexSet, Error> {
        let flat = FlatArrays::from_pseudoaligner(al);
        let mut raw = vec![std::ptr::null_mut(); devices.len()];
        check(unsafe { pa_index_create_multi(&flat.view(), devices.as_ptr(), devices.len() as i32, raw.as_mut_ptr()) })?;   // all or nothing
        Ok(AmdIndexSet { raw })
    }
}
impl Drop for AmdIndexSet { fn drop(&mut self) { for r in &self.raw { unsafe { pa_index_destroy(*r) } } } }

/// the GPUs to use: `PSEUDOALIGNER_AMD_DEVICES=0,1,2,3` (default: every GPU the process sees)
fn devices_of_env() -> Vec<i32> {
    if let Ok(v) = std::env::var("PSEUDOALIGNER_AMD_DEVICES") {
        let d: Vec<i32> = v.split(',').filter_map(|x| x.trim().parse().ok()).collect();
        if !d.is_empty() { return d; }
    }
    (0..unsafe { pa_device_count() }.max(1)).collect()
}

/// `process_reads` for a caller that has the PATH of the FASTQ file — the CLI does (`fastq::Reader::from_file(args.arg_reads_fastq)`,
/// src/bin/pseudoaligner.rs:139): the file never passes through `bio`'s reader. The library reads windows of it into pinned memory,
/// the GPUs find the records and map them (pa_process_reads_multi: one lane per GPU, tuples on stdout in input order), 150 M reads/s
/// per GPU from text in the page cache — against a few M records/s for ANY loop over `fastq::Reader::records()` on one thread, which
/// is what bounds the reader-fed `process_reads` below whatever runs behind it.
pub fn process_reads_path<K: Kmer + Sync + Send, P: AsRef<Path> + Debug, Q: AsRef<Path>>(
    reads_fastq: Q,
    index: &Pseudoaligner<K>,
    outdir: P,
    num_threads: usize,
) -> Result<(), Error> {
    info!("Done Reading index");
    info!("Starting Multi-threaded Mapping");
    info!("Output directory: {:?}", outdir);
    let set = AmdIndexSet::from_pseudoaligner(index, &devices_of_env())?;
    io::stdout().flush()?;                                            // (the library writes to the process's stdout through C stdio)
    let path = CString::new(reads_fastq.as_ref().to_string_lossy().into_owned())?;
    let dash = CString::new("-")?;
    let (mut n_reads, mut n_flagged) = (0u64, 0u64);
    // the progress line of :497-503 (exactly every 10^6-th read, f32 Display) and the `eprintln!()` behind it come from the library
    check(unsafe { pa_process_reads_multi(set.raw.as_ptr(), set.raw.len() as i32, path.as_ptr(), dash.as_ptr(), num_threads as i32,
                                          &mut n_reads, &mut n_flagged) })?;
    info!("Done Mapping Reads");
    info!("Mapped {} reads, {} flagged", n_reads, n_flagged);
    Ok(())
}

/// Single-cell UMI counts from files (pa_count_cells): a 10x run's R1 (cell barcode + UMI) and R2 (cDNA) FASTQ and its barcode
/// whitelist -> `out_dir`/matrix.mtx, barcodes.tsv, features.tsv. `index_file`: the index as `pa_host_index_save` wrote it (it keeps the
/// transcript -> gene names the matrix rows need; the reference's `Pseudoaligner` does too, but the flat interchange does not carry them).
/// 10x v3: bc_len 16, umi_len 12; v2: 16, 10. Returns the ten counters of PA_CELL_STATS.
pub fn count_cells<P: AsRef<Path>>(index_file: P, r1_fastq: P, r2_fastq: P, whitelist: P, out_dir: P, bc_len: u32, umi_len: u32,
                                   num_threads: usize, device: i32) -> Result<[u64; PA_CELL_STATS], Error> {
    let cstr = |p: &P| CString::new(p.as_ref().to_string_lossy().into_owned());
    let (ix, r1, r2, wl, out) = (cstr(&index_file)?, cstr(&r1_fastq)?, cstr(&r2_fastq)?, cstr(&whitelist)?, cstr(&out_dir)?);
    let mut h = std::ptr::null_mut();
    check(unsafe { pa_host_index_load(ix.as_ptr(), &mut h) })?;
    let mut view: PaFlatIndex = unsafe { std::mem::zeroed() };
    let mut idx = std::ptr::null_mut();
    let mut rc = unsafe { pa_host_index_view(h, &mut view) };
    if rc >= 0 { rc = unsafe { pa_index_create(&view, device, &mut idx) }; }
    let mut stats = [0u64; PA_CELL_STATS];
    if rc >= 0 {
        rc = unsafe { pa_count_cells(idx, h, r1.as_ptr(), r2.as_ptr(), wl.as_ptr(), bc_len, umi_len, out.as_ptr(), num_threads as i32, stats.as_mut_ptr()) };
    }
    let result = check(rc).map(|_| stats);   // (the message is read before the handles go)
    unsafe {
        if !idx.is_null() { pa_index_destroy(idx); }
        pa_host_index_destroy(h);
    }
    result
}

/// BUS output from files (pa_write_bus): the same R1 / R2 FASTQ pair -> `out_dir`/output.bus (sorted, collapsed BUS v1 records of
/// (barcode, UMI, equivalence class)), matrix.ec and transcripts.txt, the input of `bustools` and the tools behind it. No whitelist and
/// no correction here (that is `bustools correct`); a read with an N in its barcode or UMI is dropped and counted. bc_len + umi_len <= 32.
/// Returns the eight counters of PA_BUS_STATS: reads, r1_short, barcode_n, umi_n, unmapped, bad_class, recorded, records.
pub fn write_bus<P: AsRef<Path>>(index_file: P, r1_fastq: P, r2_fastq: P, out_dir: P, bc_len: u32, umi_len: u32, num_threads: usize,
                                 device: i32) -> Result<[u64; crate::amd_bus_ffi::PA_BUS_STATS], Error> {
    use crate::amd_bus_ffi::*;
    let cstr = |p: &P| CString::new(p.as_ref().to_string_lossy().into_owned());
    let (ix, r1, r2, out) = (cstr(&index_file)?, cstr(&r1_fastq)?, cstr(&r2_fastq)?, cstr(&out_dir)?);
    let mut h = std::ptr::null_mut();
    check(unsafe { pa_host_index_load(ix.as_ptr(), &mut h) })?;
    let mut view: PaFlatIndex = unsafe { std::mem::zeroed() };
    let mut idx = std::ptr::null_mut();
    let mut rc = unsafe { pa_host_index_view(h, &mut view) };
    if rc >= 0 { rc = unsafe { pa_index_create(&view, device, &mut idx) }; }
    let mut stats = [0u64; PA_BUS_STATS];
    if rc >= 0 {
        rc = unsafe { pa_write_bus(idx, h, r1.as_ptr(), r2.as_ptr(), bc_len, umi_len, out.as_ptr(), num_threads as i32, stats.as_mut_ptr()) };
    }
    let result = check(rc).map(|_| stats);   // (the message is read before the handles go)
    unsafe {
        if !idx.is_null() { pa_index_destroy(idx); }
        pa_host_index_destroy(h);
    }
    result
}

/// Cells x genes with fractional counts from files (pa_count_cells_em): `write_bus`'s records, never written, then per cell the
/// molecules whose records agree on one gene counted for it and the others shared out by an EM (the `bustools count --genecounts --em`
/// step) -> `out_dir`/matrix.mtx (real values), barcodes.tsv, features.tsv. No whitelist and no correction. `params`: None = the
/// library's defaults (pa_quant_default_params', not tuned for single-cell data). Returns the sixteen counters of PA_GENES_STATS.
pub fn count_cells_em<P: AsRef<Path>>(index_file: P, r1_fastq: P, r2_fastq: P, out_dir: P, bc_len: u32, umi_len: u32,
                                      params: Option<crate::amd_genes_ffi::PaGenesParams>, num_threads: usize,
                                      device: i32) -> Result<[u64; crate::amd_genes_ffi::PA_GENES_STATS], Error> {
    use crate::amd_genes_ffi::*;
    let cstr = |p: &P| CString::new(p.as_ref().to_string_lossy().into_owned());
    let (ix, r1, r2, out) = (cstr(&index_file)?, cstr(&r1_fastq)?, cstr(&r2_fastq)?, cstr(&out_dir)?);
    let mut h = std::ptr::null_mut();
    check(unsafe { pa_host_index_load(ix.as_ptr(), &mut h) })?;
    let mut view: PaFlatIndex = unsafe { std::mem::zeroed() };
    let mut idx = std::ptr::null_mut();
    let mut rc = unsafe { pa_host_index_view(h, &mut view) };
    if rc >= 0 { rc = unsafe { pa_index_create(&view, device, &mut idx) }; }
    let mut stats = [0u64; PA_GENES_STATS];
    if rc >= 0 {
        let p = params.as_ref().map_or(std::ptr::null(), |p| p as *const PaGenesParams);
        rc = unsafe { pa_count_cells_em(idx, h, r1.as_ptr(), r2.as_ptr(), bc_len, umi_len, p, out.as_ptr(), num_threads as i32, stats.as_mut_ptr()) };
    }
    let result = check(rc).map(|_| stats);   // (the message is read before the handles go)
    unsafe {
        if !idx.is_null() { pa_index_destroy(idx); }
        pa_host_index_destroy(h);
    }
    result
}

/// `write_bus` with the barcodes corrected against a whitelist file on the GPU before the files are written (pa_write_bus_corrected): a
/// barcode stays when it is whitelisted, moves to the one whitelisted barcode a single substitution away, and is dropped with its records
/// otherwise; records that meet are joined. bc_len <= 16. Returns (PA_BUS_STATS, PA_BUS_CORRECT_STATS).
pub fn write_bus_corrected<P: AsRef<Path>>(index_file: P, r1_fastq: P, r2_fastq: P, whitelist: P, out_dir: P, bc_len: u32, umi_len: u32, num_threads: usize,
                                           device: i32) -> Result<([u64; crate::amd_bus_ffi::PA_BUS_STATS], [u64; crate::amd_correct_ffi::PA_BUS_CORRECT_STATS]), Error> {
    use crate::amd_bus_ffi::*;
    use crate::amd_correct_ffi::*;
    let cstr = |p: &P| CString::new(p.as_ref().to_string_lossy().into_owned());
    let (ix, r1, r2, wl, out) = (cstr(&index_file)?, cstr(&r1_fastq)?, cstr(&r2_fastq)?, cstr(&whitelist)?, cstr(&out_dir)?);
    let mut h = std::ptr::null_mut();
    check(unsafe { pa_host_index_load(ix.as_ptr(), &mut h) })?;
    let mut view: PaFlatIndex = unsafe { std::mem::zeroed() };
    let mut idx = std::ptr::null_mut();
    let mut rc = unsafe { pa_host_index_view(h, &mut view) };
    if rc >= 0 { rc = unsafe { pa_index_create(&view, device, &mut idx) }; }
    let (mut stats, mut cstats) = ([0u64; PA_BUS_STATS], [0u64; PA_BUS_CORRECT_STATS]);
    if rc >= 0 {
        rc = unsafe { pa_write_bus_corrected(idx, h, r1.as_ptr(), r2.as_ptr(), wl.as_ptr(), bc_len, umi_len, out.as_ptr(), num_threads as i32, stats.as_mut_ptr(),
                                             cstats.as_mut_ptr()) };
    }
    let result = check(rc).map(|_| (stats, cstats));   // (the message is read before the handles go)
    unsafe {
        if !idx.is_null() { pa_index_destroy(idx); }
        pa_host_index_destroy(h);
    }
    result
}

/// `count_cells_em` with the barcodes corrected against a whitelist file between the BUS records and the gene stage
/// (pa_count_cells_em_corrected; `write_bus_corrected`'s rule). Returns (PA_GENES_STATS, PA_BUS_CORRECT_STATS).
pub fn count_cells_em_corrected<P: AsRef<Path>>(index_file: P, r1_fastq: P, r2_fastq: P, whitelist: P, out_dir: P, bc_len: u32, umi_len: u32,
                                                params: Option<crate::amd_genes_ffi::PaGenesParams>, num_threads: usize,
                                                device: i32) -> Result<([u64; crate::amd_genes_ffi::PA_GENES_STATS], [u64; crate::amd_correct_ffi::PA_BUS_CORRECT_STATS]), Error> {
    use crate::amd_correct_ffi::*;
    use crate::amd_genes_ffi::*;
    let cstr = |p: &P| CString::new(p.as_ref().to_string_lossy().into_owned());
    let (ix, r1, r2, wl, out) = (cstr(&index_file)?, cstr(&r1_fastq)?, cstr(&r2_fastq)?, cstr(&whitelist)?, cstr(&out_dir)?);
    let mut h = std::ptr::null_mut();
    check(unsafe { pa_host_index_load(ix.as_ptr(), &mut h) })?;
    let mut view: PaFlatIndex = unsafe { std::mem::zeroed() };
    let mut idx = std::ptr::null_mut();
    let mut rc = unsafe { pa_host_index_view(h, &mut view) };
    if rc >= 0 { rc = unsafe { pa_index_create(&view, device, &mut idx) }; }
    let (mut stats, mut cstats) = ([0u64; PA_GENES_STATS], [0u64; PA_BUS_CORRECT_STATS]);
    if rc >= 0 {
        let p = params.as_ref().map_or(std::ptr::null(), |p| p as *const PaGenesParams);
        rc = unsafe { pa_count_cells_em_corrected(idx, h, r1.as_ptr(), r2.as_ptr(), wl.as_ptr(), bc_len, umi_len, p, out.as_ptr(), num_threads as i32,
                                                  stats.as_mut_ptr(), cstats.as_mut_ptr()) };
    }
    let result = check(rc).map(|_| (stats, cstats));   // (the message is read before the handles go)
    unsafe {
        if !idx.is_null() { pa_index_destroy(idx); }
        pa_host_index_destroy(h);
    }
    result
}

/// Cell calling on BUS records that lie on the host (pa_bus_knee_records; an output.bus read back, for instance): the barcode table ranked by
/// molecules and the barcodes the threshold rule calls, on GPU `device` of the index in `index_file`. `params`: None = the library's
/// defaults (curve knee, lower 10, divisor 10). Returns (rows in ascending barcode order, the called barcodes packed and ascending,
/// PA_KNEE_STATS); the called list can go to pa_bus_correct / pa_bus_keep as it is.
pub fn bus_knee<P: AsRef<Path>>(index_file: P, records: &[crate::amd_bus_ffi::PaBusRecord], bc_len: u32, umi_len: u32,
                                params: Option<crate::amd_knee_ffi::PaKneeParams>,
                                device: i32) -> Result<(Vec<crate::amd_knee_ffi::PaBusBarcodeRow>, Vec<u64>, [u64; crate::amd_knee_ffi::PA_KNEE_STATS]), Error> {
    use crate::amd_knee_ffi::*;
    let ix = CString::new(index_file.as_ref().to_string_lossy().into_owned())?;
    let mut h = std::ptr::null_mut();
    check(unsafe { pa_host_index_load(ix.as_ptr(), &mut h) })?;
    let mut view: PaFlatIndex = unsafe { std::mem::zeroed() };
    let mut idx = std::ptr::null_mut();
    let mut rc = unsafe { pa_host_index_view(h, &mut view) };
    if rc >= 0 { rc = unsafe { pa_index_create(&view, device, &mut idx) }; }
    let mut stats = [0u64; PA_KNEE_STATS];
    let (mut rows, mut called) = (Vec::<PaBusBarcodeRow>::new(), Vec::<u64>::new());
    if rc >= 0 {
        let p = params.as_ref().map_or(std::ptr::null(), |p| p as *const PaKneeParams);
        let (mut n_rows, mut n_called) = (0u64, 0u64);
        // the sizes first, then the arrays
        rc = unsafe { pa_bus_knee_records(idx, records.as_ptr(), records.len() as u64, bc_len, umi_len, p, std::ptr::null_mut(), 0, &mut n_rows,
                                          std::ptr::null_mut(), 0, &mut n_called, stats.as_mut_ptr()) };
        if rc >= 0 {
            rows.resize(n_rows as usize, PaBusBarcodeRow::default());
            called.resize(n_called as usize, 0);
            rc = unsafe { pa_bus_knee_records(idx, records.as_ptr(), records.len() as u64, bc_len, umi_len, p, rows.as_mut_ptr(), n_rows, &mut n_rows,
                                              called.as_mut_ptr(), n_called, &mut n_called, stats.as_mut_ptr()) };
        }
    }
    let result = check(rc).map(|_| (rows, called, stats));   // (the message is read before the handles go)
    unsafe {
        if !idx.is_null() { pa_index_destroy(idx); }
        pa_host_index_destroy(h);
    }
    result
}

/// `write_bus` with cells called on the GPU before the files are written (pa_write_bus_called). `whitelist` None: the called barcodes are
/// the whitelist of the correction (`bustools whitelist` + `correct`); Some(file): the barcodes are corrected against it, then the records
/// of uncalled barcodes are dropped. Also writes `out_dir`/barcode_ranks.tsv. Returns (PA_BUS_STATS, PA_BUS_CORRECT_STATS, PA_KNEE_STATS).
pub fn write_bus_called<P: AsRef<Path>>(index_file: P, r1_fastq: P, r2_fastq: P, whitelist: Option<P>, out_dir: P, bc_len: u32, umi_len: u32,
                                        knee: Option<crate::amd_knee_ffi::PaKneeParams>, num_threads: usize,
                                        device: i32) -> Result<([u64; crate::amd_bus_ffi::PA_BUS_STATS], [u64; crate::amd_correct_ffi::PA_BUS_CORRECT_STATS],
                                                                [u64; crate::amd_knee_ffi::PA_KNEE_STATS]), Error> {
    use crate::amd_bus_ffi::*;
    use crate::amd_correct_ffi::*;
    use crate::amd_knee_ffi::*;
    let cstr = |p: &P| CString::new(p.as_ref().to_string_lossy().into_owned());
    let (ix, r1, r2, out) = (cstr(&index_file)?, cstr(&r1_fastq)?, cstr(&r2_fastq)?, cstr(&out_dir)?);
    let wl = match whitelist.as_ref() { Some(w) => Some(cstr(w)?), None => None };
    let mut h = std::ptr::null_mut();
    check(unsafe { pa_host_index_load(ix.as_ptr(), &mut h) })?;
    let mut view: PaFlatIndex = unsafe { std::mem::zeroed() };
    let mut idx = std::ptr::null_mut();
    let mut rc = unsafe { pa_host_index_view(h, &mut view) };
    if rc >= 0 { rc = unsafe { pa_index_create(&view, device, &mut idx) }; }
    let (mut stats, mut cstats, mut kstats) = ([0u64; PA_BUS_STATS], [0u64; PA_BUS_CORRECT_STATS], [0u64; PA_KNEE_STATS]);
    if rc >= 0 {
        let kp = knee.as_ref().map_or(std::ptr::null(), |p| p as *const PaKneeParams);
        let wlp = wl.as_ref().map_or(std::ptr::null(), |w| w.as_ptr());
        rc = unsafe { pa_write_bus_called(idx, h, r1.as_ptr(), r2.as_ptr(), wlp, bc_len, umi_len, kp, out.as_ptr(), num_threads as i32, stats.as_mut_ptr(),
                                          cstats.as_mut_ptr(), kstats.as_mut_ptr()) };
    }
    let result = check(rc).map(|_| (stats, cstats, kstats));   // (the message is read before the handles go)
    unsafe {
        if !idx.is_null() { pa_index_destroy(idx); }
        pa_host_index_destroy(h);
    }
    result
}

/// `count_cells_em` with cells called between the BUS records and the gene stage (pa_count_cells_em_called; `write_bus_called`'s rules): the
/// matrix is the filtered one. Returns (PA_GENES_STATS, PA_BUS_CORRECT_STATS, PA_KNEE_STATS).
pub fn count_cells_em_called<P: AsRef<Path>>(index_file: P, r1_fastq: P, r2_fastq: P, whitelist: Option<P>, out_dir: P, bc_len: u32, umi_len: u32,
                                             knee: Option<crate::amd_knee_ffi::PaKneeParams>, params: Option<crate::amd_genes_ffi::PaGenesParams>,
                                             num_threads: usize,
                                             device: i32) -> Result<([u64; crate::amd_genes_ffi::PA_GENES_STATS], [u64; crate::amd_correct_ffi::PA_BUS_CORRECT_STATS],
                                                                     [u64; crate::amd_knee_ffi::PA_KNEE_STATS]), Error> {
    use crate::amd_correct_ffi::*;
    use crate::amd_genes_ffi::*;
    use crate::amd_knee_ffi::*;
    let cstr = |p: &P| CString::new(p.as_ref().to_string_lossy().into_owned());
    let (ix, r1, r2, out) = (cstr(&index_file)?, cstr(&r1_fastq)?, cstr(&r2_fastq)?, cstr(&out_dir)?);
    let wl = match whitelist.as_ref() { Some(w) => Some(cstr(w)?), None => None };
    let mut h = std::ptr::null_mut();
    check(unsafe { pa_host_index_load(ix.as_ptr(), &mut h) })?;
    let mut view: PaFlatIndex = unsafe { std::mem::zeroed() };
    let mut idx = std::ptr::null_mut();
    let mut rc = unsafe { pa_host_index_view(h, &mut view) };
    if rc >= 0 { rc = unsafe { pa_index_create(&view, device, &mut idx) }; }
    let (mut stats, mut cstats, mut kstats) = ([0u64; PA_GENES_STATS], [0u64; PA_BUS_CORRECT_STATS], [0u64; PA_KNEE_STATS]);
    if rc >= 0 {
        let kp = knee.as_ref().map_or(std::ptr::null(), |p| p as *const PaKneeParams);
        let p = params.as_ref().map_or(std::ptr::null(), |p| p as *const PaGenesParams);
        let wlp = wl.as_ref().map_or(std::ptr::null(), |w| w.as_ptr());
        rc = unsafe { pa_count_cells_em_called(idx, h, r1.as_ptr(), r2.as_ptr(), wlp, bc_len, umi_len, kp, p, out.as_ptr(), num_threads as i32,
                                               stats.as_mut_ptr(), cstats.as_mut_ptr(), kstats.as_mut_ptr()) };
    }
    let result = check(rc).map(|_| (stats, cstats, kstats));   // (the message is read before the handles go)
    unsafe {
        if !idx.is_null() { pa_index_destroy(idx); }
        pa_host_index_destroy(h);
    }
    result
}

/// The UMI correction on host records (pa_bus_umi_correct_records): `records` strictly ascending by (barcode, UMI, ec), the ec table as a CSR,
/// `tx_gene[num_tx] < num_genes`, on the GPU of the index loaded from `index_file`. One step: a molecule moves to the best-supported molecule of
/// its barcode whose UMI is one substitution away and whose gene set meets its own (`mode`: PA_UMI_GREATEST or PA_UMI_DIRECTIONAL). Returns the
/// corrected records, collapsed and sorted again, and PA_BUS_UMI_STATS.
pub fn bus_umi_correct<P: AsRef<Path>>(index_file: P, records: &[crate::amd_bus_ffi::PaBusRecord], ec_offsets: &[u64], ec_ids: &[u32], tx_gene: &[u32],
                                       num_genes: u32, bc_len: u32, umi_len: u32, mode: u32,
                                       device: i32) -> Result<(Vec<crate::amd_bus_ffi::PaBusRecord>, [u64; crate::amd_umi_ffi::PA_BUS_UMI_STATS]), Error> {
    use crate::amd_umi_ffi::*;
    let ix = CString::new(index_file.as_ref().to_string_lossy().into_owned())?;
    let mut h = std::ptr::null_mut();
    check(unsafe { pa_host_index_load(ix.as_ptr(), &mut h) })?;
    let mut view: PaFlatIndex = unsafe { std::mem::zeroed() };
    let mut idx = std::ptr::null_mut();
    let mut rc = unsafe { pa_host_index_view(h, &mut view) };
    if rc >= 0 { rc = unsafe { pa_index_create(&view, device, &mut idx) }; }
    let mut out: Vec<crate::amd_bus_ffi::PaBusRecord> = Vec::with_capacity(records.len().max(1));
    let (mut n_out, mut stats) = (0u64, [0u64; PA_BUS_UMI_STATS]);
    if rc >= 0 {
        rc = unsafe { pa_bus_umi_correct_records(idx, records.as_ptr(), records.len() as u64, ec_offsets.as_ptr(), ec_ids.as_ptr(),
                                                 ec_offsets.len().saturating_sub(1) as u32, tx_gene.len() as u32, tx_gene.as_ptr(), num_genes, bc_len, umi_len, mode,
                                                 out.as_mut_ptr(), records.len() as u64, &mut n_out, stats.as_mut_ptr()) };
        if rc >= 0 { unsafe { out.set_len(n_out as usize); } }
    }
    let result = check(rc).map(|_| (out, stats));   // (the message is read before the handles go)
    unsafe {
        if !idx.is_null() { pa_index_destroy(idx); }
        pa_host_index_destroy(h);
    }
    result
}

/// `write_bus` with every record step as an option and the UMI correction behind them (pa_write_bus_umi): `whitelist` and `call_cells` run the
/// barcode steps exactly as `write_bus` / `write_bus_corrected` / `write_bus_called` run them for that pair, then the UMIs are corrected
/// (`umi_mode`), always last; barcode_ranks.tsv shows the molecule counts before that. Returns (PA_BUS_STATS, PA_BUS_CORRECT_STATS,
/// PA_KNEE_STATS, PA_BUS_UMI_STATS); the stats of a step that did not run stay 0.
pub fn write_bus_umi<P: AsRef<Path>>(index_file: P, r1_fastq: P, r2_fastq: P, whitelist: Option<P>, out_dir: P, bc_len: u32, umi_len: u32, call_cells: bool,
                                     knee: Option<crate::amd_knee_ffi::PaKneeParams>, umi_mode: u32, num_threads: usize,
                                     device: i32) -> Result<([u64; crate::amd_bus_ffi::PA_BUS_STATS], [u64; crate::amd_correct_ffi::PA_BUS_CORRECT_STATS],
                                                             [u64; crate::amd_knee_ffi::PA_KNEE_STATS], [u64; crate::amd_umi_ffi::PA_BUS_UMI_STATS]), Error> {
    use crate::amd_bus_ffi::*;
    use crate::amd_correct_ffi::*;
    use crate::amd_knee_ffi::*;
    use crate::amd_umi_ffi::*;
    let cstr = |p: &P| CString::new(p.as_ref().to_string_lossy().into_owned());
    let (ix, r1, r2, out) = (cstr(&index_file)?, cstr(&r1_fastq)?, cstr(&r2_fastq)?, cstr(&out_dir)?);
    let wl = match whitelist.as_ref() { Some(w) => Some(cstr(w)?), None => None };
    let mut h = std::ptr::null_mut();
    check(unsafe { pa_host_index_load(ix.as_ptr(), &mut h) })?;
    let mut view: PaFlatIndex = unsafe { std::mem::zeroed() };
    let mut idx = std::ptr::null_mut();
    let mut rc = unsafe { pa_host_index_view(h, &mut view) };
    if rc >= 0 { rc = unsafe { pa_index_create(&view, device, &mut idx) }; }
    let (mut stats, mut cstats, mut kstats, mut ustats) = ([0u64; PA_BUS_STATS], [0u64; PA_BUS_CORRECT_STATS], [0u64; PA_KNEE_STATS], [0u64; PA_BUS_UMI_STATS]);
    if rc >= 0 {
        let kp = knee.as_ref().map_or(std::ptr::null(), |p| p as *const PaKneeParams);
        let wlp = wl.as_ref().map_or(std::ptr::null(), |w| w.as_ptr());
        rc = unsafe { pa_write_bus_umi(idx, h, r1.as_ptr(), r2.as_ptr(), wlp, bc_len, umi_len, call_cells as i32, kp, umi_mode, out.as_ptr(), num_threads as i32,
                                       stats.as_mut_ptr(), cstats.as_mut_ptr(), kstats.as_mut_ptr(), ustats.as_mut_ptr()) };
    }
    let result = check(rc).map(|_| (stats, cstats, kstats, ustats));   // (the message is read before the handles go)
    unsafe {
        if !idx.is_null() { pa_index_destroy(idx); }
        pa_host_index_destroy(h);
    }
    result
}

/// `count_cells_em` with every record step as an option and the UMI correction between them and the gene stage (pa_count_cells_em_umi;
/// `write_bus_umi`'s rules). Returns (PA_GENES_STATS, PA_BUS_CORRECT_STATS, PA_KNEE_STATS, PA_BUS_UMI_STATS).
pub fn count_cells_em_umi<P: AsRef<Path>>(index_file: P, r1_fastq: P, r2_fastq: P, whitelist: Option<P>, out_dir: P, bc_len: u32, umi_len: u32, call_cells: bool,
                                          knee: Option<crate::amd_knee_ffi::PaKneeParams>, umi_mode: u32, params: Option<crate::amd_genes_ffi::PaGenesParams>,
                                          num_threads: usize,
                                          device: i32) -> Result<([u64; crate::amd_genes_ffi::PA_GENES_STATS], [u64; crate::amd_correct_ffi::PA_BUS_CORRECT_STATS],
                                                                  [u64; crate::amd_knee_ffi::PA_KNEE_STATS], [u64; crate::amd_umi_ffi::PA_BUS_UMI_STATS]), Error> {
    use crate::amd_correct_ffi::*;
    use crate::amd_genes_ffi::*;
    use crate::amd_knee_ffi::*;
    use crate::amd_umi_ffi::*;
    let cstr = |p: &P| CString::new(p.as_ref().to_string_lossy().into_owned());
    let (ix, r1, r2, out) = (cstr(&index_file)?, cstr(&r1_fastq)?, cstr(&r2_fastq)?, cstr(&out_dir)?);
    let wl = match whitelist.as_ref() { Some(w) => Some(cstr(w)?), None => None };
    let mut h = std::ptr::null_mut();
    check(unsafe { pa_host_index_load(ix.as_ptr(), &mut h) })?;
    let mut view: PaFlatIndex = unsafe { std::mem::zeroed() };
    let mut idx = std::ptr::null_mut();
    let mut rc = unsafe { pa_host_index_view(h, &mut view) };
    if rc >= 0 { rc = unsafe { pa_index_create(&view, device, &mut idx) }; }
    let (mut stats, mut cstats, mut kstats, mut ustats) = ([0u64; PA_GENES_STATS], [0u64; PA_BUS_CORRECT_STATS], [0u64; PA_KNEE_STATS], [0u64; PA_BUS_UMI_STATS]);
    if rc >= 0 {
        let kp = knee.as_ref().map_or(std::ptr::null(), |p| p as *const PaKneeParams);
        let p = params.as_ref().map_or(std::ptr::null(), |p| p as *const PaGenesParams);
        let wlp = wl.as_ref().map_or(std::ptr::null(), |w| w.as_ptr());
        rc = unsafe { pa_count_cells_em_umi(idx, h, r1.as_ptr(), r2.as_ptr(), wlp, bc_len, umi_len, call_cells as i32, kp, umi_mode, p, out.as_ptr(), num_threads as i32,
                                            stats.as_mut_ptr(), cstats.as_mut_ptr(), kstats.as_mut_ptr(), ustats.as_mut_ptr()) };
    }
    let result = check(rc).map(|_| (stats, cstats, kstats, ustats));   // (the message is read before the handles go)
    unsafe {
        if !idx.is_null() { pa_index_destroy(idx); }
        pa_host_index_destroy(h);
    }
    result
}

/// Transcript abundances (pa_quant_*): the EM over equivalence classes on the GPU, from a class-count table on the host
/// (`class_counts`: pa_counts_len entries, as the reduce over GPUs leaves it) and, optionally, the serialised overflow words
/// (pa_overflow_fetch / pa_overflow_allgather; without them the novel reads are left out). Runs to the stop rule and returns
/// (est_counts, tpm) per transcript; `tsv`, when given, also receives kallisto's abundance.tsv columns.
pub fn quantify(idx: *mut PaIndex, h: *const PaHostIndex, class_counts: &[u64], overflow_words: Option<&[u32]>, mean_read_len: f64,
                tsv: Option<&Path>) -> Result<(Vec<f64>, Vec<f64>), Error> {
    use crate::amd_quant_ffi::*;
    let mut p: PaQuantParams = unsafe { std::mem::zeroed() };
    unsafe { pa_quant_default_params(&mut p) };
    p.mean_read_len = mean_read_len;
    let mut q = std::ptr::null_mut();
    check(unsafe { pa_quant_create(idx, h, &p, &mut q) })?;
    let n = unsafe { pa_host_index_num_transcripts(h) } as usize;
    let (mut est, mut tpm) = (vec![0f64; n], vec![0f64; n]);
    let (words, n_words) = match overflow_words { Some(w) => (w.as_ptr(), w.len() as u64), None => (std::ptr::null(), 0) };
    let mut rc = unsafe { pa_quant_set_counts(q, class_counts.as_ptr(), class_counts.len() as u64, words, n_words) };
    let (mut iters, mut converged) = (0u32, 0);
    if rc >= 0 { rc = unsafe { pa_quant_run(q, &mut iters, &mut converged) }; }
    if rc >= 0 { rc = unsafe { pa_quant_fetch(q, est.as_mut_ptr(), tpm.as_mut_ptr(), std::ptr::null_mut()) }; }
    if rc >= 0 {
        if let Some(path) = tsv {
            let c = CString::new(path.to_string_lossy().into_owned())?;
            rc = unsafe { pa_write_abundance_tsv(q, c.as_ptr()) };
        }
    }
    let result = check(rc).map(|_| (est, tpm));   // (the message is read before the handle goes)
    unsafe { pa_quant_destroy(q) };
    info!("EM: {} iterations, converged: {}", iters, converged != 0);
    result
}

/// Bootstrap replicates of `quantify` (pa_quant_bootstrap_*): `n` resampled EM runs of the same table, batched on the GPU in groups of
/// at most `batch` (1 ..= PA_QUANT_BOOT_MAX_BATCH). Replicate b depends on (table, seed, b) alone, so any batch size gives the same bits.
/// Returns est_counts replicate-major (`n * num_transcripts`) and the iterations of every replicate.
pub fn quantify_bootstrap(idx: *mut PaIndex, h: *const PaHostIndex, class_counts: &[u64], overflow_words: Option<&[u32]>, mean_read_len: f64,
                          n: u32, seed: u64, batch: u32) -> Result<(Vec<f64>, Vec<u32>), Error> {
    use crate::amd_quant_ffi::*;
    let mut p: PaQuantParams = unsafe { std::mem::zeroed() };
    unsafe { pa_quant_default_params(&mut p) };
    p.mean_read_len = mean_read_len;
    let mut q = std::ptr::null_mut();
    check(unsafe { pa_quant_create(idx, h, &p, &mut q) })?;
    let t = unsafe { pa_host_index_num_transcripts(h) } as usize;
    let (mut est, mut iters) = (vec![0f64; n as usize * t], vec![0u32; n as usize]);
    let (words, n_words) = match overflow_words { Some(w) => (w.as_ptr(), w.len() as u64), None => (std::ptr::null(), 0) };
    let mut rc = unsafe { pa_quant_set_counts(q, class_counts.as_ptr(), class_counts.len() as u64, words, n_words) };
    let batch = batch.clamp(1, PA_QUANT_BOOT_MAX_BATCH);
    let mut first = 0u32;
    while rc >= 0 && first < n {
        let m = batch.min(n - first);
        rc = unsafe { pa_quant_bootstrap_draw(q, seed, first, m) };
        if rc >= 0 { rc = unsafe { pa_quant_bootstrap_run(q, iters[first as usize..].as_mut_ptr(), std::ptr::null_mut()) }; }
        if rc >= 0 { rc = unsafe { pa_quant_bootstrap_fetch(q, est[first as usize * t..].as_mut_ptr(), std::ptr::null_mut()) }; }
        first += m;
    }
    let result = check(rc).map(|_| (est, iters));
    unsafe { pa_quant_destroy(q) };
    result
}

// ---------------------------------------------------------------------------------------------------------------------------
// Drop-in entry points with the reference's EXACT signatures. The GPU copy of an index is made on first use and cached by the
// CONTENT of the `Pseudoaligner`: k, node / class / transcript counts and a fingerprint of EVERY base of every node, every node's
// colour and extension byte and EVERY id of every class — two indexes of the same shape with different sequence (SNP-personalised
// transcriptomes) or classes such as [1,5,9] / [1,6,9] never share a GPU copy; an index that was dropped and another one
// allocated in its place never meets a stale copy; a moved or cloned one finds its copy again. The cache holds at most
// CACHE_MAX GPU copies (least recently used goes: `pa_index_destroy` frees its HBM when the last `Arc` is dropped).
// ---------------------------------------------------------------------------------------------------------------------------
const CACHE_MAX: usize = 2;
type CacheKey = (usize, usize, usize, usize, u64);
fn fingerprint<K: Kmer>(index: &Pseudoaligner<K>) -> u64 {
    let mut h = 0xcbf2_9ce4_8422_2325u64;                                  // FNV-1a over 64-bit words
    let mut mix = |v: u64| { h ^= v; h = h.wrapping_mul(0x0000_0100_0000_01b3); };
    for c in &index.eq_classes {                                           // every class: its length and every id
        mix(c.len() as u64);
        for pair in c.chunks(2) { mix(((pair[0] as u64) << 32) | *pair.get(1).unwrap_or(&u32::MAX) as u64); }
    }
    for node in index.dbg.iter_nodes() {                                   // every node: length, colour, extensions, every base
        let s = node.sequence();
        mix(((s.len() as u64) << 32) | *node.data() as u64);
        mix(node.exts().val as u64);
        let (mut w, mut n) = (0u64, 0u32);
        for i in 0..s.len() {
            w |= (s.get(i) as u64) << (2 * n); n += 1;
            if n == 32 { mix(w); w = 0; n = 0; }
        }
        if n > 0 { mix(w); }
    }
    h
}
struct Cache { map: HashMap<CacheKey, Arc<AmdIndex>>, order: Vec<CacheKey> }   // order: least recently used first
fn cache() -> &'static Mutex<Cache> {
    static CACHE: OnceLock<Mutex<Cache>> = OnceLock::new();
    CACHE.get_or_init(|| Mutex::new(Cache { map: HashMap::new(), order: Vec::new() }))
}
fn key_of<K: Kmer>(index: &Pseudoaligner<K>) -> CacheKey {
    (index.dbg.len(), index.eq_classes.len(), index.tx_names.len(), K::k(), fingerprint(index))
}
// (the fingerprint walks every base once per call — tenths of a second at 200 k transcripts; `process_reads` and `map_reads` look
// their index up once per call, a host that calls `map_read` per read keeps the `Arc<AmdIndex>` of `gpu_index` instead)
fn device_of_env() -> i32 { std::env::var("PSEUDOALIGNER_AMD_DEVICE").ok().and_then(|v| v.parse().ok()).unwrap_or(0) }

/// the GPU copy of `index` (built once: about half a second for a 200 k-transcript index)
pub fn gpu_index<K: Kmer>(index: &Pseudoaligner<K>) -> Result<Arc<AmdIndex>, Error> {
    let key = key_of(index);
    {
        let mut c = cache().lock().unwrap();
        if let Some(hit) = c.map.get(&key).cloned() {
            c.order.retain(|k| *k != key); c.order.push(key);
            return Ok(hit);
        }
    }
    let made = Arc::new(AmdIndex::from_pseudoaligner(index, device_of_env())?);
    let mut c = cache().lock().unwrap();
    let got = c.map.entry(key).or_insert(made).clone();
    c.order.retain(|k| *k != key); c.order.push(key);
    while c.order.len() > CACHE_MAX { let old = c.order.remove(0); c.map.remove(&old); }   // the GPU copy goes with its last Arc
    Ok(got)
}
/// call before dropping a `Pseudoaligner` whose GPU copy should go too
pub fn forget<K: Kmer>(index: &Pseudoaligner<K>) {
    let key = key_of(index);
    let mut c = cache().lock().unwrap();
    c.map.remove(&key); c.order.retain(|k| *k != key);
}

/// MANY reads in one launch — what a caller that loops over `map_read` should call instead (the reference's own test maps every
/// transcript one call at a time, src/build_index.rs:309). One `map_read` call is one H2D + one kernel launch + one D2H: tens of
/// microseconds per read, slower than the CPU path it replaces; a batch amortises them over all its reads.
/// Result i is what `map_read(&reads[i])` returns (src/pseudoaligner.rs:381-384).
pub fn map_reads<K: Kmer + Sync + Send>(index: &Pseudoaligner<K>, reads: &[DnaString]) -> Result<Vec<Option<(Vec<u32>, usize)>>, Error> {
    let gpu = gpu_index(index)?;
    let (mut words, mut word_off, mut lens) = (Vec::new(), vec![0u64], Vec::with_capacity(reads.len()));
    for r in reads {                                                       // every read starts on a word boundary, LSB-first words
        let base = words.len();
        words.resize(base + (r.len() + 31) / 32, 0u64);
        for i in 0..r.len() { words[base + i / 32] |= (r.get(i) as u64) << (2 * (i % 32)); }
        word_off.push(words.len() as u64);
        lens.push(r.len() as u32);
    }
    words.push(0);
    let mut results = vec![PaReadResult::default(); reads.len()];
    let mut class_off = vec![0u64; reads.len() + 1];
    let mut class_ids: *const u32 = std::ptr::null();
    check(unsafe { pa_map_batch_packed(gpu.raw, words.as_ptr(), word_off.as_ptr(), lens.as_ptr(), reads.len() as u64, PA_PACKED_LSB_FIRST,
                                       DEFAULT_ALLOWED_MISMATCHES as u32, results.as_mut_ptr(), class_off.as_mut_ptr(), &mut class_ids) })?;
    Ok((0..reads.len()).map(|i| {
        if results[i].mismatches & PA_MAPPED_BIT == 0 { return None; }
        let ids = unsafe { std::slice::from_raw_parts(class_ids.add(class_off[i] as usize), (class_off[i + 1] - class_off[i]) as usize) };
        Some((ids.to_vec(), results[i].coverage as usize))                 // (library-owned ids: copied before the next call on this index)
    }).collect())
}

/// `Pseudoaligner::map_read` (src/pseudoaligner.rs:381), same arguments and result: replace its body by
/// `crate::amd::map_read(self, read_seq)`. Panics where the reference panics (it has no error path, :307,446).
pub fn map_read<K: Kmer + Sync + Send>(index: &Pseudoaligner<K>, read_seq: &DnaString) -> Option<(Vec<u32>, usize)> {
    let gpu = gpu_index(index).expect("pseudoaligner_amd: GPU index");
    gpu.map_read_with_mismatch(read_seq, DEFAULT_ALLOWED_MISMATCHES).expect("pseudoaligner_amd: map_read")
        .map(|(eq_class, read_coverage, _mismatches)| (eq_class, read_coverage))
}

/// `process_reads` (src/pseudoaligner.rs:420-425) with the reference's signature. The worker pool, the reader mutex
/// (utils.rs:152-157) and the sync_channel (:430) become: read a chunk of records -> pa_records_push (packs and launches full
/// batches on the GPU while this thread goes on reading) -> pa_records_pull (the Debug tuples of :490, in input order) -> stdout.
/// BOUND BY ITS READER: the signature hands over an open `fastq::Reader`, so ONE thread iterates `records()` (a few M records/s:
/// a line scan, two allocations and a UTF-8 check per record) — one GPU maps 150 M reads/s from text and 13 G reads/s from HBM
/// behind it. A caller that knows the file's path (the CLI does) calls `process_reads_path` above: two lines of
/// src/bin/pseudoaligner.rs.
pub fn process_reads<K: Kmer + Sync + Send, P: AsRef<Path> + Debug>(
    reader: fastq::Reader<io::BufReader<File>>,
    index: &Pseudoaligner<K>,
    outdir: P,
    num_threads: usize,
) -> Result<(), Error> {
    info!("Done Reading index");
    info!("Starting Multi-threaded Mapping");
    info!("Output directory: {:?}", outdir);
    let gpu = gpu_index(index)?;
    let mut stream = std::ptr::null_mut();
    check(unsafe { pa_record_stream_create(gpu.raw, num_threads as i32, 0, &mut stream) })?;
    struct Guard(*mut PaRecordStream);
    impl Drop for Guard { fn drop(&mut self) { unsafe { pa_record_stream_destroy(self.0) } } }
    let _guard = Guard(stream);

    let stdout = io::stdout();
    let mut out = io::BufWriter::with_capacity(1 << 22, stdout.lock());
    let mut text = vec![0u8; 1 << 26];   // (big pulls are copied by the library's worker pool)
    let mut millions_reported = 0u64;
    let mut drain = |out: &mut dyn Write| -> Result<(), Error> {
        loop {
            let mut n = 0usize;
            let rc = unsafe { pa_records_pull(stream, text.as_mut_ptr() as *mut _, text.len(), &mut n) };
            if rc == PA_ERR_BUFFER_TOO_SMALL && text.len() < (1usize << 31) {
                // one tuple longer than the buffer (a class of hundreds of thousands of ids): n = the bytes it needs; grow and ask again
                text.resize(n.max(text.len() * 2), 0);
                continue;
            }
            check(rc)?;
            if n == 0 { break; }
            out.write_all(&text[..n])?;
        }
        // the reference's progress line (src/pseudoaligner.rs:497-503), whenever another million reads have been printed
        // (batch granular: the counts are those of the batches rendered so far)
        let (mut n_reads, mut n_flagged) = (0u64, 0u64);
        check(unsafe { pa_record_stream_stats(stream, &mut n_reads, &mut n_flagged) })?;
        if n_reads / 1_000_000 > millions_reported {
            millions_reported = n_reads / 1_000_000;
            eprint!("\rDone Mapping {} reads w/ Rate: {}", n_reads, n_flagged as f32 * 100.0 / n_reads as f32);
            io::stderr().flush().expect("Could not flush stdout");
        }
        Ok(())
    };
    let mut records = reader.records();
    loop {
        let (mut ids, mut id_off, mut seqs, mut seq_off) = (Vec::new(), vec![0u64], Vec::new(), vec![0u64]);
        for r in records.by_ref().take(1 << 16) {
            let r = r?;
            ids.extend_from_slice(r.id().as_bytes()); id_off.push(ids.len() as u64);       // record.id() (:456)
            seqs.extend_from_slice(r.seq()); seq_off.push(seqs.len() as u64);             // record.seq() (:449)
        }
        let n = id_off.len() - 1;
        if n == 0 { break; }
        check(unsafe { pa_records_push(stream, ids.as_ptr(), id_off.as_ptr(), seqs.as_ptr(), seq_off.as_ptr(), n as u64) })?;
        drain(&mut out)?;
    }
    check(unsafe { pa_records_flush(stream) })?;
    drain(&mut out)?;
    out.flush()?;
    let (mut n_reads, mut n_flagged) = (0u64, 0u64);
    check(unsafe { pa_record_stream_stats(stream, &mut n_reads, &mut n_flagged) })?;
    eprintln!();
    info!("Done Mapping Reads");
    info!("Mapped {} reads, {} flagged", n_reads, n_flagged);
    Ok(())
}
