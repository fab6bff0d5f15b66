"""MI355X-native pseudoalignment hot path behind the API surface of rust-pseudoaligner's `Pseudoaligner`.

Python here is plumbing over the C ABI (include/pseudoaligner_amd.h): the product is libpseudoaligner_amd.so
(hand-written HIP for gfx950 + a C++ host runtime). Nothing in this package imports the CPU oracle and there is no
CPU fallback: without the built library or without a GPU the mapping entry points raise.

Mirrors (names and argument meaning follow the reference):
    Pseudoaligner.map_read / map_read_with_mismatch / map_read_to_nodes   src/pseudoaligner.rs:381, 361, 54
    process_reads                                                          src/pseudoaligner.rs:420
    build_index                                                            src/build_index.rs:27 (CPU)
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _build, _ffi
from ._ffi import (PA_DEFAULT_ALLOWED_MISMATCHES, PA_ERR_ARENA_FULL, PA_MAPPED_BIT, PA_OK, PA_READ_COVERAGE_THRESHOLD, FlatIndex,
                   IndexStats, PaError, ReadResult, check, lib, vp)

__all__ = ["HostIndex", "Txome", "Pseudoaligner", "build_index", "process_reads", "process_reads_multi", "PaError", "lib", "concat_reads",
           "gather_classes", "unpack_compact", "unpack_tiles", "RESULT_DTYPE", "PA_MAPPED_BIT", "PA_DEFAULT_ALLOWED_MISMATCHES",
           "PA_READ_COVERAGE_THRESHOLD", "PA_CLASS_REF", "Overflow", "Comm", "parse_overflow", "serialise_overflow", "overflow_merge",
           "CellCounter", "load_whitelist", "Quantifier", "BusWriter", "BUS_RECORD_DTYPE", "GeneCounter", "bus_whitelist_pack", "bus_correct", "bus_correct_phase_ms",
           "CORRECT_STAT_NAMES", "BARCODE_ROW_DTYPE", "bus_knee", "bus_keep", "bus_knee_phase_ms", "write_barcode_ranks_tsv", "KNEE_STAT_NAMES", "KEEP_STAT_NAMES"]

PA_CLASS_REF = 0x80000000
RESULT_DTYPE = np.dtype([("coverage", "<u4"), ("mismatches", "<u4"), ("class_off", "<u4"), ("class_len", "<u4")])


def _np_view(ptr: int, n: int, dtype, owner=None) -> np.ndarray:
    """numpy view of library-owned memory; `owner` (the wrapper object whose handle owns it) is kept alive by the view"""
    if n == 0 or not ptr:
        return np.zeros(0, dtype=dtype)
    buf = (C.c_uint8 * (int(n) * np.dtype(dtype).itemsize)).from_address(ptr)
    buf._pa_owner = owner          # ndarray.base -> buf -> owner: the index cannot be destroyed under a live view
    return np.frombuffer(buf, dtype=dtype)


def concat_reads(reads: Sequence) -> Tuple[np.ndarray, np.ndarray]:
    """ASCII reads -> (concatenated uint8, offsets[n+1] uint64)."""
    bs = [r.encode() if isinstance(r, str) else bytes(r) for r in reads]
    offsets = np.zeros(len(bs) + 1, dtype=np.uint64)
    if bs:
        offsets[1:] = np.cumsum([len(b) for b in bs], dtype=np.uint64)
    data = np.frombuffer(b"".join(bs), dtype=np.uint8) if bs else np.zeros(0, np.uint8)
    return np.ascontiguousarray(data), offsets


class HostIndex:
    """CPU-side index: the flat form of `pub struct Pseudoaligner<K>` (src/pseudoaligner.rs:26-33)."""

    def __init__(self, handle: int):
        self._h = vp(handle)

    @classmethod
    def build_fasta(cls, fasta_path: str, k: int, num_threads: int = 0) -> "HostIndex":
        h = vp()
        check(lib().pa_host_index_build_fasta(str(fasta_path).encode(), k, num_threads, C.byref(h)))
        return cls(h.value)

    @classmethod
    def build_packed(cls, packed: np.ndarray, tx_start: np.ndarray, k: int, num_threads: int = 0) -> "HostIndex":
        packed = np.ascontiguousarray(packed, dtype=np.uint64)
        tx_start = np.ascontiguousarray(tx_start, dtype=np.uint64)
        h = vp()
        check(lib().pa_host_index_build_packed(packed.ctypes.data, tx_start.ctypes.data, len(tx_start) - 1, k, num_threads, C.byref(h)))
        return cls(h.value)

    @classmethod
    def from_txome(cls, txome: "Txome", k: int, num_threads: int = 0) -> "HostIndex":
        packed, tx_start = txome.arrays()
        return cls.build_packed(packed, tx_start, k, num_threads)

    # the same index with the graph construction on the GPU (csrc/index_build.hip)
    @classmethod
    def build_fasta_device(cls, fasta_path: str, k: int, device: int = 0) -> "HostIndex":
        h = vp()
        check(lib().pa_host_index_build_fasta_device(str(fasta_path).encode(), k, device, C.byref(h)))
        return cls(h.value)

    @classmethod
    def build_packed_device(cls, packed: np.ndarray, tx_start: np.ndarray, k: int, device: int = 0) -> "HostIndex":
        packed = np.ascontiguousarray(packed, dtype=np.uint64)
        tx_start = np.ascontiguousarray(tx_start, dtype=np.uint64)
        h = vp()
        check(lib().pa_host_index_build_packed_device(packed.ctypes.data, tx_start.ctypes.data, len(tx_start) - 1, k, device, C.byref(h)))
        return cls(h.value)

    @classmethod
    def from_txome_device(cls, txome: "Txome", k: int, device: int = 0) -> "HostIndex":
        packed, tx_start = txome.arrays()
        return cls.build_packed_device(packed, tx_start, k, device)

    @classmethod
    def from_flat(cls, flat: FlatIndex) -> "HostIndex":
        h = vp()
        check(lib().pa_host_index_from_flat(C.byref(flat), C.byref(h)))
        return cls(h.value)

    @classmethod
    def load(cls, path: str) -> "HostIndex":
        h = vp()
        check(lib().pa_host_index_load(str(path).encode(), C.byref(h)))
        return cls(h.value)

    def save(self, path: str) -> None:
        check(lib().pa_host_index_save(self._h, str(path).encode()))

    def compare(self, other: "HostIndex", max_kmers: int = 1 << 26) -> Tuple[int, str]:
        """pa_host_index_compare: (0 equivalent | 1 different | 2 undecided, one line of explanation)"""
        buf = C.create_string_buffer(512)
        rc = check(lib().pa_host_index_compare(self._h, other._h, max_kmers, buf, len(buf)))
        return rc, buf.value.decode()

    def flat(self) -> FlatIndex:
        f = FlatIndex()
        check(lib().pa_host_index_view(self._h, C.byref(f)))
        return f

    def arrays(self) -> dict:
        """numpy views (no copy) of the flat arrays; valid while this object is alive."""
        f = self.flat()
        n, c = f.num_nodes, f.num_classes
        ec_offset = _np_view(f.ec_offset, c + 1, np.uint64, owner=self)
        return dict(k=f.k, num_nodes=n, num_classes=c, num_transcripts=f.num_transcripts,
                    node_seq=_np_view(f.node_seq, (f.seq_bases + 31) // 32 + 1, np.uint64, owner=self),
                    node_start=_np_view(f.node_start, n + 1, np.uint64, owner=self), node_len=_np_view(f.node_len, n, np.uint32, owner=self),
                    node_exts=_np_view(f.node_exts, n, np.uint8, owner=self), node_colour=_np_view(f.node_colour, n, np.uint32, owner=self),
                    ec_offset=ec_offset, ec_ids=_np_view(f.ec_ids, int(ec_offset[-1]) if c else 0, np.uint32, owner=self))

    @property
    def k(self) -> int:
        return self.flat().k

    @property
    def num_transcripts(self) -> int:
        return lib().pa_host_index_num_transcripts(self._h)

    def tx_names(self) -> List[str]:
        return [lib().pa_host_index_tx_name(self._h, i).decode() for i in range(self.num_transcripts)]

    def tx_genes(self) -> List[str]:
        return [lib().pa_host_index_tx_gene(self._h, i).decode() for i in range(self.num_transcripts)]

    def genes(self) -> Tuple[np.ndarray, List[str]]:
        """(gene id of each transcript, gene names): tx_gene_mapping (src/pseudoaligner.rs:32), genes numbered by first appearance"""
        n = C.c_uint32()
        tx_gene = np.zeros(max(self.num_transcripts, 1), np.uint32)
        check(lib().pa_host_index_genes(self._h, tx_gene.ctypes.data, C.byref(n)))
        return tx_gene[: self.num_transcripts], [lib().pa_host_index_gene_name(self._h, g).decode() for g in range(n.value)]

    def collapse_to_genes(self, class_counts: np.ndarray) -> np.ndarray:
        """gene-level counts (last entry: classes spanning several genes) from a class-count table of counts_len entries"""
        n = C.c_uint32()
        check(lib().pa_host_index_genes(self._h, None, C.byref(n)))
        cc = np.ascontiguousarray(class_counts, np.uint64)
        out = np.zeros(n.value + 1, np.uint64)
        check(lib().pa_counts_collapse_genes(self._h, cc.ctypes.data, len(cc), out.ctypes.data))
        return out

    def mappability(self) -> Tuple[np.ndarray, np.ndarray]:
        """analyze_graph (src/mappability.rs:120-156): (tx_multiplicity, gene_multiplicity), each [num_transcripts, 11]"""
        W = 11   # PA_MAPPABILITY_COUNTS_LEN
        tm = np.zeros((max(self.num_transcripts, 1), W), np.uint64)
        gm = np.zeros_like(tm)
        check(lib().pa_host_index_mappability(self._h, tm.ctypes.data, gm.ctypes.data))
        return tm[: self.num_transcripts], gm[: self.num_transcripts]

    def write_mappability_tsv(self, path: str) -> None:
        """write_mappability_tsv (src/mappability.rs:91-104)"""
        check(lib().pa_write_mappability_tsv(self._h, str(path).encode()))

    def transcripts(self) -> Tuple[np.ndarray, np.ndarray]:
        p, s, n = vp(), vp(), C.c_uint32()
        check(lib().pa_host_index_transcripts(self._h, C.byref(p), C.byref(s), C.byref(n)))
        tx_start = _np_view(s.value, n.value + 1, np.uint64, owner=self)
        return _np_view(p.value, (int(tx_start[-1]) + 31) // 32 + 1, np.uint64, owner=self), tx_start

    def __del__(self):
        try:
            if self._h:
                lib().pa_host_index_destroy(self._h)
                self._h = vp()
        except Exception:
            pass


class Txome:
    """A transcript set (packed) used to build indices and to simulate reads."""

    def __init__(self, handle: int):
        self._h = vp(handle)
        self._dev = {}

    @classmethod
    def synthesize(cls, num_genes: int, target_transcripts: int, seed: int) -> "Txome":
        h = vp()
        check(lib().pa_txome_synthesize(num_genes, target_transcripts, seed, C.byref(h)))
        return cls(h.value)

    # bench.py's "config3r": 40 old (10-15 % diverged) + 10 young (3-6 %) repeat families of 300 bases in the last exon of 13 % of the genes, 200 low-complexity tracts
    REPEATS_DEFAULT = dict(families=40, element_len=300, div_lo_ppm=100000, div_hi_ppm=150000, young_families=10, young_div_lo_ppm=30000, young_div_hi_ppm=60000,
                           gene_fraction_ppm=130000, low_complexity_genes=200)

    @classmethod
    def synthesize_repeats(cls, num_genes: int, target_transcripts: int, seed: int, **repeats) -> "Txome":
        """pa_txome_synthesize_repeats: the transcriptome of synthesize() with interspersed repeats and low-complexity tracts"""
        cfg = dict(cls.REPEATS_DEFAULT, **repeats)
        r = _ffi.SynthRepeats(**cfg)
        h = vp()
        check(lib().pa_txome_synthesize_repeats(num_genes, target_transcripts, seed, C.byref(r), C.byref(h)))
        return cls(h.value)

    @classmethod
    def from_fasta(cls, path: str) -> "Txome":
        h = vp()
        check(lib().pa_txome_from_fasta(str(path).encode(), C.byref(h)))
        return cls(h.value)

    @classmethod
    def from_host_index(cls, index: HostIndex) -> "Txome":
        h = vp()
        check(lib().pa_txome_from_host_index(index._h, C.byref(h)))
        return cls(h.value)

    def arrays(self) -> Tuple[np.ndarray, np.ndarray]:
        p, s, n = vp(), vp(), C.c_uint32()
        check(lib().pa_txome_view(self._h, C.byref(p), C.byref(s), C.byref(n)))
        tx_start = _np_view(s.value, n.value + 1, np.uint64, owner=self)
        return _np_view(p.value, (int(tx_start[-1]) + 31) // 32 + 1, np.uint64, owner=self), tx_start

    @property
    def num_transcripts(self) -> int:
        return len(self.arrays()[1]) - 1

    def simulate_host(self, read_len: int, seed: int, n_reads: int, sub_rate_ppm: int = 0, first_read: int = 0,
                      words_per_read: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray]:
        wpr = words_per_read or lib().pa_words_per_read(read_len)
        tiles = np.zeros(lib().pa_tiles_words(n_reads, wpr), dtype=np.uint64)
        lens = np.zeros(n_reads, dtype=np.uint32)
        check(lib().pa_simulate_reads_host(self._h, read_len, seed, sub_rate_ppm, first_read, n_reads, wpr, tiles.ctypes.data, lens.ctypes.data))
        return tiles, lens

    def device_handle(self, read_len: int, device: int = 0) -> vp:
        key = (read_len, device)
        if key not in self._dev:
            h = vp()
            check(lib().pa_txome_upload(self._h, read_len, device, C.byref(h)))
            self._dev[key] = h
        return self._dev[key]

    def simulate_device(self, read_len: int, seed: int, n_reads: int, d_tiles: int, d_lens: int, sub_rate_ppm: int = 0,
                        first_read: int = 0, words_per_read: Optional[int] = None, device: int = 0, stream: int = 0) -> None:
        wpr = words_per_read or lib().pa_words_per_read(read_len)
        check(lib().pa_simulate_reads_device(self.device_handle(read_len, device), seed, sub_rate_ppm, first_read, n_reads, wpr,
                                             d_tiles, d_lens, stream or None))

    def __del__(self):
        try:
            for h in self._dev.values():
                lib().pa_txome_device_destroy(h)
            self._dev = {}
            if self._h:
                lib().pa_txome_destroy(self._h)
                self._h = vp()
        except Exception:
            pass


def build_index(fasta_path: str, k: int, num_threads: int = 0) -> HostIndex:
    """build_index (src/build_index.rs:27-32) over utils::read_transcripts (src/utils.rs:61); CPU."""
    return HostIndex.build_fasta(fasta_path, k, num_threads)


def encode_reads_host(reads: Sequence, words_per_read: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray, int]:
    """ASCII reads -> (tiles, lens, words_per_read) in the device tile layout, packed on the host."""
    data, offsets = reads if isinstance(reads, tuple) else concat_reads(reads)
    n = len(offsets) - 1
    maxlen = int((offsets[1:] - offsets[:-1]).max()) if n else 1
    wpr = words_per_read or lib().pa_words_per_read(maxlen)
    tiles = np.zeros(lib().pa_tiles_words(n, wpr), dtype=np.uint64)
    lens = np.zeros(max(n, 1), dtype=np.uint32)
    check(lib().pa_encode_reads_host(data.ctypes.data, offsets.ctypes.data, n, wpr, tiles.ctypes.data, lens.ctypes.data))
    return tiles, lens[:n], wpr


def unpack_tiles(tiles: np.ndarray, lens: np.ndarray, words_per_read: int) -> List[str]:
    """tile layout -> ASCII strings (tests / debugging)."""
    t = tiles.reshape(-1, words_per_read, 64)
    out = []
    for i, L in enumerate(lens):
        words = t[i >> 6, :, i & 63]
        out.append("".join("ACGT"[(int(words[j >> 5]) >> (2 * (j & 31))) & 3] for j in range(int(L))))
    return out


class Pseudoaligner:
    """GPU-resident index with the reference's mapping API (src/pseudoaligner.rs:35-385)."""

    def __init__(self, index: HostIndex, device: int = 0):
        self.host = index
        self.device = device
        flat = index.flat()
        h = vp()
        check(lib().pa_index_create(C.byref(flat), device, C.byref(h)))
        self._h = h

    def stats(self) -> IndexStats:
        s = IndexStats()
        check(lib().pa_index_get_stats(self._h, C.byref(s)))
        return s

    # ---- single reads -------------------------------------------------------------------------------
    def map_read_with_mismatch(self, read_seq, allowed_mismatches: int) -> Optional[Tuple[List[int], int, int]]:
        """-> Some((eq_class, read_coverage, mismatches)) | None (src/pseudoaligner.rs:361-376)"""
        seq = read_seq.encode() if isinstance(read_seq, str) else bytes(read_seq)
        cap = max(64, self.stats().max_class_len)
        buf = (C.c_uint32 * cap)()
        n, cov, mm = C.c_uint32(), C.c_uint32(), C.c_uint32()
        rc = check(lib().pa_map_read_with_mismatch(self._h, seq, len(seq), allowed_mismatches, buf, cap, C.byref(n), C.byref(cov), C.byref(mm)))
        if rc == 0:
            return None
        return list(buf[: n.value]), cov.value, mm.value

    def map_read(self, read_seq) -> Optional[Tuple[List[int], int]]:
        """-> Some((eq_class, read_coverage)) | None with allowed mismatches = 2 (src/pseudoaligner.rs:381-384)"""
        r = self.map_read_with_mismatch(read_seq, PA_DEFAULT_ALLOWED_MISMATCHES)
        return None if r is None else (r[0], r[1])

    def map_read_to_nodes(self, read_seq, allowed_mismatches: int = PA_DEFAULT_ALLOWED_MISMATCHES) -> Optional[Tuple[List[int], int]]:
        """-> Some((nodes in visit order, read_coverage)) | None (src/pseudoaligner.rs:54-61)"""
        seq = read_seq.encode() if isinstance(read_seq, str) else bytes(read_seq)
        cap = 2 * len(seq) + 8
        buf = (C.c_uint32 * cap)()
        n, cov, mm = C.c_uint32(), C.c_uint32(), C.c_uint32()
        rc = check(lib().pa_map_read_to_nodes(self._h, seq, len(seq), allowed_mismatches, buf, cap, C.byref(n), C.byref(cov), C.byref(mm)))
        if rc == 0:
            return None
        return list(buf[: n.value]), cov.value

    # ---- batches ------------------------------------------------------------------------------------
    def map_batch(self, reads: Sequence, allowed_mismatches: int = PA_DEFAULT_ALLOWED_MISMATCHES, strand: str = "fwd"):
        """-> (results[n] RESULT_DTYPE, class_offsets[n+1], class_ids) in input order; `mismatches` has bit 31 = mapped.
        strand: "fwd" the reads as given (pa_map_batch), "rev" their reverse complements, "both" both strands mapped and the two answers
        merged by the rule of unstranded libraries (pa_map_batch_strand)"""
        if strand not in _ffi.STRANDS:
            raise ValueError("strand %r: one of %s" % (strand, sorted(_ffi.STRANDS)))
        data, offsets = reads if isinstance(reads, tuple) else concat_reads(reads)
        n = len(offsets) - 1
        results = np.zeros(n, dtype=RESULT_DTYPE)
        coff = np.zeros(n + 1, dtype=np.uint64)
        ids = vp()
        if strand != "fwd":
            check(lib().pa_map_batch_strand(self._h, data.ctypes.data, offsets.ctypes.data, n, _ffi.STRANDS[strand], allowed_mismatches, results.ctypes.data,
                                            coff.ctypes.data, C.byref(ids)))
            return results, coff, _np_view(ids.value, int(coff[-1]), np.uint32).copy()
        check(lib().pa_map_batch(self._h, data.ctypes.data, offsets.ctypes.data, n, allowed_mismatches, results.ctypes.data,
                                 coff.ctypes.data, C.byref(ids)))
        class_ids = _np_view(ids.value, int(coff[-1]), np.uint32).copy()
        return results, coff, class_ids

    def map_batch_packed(self, words: np.ndarray, word_offsets: np.ndarray, lens: np.ndarray, layout: int = 0,
                         allowed_mismatches: int = PA_DEFAULT_ALLOWED_MISMATCHES):
        """map_batch for reads held 2-bit packed (a DnaString, :450): read i = lens[i] bases in words[word_offsets[i]:word_offsets[i+1]];
        layout 0 = LSB-first words, 1 = MSB-first words"""
        words = np.ascontiguousarray(words, dtype=np.uint64)
        word_offsets = np.ascontiguousarray(word_offsets, dtype=np.uint64)
        lens = np.ascontiguousarray(lens, dtype=np.uint32)
        n = len(lens)
        results = np.zeros(n, dtype=RESULT_DTYPE)
        coff = np.zeros(n + 1, dtype=np.uint64)
        ids = vp()
        check(lib().pa_map_batch_packed(self._h, words.ctypes.data, word_offsets.ctypes.data, lens.ctypes.data, n, layout, allowed_mismatches,
                                        results.ctypes.data, coff.ctypes.data, C.byref(ids)))
        return results, coff, _np_view(ids.value, int(coff[-1]), np.uint32).copy()

    def map_read_packed(self, words: np.ndarray, length: int, layout: int = 0, allowed_mismatches: int = PA_DEFAULT_ALLOWED_MISMATCHES, cap: int = 1 << 16):
        """map_read_with_mismatch (:361) of one packed read -> (ids, coverage, mismatches) or None"""
        words = np.ascontiguousarray(words, dtype=np.uint64)
        buf = np.zeros(cap, dtype=np.uint32)
        clen, cov, mm = C.c_uint32(), C.c_uint32(), C.c_uint32()
        rc = lib().pa_map_read_packed(self._h, words.ctypes.data, length, layout, allowed_mismatches, buf.ctypes.data, cap, C.byref(clen), C.byref(cov), C.byref(mm))
        if rc < 0:
            check(rc)
        return (buf[: clen.value].tolist(), cov.value, mm.value) if rc == 1 else None

    def map_batch_nodes(self, reads: Sequence, allowed_mismatches: int = PA_DEFAULT_ALLOWED_MISMATCHES):
        data, offsets = reads if isinstance(reads, tuple) else concat_reads(reads)
        n = len(offsets) - 1
        maxlen = int((offsets[1:] - offsets[:-1]).max()) if n else 1
        stride = 2 * maxlen + 8
        results = np.zeros(n, dtype=RESULT_DTYPE)
        nodes = np.zeros((n, stride), dtype=np.uint32)
        nlen = np.zeros(n, dtype=np.uint32)
        check(lib().pa_map_batch_nodes(self._h, data.ctypes.data, offsets.ctypes.data, n, allowed_mismatches, results.ctypes.data,
                                       nodes.ctypes.data, stride, nlen.ctypes.data))
        return results, nodes, nlen

    def map_batch_device(self, d_tiles: int, d_lens: int, n_reads: int, words_per_read: int, d_results: int, d_arena: int,
                         arena_cap: int, allowed_mismatches: int = PA_DEFAULT_ALLOWED_MISMATCHES, d_colour: int = 0, stream: int = 0) -> None:
        """Asynchronous launch of the hot path on device-resident tiles (raw device pointers)."""
        check(lib().pa_map_batch_device(self._h, d_tiles, d_lens, n_reads, words_per_read, allowed_mismatches, d_results, d_arena,
                                        arena_cap, d_colour or None, stream or None))

    def map_count_batch_device(self, d_tiles: int, d_lens: int, n_reads: int, words_per_read: int, d_results: int, d_arena: int,
                               arena_cap: int, d_counts: int, allowed_mismatches: int = PA_DEFAULT_ALLOWED_MISMATCHES, stream: int = 0) -> None:
        """map_batch_device with the class-count table (u64[counts_len()]) accumulated in the same kernel."""
        check(lib().pa_map_count_batch_device(self._h, d_tiles, d_lens, n_reads, words_per_read, allowed_mismatches, d_results, d_arena,
                                              arena_cap, d_counts, stream or None))

    def map_count_batch_uniform_device(self, d_tiles: int, read_len: int, n_reads: int, words_per_read: int, d_results: int, d_arena: int,
                                       arena_cap: int, d_counts: int, allowed_mismatches: int = PA_DEFAULT_ALLOWED_MISMATCHES, stream: int = 0) -> None:
        """map_count_batch_device for a batch whose reads all have read_len bases: no length array"""
        check(lib().pa_map_count_batch_uniform_device(self._h, d_tiles, read_len, n_reads, words_per_read, allowed_mismatches, d_results, d_arena,
                                                      arena_cap, d_counts, stream or None))

    def map_tiles_host(self, h_tiles: int, n_reads: int, words_per_read: int, h_compact: int, h_packed: int, packed_cap: int, h_lens: int = 0, uniform_len: int = 0,
                       h_counts: int = 0, allowed_mismatches: int = PA_DEFAULT_ALLOWED_MISMATCHES, chunk_reads: int = 0, n_streams: int = 0) -> int:
        """pa_map_tiles_host: a batch in (pinned) host memory -> compact records + packed classes (+ count table) on the host, chunks pipelined
        over several streams; returns the words of the packed stream. Raw host pointers. Reads longer than PA_COMPACT_MAX_READ_LEN bases do not fit
        the compact records: PaError (PA_ERR_INVALID_ARG) before anything is copied."""
        pw = C.c_uint64()
        check(lib().pa_map_tiles_host(self._h, h_tiles, h_lens or None, uniform_len, n_reads, words_per_read, allowed_mismatches, h_compact, h_packed or None, packed_cap,
                                      C.byref(pw), h_counts or None, chunk_reads, n_streams))
        return pw.value

    def map_finish(self, stream: int = 0) -> Tuple[int, int]:
        used, need = C.c_uint64(), C.c_uint64()
        check(lib().pa_map_finish(self._h, stream or None, C.byref(used), C.byref(need)))
        return used.value, need.value

    def set_timing(self, on: bool = True) -> None:
        """HIP events around the mapping kernel of every launch (pa_map_kernel_ms)"""
        check(lib().pa_index_set_timing(self._h, 1 if on else 0))

    def map_kernel_ms(self, stream: int = 0) -> float:
        ms = C.c_float()
        check(lib().pa_map_kernel_ms(self._h, stream or None, C.byref(ms)))
        return ms.value

    def map_stage_ms(self, stream: int = 0):
        """(mapping kernel, resolve kernel, count kernels) of the last timed launch, ms"""
        ms = (C.c_float * 3)()
        check(lib().pa_map_stage_ms(self._h, stream or None, ms))
        return ms[0], ms[1], ms[2]

    def release_stream(self, stream: int = 0) -> None:
        check(lib().pa_index_release_stream(self._h, stream or None))

    def arena_hint(self, n_reads: int) -> int:
        return lib().pa_map_arena_hint(self._h, n_reads)

    def counts_len(self) -> int:
        return lib().pa_counts_len(self._h)

    def counts_by_barcode_device(self, d_results: int, d_arena: int, d_barcode: int, n_reads: int, d_keys: int, d_vals: int,
                                 barcode_bits: int = 0, stream: int = 0) -> int:
        """sparse (barcode, class) -> reads matrix as sorted keys (barcode << 32 | column) + counts; returns the number of cells"""
        n = C.c_uint64()
        check(lib().pa_counts_by_barcode_device(self._h, d_results, d_arena, d_barcode, n_reads, barcode_bits, d_keys, d_vals, C.byref(n), stream or None))
        return n.value

    def count_cells(self, host_index: HostIndex, r1: str, r2: str, whitelist: str, out_dir: str, bc_len: int = 16, umi_len: int = 12,
                    num_threads: int = 0) -> dict:
        """The single-cell chain from files (pa_count_cells): paired R1 (barcode + UMI) / R2 (cDNA) FASTQ and a barcode whitelist ->
        out_dir/matrix.mtx, barcodes.tsv, features.tsv (UMI counts, cells x genes). Returns the stats (CellCounter.stats)."""
        st = np.zeros(_ffi.PA_CELL_STATS, np.uint64)
        check(lib().pa_count_cells(self._h, host_index._h, str(r1).encode(), str(r2).encode(), str(whitelist).encode(), bc_len, umi_len,
                                   str(out_dir).encode(), num_threads, st.ctypes.data))
        return dict(zip(_ffi.CELL_STAT_NAMES, (int(x) for x in st)))

    def write_bus(self, host_index: HostIndex, r1: str, r2: str, out_dir: str, bc_len: int = 16, umi_len: int = 12, num_threads: int = 0,
                  whitelist: Optional[str] = None, call_cells=None, umi_correct: Optional[str] = None) -> dict:
        """Paired R1 (barcode + UMI) / R2 (cDNA) FASTQ -> out_dir/output.bus (sorted, collapsed BUS v1 records), matrix.ec and
        transcripts.txt (pa_write_bus): the input of the kallisto | bustools family. Returns the stats (BusWriter.stats). With `whitelist`
        (the path of a barcode whitelist file) the barcodes are corrected against it before the files are written
        (pa_write_bus_corrected), and the stats hold the correction's under "correct" (BusWriter.correct). With `call_cells` (True for the
        defaults, or a dict of knee params as BusWriter.knee takes them) cells are called (pa_write_bus_called): without a whitelist the called
        barcodes are the whitelist of the correction, with one the corrected records of uncalled barcodes are dropped; out_dir/barcode_ranks.tsv
        holds the table, and the stats hold the knee's under "knee". With `umi_correct` ("greatest" or "directional") the UMIs are corrected
        after those steps, last of all (pa_write_bus_umi; BusWriter.umi_correct), and the stats hold that step's under "umi"; barcode_ranks.tsv
        shows the molecule counts before it."""
        st = np.zeros(_ffi.PA_BUS_STATS, np.uint64)
        if umi_correct is not None:
            return self._umi_call(lambda *a: lib().pa_write_bus_umi(self._h, host_index._h, str(r1).encode(), str(r2).encode(), *a), st, _ffi.BUS_STAT_NAMES, whitelist,
                                  bc_len, umi_len, call_cells, umi_correct, (str(out_dir).encode(), num_threads))
        if call_cells is not None and call_cells is not False:
            kp = _knee_params(call_cells)
            cs, ks = np.zeros(_ffi.PA_BUS_CORRECT_STATS, np.uint64), np.zeros(_ffi.PA_KNEE_STATS, np.uint64)
            check(lib().pa_write_bus_called(self._h, host_index._h, str(r1).encode(), str(r2).encode(), str(whitelist).encode() if whitelist is not None else None, bc_len,
                                            umi_len, C.byref(kp), str(out_dir).encode(), num_threads, st.ctypes.data, cs.ctypes.data, ks.ctypes.data))
            out = dict(zip(_ffi.BUS_STAT_NAMES, (int(x) for x in st)))
            out["correct"] = dict(zip(_ffi.CORRECT_STAT_NAMES, (int(x) for x in cs)))
            out["knee"] = dict(zip(_ffi.KNEE_STAT_NAMES, (int(x) for x in ks)))
            return out
        if whitelist is not None:
            cs = np.zeros(_ffi.PA_BUS_CORRECT_STATS, np.uint64)
            check(lib().pa_write_bus_corrected(self._h, host_index._h, str(r1).encode(), str(r2).encode(), str(whitelist).encode(), bc_len, umi_len,
                                               str(out_dir).encode(), num_threads, st.ctypes.data, cs.ctypes.data))
            out = dict(zip(_ffi.BUS_STAT_NAMES, (int(x) for x in st)))
            out["correct"] = dict(zip(_ffi.CORRECT_STAT_NAMES, (int(x) for x in cs)))
            return out
        check(lib().pa_write_bus(self._h, host_index._h, str(r1).encode(), str(r2).encode(), bc_len, umi_len, str(out_dir).encode(), num_threads,
                                 st.ctypes.data))
        return dict(zip(_ffi.BUS_STAT_NAMES, (int(x) for x in st)))

    def count_cells_em(self, host_index: HostIndex, r1: str, r2: str, out_dir: str, bc_len: int = 16, umi_len: int = 12, num_threads: int = 0,
                       whitelist: Optional[str] = None, call_cells=None, umi_correct: Optional[str] = None, **params) -> dict:
        """Paired R1 (barcode + UMI) / R2 (cDNA) FASTQ -> out_dir/matrix.mtx (real values), barcodes.tsv, features.tsv (pa_count_cells_em):
        write_bus's records, never written, shared out over genes by a per-cell EM (GeneCounter). params: GeneCounter's. Returns the stats
        (GeneCounter.stats). With `whitelist` (the path of a barcode whitelist file) the barcodes are corrected against it before the
        gene stage (pa_count_cells_em_corrected), and the stats hold the correction's under "correct". With `call_cells` (True or a dict of
        knee params) cells are called before the gene stage as write_bus calls them (pa_count_cells_em_called): the matrix is the filtered
        one, out_dir/barcode_ranks.tsv holds the table, and the stats hold the knee's under "knee". With `umi_correct` ("greatest" or
        "directional") the UMIs are corrected after those steps and before the gene stage (pa_count_cells_em_umi), and the stats hold that
        step's under "umi"."""
        p = _genes_params(params)
        st = np.zeros(_ffi.PA_GENES_STATS, np.uint64)
        if umi_correct is not None:
            return self._umi_call(lambda *a: lib().pa_count_cells_em_umi(self._h, host_index._h, str(r1).encode(), str(r2).encode(), *a), st, _ffi.GENES_STAT_NAMES, whitelist,
                                  bc_len, umi_len, call_cells, umi_correct, (C.byref(p), str(out_dir).encode(), num_threads))
        if call_cells is not None and call_cells is not False:
            kp = _knee_params(call_cells)
            cs, ks = np.zeros(_ffi.PA_BUS_CORRECT_STATS, np.uint64), np.zeros(_ffi.PA_KNEE_STATS, np.uint64)
            check(lib().pa_count_cells_em_called(self._h, host_index._h, str(r1).encode(), str(r2).encode(), str(whitelist).encode() if whitelist is not None else None,
                                                 bc_len, umi_len, C.byref(kp), C.byref(p), str(out_dir).encode(), num_threads, st.ctypes.data, cs.ctypes.data, ks.ctypes.data))
            out = dict(zip(_ffi.GENES_STAT_NAMES, (int(x) for x in st)))
            out["correct"] = dict(zip(_ffi.CORRECT_STAT_NAMES, (int(x) for x in cs)))
            out["knee"] = dict(zip(_ffi.KNEE_STAT_NAMES, (int(x) for x in ks)))
            return out
        if whitelist is not None:
            cs = np.zeros(_ffi.PA_BUS_CORRECT_STATS, np.uint64)
            check(lib().pa_count_cells_em_corrected(self._h, host_index._h, str(r1).encode(), str(r2).encode(), str(whitelist).encode(), bc_len, umi_len, C.byref(p),
                                                    str(out_dir).encode(), num_threads, st.ctypes.data, cs.ctypes.data))
            out = dict(zip(_ffi.GENES_STAT_NAMES, (int(x) for x in st)))
            out["correct"] = dict(zip(_ffi.CORRECT_STAT_NAMES, (int(x) for x in cs)))
            return out
        check(lib().pa_count_cells_em(self._h, host_index._h, str(r1).encode(), str(r2).encode(), bc_len, umi_len, C.byref(p), str(out_dir).encode(), num_threads,
                                      st.ctypes.data))
        return dict(zip(_ffi.GENES_STAT_NAMES, (int(x) for x in st)))

    @staticmethod
    def _umi_call(call, st, names, whitelist, bc_len, umi_len, call_cells, umi_correct, tail) -> dict:
        """the arguments that pa_write_bus_umi and pa_count_cells_em_umi share, and their stats: "correct" / "knee" only for a step that ran"""
        calling = call_cells is not None and call_cells is not False
        kp = _knee_params(call_cells if calling else True)
        cs, ks, us = np.zeros(_ffi.PA_BUS_CORRECT_STATS, np.uint64), np.zeros(_ffi.PA_KNEE_STATS, np.uint64), np.zeros(_ffi.PA_BUS_UMI_STATS, np.uint64)
        check(call(str(whitelist).encode() if whitelist is not None else None, bc_len, umi_len, 1 if calling else 0, C.byref(kp), _umi_mode(umi_correct), *tail, st.ctypes.data,
                   cs.ctypes.data, ks.ctypes.data, us.ctypes.data))
        out = dict(zip(names, (int(x) for x in st)))
        if whitelist is not None or calling:
            out["correct"] = dict(zip(_ffi.CORRECT_STAT_NAMES, (int(x) for x in cs)))
        if calling:
            out["knee"] = dict(zip(_ffi.KNEE_STAT_NAMES, (int(x) for x in ks)))
        out["umi"] = dict(zip(_ffi.UMI_STAT_NAMES, (int(x) for x in us)))
        return out

    def quantify(self, d_counts: int, overflow: Optional["Overflow"] = None, **params) -> "Quantifier":
        """Transcript abundances from a class-count table on this GPU (d_counts: the device pointer the count launches accumulated into,
        their streams synchronised) and, optionally, the overflow table that was attached: copies the table back, fetches the overflow,
        runs the EM to its stop rule and returns the Quantifier (fetch / genes / write_tsv; .iterations, .converged)."""
        counts = np.zeros(self.counts_len(), np.uint64)
        check(lib().pa_memcpy_d2h(counts.ctypes.data, d_counts, counts.nbytes, None))
        check(lib().pa_stream_synchronize(None))
        q = Quantifier(self, self.host, **params)
        q.set_counts(counts, overflow.fetch() if overflow is not None else None)
        q.iterations, q.converged = q.run()
        return q

    def set_overflow(self, overflow: Optional["Overflow"]) -> None:
        """attach the table that remembers WHICH novel classes the fused count launches met (None detaches)"""
        check(lib().pa_index_set_overflow(self._h, overflow._h if overflow else None))
        self._overflow = overflow   # keep it alive while attached

    def counts_allreduce(self, d_counts: int, comm: Optional["Comm"], stream: int = 0) -> None:
        """RCCL all-reduce (sum) of the dense count table, in place"""
        check(lib().pa_counts_allreduce(self._h, d_counts, comm._h if comm else None, stream or None))

    def counts_accumulate_device(self, d_results: int, d_arena: int, d_colour: int, n_reads: int, d_counts: int, stream: int = 0) -> None:
        check(lib().pa_counts_accumulate_device(self._h, d_results, d_arena, d_colour or None, n_reads, d_counts, stream or None))

    # ---- paired-end reads (include/pseudoaligner_amd.h, "paired-end reads") -------------------------
    def revcomp_tiles_device(self, d_tiles_in: int, d_lens: int, n_reads: int, words_per_read: int, d_tiles_out: int, stream: int = 0) -> None:
        """reverse complement of packed reads in the tile layout, not in place (raw device pointers; asynchronous)"""
        check(lib().pa_revcomp_tiles_device(self._h, d_tiles_in or None, d_lens or None, n_reads, words_per_read, d_tiles_out or None, stream or None))

    @staticmethod
    def pairs_scratch_bytes(n_pairs: int) -> int:
        return lib().pa_pairs_scratch_bytes(n_pairs)

    def pairs_combine_device(self, d_res1: int, d_arena1: int, d_res2: int, d_arena2: int, n_pairs: int, d_results: int, d_arena: int, arena_cap: int,
                             d_scratch: int, scratch_bytes: int, d_counts: int = 0, stream: int = 0) -> None:
        """the two mates' records (two finished map_batch_device launches) -> one record per pair + ids in the pair arena; asynchronous"""
        check(lib().pa_pairs_combine_device(self._h, d_res1 or None, d_arena1 or None, d_res2 or None, d_arena2 or None, n_pairs, d_results or None,
                                            d_arena or None, arena_cap, d_counts or None, d_scratch or None, scratch_bytes, stream or None))

    def pairs_finish(self, d_scratch: int, stream: int = 0) -> Tuple[dict, int, int]:
        """waits for pairs_combine_device -> (stats, arena_used, arena_needed); a full arena raises PaError(PA_ERR_ARENA_FULL) whose
        .arena_needed is the capacity that suffices and .stats the launch's stats"""
        st = np.zeros(_ffi.PA_PAIR_STATS, np.uint64)
        used, need = C.c_uint64(), C.c_uint64()
        rc = lib().pa_pairs_finish(self._h, d_scratch or None, stream or None, st.ctypes.data, C.byref(used), C.byref(need))
        stats = dict(zip(_ffi.PAIR_STAT_NAMES, (int(x) for x in st)))
        if rc == PA_ERR_ARENA_FULL:
            err = PaError(rc, (lib().pa_last_error() or b"").decode("utf-8", "replace"))
            err.arena_needed, err.stats = need.value, stats
            raise err
        check(rc)
        return stats, used.value, need.value

    # ---- unstranded libraries (include/pseudoaligner_amd.h, "unstranded libraries") ------------------
    @staticmethod
    def strands_scratch_bytes(n: int) -> int:
        return lib().pa_strands_scratch_bytes(n)

    def strands_merge_device(self, d_res_s: int, d_arena_s: int, d_res_r: int, d_arena_r: int, n: int, d_results: int, d_arena: int, arena_cap: int,
                             d_scratch: int, scratch_bytes: int, d_counts: int = 0, stream: int = 0) -> None:
        """the sense and the antisense candidate of every item (records + arenas) -> one record per item + ids in the output arena; asynchronous"""
        check(lib().pa_strands_merge_device(self._h, d_res_s or None, d_arena_s or None, d_res_r or None, d_arena_r or None, n, d_results or None,
                                            d_arena or None, arena_cap, d_counts or None, d_scratch or None, scratch_bytes, stream or None))

    def strands_finish(self, d_scratch: int, stream: int = 0) -> Tuple[dict, int, int]:
        """waits for strands_merge_device -> (stats, arena_used, arena_needed); a full arena raises PaError(PA_ERR_ARENA_FULL) whose
        .arena_needed is the capacity that suffices and .stats the launch's stats"""
        st = np.zeros(_ffi.PA_STRAND_STATS, np.uint64)
        used, need = C.c_uint64(), C.c_uint64()
        rc = lib().pa_strands_finish(self._h, d_scratch or None, stream or None, st.ctypes.data, C.byref(used), C.byref(need))
        stats = dict(zip(_ffi.STRAND_STAT_NAMES, (int(x) for x in st)))
        if rc == PA_ERR_ARENA_FULL:
            err = PaError(rc, (lib().pa_last_error() or b"").decode("utf-8", "replace"))
            err.arena_needed, err.stats = need.value, stats
            raise err
        check(rc)
        return stats, used.value, need.value

    def map_pairs(self, reads1: Sequence, reads2: Sequence, orient: str = "fr", allowed_mismatches: int = PA_DEFAULT_ALLOWED_MISMATCHES):
        """map_batch for read pairs: mates oriented ("fr": mate 2 reverse-complemented, "rf": mate 1, "ff": neither), mapped, their classes
        intersected; "un": an unstranded library, "fr" and "rf" both and the two answers merged -> (results[n] RESULT_DTYPE, class_offsets[n+1], class_ids) in pair order"""
        if orient != "un" and orient not in _ffi.PAIR_ORIENTATIONS:
            raise ValueError("orient %r: one of %s" % (orient, sorted(_ffi.PAIR_ORIENTATIONS) + ["un"]))
        d1, o1 = reads1 if isinstance(reads1, tuple) else concat_reads(reads1)
        d2, o2 = reads2 if isinstance(reads2, tuple) else concat_reads(reads2)
        if len(o1) != len(o2):
            raise ValueError("%d first mates, %d second mates" % (len(o1) - 1, len(o2) - 1))
        n = len(o1) - 1
        results = np.zeros(n, dtype=RESULT_DTYPE)
        coff = np.zeros(n + 1, dtype=np.uint64)
        ids = vp()
        if orient == "un":   # an unstranded library: both orientations mapped, the two answers merged
            check(lib().pa_map_pairs_unstranded(self._h, d1.ctypes.data, o1.ctypes.data, d2.ctypes.data, o2.ctypes.data, n, allowed_mismatches,
                                                results.ctypes.data, coff.ctypes.data, C.byref(ids)))
            return results, coff, _np_view(ids.value, int(coff[-1]), np.uint32).copy()
        check(lib().pa_map_pairs(self._h, d1.ctypes.data, o1.ctypes.data, d2.ctypes.data, o2.ctypes.data, n, _ffi.PAIR_ORIENTATIONS[orient], allowed_mismatches,
                                 results.ctypes.data, coff.ctypes.data, C.byref(ids)))
        return results, coff, _np_view(ids.value, int(coff[-1]), np.uint32).copy()

    def count_pairs(self, r1: str, r2: str, orient: str = "fr", allowed_mismatches: int = PA_DEFAULT_ALLOWED_MISMATCHES, num_threads: int = 0):
        """pa_count_pairs: two FASTQ files (plain or gzip'ed) -> (class-count table uint64[counts_len()], stats dict); an attached overflow
        table receives the novel results, so that Quantifier.set_counts(counts, overflow.fetch()) takes the pair"""
        if orient != "un" and orient not in _ffi.PAIR_ORIENTATIONS:
            raise ValueError("orient %r: one of %s" % (orient, sorted(_ffi.PAIR_ORIENTATIONS) + ["un"]))
        counts = np.zeros(self.counts_len(), np.uint64)
        st = np.zeros(_ffi.PA_PAIR_STATS, np.uint64)
        n = C.c_uint64()
        if orient == "un":   # pa_count_pairs_unstranded: the stats are the merge's (STRAND_STAT_NAMES)
            check(lib().pa_count_pairs_unstranded(self._h, str(r1).encode(), str(r2).encode(), allowed_mismatches, num_threads, counts.ctypes.data, C.byref(n),
                                                  st.ctypes.data))
            return counts, dict(zip(_ffi.STRAND_STAT_NAMES, (int(x) for x in st)))
        check(lib().pa_count_pairs(self._h, str(r1).encode(), str(r2).encode(), _ffi.PAIR_ORIENTATIONS[orient], allowed_mismatches, num_threads,
                                   counts.ctypes.data, C.byref(n), st.ctypes.data))
        return counts, dict(zip(_ffi.PAIR_STAT_NAMES, (int(x) for x in st)))

    def encode_reads_device(self, d_ascii: int, d_offsets: int, n_reads: int, words_per_read: int, d_tiles: int, d_lens: int, stream: int = 0):
        check(lib().pa_encode_reads_device(self._h, d_ascii, d_offsets, n_reads, words_per_read, d_tiles, d_lens, stream or None))

    def __del__(self):
        try:
            if self._h:
                lib().pa_index_destroy(self._h)
                self._h = vp()
        except Exception:
            pass


def load_whitelist(path: str, bc_len: int) -> List[str]:
    """pa_whitelist_load: the barcodes of a whitelist file (plain or gzip'ed), line i = cell i"""
    n = C.c_uint64()
    check(lib().pa_whitelist_load(str(path).encode(), bc_len, None, 0, C.byref(n)))
    buf = C.create_string_buffer(max(n.value * bc_len, 1))
    check(lib().pa_whitelist_load(str(path).encode(), bc_len, buf, n.value, C.byref(n)))
    raw = buf.raw[: n.value * bc_len].decode()
    return [raw[i * bc_len:(i + 1) * bc_len] for i in range(n.value)]


class CellCounter:
    """Single-cell UMI counter on the index's GPU (pa_cell_counter): feed it device-resident batches (the mapping's records of the
    R2s + the R1s), then finish() and read the (cell, gene) -> UMIs matrix."""

    def __init__(self, aligner: "Pseudoaligner", host_index: HostIndex, tx_gene, num_genes: int, whitelist: Sequence[str],
                 bc_len: int = 16, umi_len: int = 12):
        self._h = vp()
        tg = np.ascontiguousarray(tx_gene, np.uint32)
        wl = "".join(whitelist).encode()
        self._aligner = aligner   # the index outlives the counter
        check(lib().pa_cell_counter_create(aligner._h if aligner is not None else None, host_index._h if host_index is not None else None,
                                           tg.ctypes.data, num_genes, wl, len(whitelist), bc_len, umi_len, C.byref(self._h)))

    def add_device(self, d_results: int, d_arena: int, d_r1: int, d_r1_offsets: int, n_reads: int, stream: int = 0) -> None:
        check(lib().pa_cell_counter_add_device(self._h, d_results, d_arena, d_r1, d_r1_offsets, n_reads, stream or None))

    def finish(self) -> int:
        n = C.c_uint64()
        check(lib().pa_cell_counter_finish(self._h, C.byref(n)))
        return n.value

    def matrix(self) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(cell, gene, umis) after finish, sorted by (cell, gene)"""
        n = self.finish()
        cell, gene, umis = (np.zeros(max(n, 1), np.uint32) for _ in range(3))
        check(lib().pa_cell_counter_matrix(self._h, cell.ctypes.data, gene.ctypes.data, umis.ctypes.data, n))
        return cell[:n], gene[:n], umis[:n]

    def stats(self) -> dict:
        st = np.zeros(_ffi.PA_CELL_STATS, np.uint64)
        check(lib().pa_cell_counter_stats(self._h, st.ctypes.data))
        return dict(zip(_ffi.CELL_STAT_NAMES, (int(x) for x in st)))

    def __del__(self):
        try:
            if self._h:
                lib().pa_cell_counter_destroy(self._h)
                self._h = vp()
        except Exception:
            pass


BUS_RECORD_DTYPE = np.dtype([("barcode", "<u8"), ("umi", "<u8"), ("ec", "<i4"), ("count", "<u4"), ("flags", "<u4"), ("pad", "<u4")])   # pa_bus_record


class BusWriter:
    """Sorted (barcode, UMI, equivalence class) records on the index's GPU (pa_bus): feed it device-resident batches (the mapping's
    records of the R2s + the R1s), then finish() and read records() / ecs(), or write() the three files of a BUS run."""

    def __init__(self, aligner: "Pseudoaligner", host_index: HostIndex, bc_len: int = 16, umi_len: int = 12):
        self._h = vp()
        self._aligner, self._host = aligner, host_index   # the index and the host index outlive the writer
        check(lib().pa_bus_create(aligner._h if aligner is not None else None, host_index._h if host_index is not None else None, bc_len, umi_len,
                                  C.byref(self._h)))

    def add_device(self, d_results: int, d_arena: int, arena_len: int, d_r1: int, d_r1_offsets: int, n_reads: int, stream: int = 0) -> None:
        check(lib().pa_bus_add_device(self._h, d_results, d_arena, arena_len, d_r1, d_r1_offsets, n_reads, stream or None))

    def finish(self) -> Tuple[int, int]:
        """(records, ecs)"""
        n, e = C.c_uint64(), C.c_uint32()
        check(lib().pa_bus_finish(self._h, C.byref(n), C.byref(e)))
        return n.value, e.value

    def records(self) -> np.ndarray:
        """the records after finish (BUS_RECORD_DTYPE), ascending by barcode, UMI, ec"""
        n, _ = self.finish()
        out = np.zeros(max(n, 1), BUS_RECORD_DTYPE)
        check(lib().pa_bus_records(self._h, out.ctypes.data, n))
        return out[:n]

    def ecs(self) -> Tuple[np.ndarray, np.ndarray]:
        """(offsets[n_ecs + 1], ids): ec e = ids[offsets[e]:offsets[e + 1]]"""
        _, n_ecs = self.finish()
        n_ids = C.c_uint64()
        check(lib().pa_bus_ecs(self._h, None, None, 0, C.byref(n_ids)))
        off, ids = np.zeros(n_ecs + 1, np.uint64), np.zeros(max(n_ids.value, 1), np.uint32)
        check(lib().pa_bus_ecs(self._h, off.ctypes.data, ids.ctypes.data, n_ids.value, C.byref(n_ids)))
        return off, ids[:n_ids.value]

    def stats(self) -> dict:
        st = np.zeros(_ffi.PA_BUS_STATS, np.uint64)
        check(lib().pa_bus_stats(self._h, st.ctypes.data))
        return dict(zip(_ffi.BUS_STAT_NAMES, (int(x) for x in st)))

    def correct(self, whitelist) -> dict:
        """pa_bus_correct: the barcodes of the finished records (finished here if they are not yet) corrected against `whitelist` (barcode
        strings, or packed values as bus_whitelist_pack gives them) in place, collapsed again -> the stats (CORRECT_STAT_NAMES)"""
        self.finish()
        wl = _packed_whitelist(whitelist)
        st = np.zeros(_ffi.PA_BUS_CORRECT_STATS, np.uint64)
        check(lib().pa_bus_correct(self._h, wl.ctypes.data if len(wl) else None, len(wl), st.ctypes.data))
        return dict(zip(_ffi.CORRECT_STAT_NAMES, (int(x) for x in st)))

    def knee(self, **params) -> Tuple[np.ndarray, np.ndarray, dict]:
        """pa_bus_knee: the barcode table of the finished records (finished here if they are not yet), ranked by molecules, and the barcodes
        the threshold rule calls -> (rows as BARCODE_ROW_DTYPE in ascending barcode order, the called barcodes packed and ascending, the
        stats (KNEE_STAT_NAMES)). params: the fields of pa_knee_params (mode = "curve" | "expected" | "min", lower, divisor, expected_cells,
        min_umis); what is not given keeps the library's default. The writer is unchanged; correct(called) or keep(called) apply the call."""
        self.finish()
        p = _knee_params(params)
        return _knee_call(lambda *out: lib().pa_bus_knee(self._h, C.byref(p), *out))

    def keep(self, barcodes) -> dict:
        """pa_bus_keep: only the records whose barcode is in `barcodes` (packed values, strictly ascending) stay, in place; no neighbour is
        rescued and nothing is sorted or joined -> the stats (KEEP_STAT_NAMES)"""
        self.finish()
        bc = np.ascontiguousarray(barcodes, np.uint64)
        st = np.zeros(_ffi.PA_BUS_KEEP_STATS, np.uint64)
        check(lib().pa_bus_keep(self._h, bc.ctypes.data if len(bc) else None, len(bc), st.ctypes.data))
        return dict(zip(_ffi.KEEP_STAT_NAMES, (int(x) for x in st)))

    def umi_correct(self, tx_gene=None, mode="greatest", num_genes: Optional[int] = None) -> dict:
        """pa_bus_umi_correct: the UMIs of the finished records (finished here if they are not yet) corrected in place, one step: a molecule moves
        to the best-supported molecule of its barcode whose UMI is one substitution away and whose gene set meets its own -> the stats
        (UMI_STAT_NAMES). tx_gene[transcripts] (with num_genes) defaults to the host index's genes; mode: "greatest" | "directional"."""
        self.finish()
        if tx_gene is None:
            tx_gene, names = self._host.genes()
            num_genes = len(names)
        tg = np.ascontiguousarray(tx_gene, np.uint32)
        if num_genes is None:
            num_genes = int(tg.max()) + 1 if len(tg) else 0
        st = np.zeros(_ffi.PA_BUS_UMI_STATS, np.uint64)
        check(lib().pa_bus_umi_correct(self._h, tg.ctypes.data if len(tg) else None, num_genes, _umi_mode(mode), st.ctypes.data))
        return dict(zip(_ffi.UMI_STAT_NAMES, (int(x) for x in st)))

    def write(self, out_dir: str) -> None:
        """out_dir/output.bus, matrix.ec, transcripts.txt"""
        self.finish()
        check(lib().pa_bus_write(self._h, str(out_dir).encode()))

    def __del__(self):
        try:
            if self._h:
                lib().pa_bus_destroy(self._h)
                self._h = vp()
        except Exception:
            pass


CORRECT_STAT_NAMES = _ffi.CORRECT_STAT_NAMES


def bus_whitelist_pack(whitelist: Sequence[str]) -> np.ndarray:
    """pa_bus_whitelist_pack: barcode strings of one length -> uint64, 2 bits per base, A=0 C=1 G=2 T=3, first base most significant"""
    wl = list(whitelist)
    bc_len = len(wl[0]) if wl else 1
    if any(len(b) != bc_len for b in wl):
        raise ValueError("the barcodes of a whitelist have one length")
    out = np.zeros(max(len(wl), 1), np.uint64)
    check(lib().pa_bus_whitelist_pack("".join(wl).encode(), len(wl), bc_len, out.ctypes.data))
    return out[:len(wl)]


def _packed_whitelist(whitelist) -> np.ndarray:
    if isinstance(whitelist, np.ndarray):
        return np.ascontiguousarray(whitelist, np.uint64)
    wl = list(whitelist)
    return bus_whitelist_pack(wl) if wl and isinstance(wl[0], str) else np.ascontiguousarray(wl, np.uint64)


def bus_correct(records, whitelist, bc_len: int, umi_len: int, index: Optional["Pseudoaligner"]) -> Tuple[np.ndarray, dict]:
    """pa_bus_correct_records: host records (BUS_RECORD_DTYPE, strictly ascending by barcode, UMI, ec) corrected against `whitelist`
    (barcode strings or packed values) on `index`'s GPU -> (the corrected records, collapsed and sorted again; the stats)"""
    rec = np.ascontiguousarray(records, BUS_RECORD_DTYPE)
    wl = _packed_whitelist(whitelist)
    st = np.zeros(_ffi.PA_BUS_CORRECT_STATS, np.uint64)
    out = np.zeros(max(len(rec), 1), BUS_RECORD_DTYPE)
    n = C.c_uint64()
    check(lib().pa_bus_correct_records(index._h if index is not None else None, rec.ctypes.data if len(rec) else None, len(rec), bc_len, umi_len,
                                       wl.ctypes.data if len(wl) else None, len(wl), out.ctypes.data, len(rec), C.byref(n), st.ctypes.data))
    return out[:n.value], dict(zip(_ffi.CORRECT_STAT_NAMES, (int(x) for x in st)))


def bus_correct_phase_ms() -> dict:
    """pa_bus_correct_phase_ms: the GPU milliseconds of this thread's last correction, by phase"""
    ms = (C.c_float * _ffi.PA_BUS_CORRECT_PHASES)()
    check(lib().pa_bus_correct_phase_ms(ms))
    return dict(zip(_ffi.CORRECT_PHASE_NAMES, (float(x) for x in ms)))


UMI_STAT_NAMES, UMI_PHASE_NAMES = _ffi.UMI_STAT_NAMES, _ffi.UMI_PHASE_NAMES


def _umi_mode(mode) -> int:
    """"greatest" | "directional", or the number itself (an unknown one is the library's to refuse)"""
    if isinstance(mode, str):
        if mode not in _ffi.UMI_MODES:
            raise ValueError("umi_correct: %r is neither 'greatest' nor 'directional'" % mode)
        return _ffi.UMI_MODES[mode]
    return int(mode)


def bus_umi_correct(records, ec_offsets, ec_ids, tx_gene, num_genes: int, bc_len: int, umi_len: int, aligner: Optional["Pseudoaligner"], mode="greatest") -> Tuple[np.ndarray, dict]:
    """pa_bus_umi_correct_records: host records (BUS_RECORD_DTYPE, strictly ascending by barcode, UMI, ec) with their ec table as a CSR and
    tx_gene, as GeneCounter.from_arrays takes them, on `aligner`'s GPU -> (the records with the UMIs corrected, collapsed and sorted again; the
    stats (UMI_STAT_NAMES))"""
    rec = np.ascontiguousarray(records, BUS_RECORD_DTYPE)
    off = np.ascontiguousarray(ec_offsets, np.uint64)
    ids = np.ascontiguousarray(ec_ids, np.uint32)
    tg = np.ascontiguousarray(tx_gene, np.uint32)
    st = np.zeros(_ffi.PA_BUS_UMI_STATS, np.uint64)
    out = np.zeros(max(len(rec), 1), BUS_RECORD_DTYPE)
    n = C.c_uint64()
    check(lib().pa_bus_umi_correct_records(aligner._h if aligner is not None else None, rec.ctypes.data if len(rec) else None, len(rec), off.ctypes.data if len(off) else None,
                                           ids.ctypes.data if len(ids) else None, max(len(off), 1) - 1, len(tg), tg.ctypes.data if len(tg) else None, num_genes, bc_len, umi_len,
                                           _umi_mode(mode), out.ctypes.data, len(rec), C.byref(n), st.ctypes.data))
    return out[:n.value], dict(zip(_ffi.UMI_STAT_NAMES, (int(x) for x in st)))


def bus_umi_correct_phase_ms() -> dict:
    """pa_bus_umi_correct_phase_ms: the GPU milliseconds of this thread's last UMI correction, by phase"""
    ms = (C.c_float * _ffi.PA_BUS_UMI_PHASES)()
    check(lib().pa_bus_umi_correct_phase_ms(ms))
    return dict(zip(_ffi.UMI_PHASE_NAMES, (float(x) for x in ms)))


BARCODE_ROW_DTYPE = np.dtype([("barcode", "<u8"), ("reads", "<u8"), ("records", "<u4"), ("umis", "<u4"), ("rank", "<u4"), ("called", "<u4")])   # pa_bus_barcode_row
KNEE_STAT_NAMES, KEEP_STAT_NAMES = _ffi.KNEE_STAT_NAMES, _ffi.KEEP_STAT_NAMES


def _knee_params(params) -> "_ffi.KneeParams":
    """True or an empty dict: the defaults; else the fields of pa_knee_params by name"""
    p = _ffi.KneeParams()
    lib().pa_knee_default_params(C.byref(p))
    for name, value in ({} if params is True else dict(params)).items():
        if name not in dict(_ffi.KneeParams._fields_) or name == "reserved":
            raise TypeError("unknown knee parameter %r" % name)
        setattr(p, name, _ffi.KNEE_MODES[value] if name == "mode" and isinstance(value, str) else value)
    return p


def _knee_call(call) -> Tuple[np.ndarray, np.ndarray, dict]:
    """call(rows, rows_cap, n_rows, called, called_cap, n_called, stats): once for the sizes, once for the arrays"""
    n_rows, n_called = C.c_uint64(), C.c_uint64()
    st = np.zeros(_ffi.PA_KNEE_STATS, np.uint64)
    check(call(None, 0, C.byref(n_rows), None, 0, C.byref(n_called), st.ctypes.data))
    rows, called = np.zeros(max(n_rows.value, 1), BARCODE_ROW_DTYPE), np.zeros(max(n_called.value, 1), np.uint64)
    check(call(rows.ctypes.data, n_rows.value, C.byref(n_rows), called.ctypes.data, n_called.value, C.byref(n_called), st.ctypes.data))
    return rows[:n_rows.value], called[:n_called.value], dict(zip(_ffi.KNEE_STAT_NAMES, (int(x) for x in st)))


def bus_knee(records, bc_len: int, umi_len: int, index: Optional["Pseudoaligner"], **params) -> Tuple[np.ndarray, np.ndarray, dict]:
    """pa_bus_knee_records: host records (BUS_RECORD_DTYPE, strictly ascending by barcode, UMI, ec) on `index`'s GPU -> (rows, called, stats) as
    BusWriter.knee gives them"""
    rec = np.ascontiguousarray(records, BUS_RECORD_DTYPE)
    p = _knee_params(params)
    return _knee_call(lambda *out: lib().pa_bus_knee_records(index._h if index is not None else None, rec.ctypes.data if len(rec) else None, len(rec), bc_len, umi_len,
                                                             C.byref(p), *out))


def bus_keep(records, barcodes, bc_len: int, umi_len: int, index: Optional["Pseudoaligner"]) -> Tuple[np.ndarray, dict]:
    """pa_bus_keep_records: the host records whose barcode is in `barcodes` (packed values, strictly ascending), in their order -> (records, stats)"""
    rec = np.ascontiguousarray(records, BUS_RECORD_DTYPE)
    bc = np.ascontiguousarray(barcodes, np.uint64)
    st = np.zeros(_ffi.PA_BUS_KEEP_STATS, np.uint64)
    out = np.zeros(max(len(rec), 1), BUS_RECORD_DTYPE)
    n = C.c_uint64()
    check(lib().pa_bus_keep_records(index._h if index is not None else None, rec.ctypes.data if len(rec) else None, len(rec), bc_len, umi_len,
                                    bc.ctypes.data if len(bc) else None, len(bc), out.ctypes.data, len(rec), C.byref(n), st.ctypes.data))
    return out[:n.value], dict(zip(_ffi.KEEP_STAT_NAMES, (int(x) for x in st)))


def bus_knee_phase_ms() -> dict:
    """pa_bus_knee_phase_ms: the GPU milliseconds of this thread's last knee, by phase"""
    ms = (C.c_float * _ffi.PA_KNEE_PHASES)()
    check(lib().pa_bus_knee_phase_ms(ms))
    return dict(zip(_ffi.KNEE_PHASE_NAMES, (float(x) for x in ms)))


def write_barcode_ranks_tsv(rows, bc_len: int, path: str) -> None:
    """pa_write_barcode_ranks_tsv: the rows of a knee as barcode_ranks.tsv"""
    r = np.ascontiguousarray(rows, BARCODE_ROW_DTYPE)
    check(lib().pa_write_barcode_ranks_tsv(r.ctypes.data if len(r) else None, len(r), bc_len, str(path).encode()))


def _genes_params(params: dict) -> "_ffi.GenesParams":
    p = _ffi.GenesParams()
    lib().pa_genes_default_params(C.byref(p))
    for name, value in params.items():
        if name not in dict(_ffi.GenesParams._fields_) or name == "reserved":
            raise TypeError("unknown gene counter parameter %r" % name)
        setattr(p, name, _ffi.GENES_MODES[value] if name == "mode" and isinstance(value, str) else value)
    return p


class GeneCounter:
    """Cells x genes from BUS records on the index's GPU (pa_genes): molecules whose records agree on one gene count for it, the others
    are shared out by an EM per cell. from_bus() / from_arrays(), then step() / run(), then values() / matrix() / write(). params: the fields
    of pa_genes_params (alpha_limit, alpha_change_limit, alpha_change, min_iters, max_iters, check_every, mode = "em" | "unique"); what is
    not given keeps the library's default."""

    def __init__(self):
        self._h = vp()
        self._keep = ()

    @classmethod
    def from_bus(cls, writer: "BusWriter", tx_gene, num_genes: int, **params) -> "GeneCounter":
        """the records of a BusWriter (finished here if it is not yet) where they lie in HBM, with the writer's ec table;
        tx_gene[transcripts] < num_genes (HostIndex.genes())"""
        g = cls()
        if writer is not None:
            writer.finish()
        p = _genes_params(params)
        tg = np.ascontiguousarray(tx_gene, np.uint32)
        g.params = p
        check(lib().pa_genes_create_from_bus(writer._h if writer is not None else None, tg.ctypes.data if len(tg) else None, num_genes, C.byref(p), C.byref(g._h)))
        g._keep = (writer._aligner,)
        return g

    @classmethod
    def from_arrays(cls, aligner: "Pseudoaligner", records, ec_offsets, ec_ids, tx_gene, num_genes: int, bc_len: int, umi_len: int, **params) -> "GeneCounter":
        """host arrays of any origin: records (BUS_RECORD_DTYPE, strictly ascending by barcode, UMI, ec), the ec table as a CSR, tx_gene.
        The files of a BUS run, for instance:
            records = np.fromfile("output.bus", BUS_RECORD_DTYPE, offset=20)        # 20 header bytes when tlen = 0
            lists = [[int(t) for t in line.split("\t")[1].split(",")] for line in open("matrix.ec")]
            ec_offsets = np.cumsum([0] + [len(l) for l in lists]); ec_ids = np.concatenate(lists)"""
        g = cls()
        p = _genes_params(params)
        rec = np.ascontiguousarray(records, BUS_RECORD_DTYPE)
        off = np.ascontiguousarray(ec_offsets, np.uint64)
        ids = np.ascontiguousarray(ec_ids, np.uint32)
        tg = np.ascontiguousarray(tx_gene, np.uint32)
        g.params = p
        check(lib().pa_genes_create(aligner._h if aligner is not None else None, rec.ctypes.data if len(rec) else None, len(rec), off.ctypes.data if len(off) else None,
                                    ids.ctypes.data if len(ids) else None, max(len(off), 1) - 1, len(tg), tg.ctypes.data if len(tg) else None, num_genes, bc_len, umi_len,
                                    C.byref(p), C.byref(g._h)))
        g._keep = (aligner,)
        return g

    def step(self, n_iters: int = 1) -> None:
        """every cell with multi rows, exactly n iterations: no stop rule, no freeze"""
        check(lib().pa_genes_step(self._h, n_iters))

    def run(self) -> Tuple[int, int]:
        """the stop rule per cell + truncation -> (most iterations run by a cell, cells not converged)"""
        it, nc = C.c_uint32(), C.c_uint64()
        check(lib().pa_genes_run(self._h, C.byref(it), C.byref(nc)))
        return it.value, nc.value

    def layout(self) -> Tuple[int, int]:
        """(cells, values)"""
        nc, nv = C.c_uint64(), C.c_uint64()
        check(lib().pa_genes_layout(self._h, C.byref(nc), C.byref(nv)))
        return nc.value, nv.value

    def values(self) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
        """(barcode[cells], cell, gene, alpha): the current alpha of every (cell, gene) that has a row, sorted, zeros kept"""
        nc, nv = self.layout()
        bc, cell, gene, alpha = np.zeros(max(nc, 1), np.uint64), np.zeros(max(nv, 1), np.uint32), np.zeros(max(nv, 1), np.uint32), np.zeros(max(nv, 1), np.float64)
        check(lib().pa_genes_values(self._h, bc.ctypes.data, cell.ctypes.data, gene.ctypes.data, alpha.ctypes.data, nv))
        return bc[:nc], cell[:nv], gene[:nv], alpha[:nv]

    def cell_iters(self) -> np.ndarray:
        nc, _ = self.layout()
        it = np.zeros(max(nc, 1), np.uint32)
        check(lib().pa_genes_cell_iters(self._h, it.ctypes.data))
        return it[:nc]

    def matrix(self) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """after run(): (cell, gene, value) sorted by (cell, gene), zeros dropped"""
        n = C.c_uint64()
        check(lib().pa_genes_matrix(self._h, None, None, None, 0, C.byref(n)))
        cell, gene, value = np.zeros(max(n.value, 1), np.uint32), np.zeros(max(n.value, 1), np.uint32), np.zeros(max(n.value, 1), np.float64)
        check(lib().pa_genes_matrix(self._h, cell.ctypes.data, gene.ctypes.data, value.ctypes.data, n.value, C.byref(n)))
        return cell[:n.value], gene[:n.value], value[:n.value]

    def stats(self) -> dict:
        st = np.zeros(_ffi.PA_GENES_STATS, np.uint64)
        check(lib().pa_genes_stats(self._h, st.ctypes.data))
        return dict(zip(_ffi.GENES_STAT_NAMES, (int(x) for x in st)))

    def write(self, host_index: HostIndex, out_dir: str) -> None:
        """after run(): out_dir/matrix.mtx, barcodes.tsv, features.tsv"""
        check(lib().pa_genes_write(self._h, host_index._h if host_index is not None else None, str(out_dir).encode()))

    def __del__(self):
        try:
            if self._h:
                lib().pa_genes_destroy(self._h)
                self._h = vp()
        except Exception:
            pass


class Quantifier:
    """Transcript abundances by EM over the class-count table on the index's GPU (pa_quant): set_counts(), then step() / run(), then
    fetch() / genes() / write_tsv(). params: the fields of pa_quant_params (mean_read_len, alpha_limit, alpha_change_limit, alpha_change,
    min_iters, max_iters, check_every); what is not given keeps the library's default."""

    def __init__(self, aligner: "Pseudoaligner", host_index: HostIndex, **params):
        self._h = vp()
        p = _ffi.QuantParams()
        lib().pa_quant_default_params(C.byref(p))
        for name, value in params.items():
            if name not in dict(_ffi.QuantParams._fields_) or name == "reserved":
                raise TypeError("unknown quantification parameter %r" % name)
            setattr(p, name, value)
        self.params = p
        self._aligner, self._host = aligner, host_index   # the index outlives the quantifier
        self.num_transcripts = host_index.num_transcripts if host_index is not None else 0
        self._counts_len, self._n_records, self._boot_n = 0, 0, 0
        check(lib().pa_quant_create(aligner._h if aligner is not None else None, host_index._h if host_index is not None else None, C.byref(p),
                                    C.byref(self._h)))

    def set_counts(self, class_counts: np.ndarray, overflow: Optional[np.ndarray] = None) -> None:
        """class_counts: u64[counts_len()] on the host; overflow: the serialised overflow words (Overflow.fetch / allgather) or None"""
        cc = np.ascontiguousarray(class_counts, np.uint64)
        if overflow is None:
            check(lib().pa_quant_set_counts(self._h, cc.ctypes.data, len(cc), None, 0))
        else:
            w = np.ascontiguousarray(overflow, np.uint32)
            check(lib().pa_quant_set_counts(self._h, cc.ctypes.data, len(cc), w.ctypes.data, len(w)))
        self._counts_len, self._n_records, self._boot_n = len(cc), (int(w[0]) if overflow is not None else 0), 0   # what the bootstrap calls size their arrays by

    def step(self, n_iters: int = 1) -> None:
        check(lib().pa_quant_step(self._h, n_iters))

    def run(self) -> Tuple[int, bool]:
        """the stop rule + truncation from the current alpha -> (iterations, converged)"""
        it, conv = C.c_uint32(), C.c_int()
        check(lib().pa_quant_run(self._h, C.byref(it), C.byref(conv)))
        return it.value, bool(conv.value)

    def alpha(self) -> np.ndarray:
        a = np.zeros(max(self.num_transcripts, 1), np.float64)
        check(lib().pa_quant_alpha(self._h, a.ctypes.data))
        return a[: self.num_transcripts]

    def fetch(self) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(est_counts, tpm, eff_len), each [num_transcripts]"""
        est, tpm, eff = (np.zeros(max(self.num_transcripts, 1), np.float64) for _ in range(3))
        check(lib().pa_quant_fetch(self._h, est.ctypes.data, tpm.ctypes.data, eff.ctypes.data))
        n = self.num_transcripts
        return est[:n], tpm[:n], eff[:n]

    def genes(self) -> Tuple[np.ndarray, np.ndarray]:
        """(est_counts, tpm) per gene of HostIndex.genes()"""
        n = C.c_uint32()
        check(lib().pa_host_index_genes(self._host._h, None, C.byref(n)))
        est, tpm = np.zeros(max(n.value, 1), np.float64), np.zeros(max(n.value, 1), np.float64)
        check(lib().pa_quant_fetch_genes(self._h, est.ctypes.data, tpm.ctypes.data))
        return est[: n.value], tpm[: n.value]

    def stats(self) -> dict:
        st = np.zeros(_ffi.PA_QUANT_STATS, np.uint64)
        check(lib().pa_quant_stats(self._h, st.ctypes.data))
        return dict(zip(_ffi.QUANT_STAT_NAMES, (int(x) for x in st)))

    def write_tsv(self, path: str) -> None:
        check(lib().pa_write_abundance_tsv(self._h, str(path).encode()))

    # ---- bootstrap replicates (pa_quant_bootstrap_*): a batch of at most PA_QUANT_BOOT_MAX_BATCH resampled EM runs ----
    def bootstrap_draw(self, seed: int, first: int, n: int) -> None:
        """resample replicates first .. first + n - 1 of the table last set; their alpha goes to the start"""
        check(lib().pa_quant_bootstrap_draw(self._h, seed, first, n))
        self._boot_n = n

    def bootstrap_counts(self, k: int) -> Tuple[np.ndarray, np.ndarray]:
        """the k-th replicate of the batch -> (class_counts u64[counts_len], overflow counts u64[records] in record order)"""
        cc = np.zeros(self._counts_len, np.uint64)
        oc = np.zeros(max(self._n_records, 1), np.uint64)
        check(lib().pa_quant_bootstrap_counts(self._h, k, cc.ctypes.data, len(cc), oc.ctypes.data if self._n_records else None, self._n_records))
        return cc, oc[: self._n_records]

    def bootstrap_step(self, n_iters: int = 1) -> None:
        check(lib().pa_quant_bootstrap_step(self._h, n_iters))

    def bootstrap_run(self) -> Tuple[np.ndarray, np.ndarray]:
        """the stop rule per replicate -> (iterations u32[n], converged bool[n])"""
        it, conv = np.zeros(self._boot_n, np.uint32), np.zeros(self._boot_n, np.int32)
        check(lib().pa_quant_bootstrap_run(self._h, it.ctypes.data, conv.ctypes.data))
        return it, conv.astype(bool)

    def bootstrap_fetch(self) -> Tuple[np.ndarray, np.ndarray]:
        """(est_counts, tpm), each [n, num_transcripts]"""
        est, tpm = (np.zeros((self._boot_n, self.num_transcripts), np.float64) for _ in range(2))
        check(lib().pa_quant_bootstrap_fetch(self._h, est.ctypes.data, tpm.ctypes.data))
        return est, tpm

    def bootstrap(self, n: int, seed: int, batch: int = 32, run: bool = True) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """replicates 0 .. n - 1 in batches of `batch` -> (est_counts[n, T], iters[n], converged[n]); run=False: the start, no iteration"""
        est, iters, conv = np.zeros((n, self.num_transcripts)), np.zeros(n, np.uint32), np.zeros(n, bool)
        for first in range(0, n, batch):
            m = min(batch, n - first)
            self.bootstrap_draw(seed, first, m)
            if run:
                iters[first:first + m], conv[first:first + m] = self.bootstrap_run()
            est[first:first + m] = self.bootstrap_fetch()[0]
        return est, iters, conv

    def __del__(self):
        try:
            if self._h:
                lib().pa_quant_destroy(self._h)
                self._h = vp()
        except Exception:
            pass


def parse_overflow(words: np.ndarray) -> dict:
    """serialised overflow table (include/pseudoaligner_amd.h) -> {tuple(ids): count}"""
    out = {}
    if len(words) < 2:
        return out
    p = 2
    for _ in range(int(words[0])):
        n = int(words[p])
        out[tuple(int(x) for x in words[p + 3:p + 3 + n])] = int(words[p + 1]) | (int(words[p + 2]) << 32)
        p += 3 + n
    assert p == int(words[1]), "overflow table: header says %d words, records end at %d" % (int(words[1]), p)
    return out


def serialise_overflow(classes: dict) -> np.ndarray:
    """{tuple(ids): count} -> the serialised form (canonical order), e.g. to feed pa_overflow_merge"""
    w = [0, 0]
    for ids in sorted(classes):
        c = int(classes[ids])
        w += [len(ids), c & 0xFFFFFFFF, c >> 32] + list(ids)
    w[0], w[1] = len(classes), len(w)
    return np.array(w, dtype=np.uint32)


def overflow_merge(buffers: Sequence[np.ndarray]) -> np.ndarray:
    """pa_overflow_merge: serialised tables of several GPUs -> one canonical table (host side)"""
    bufs = [np.ascontiguousarray(b, dtype=np.uint32) for b in buffers]
    ptrs = (C.c_void_p * max(len(bufs), 1))(*[b.ctypes.data for b in bufs])
    sizes = (C.c_uint64 * max(len(bufs), 1))(*[len(b) for b in bufs])
    need = C.c_uint64()
    rc = lib().pa_overflow_merge(ptrs, sizes, len(bufs), None, 0, C.byref(need))
    if rc not in (PA_OK, PA_ERR_ARENA_FULL):
        check(rc)
    out = np.zeros(max(need.value, 2), dtype=np.uint32)
    check(lib().pa_overflow_merge(ptrs, sizes, len(bufs), out.ctypes.data, len(out), C.byref(need)))
    return out[: need.value]


class Overflow:
    """Per-GPU table of the NOVEL classes (results that are no index class), keyed by content."""

    def __init__(self, device: int = 0, max_classes: int = 1 << 20, max_ids: int = 1 << 24):
        h = vp()
        check(lib().pa_overflow_create(device, max_classes, max_ids, C.byref(h)))
        self._h = h

    def reset(self, stream: int = 0) -> None:
        check(lib().pa_overflow_reset(self._h, stream or None))

    def fetch(self, stream: int = 0) -> np.ndarray:
        w, n = vp(), C.c_uint64()
        check(lib().pa_overflow_fetch(self._h, stream or None, C.byref(w), C.byref(n)))
        return _np_view(w.value, n.value, np.uint32).copy()

    def allgather(self, comm: Optional["Comm"], stream: int = 0) -> np.ndarray:
        w, n = vp(), C.c_uint64()
        check(lib().pa_overflow_allgather(self._h, comm._h if comm else None, stream or None, C.byref(w), C.byref(n)))
        return _np_view(w.value, n.value, np.uint32).copy()

    def __del__(self):
        try:
            if self._h:
                lib().pa_overflow_destroy(self._h)
                self._h = vp()
        except Exception:
            pass


class RecordStream:
    """pa_record_stream: process_reads for a caller that holds the reader — push records, pull the reference's Debug tuples"""

    def __init__(self, aligner, num_threads: int = 0, batch_reads: int = 0):
        """aligner: a Pseudoaligner, or a list of them (replicas of one index: pa_record_stream_create_multi — batches round-robin over the handles)"""
        h = vp()
        if isinstance(aligner, (list, tuple)):
            hs = (vp * len(aligner))(*[a._h for a in aligner])
            check(lib().pa_record_stream_create_multi(hs, len(aligner), num_threads, batch_reads, C.byref(h)))
        else:
            check(lib().pa_record_stream_create(aligner._h, num_threads, batch_reads, C.byref(h)))
        self._h = h
        self._aligner = aligner   # (the index must outlive the stream)

    def push(self, ids: Sequence, seqs: Sequence) -> None:
        i_data, i_off = concat_reads(ids)
        s_data, s_off = concat_reads(seqs)
        check(lib().pa_records_push(self._h, i_data.ctypes.data, i_off.ctypes.data, s_data.ctypes.data, s_off.ctypes.data, len(i_off) - 1))

    def pull(self, cap: int = 1 << 20, grow: bool = True) -> bytes:
        """rendered tuples, whole lines. A tuple longer than `cap` (a class of ~100 k ids) makes the library answer PA_ERR_BUFFER_TOO_SMALL with the
        bytes it needs: the buffer is grown to that and the pull repeated (grow=False: the error is raised instead)"""
        from ._ffi import PA_ERR_BUFFER_TOO_SMALL
        for _ in range(4):
            buf = C.create_string_buffer(cap)
            n = C.c_size_t()
            rc = lib().pa_records_pull(self._h, buf, cap, C.byref(n))
            if rc == PA_ERR_BUFFER_TOO_SMALL and grow and n.value > cap:
                cap = int(n.value)
                continue
            check(rc)
            return buf.raw[: n.value]
        raise PaError(PA_ERR_BUFFER_TOO_SMALL, "pa_records_pull keeps asking for a larger buffer")

    def flush(self) -> None:
        check(lib().pa_records_flush(self._h))

    def drain(self, cap: int = 1 << 20) -> bytes:
        out = []
        while True:
            b = self.pull(cap)
            if not b:
                return b"".join(out)
            out.append(b)

    def stats(self) -> Tuple[int, int]:
        n, f = C.c_uint64(), C.c_uint64()
        check(lib().pa_record_stream_stats(self._h, C.byref(n), C.byref(f)))
        return n.value, f.value

    def stage_seconds(self) -> dict:
        st = (C.c_double * 8)()
        check(lib().pa_record_stream_stage_seconds(self._h, st))
        return dict(zip(INGEST_STAGES, st))

    def close(self) -> None:
        if self._h:
            lib().pa_record_stream_destroy(self._h)
            self._h = vp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Comm:
    """RCCL communicator owned by the library: one rank per GPU."""

    @staticmethod
    def unique_id() -> bytes:
        buf = (C.c_uint8 * 128)()
        check(lib().pa_comm_unique_id(buf))
        return bytes(buf)

    def __init__(self, device: int, nranks: int, rank: int, unique_id: bytes):
        assert len(unique_id) == 128
        buf = (C.c_uint8 * 128).from_buffer_copy(unique_id)
        h = vp()
        check(lib().pa_comm_create(device, nranks, rank, buf, C.byref(h)))
        self._h = h

    @property
    def rank(self) -> int:
        return lib().pa_comm_rank(self._h)

    @property
    def size(self) -> int:
        return lib().pa_comm_size(self._h)

    def __del__(self):
        try:
            if self._h:
                lib().pa_comm_destroy(self._h)
                self._h = vp()
        except Exception:
            pass


INGEST_STAGES = ("scan_s", "pack_s", "gpu_wait_s", "launch_s", "render_s", "writer_wait_s", "total_s", "reads")


def process_reads_stage_seconds() -> dict:
    """host-stage wall seconds of this thread's last process_reads call (pa_process_reads_stage_seconds)"""
    st = (C.c_double * 8)()
    check(lib().pa_process_reads_stage_seconds(st))
    return dict(zip(INGEST_STAGES, st))


INPUT_STATS = ("text_kind", "members_total", "members_gpu", "members_host", "bytes_h2d", "text_bytes_gpu")


def process_reads_input_stats() -> dict:
    """what this thread's last process_reads call read (pa_process_reads_input_stats): text_kind 0 plain, 1 gzip inflated by the host, 2 BGZF inflated on the GPU"""
    st = (C.c_uint64 * 6)()
    check(lib().pa_process_reads_input_stats(st))
    return dict(zip(INPUT_STATS, [int(x) for x in st]))


def process_reads(fastq_path: str, index: Pseudoaligner, out_path: str = "-", num_threads: int = 2) -> Tuple[int, int]:
    """process_reads (src/pseudoaligner.rs:420-425): one `(flag, "id", [ids], coverage)` line per read, input order.
    Returns (reads, reads flagged true by the rule at :455)."""
    n, flagged = C.c_uint64(), C.c_uint64()
    check(lib().pa_process_reads(index._h, str(fastq_path).encode(), str(out_path).encode(), num_threads, C.byref(n), C.byref(flagged)))
    return n.value, flagged.value


def process_reads_multi(fastq_path: str, indexes: Sequence[Pseudoaligner], out_path: str = "-", num_threads: int = 2) -> Tuple[int, int]:
    """pa_process_reads_multi: process_reads over several handles of one index (the GPUs of a node; a handle listed twice = two lanes
    on its GPU); the output is byte for byte that of process_reads on one handle"""
    n, flagged = C.c_uint64(), C.c_uint64()
    hs = (vp * len(indexes))(*[a._h for a in indexes])
    check(lib().pa_process_reads_multi(hs, len(indexes), str(fastq_path).encode(), str(out_path).encode(), num_threads, C.byref(n), C.byref(flagged)))
    return n.value, flagged.value


def fastq_scan(fastq_path: str, num_threads: int = 2) -> Tuple[np.ndarray, np.ndarray, np.ndarray, int]:
    """pa_fastq_scan_host: the scan stage of process_reads alone (no GPU) -> (starts, header_len, seq_len, text_kind)"""
    n, kind = C.c_uint64(), C.c_int()
    check(lib().pa_fastq_scan_host(str(fastq_path).encode(), num_threads, C.byref(n), None, None, None, 0, C.byref(kind)))
    starts, hdr, seq = np.zeros(n.value, np.uint64), np.zeros(n.value, np.uint32), np.zeros(n.value, np.uint32)
    if n.value:
        check(lib().pa_fastq_scan_host(str(fastq_path).encode(), num_threads, C.byref(n), starts.ctypes.data_as(_ffi.u64p),
                                       hdr.ctypes.data_as(_ffi.u32p), seq.ctypes.data_as(_ffi.u32p), len(starts), C.byref(kind)))
    return starts, hdr, seq, kind.value


BGZF_MEMBER_DTYPE = np.dtype([("in_off", "<u8"), ("out_off", "<u8"), ("file_off", "<u8"), ("in_len", "<u4"), ("out_len", "<u4"), ("crc32", "<u4"), ("reserved", "<u4")])


def bgzf_scan(path_or_bytes) -> Optional[Tuple[np.ndarray, int]]:
    """pa_bgzf_scan: the member table of a BGZF file (BGZF_MEMBER_DTYPE, one row per member) and the bytes of text it holds, found from
    header to header without inflating; None when the bytes are not BGZF from first to last (ordinary gzip, a truncated member, ...)"""
    data = path_or_bytes if isinstance(path_or_bytes, (bytes, bytearray, memoryview)) else open(path_or_bytes, "rb").read()
    buf = np.frombuffer(bytes(data), np.uint8)
    n, text = C.c_uint64(), C.c_uint64()
    rc = lib().pa_bgzf_scan(buf.ctypes.data, len(buf), None, 0, C.byref(n), C.byref(text))
    if rc == _ffi.PA_ERR_NOT_BGZF:
        return None
    check(rc)
    members = np.zeros(n.value, BGZF_MEMBER_DTYPE)
    check(lib().pa_bgzf_scan(buf.ctypes.data, len(buf), members.ctypes.data_as(C.POINTER(_ffi.BgzfMember)), len(members), C.byref(n), C.byref(text)))
    return members, text.value


def bgzf_inflate_device(device: int, d_comp: int, comp_bytes: int, d_members: int, n_members: int, d_text: int, text_cap: int, d_status: int, stream: int = 0) -> None:
    """pa_bgzf_inflate_device on device pointers (ints): members d_members[0, n_members) of the compressed bytes at d_comp inflated to
    d_text[out_off - out_off of the first ...), one status word per member; asynchronous on `stream`"""
    check(lib().pa_bgzf_inflate_device(device, d_comp, comp_bytes, d_members, n_members, d_text, text_cap, d_status, stream or None))


def inflate_status_name(status: int) -> str:
    return lib().pa_inflate_status_name(status).decode()


def bgzf_inflate(data: bytes, device: int = 0) -> Tuple[bytes, np.ndarray]:
    """A whole BGZF file inflated on the GPU -> (text, statuses). The text of a member whose status is not 0 is unspecified. PaError when
    the bytes are not BGZF (there is no host fallback here: use gzip for anything else)."""
    scanned = bgzf_scan(data)
    if scanned is None:
        raise PaError(_ffi.PA_ERR_NOT_BGZF, "not BGZF")
    members, text_bytes = scanned
    L = lib()
    status = np.zeros(len(members), np.uint32)
    text = np.zeros(text_bytes, np.uint8)
    ptrs = []

    def dev(nbytes):
        p = vp()
        check(L.pa_device_malloc(device, max(nbytes, 16), C.byref(p)))
        ptrs.append(p)
        return p
    try:
        comp = np.frombuffer(bytes(data), np.uint8)
        d_comp, d_mem, d_text, d_status = dev(comp.nbytes), dev(members.nbytes), dev(text.nbytes), dev(status.nbytes)
        check(L.pa_memcpy_h2d(d_comp, comp.ctypes.data, comp.nbytes, None))
        check(L.pa_memcpy_h2d(d_mem, members.ctypes.data, members.nbytes, None))
        check(L.pa_memset_device(d_text, 0, max(text.nbytes, 16), None))
        check(L.pa_bgzf_inflate_device(device, d_comp, comp.nbytes, d_mem, len(members), d_text, text.nbytes, d_status, None))
        if text.nbytes:
            check(L.pa_memcpy_d2h(text.ctypes.data, d_text, text.nbytes, None))
        check(L.pa_memcpy_d2h(status.ctypes.data, d_status, status.nbytes, None))
        check(L.pa_stream_synchronize(None))
    finally:
        for p in ptrs:
            L.pa_device_free(p)
    return text.tobytes(), status


def pairs_input_stats() -> dict:
    """what this thread's last count_cells / write_bus / count_pairs call read (pa_pairs_input_stats, pa_pairs_input_path):
    {"device_path": whether the GPU scanned, compared and gathered, "r1": {...}, "r2": {...}} with the entries of process_reads_input_stats per file"""
    st = (C.c_uint64 * 12)()
    check(lib().pa_pairs_input_stats(st))
    v = [int(x) for x in st]
    return {"device_path": lib().pa_pairs_input_path() == 1, "r1": dict(zip(INPUT_STATS, v[:6])), "r2": dict(zip(INPUT_STATS, v[6:]))}


def pairs_gather_scratch_bytes(m: int) -> int:
    """pa_pairs_gather_scratch_bytes: the scratch one segment of m pairs needs (0: more pairs than a segment takes)"""
    return lib().pa_pairs_gather_scratch_bytes(m)


def pairs_gather_device(text1, rec1, text2, rec2, prefix: int, base: int, bytes1, off1, bytes2, off2, ctl, m: Optional[int] = None, scratch=None) -> None:
    """pa_pairs_gather_device on torch tensors of one GPU, asynchronous on torch's current stream: one SEGMENT of a batch of pairs.
      text1, text2   uint8: the two texts
      rec1, rec2     int32 [m, 4], contiguous: {id offset, id length, sequence offset, sequence length} per record (the bits of u32)
      prefix         bytes of every R1 sequence that are kept (_ffi.PA_PAIRS_WHOLE_READ: all)
      base           the batch position of the segment's first pair; 0 opens a batch (ctl is reset)
      bytes1, bytes2 uint8: the gathered pieces (nothing is written beyond their sizes)
      off1, off2     int64, at least base + m + 1 entries
      ctl            int64 [8]: _ffi.PAIRS_CTL_NAMES, then two unused words
      scratch        uint8, pairs_gather_scratch_bytes(m) bytes (allocated here when None)"""
    import torch
    m = int(rec1.shape[0]) if m is None else int(m)
    dev = ctl.device
    for name, t, dt in (("text1", text1, torch.uint8), ("rec1", rec1, torch.int32), ("text2", text2, torch.uint8), ("rec2", rec2, torch.int32), ("bytes1", bytes1, torch.uint8),
                        ("off1", off1, torch.int64), ("bytes2", bytes2, torch.uint8), ("off2", off2, torch.int64), ("ctl", ctl, torch.int64)):
        if t.dtype != dt or not t.is_contiguous() or t.device != dev or dev.type != "cuda":
            raise ValueError("%s: a contiguous %s tensor on %s is expected" % (name, dt, dev))
    if rec1.numel() < 4 * m or rec2.numel() < 4 * m or off1.numel() < base + m + 1 or off2.numel() < base + m + 1 or ctl.numel() < _ffi.PA_PAIRS_CTL_WORDS:
        raise ValueError("record tables of m rows, offsets of base + m + 1 entries and a control block of %d words are expected" % _ffi.PA_PAIRS_CTL_WORDS)
    need = pairs_gather_scratch_bytes(m)
    if scratch is None:
        scratch = torch.empty(need + 256, dtype=torch.uint8, device=dev)
    pad = (-scratch.data_ptr()) % 256
    check(lib().pa_pairs_gather_device(dev.index or 0, text1.data_ptr() or None, text1.numel(), rec1.data_ptr() or None, text2.data_ptr() or None, text2.numel(),
                                       rec2.data_ptr() or None, m, prefix, base, bytes1.data_ptr() or None, bytes1.numel(), off1.data_ptr(), bytes2.data_ptr() or None,
                                       bytes2.numel(), off2.data_ptr(), ctl.data_ptr(), scratch.data_ptr() + pad, scratch.numel() - pad,
                                       torch.cuda.current_stream(dev).cuda_stream or None))


PA_COMPACT_MAPPED, PA_COMPACT_BY_REF, PA_COMPACT_PACKED = 0x10000000, 0x20000000, 0x40000000
PA_COMPACT_MAX_READ_LEN = 16383   # coverage and mismatches take 14 bits each: map_tiles_host refuses longer reads (PA_ERR_INVALID_ARG)


def unpack_compact(compact: np.ndarray, packed: np.ndarray, index: "HostIndex") -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """pa_results_compact_device's 8-byte records + packed stream -> (results RESULT_DTYPE with class_off = 0, class_offsets[n+1], class_ids)
    in read order (vectorised): a by-reference class is eq_classes[id] of the flat index, a packed one the next {length, ids...} entry"""
    a = index.arrays()
    lo = (compact & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    hi = (compact >> np.uint64(32)).astype(np.int64)
    n = len(compact)
    res = np.zeros(n, RESULT_DTYPE)
    res["coverage"] = lo & 0x3FFF
    res["mismatches"] = ((lo >> 14) & 0x3FFF) | np.where(lo & PA_COMPACT_MAPPED, np.uint32(PA_MAPPED_BIT), np.uint32(0))
    by_ref = (lo & PA_COMPACT_BY_REF) != 0
    pk = (lo & PA_COMPACT_PACKED) != 0
    assert not (by_ref & pk).any(), "a class was lost to a full arena"
    ec_offset = a["ec_offset"].astype(np.int64)
    lens = np.zeros(n, np.int64)
    lens[by_ref] = (ec_offset[1:] - ec_offset[:-1])[hi[by_ref]]
    packed = np.asarray(packed, np.uint32)
    # packed entries in read order: walk their lengths
    pidx = np.flatnonzero(pk)
    pstart = np.zeros(len(pidx), np.int64)
    pos = 0
    plen = np.zeros(len(pidx), np.int64)
    for j in range(len(pidx)):     # (sequential by construction: entry j starts where entry j - 1 ends)
        plen[j] = int(packed[pos])
        pstart[j] = pos + 1
        pos += 1 + int(plen[j])
    assert pos == len(packed), "packed stream: %d words walked, %d given" % (pos, len(packed))
    lens[pidx] = plen
    res["class_len"] = lens
    coff = np.zeros(n + 1, np.uint64)
    coff[1:] = np.cumsum(lens)
    total = int(coff[-1])
    if total == 0:
        return res, coff, np.zeros(0, np.uint32)
    src = np.concatenate([packed, a["ec_ids"]])
    start = np.zeros(n, np.int64)
    start[by_ref] = len(packed) + ec_offset[hi[by_ref]]
    start[pidx] = pstart
    within = np.arange(total, dtype=np.int64) - np.repeat(coff[:-1].astype(np.int64), lens)
    return res, coff, src[np.repeat(start, lens) + within].astype(np.uint32)


def gather_classes(results: np.ndarray, arena: np.ndarray, index: "HostIndex") -> Tuple[np.ndarray, np.ndarray]:
    """Device-format results -> (class_offsets[n+1], class_ids) in read order (vectorised). A class is either given by
    reference (class_off has PA_CLASS_REF set: it is eq_classes[class_off & 0x7FFFFFFF] of the flat index) or by its
    offset in the arena."""
    a = index.arrays()
    lens = results["class_len"].astype(np.int64)
    coff = np.zeros(len(results) + 1, dtype=np.uint64)
    coff[1:] = np.cumsum(lens)
    total = int(coff[-1])
    if total == 0:
        return coff, np.zeros(0, np.uint32)
    off = results["class_off"].astype(np.int64)
    is_ref = (off & 0x80000000) != 0
    ec_offset = a["ec_offset"].astype(np.int64)
    src = np.concatenate([np.asarray(arena, dtype=np.uint32), a["ec_ids"]])
    cid = np.where(is_ref & (lens > 0), off & 0x7FFFFFFF, 0)
    start = np.where(is_ref, len(arena) + ec_offset[cid], off)
    starts = np.repeat(start, lens)
    within = np.arange(total, dtype=np.int64) - np.repeat(coff[:-1].astype(np.int64), lens)
    return coff, src[starts + within].astype(np.uint32)
