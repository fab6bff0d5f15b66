"""The unstranded stage at the ABI's edges: integration/rust/src/amd_strands_ffi.rs (which cannot be compiled here) against the header,
prototype by prototype and constant by constant, with the comparison tools of tests/abi_sigs.py; the C client and the ctypes table name
every entry point; the scratch size is a host-side function; the refusals that come before any device call."""
import ctypes as C

import numpy as np

import abi_sigs
import helpers

pa = helpers.pa
RUST = helpers.ROOT / "integration" / "rust" / "src" / "amd_strands_ffi.rs"
HEADER = helpers.ROOT / "include" / "pseudoaligner_amd.h"
NAMES = {"pa_strands_scratch_bytes", "pa_strands_merge_device", "pa_strands_finish", "pa_map_batch_strand", "pa_map_pairs_unstranded", "pa_count_pairs_unstranded"}


def test_rust_strands_binding_matches_the_header():
    header, rust = HEADER.read_text(), RUST.read_text()
    hp, rp = abi_sigs.header_prototypes(header), abi_sigs.rust_prototypes(rust)
    assert set(rp) == NAMES
    for name, sig in rp.items():
        assert hp[name] == sig, "%s: Rust says %s, the header %s" % (name, sig, hp[name])
    assert len(hp["pa_strands_merge_device"][1]) == 13 and hp["pa_strands_merge_device"][1] == hp["pa_pairs_combine_device"][1]
    assert hp["pa_strands_finish"] == hp["pa_pairs_finish"]
    hc, rc = abi_sigs.header_consts(header), abi_sigs.rust_consts(rust)
    assert rc == {"PA_STRAND_FWD": 0, "PA_STRAND_REV": 1, "PA_STRAND_BOTH": 2, "PA_STRAND_STATS": 8}
    assert all(hc.get(k) == v for k, v in rc.items()), {k: (v, hc.get(k)) for k, v in rc.items()}
    F = pa._ffi
    assert (F.PA_STRAND_FWD, F.PA_STRAND_REV, F.PA_STRAND_BOTH, F.PA_STRAND_STATS) == (0, 1, 2, 8) and len(F.STRAND_STAT_NAMES) == F.PA_STRAND_STATS
    assert F.STRANDS == {"fwd": 0, "rev": 1, "both": 2}
    # not vacuous: a drifted width or a swapped pair of arguments is caught
    for name, was, now in (("pa_map_batch_strand", "n_reads: u64, strand: c_int", "n_reads: u32, strand: c_int"),
                           ("pa_count_pairs_unstranded", "allowed_mismatches: u32, num_threads: c_int,\n", "num_threads: c_int, allowed_mismatches: u32,\n")):
        assert was in rust
        assert abi_sigs.rust_prototypes(rust.replace(was, now, 1))[name] != hp[name]
    amd = (helpers.ROOT / "integration" / "rust" / "src" / "amd.rs").read_text()
    for fn in ("pub fn map_pairs_unstranded(", "pub fn count_pairs_unstranded<", "pub fn map_reads_strand("):
        assert fn in amd
    assert "amd_strands_ffi::" in amd
    old = (helpers.ROOT / "integration" / "rust" / "src" / "amd_ffi.rs").read_text()
    assert not any(n + "(" in old for n in NAMES)
    assert pa.lib().pa_abi_version() == 1


def test_symbols_are_exported_bound_and_called_from_c(built):
    lib = C.CDLL(str(pa._ffi.library_path()))
    src = (helpers.ROOT / "integration" / "c" / "abi_check.c").read_text()
    for n in NAMES:
        assert hasattr(lib, n), "library does not export %s" % n
        assert n in pa._ffi.SIGNATURES and n + "(" in src
    assert len(pa._ffi.SIGNATURES["pa_strands_merge_device"][1]) == 13 and pa._ffi.SIGNATURES["pa_strands_scratch_bytes"][0] is C.c_size_t
    for m in ("strands_scratch_bytes", "strands_merge_device", "strands_finish"):
        assert callable(getattr(pa.Pseudoaligner, m))


def test_scratch_size_is_a_host_function(built):
    sizes = [pa.Pseudoaligner.strands_scratch_bytes(n) for n in (0, 1, 64, 65, 1000, 1 << 20)]
    assert sizes[0] >= 256 and all(a <= b for a, b in zip(sizes, sizes[1:])) and all(s % 256 == 0 for s in sizes)
    assert sizes[5] >= (1 << 20) * (8 + 8 + 4 + 8)          # two bins of flags, their scan, the item list, the novel list
    assert pa.Pseudoaligner.strands_scratch_bytes(0x7FFFFFF0) > 0 and pa.Pseudoaligner.strands_scratch_bytes(0x7FFFFFF1) == 0
    assert pa.Pseudoaligner.strands_scratch_bytes(1 << 40) == 0


def test_arguments_are_checked_before_any_device_call(built):
    L, E = pa.lib(), pa._ffi.PA_ERR_INVALID_ARG
    fake = C.c_void_p(0x1000)                                 # an index handle that is never looked at: every refusal below comes first
    buf = np.zeros(4096, np.uint8)
    p = buf.ctypes.data
    al = (p + 255) & ~255
    # null arguments
    assert L.pa_strands_merge_device(None, None, None, None, None, 0, None, None, 0, None, al, 1 << 20, None) == E
    assert L.pa_strands_merge_device(fake, None, None, None, None, 0, None, None, 0, None, None, 1 << 20, None) == E
    assert L.pa_strands_merge_device(fake, None, None, None, None, 1, None, None, 0, None, al, 1 << 20, None) == E      # an item and no records
    assert L.pa_strands_merge_device(fake, p, None, p, None, 1, p, None, 8, None, al, 1 << 20, None) == E               # a capacity and no arena
    assert L.pa_strands_finish(None, al, None, None, None, None) == E and L.pa_strands_finish(fake, None, None, None, None, None) == E
    # a scratch that is not 256-byte aligned, or too small
    assert L.pa_strands_merge_device(fake, None, None, None, None, 0, None, None, 0, None, al + 8, 1 << 20, None) == E
    assert "aligned" in L.pa_last_error().decode()
    assert L.pa_strands_merge_device(fake, None, None, None, None, 0, None, None, 0, None, al, pa.Pseudoaligner.strands_scratch_bytes(0) - 1, None) == E
    assert "needed" in L.pa_last_error().decode()
    assert L.pa_strands_merge_device(fake, None, None, None, None, 1 << 40, None, None, 0, None, al, 1 << 20, None) in (E, pa._ffi.PA_ERR_UNSUPPORTED)
    # strands that do not exist; null arguments of the host-buffer paths
    d, o = pa.concat_reads(["ACGT"])
    out = np.zeros(1, pa.RESULT_DTYPE)
    for strand in (3, -1):
        assert L.pa_map_batch_strand(fake, d.ctypes.data, o.ctypes.data, 1, strand, 2, out.ctypes.data, None, None) == E
        assert "strand" in L.pa_last_error().decode()
    assert L.pa_map_batch_strand(None, d.ctypes.data, o.ctypes.data, 1, 2, 2, out.ctypes.data, None, None) == E
    assert L.pa_map_batch_strand(fake, d.ctypes.data, None, 1, 2, 2, out.ctypes.data, None, None) == E
    assert L.pa_map_batch_strand(fake, d.ctypes.data, o.ctypes.data, 1, 2, 2, None, None, None) == E
    assert L.pa_map_batch_strand(fake, None, o.ctypes.data, 1, 2, 2, out.ctypes.data, None, None) == E
    bad = np.array([4, 0], np.uint64)
    assert L.pa_map_batch_strand(fake, d.ctypes.data, bad.ctypes.data, 1, 2, 2, out.ctypes.data, None, None) == E
    assert L.pa_map_pairs_unstranded(None, d.ctypes.data, o.ctypes.data, d.ctypes.data, o.ctypes.data, 1, 2, out.ctypes.data, None, None) == E
    assert L.pa_map_pairs_unstranded(fake, d.ctypes.data, None, d.ctypes.data, o.ctypes.data, 1, 2, out.ctypes.data, None, None) == E
    assert L.pa_map_pairs_unstranded(fake, d.ctypes.data, o.ctypes.data, None, o.ctypes.data, 1, 2, out.ctypes.data, None, None) == E
    assert L.pa_map_pairs_unstranded(fake, d.ctypes.data, o.ctypes.data, d.ctypes.data, o.ctypes.data, 1, 2, None, None, None) == E
    counts = np.zeros(8, np.uint64)
    assert L.pa_count_pairs_unstranded(None, b"a", b"b", 2, 1, counts.ctypes.data, None, None) == E
    assert L.pa_count_pairs_unstranded(fake, None, b"b", 2, 1, counts.ctypes.data, None, None) == E
    assert L.pa_count_pairs_unstranded(fake, b"a", b"b", 2, 1, None, None, None) == E
