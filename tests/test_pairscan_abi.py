"""The pair scan at the ABI's edges: integration/rust/src/amd_pairscan_ffi.rs (which cannot be compiled here) against the header, prototype
by prototype and constant by constant, with the comparison tools of tests/abi_sigs.py; the symbols exported and bound; the scratch size a
host-side function; without a GPU the device entry point refuses."""
import ctypes as C

import numpy as np
import pytest

import abi_sigs
import helpers

pa = helpers.pa
RUST = helpers.ROOT / "integration" / "rust" / "src" / "amd_pairscan_ffi.rs"
HEADER = helpers.ROOT / "include" / "pseudoaligner_amd.h"
NAMES = {"pa_pairs_gather_scratch_bytes", "pa_pairs_gather_device", "pa_pairs_input_stats", "pa_pairs_input_path"}


def test_rust_pairscan_binding_matches_the_header():
    header, rust = HEADER.read_text(), RUST.read_text()
    hp, rp = abi_sigs.header_prototypes(header), abi_sigs.rust_prototypes(rust)
    assert set(rp) == NAMES
    for name, sig in rp.items():
        assert hp[name] == sig, "%s: Rust says %s, the header %s" % (name, sig, hp[name])
    assert len(hp["pa_pairs_gather_device"][1]) == 20
    hc, rc = abi_sigs.header_consts(header), abi_sigs.rust_consts(rust)
    assert rc == {"PA_PAIRS_CTL_WORDS": 8, "PA_PAIRS_WHOLE_READ": 0xFFFFFFFF}
    assert all(hc.get(k) == v for k, v in rc.items()), {k: (v, hc.get(k)) for k, v in rc.items()}
    assert pa._ffi.PA_PAIRS_CTL_WORDS == hc["PA_PAIRS_CTL_WORDS"] and pa._ffi.PA_PAIRS_WHOLE_READ == hc["PA_PAIRS_WHOLE_READ"]
    assert len(pa._ffi.PAIRS_CTL_NAMES) <= pa._ffi.PA_PAIRS_CTL_WORDS
    # not vacuous: a drifted width or a swapped pair of arguments is caught
    for was, now in (("prefix: u32, base: u64", "prefix: u64, base: u64"), ("d_bytes1: *mut u8, cap1: u64", "cap1: u64, d_bytes1: *mut u8")):
        assert was in rust
        assert abi_sigs.rust_prototypes(rust.replace(was, now, 1))["pa_pairs_gather_device"] != hp["pa_pairs_gather_device"]
    amd = (helpers.ROOT / "integration" / "rust" / "src" / "amd.rs").read_text()
    assert "pub fn pairs_input_stats" in amd and "pub unsafe fn pairs_gather_segment" in amd and "amd_pairscan_ffi::" in amd


def test_symbols_are_exported_and_bound(built):
    lib = C.CDLL(str(pa._ffi.library_path()))
    for n in NAMES:
        assert hasattr(lib, n), "library does not export %s" % n
        assert n in pa._ffi.SIGNATURES
    res, args = pa._ffi.SIGNATURES["pa_pairs_gather_device"]
    assert res is C.c_int and len(args) == 20
    assert callable(pa.pairs_gather_device) and callable(pa.pairs_gather_scratch_bytes)
    st = pa.pairs_input_stats()
    assert set(st) == {"device_path", "r1", "r2"} and tuple(st["r1"]) == pa.INPUT_STATS == tuple(st["r2"])
    assert pa.lib().pa_pairs_input_stats(None) == pa._ffi.PA_ERR_INVALID_ARG


def test_scratch_size_is_a_host_function(built):
    sizes = [pa.pairs_gather_scratch_bytes(m) for m in (0, 1, 64, 1000, 1 << 20)]
    assert sizes[0] >= 256 and all(a <= b for a, b in zip(sizes, sizes[1:])) and all(s % 256 == 0 for s in sizes)
    assert sizes[4] >= (1 << 20) * (4 + 4 + 8 + 8 + 8)     # two lengths, two offsets and two list entries per pair
    assert pa.pairs_gather_scratch_bytes((1 << 30) + 1) == 0


def test_arguments_are_checked_before_any_device_call(built):
    L = pa.lib()
    off, ctl = np.zeros(4, np.uint64), np.zeros(8, np.uint64)
    p = lambda a: a.ctypes.data
    assert L.pa_pairs_gather_device(0, None, 0, None, None, 0, None, 0, 0, 0, None, 0, None, None, 0, p(off), p(ctl), 256, 4096, None) == pa._ffi.PA_ERR_INVALID_ARG
    # two pairs and no record tables
    assert L.pa_pairs_gather_device(0, None, 0, None, None, 0, None, 2, 0, 0, None, 0, p(off), None, 0, p(off), p(ctl), 256, 1 << 20, None) == pa._ffi.PA_ERR_INVALID_ARG
    # a scratch block that is not 256-byte aligned
    assert L.pa_pairs_gather_device(0, None, 0, None, None, 0, None, 0, 0, 0, None, 0, p(off), None, 0, p(off), p(ctl), 264, 4096, None) == pa._ffi.PA_ERR_INVALID_ARG


def test_gather_without_a_gpu_refuses(built):
    if pa.lib().pa_device_count() > 0:
        pytest.skip("a GPU is present")
    off, ctl = np.zeros(4, np.uint64), np.zeros(8, np.uint64)
    rc = pa.lib().pa_pairs_gather_device(0, None, 0, None, None, 0, None, 0, 2, 0, None, 0, off.ctypes.data, None, 0, off.ctypes.data + 16, ctl.ctypes.data, 256, 4096, None)
    assert rc == pa._ffi.PA_ERR_NO_DEVICE and "no CPU fallback" in pa.lib().pa_last_error().decode()
