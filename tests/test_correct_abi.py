"""The BUS barcode correction at the ABI's edges: integration/rust/src/amd_correct_ffi.rs (which cannot be compiled here) against the header,
prototype by prototype and constant by constant, with the comparison tools of tests/abi_sigs.py; the C client and the ctypes table name
every entry point; pa_bus_whitelist_pack against the model; the refusals that come before any device call."""
import ctypes as C

import numpy as np
import pytest

import abi_sigs
import correct_cases as cc
import correct_model as cm
import helpers

pa = helpers.pa
RUST = helpers.ROOT / "integration" / "rust" / "src" / "amd_correct_ffi.rs"
HEADER = helpers.ROOT / "include" / "pseudoaligner_amd.h"
ENTRY_POINTS = {"pa_bus_whitelist_pack", "pa_bus_correct_records", "pa_bus_correct", "pa_bus_correct_phase_ms", "pa_write_bus_corrected", "pa_count_cells_em_corrected"}


def test_rust_correct_binding_matches_the_header(monkeypatch):
    for r, c in (("PaBusRecord", "pa_bus_record"), ("PaBus", "pa_bus"), ("PaGenesParams", "pa_genes_params")):
        monkeypatch.setitem(abi_sigs.RUST_SCALARS, r, c)
    header, rust = HEADER.read_text(), RUST.read_text()
    hp, rp = abi_sigs.header_prototypes(header), abi_sigs.rust_prototypes(rust)
    assert set(rp) == ENTRY_POINTS
    for name, sig in rp.items():
        assert hp[name] == sig, "%s: Rust says %s, the header %s" % (name, sig, hp[name])
    hc, rc = abi_sigs.header_consts(header), abi_sigs.rust_consts(rust)
    assert rc == {"PA_BUS_CORRECT_STATS": 13, "PA_BUS_CORRECT_PHASES": 4} and all(hc[k] == v for k, v in rc.items())
    assert abi_sigs.rust_structs(rust) == {}
    assert pa._ffi.PA_BUS_CORRECT_STATS == 13 == len(pa._ffi.CORRECT_STAT_NAMES) and pa._ffi.CORRECT_STAT_NAMES == cm.STAT_NAMES == pa.CORRECT_STAT_NAMES
    assert pa._ffi.PA_BUS_CORRECT_PHASES == 4 == len(pa._ffi.CORRECT_PHASE_NAMES)
    # not vacuous: a drifted width, a dropped const and a swapped pair of arguments are caught
    for good, bad, fn in (("n_whitelist: u64, out: *mut PaBusRecord", "n_whitelist: u32, out: *mut PaBusRecord", "pa_bus_correct_records"),
                          ("finished: *mut PaBus, whitelist: *const u64", "finished: *mut PaBus, whitelist: *mut u64", "pa_bus_correct"),
                          ("bc_len: u32, umi_len: u32, p: *const PaGenesParams", "bc_len: u32, p: *const PaGenesParams, umi_len: u32", "pa_count_cells_em_corrected")):
        drift = rust.replace(good, bad)
        assert drift != rust and abi_sigs.rust_prototypes(drift)[fn] != hp[fn], fn
    amd = (helpers.ROOT / "integration" / "rust" / "src" / "amd.rs").read_text()
    assert "pub fn write_bus_corrected" in amd and "pa_write_bus_corrected(idx, h," in amd
    assert "pub fn count_cells_em_corrected" in amd and "pa_count_cells_em_corrected(idx, h," in amd
    assert pa.lib().pa_abi_version() == 1


def test_every_entry_point_is_named(built):
    src = (helpers.ROOT / "integration" / "c" / "abi_check.c").read_text()
    for fn in ENTRY_POINTS:
        assert fn + "(" in src and fn in pa._ffi.SIGNATURES, fn
    assert "bus_correct.hip" in helpers._build.HIP_SOURCES and "bus_correct_host.cpp" in helpers._build.HOST_SOURCES


def test_whitelist_pack_equals_the_model(built):
    rng = np.random.default_rng(2)
    for bc_len in (1, 4, 16, 31):
        strings = ["".join(cm.BASES[x] for x in rng.integers(0, 4, bc_len)) for _ in range(50)] + ["A" * bc_len, "T" * bc_len]
        assert pa.bus_whitelist_pack(strings).tolist() == [cm.pack(s) for s in strings]
    assert len(pa.bus_whitelist_pack([])) == 0
    for at, byte in ((0, "N"), (3, "a"), (6, "\n")):
        strings = ["ACGT"] * 7
        strings[at] = "AC" + byte + "T"
        with pytest.raises(pa.PaError) as e:
            pa.bus_whitelist_pack(strings)
        assert e.value.code == pa._ffi.PA_ERR_INVALID_ARG and "entry %d:" % at in str(e.value) and "byte 3" in str(e.value)
    with pytest.raises(pa.PaError) as e:
        pa.bus_whitelist_pack(["A" * 32])
    assert e.value.code == pa._ffi.PA_ERR_UNSUPPORTED


def test_refusals_come_before_any_device_call(built):
    """every host argument is checked first: without a GPU a VALID call gets PA_ERR_NO_DEVICE, an invalid one PA_ERR_INVALID_ARG; with a GPU
    the valid call (no index handle) is refused for the null index"""
    E = pa._ffi
    no_gpu = pa.lib().pa_device_count() < 1
    rec, wl, bc_len, umi_len = cc.sized_case(3, 10, 6, 4, bc_len=8, umi_len=4, n_whitelist=40)
    n = len(rec)
    for records in (rec, []):                                          # n = 0 is a valid call too
        with pytest.raises(pa.PaError) as e:
            pa.bus_correct(cc.to_array(records), np.array(wl, np.uint64), bc_len, umi_len, None)
        assert e.value.code == (E.PA_ERR_NO_DEVICE if no_gpu else E.PA_ERR_INVALID_ARG), str(e.value)

    def refused(records, whitelist, *needles, code=E.PA_ERR_INVALID_ARG, lens=(bc_len, umi_len)):
        with pytest.raises(pa.PaError) as e:
            pa.bus_correct(cc.to_array(records), np.array(whitelist, np.uint64), lens[0], lens[1], None)
        assert e.value.code == code, str(e.value)
        for s in needles:
            assert s in str(e.value), (s, str(e.value))

    for at in (0, n // 2, n - 1):                                      # each invalid-record kind at the first, a middle and the last record
        bad = [list(r) for r in rec]
        bad[at][0] = 4 ** bc_len
        refused(bad, wl, "record %d:" % at, "barcode")
        bad = [list(r) for r in rec]
        bad[at][1] = 4 ** umi_len
        refused(bad, wl, "record %d:" % at, "UMI")
        if at:
            bad = list(rec)
            bad[at] = bad[at - 1]
            refused(bad, wl, "record %d:" % at)
            bad = [list(r) for r in rec]
            bad[at][0] = 0
            refused(bad, wl, "record %d:" % at)
    m = len(wl)
    for at in (0, m // 2, m - 1):                                      # ... and each invalid whitelist entry
        bad = list(wl)
        bad[at] = 4 ** bc_len
        refused(rec, bad, "entry %d:" % at)
        other = (at + 7) % m
        bad = list(wl)
        bad[max(at, other)] = bad[min(at, other)]
        refused(rec, bad, "entry %d:" % min(at, other), "entry %d " % max(at, other))
    refused(rec, [])                                                   # n_whitelist = 0
    for lens in ((0, 4), (4, 0), (17, 16), (32, 1)):
        refused(rec, wl, "barcode length", code=E.PA_ERR_UNSUPPORTED, lens=lens)
    n_out = C.c_uint64(5)
    arr, w = cc.to_array(rec), np.array(wl, np.uint64)
    assert pa.lib().pa_bus_correct_records(None, arr.ctypes.data, 2 ** 31, bc_len, umi_len, w.ctypes.data, len(w), None, 0, C.byref(n_out), None) == E.PA_ERR_UNSUPPORTED
    assert n_out.value == 0
    with pytest.raises(pa.PaError) as e:
        pa.check(pa.lib().pa_bus_correct(None, w.ctypes.data, len(w), None))
    assert e.value.code == E.PA_ERR_INVALID_ARG
