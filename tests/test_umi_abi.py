"""The UMI correction at the ABI's edges: integration/rust/src/amd_umi_ffi.rs (which cannot be compiled here) against the header, prototype by
prototype and constant by constant, with the comparison tools of tests/abi_sigs.py; the C client and the ctypes table name every entry point; the
refusals that come before any device call."""
import ctypes as C

import numpy as np
import pytest

import abi_sigs
import helpers
import umi_cases as uc
import umi_model as um

pa = helpers.pa
RUST = helpers.ROOT / "integration" / "rust" / "src" / "amd_umi_ffi.rs"
HEADER = helpers.ROOT / "include" / "pseudoaligner_amd.h"
ENTRY_POINTS = {"pa_bus_umi_correct_records", "pa_bus_umi_correct", "pa_bus_umi_correct_phase_ms", "pa_write_bus_umi", "pa_count_cells_em_umi"}
CONSTS = {"PA_UMI_GREATEST": 0, "PA_UMI_DIRECTIONAL": 1, "PA_BUS_UMI_STATS": 15, "PA_BUS_UMI_PHASES": 4}


def test_rust_umi_binding_matches_the_header(monkeypatch):
    for r, c in (("PaBusRecord", "pa_bus_record"), ("PaBus", "pa_bus"), ("PaGenesParams", "pa_genes_params"), ("PaKneeParams", "pa_knee_params")):
        monkeypatch.setitem(abi_sigs.RUST_SCALARS, r, c)
    header, rust = HEADER.read_text(), RUST.read_text()
    hp, rp = abi_sigs.header_prototypes(header), abi_sigs.rust_prototypes(rust)
    assert set(rp) == ENTRY_POINTS
    for name, sig in rp.items():
        assert hp[name] == sig, "%s: Rust says %s, the header %s" % (name, sig, hp[name])
    hc, rc = abi_sigs.header_consts(header), abi_sigs.rust_consts(rust)
    assert rc == CONSTS and all(hc[k] == v for k, v in rc.items())
    assert abi_sigs.rust_structs(rust) == {}
    assert pa._ffi.PA_BUS_UMI_STATS == 15 == len(pa._ffi.UMI_STAT_NAMES) and pa._ffi.UMI_STAT_NAMES == um.STAT_NAMES == pa.UMI_STAT_NAMES
    assert pa._ffi.PA_BUS_UMI_PHASES == 4 == len(pa._ffi.UMI_PHASE_NAMES) == len(pa.UMI_PHASE_NAMES) and pa._ffi.UMI_MODES == um.MODES
    # not vacuous: a drifted width, a dropped const and a swapped pair of arguments are caught
    for good, bad, fn in (("num_genes: u32, bc_len: u32, umi_len: u32, mode: u32, out: *mut PaBusRecord", "num_genes: u32, bc_len: u32, umi_len: u32, mode: u64, out: *mut PaBusRecord",
                           "pa_bus_umi_correct_records"),
                          ("finished: *mut PaBus, tx_gene: *const u32", "finished: *mut PaBus, tx_gene: *mut u32", "pa_bus_umi_correct"),
                          ("call_cells: c_int, kp: *const PaKneeParams, umi_mode: u32,\n", "kp: *const PaKneeParams, call_cells: c_int, umi_mode: u32,\n", "pa_count_cells_em_umi")):
        drift = rust.replace(good, bad)
        assert drift != rust and abi_sigs.rust_prototypes(drift)[fn] != hp[fn], fn
    amd = (helpers.ROOT / "integration" / "rust" / "src" / "amd.rs").read_text()
    assert "pub fn bus_umi_correct" in amd and "pa_bus_umi_correct_records(idx, records.as_ptr()," in amd
    assert "pub fn write_bus_umi" in amd and "pa_write_bus_umi(idx, h," in amd
    assert "pub fn count_cells_em_umi" in amd and "pa_count_cells_em_umi(idx, h," in amd
    assert pa.lib().pa_abi_version() == 1


def test_every_entry_point_is_named(built):
    src = (helpers.ROOT / "integration" / "c" / "abi_check.c").read_text()
    for fn in ENTRY_POINTS:
        assert fn + "(" in src and fn in pa._ffi.SIGNATURES, fn
    assert "bus_umi.hip" in helpers._build.HIP_SOURCES and "bus_umi_host.cpp" in helpers._build.HOST_SOURCES
    for name in ("bus_umi_correct", "bus_umi_correct_phase_ms", "UMI_STAT_NAMES", "UMI_PHASE_NAMES"):
        assert hasattr(pa, name), name
    assert hasattr(pa.BusWriter, "umi_correct")


def test_refusals_come_before_any_device_call(built):
    """every host argument is checked first: without a GPU a VALID call gets PA_ERR_NO_DEVICE, an invalid one its own status; with a GPU the valid
    call (no index handle) is refused for the null index"""
    E = pa._ffi
    no_gpu = pa.lib().pa_device_count() < 1
    rec, off, ids, tx_gene, num_genes, bc_len, umi_len = uc.random_case(1)
    n, n_ecs = len(rec), len(off) - 1
    for records in (rec, rec[:0]):                                      # n = 0 is a valid call too
        for mode in ("greatest", "directional"):
            with pytest.raises(pa.PaError) as e:
                pa.bus_umi_correct(records, off, ids, tx_gene, num_genes, bc_len, umi_len, None, mode=mode)
            assert e.value.code == (E.PA_ERR_NO_DEVICE if no_gpu else E.PA_ERR_INVALID_ARG), str(e.value)

    def refused(*needles, records=rec, tx_gene=tx_gene, ids=ids, lens=(bc_len, umi_len), mode=0, code=E.PA_ERR_INVALID_ARG):
        with pytest.raises(pa.PaError) as e:
            pa.bus_umi_correct(records, off, ids, tx_gene, num_genes, lens[0], lens[1], None, mode=mode)
        assert e.value.code == code, str(e.value)
        for s in needles:
            assert s in str(e.value), (s, str(e.value))

    for at in (0, n // 2, n - 1):                                       # each invalid-record kind at the first, a middle and the last record
        for field, value, word in (("barcode", 4 ** bc_len, "barcode"), ("umi", 4 ** umi_len, "UMI"), ("ec", n_ecs, "ec %d" % n_ecs), ("ec", -1, "ec -1")):
            bad = rec.copy()
            bad[field][at] = value
            refused("record %d:" % at, word, records=bad)
        if at:
            bad = rec.copy()
            bad[at] = bad[at - 1]
            refused("record %d:" % at, records=bad)
            bad = rec.copy()
            bad["barcode"][at] = 0
            refused("record %d:" % at, records=bad)
    refused("mode 2", mode=2)
    bad = tx_gene.copy()
    bad[5] = num_genes
    refused("tx_gene[5]", tx_gene=bad)
    bad = ids.copy()
    bad[0] = len(tx_gene)
    refused("is no transcript", ids=bad)
    for lens in ((0, 4), (4, 0), (17, 16), (32, 1)):
        refused("barcode length", lens=lens)
    n_out, st = C.c_uint64(5), np.ones(15, np.uint64)
    call = lambda count, mode: pa.lib().pa_bus_umi_correct_records(None, rec.ctypes.data, count, off.ctypes.data, ids.ctypes.data, n_ecs, len(tx_gene), tx_gene.ctypes.data,
                                                                   num_genes, bc_len, umi_len, mode, None, 0, C.byref(n_out), st.ctypes.data)
    assert call(2 ** 31, 0) == E.PA_ERR_UNSUPPORTED and n_out.value == 0 and not st.any()
    assert call(n, 0) == (E.PA_ERR_NO_DEVICE if no_gpu else E.PA_ERR_INVALID_ARG)
    assert pa.lib().pa_bus_umi_correct(None, tx_gene.ctypes.data, num_genes, 0, st.ctypes.data) == E.PA_ERR_INVALID_ARG
    assert pa.lib().pa_bus_umi_correct_phase_ms(None) == E.PA_ERR_INVALID_ARG
    assert set(pa.bus_umi_correct_phase_ms()) == set(pa.UMI_PHASE_NAMES)
    for call in (lambda: pa.lib().pa_write_bus_umi(None, None, b"a", b"b", None, 16, 12, 0, None, 0, b"/tmp", 1, None, None, None, None),
                 lambda: pa.lib().pa_count_cells_em_umi(None, None, b"a", b"b", None, 16, 12, 0, None, 0, None, b"/tmp", 1, None, None, None, None)):
        assert call() == E.PA_ERR_INVALID_ARG
