"""The cell calling on BUS records at the ABI's edges: integration/rust/src/amd_knee_ffi.rs (which cannot be compiled here) against the header,
prototype by prototype, constant by constant and the row struct field by field, with the comparison tools of tests/abi_sigs.py; the C client and
the ctypes table name every entry point; the refusals that come before any device call."""
import ctypes as C

import numpy as np
import pytest

import abi_sigs
import helpers
import knee_cases as kc
import knee_model as km

pa = helpers.pa
RUST = helpers.ROOT / "integration" / "rust" / "src" / "amd_knee_ffi.rs"
HEADER = helpers.ROOT / "include" / "pseudoaligner_amd.h"
ENTRY_POINTS = {"pa_knee_default_params", "pa_bus_knee_records", "pa_bus_knee", "pa_bus_knee_phase_ms", "pa_bus_keep_records", "pa_bus_keep",
                "pa_write_barcode_ranks_tsv", "pa_write_bus_called", "pa_count_cells_em_called"}
CONSTS = {"PA_KNEE_CURVE": 0, "PA_KNEE_EXPECTED": 1, "PA_KNEE_MIN": 2, "PA_KNEE_STATS": 10, "PA_KNEE_PHASES": 3, "PA_BUS_KEEP_STATS": 7}


def test_rust_knee_binding_matches_the_header(monkeypatch):
    for r, c in (("PaBusRecord", "pa_bus_record"), ("PaBus", "pa_bus"), ("PaGenesParams", "pa_genes_params"), ("PaKneeParams", "pa_knee_params"),
                 ("PaBusBarcodeRow", "pa_bus_barcode_row"), ("[u32; 3]", "uint32_t[3]")):
        monkeypatch.setitem(abi_sigs.RUST_SCALARS, r, c)
    header, rust = HEADER.read_text(), RUST.read_text()
    hp, rp = abi_sigs.header_prototypes(header), abi_sigs.rust_prototypes(rust)
    assert set(rp) == ENTRY_POINTS
    for name, sig in rp.items():
        assert hp[name] == sig, "%s: Rust says %s, the header %s" % (name, sig, hp[name])
    hc, rc = abi_sigs.header_consts(header), abi_sigs.rust_consts(rust)
    assert rc == CONSTS and all(hc[k] == v for k, v in rc.items())
    # the structs: field order, names and types; the row's offsets under natural alignment are those of the numpy dtype the package reads rows with
    hs, rs = abi_sigs.header_structs(header), abi_sigs.rust_structs(rust)
    assert set(rs) == {"pa_knee_params", "pa_bus_barcode_row"}
    assert rs["pa_bus_barcode_row"] == hs["pa_bus_barcode_row"]
    offs, size = abi_sigs.layout(rs["pa_bus_barcode_row"])
    assert size == 32 == pa.BARCODE_ROW_DTYPE.itemsize == kc.ROW_DTYPE.itemsize and offs == {n: pa.BARCODE_ROW_DTYPE.fields[n][1] for n in pa.BARCODE_ROW_DTYPE.names}
    assert pa.BARCODE_ROW_DTYPE == kc.ROW_DTYPE
    as_array = lambda fields: [("reserved[3]", "uint32_t") if f == ("reserved", "uint32_t[3]") else f for f in fields]
    assert as_array(rs["pa_knee_params"]) == hs["pa_knee_params"] and C.sizeof(pa._ffi.KneeParams) == 32
    assert [n for n, _ in pa._ffi.KneeParams._fields_] == [n for n, _ in rs["pa_knee_params"]]
    assert pa._ffi.PA_KNEE_STATS == 10 == len(pa._ffi.KNEE_STAT_NAMES) and pa._ffi.KNEE_STAT_NAMES == km.STAT_NAMES == pa.KNEE_STAT_NAMES
    assert pa._ffi.PA_BUS_KEEP_STATS == 7 == len(pa._ffi.KEEP_STAT_NAMES) and pa._ffi.KEEP_STAT_NAMES == km.KEEP_STAT_NAMES == pa.KEEP_STAT_NAMES
    assert pa._ffi.PA_KNEE_PHASES == 3 == len(pa._ffi.KNEE_PHASE_NAMES) and pa._ffi.KNEE_MODES == km.MODES
    # not vacuous: a drifted width, a swapped pair of arguments and a dropped const are caught; so is a drifted field of the row
    for good, bad, fn in (("rows_cap: u64, n_rows: *mut u64, called: *mut u64, called_cap: u64, n_called: *mut u64,\n                               stats",
                           "rows_cap: u32, n_rows: *mut u64, called: *mut u64, called_cap: u64, n_called: *mut u64,\n                               stats", "pa_bus_knee_records"),
                          ("barcodes: *const u64, n_barcodes: u64, stats", "n_barcodes: u64, barcodes: *const u64, stats", "pa_bus_keep"),
                          ("kp: *const PaKneeParams, p: *const PaGenesParams", "p: *const PaGenesParams, kp: *const PaKneeParams", "pa_count_cells_em_called")):
        drift = rust.replace(good, bad)
        assert drift != rust and abi_sigs.rust_prototypes(drift)[fn] != hp[fn], fn
    dropped = rust.replace("pub const PA_KNEE_PHASES: usize = 3;\n", "")
    assert dropped != rust and abi_sigs.rust_consts(dropped) != CONSTS
    drift = rust.replace("pub reads: u64,", "pub reads: u32,")
    assert drift != rust and abi_sigs.rust_structs(drift)["pa_bus_barcode_row"] != hs["pa_bus_barcode_row"]
    amd = (helpers.ROOT / "integration" / "rust" / "src" / "amd.rs").read_text()
    assert "pub fn bus_knee" in amd and "pa_bus_knee_records(idx, records.as_ptr()," in amd
    assert "pub fn write_bus_called" in amd and "pa_write_bus_called(idx, h," in amd
    assert "pub fn count_cells_em_called" in amd and "pa_count_cells_em_called(idx, h," in amd
    assert pa.lib().pa_abi_version() == 1


def test_every_entry_point_is_named(built):
    src = (helpers.ROOT / "integration" / "c" / "abi_check.c").read_text()
    for fn in ENTRY_POINTS:
        assert fn + "(" in src and fn in pa._ffi.SIGNATURES, fn
    assert "bus_knee.hip" in helpers._build.HIP_SOURCES and "bus_knee_host.cpp" in helpers._build.HOST_SOURCES


def test_defaults_and_tsv_writer(built, tmp_path):
    p = pa._ffi.KneeParams()
    pa.lib().pa_knee_default_params(C.byref(p))
    assert {k: getattr(p, k) for k in km.DEFAULTS} == km.DEFAULTS and list(p.reserved) == [0, 0, 0]
    rows, _, _ = km.knee(kc.from_umis([3, 1, 2, 7]), mode="min", min_umis=2)
    pa.write_barcode_ranks_tsv(np.array(rows, pa.BARCODE_ROW_DTYPE), 5, tmp_path / "ranks.tsv")
    assert (tmp_path / "ranks.tsv").read_text() == km.ranks_tsv(rows, 5)
    pa.write_barcode_ranks_tsv(np.zeros(0, pa.BARCODE_ROW_DTYPE), 5, tmp_path / "empty.tsv")
    assert (tmp_path / "empty.tsv").read_text() == km.TSV_HEADER
    with pytest.raises(TypeError):
        pa.bus_knee(np.zeros(0, pa.BUS_RECORD_DTYPE), 4, 4, None, upper=3)


def test_refusals_come_before_any_device_call(built):
    """every host argument is checked first: without a GPU a VALID call gets PA_ERR_NO_DEVICE, an invalid one its own code; with a GPU the
    valid call (no index handle) is refused for the null index"""
    E = pa._ffi
    valid = E.PA_ERR_NO_DEVICE if pa.lib().pa_device_count() < 1 else E.PA_ERR_INVALID_ARG
    bc_len, umi_len = 8, 6
    rec = kc.from_umis([3, 1, 2, 7, 1])
    n = len(rec)

    def knee_refused(records, *needles, code=E.PA_ERR_INVALID_ARG, lens=(bc_len, umi_len), **params):
        with pytest.raises(pa.PaError) as e:
            pa.bus_knee(kc.to_array(records), lens[0], lens[1], None, **params)
        assert e.value.code == code, str(e.value)
        for s in needles:
            assert s in str(e.value), (s, str(e.value))

    def keep_refused(records, barcodes, *needles, code=E.PA_ERR_INVALID_ARG, lens=(bc_len, umi_len)):
        with pytest.raises(pa.PaError) as e:
            pa.bus_keep(kc.to_array(records), np.array(barcodes, np.uint64), lens[0], lens[1], None)
        assert e.value.code == code, str(e.value)
        for s in needles:
            assert s in str(e.value), (s, str(e.value))

    for records in (rec, []):                                          # n = 0 is a valid call too
        knee_refused(records, code=valid)
        keep_refused(records, [1, 4], code=valid)
        keep_refused(records, [], code=valid)                          # an empty list is legal
    for field in ("lower", "divisor", "min_umis", "expected_cells"):
        knee_refused(rec, field, **{field: 0})
    knee_refused(rec, "mode", mode=3)
    for at in (0, n // 2, n - 1):                                      # each invalid-record kind at the first, a middle and the last record
        for field, value, word in ((0, 4 ** bc_len, "barcode"), (1, 4 ** umi_len, "UMI")):
            bad = [list(r) for r in rec]
            bad[at][field] = value
            knee_refused(bad, "record %d:" % at, word)
            keep_refused(bad, [1], "record %d:" % at, word)
        if at:
            bad = list(rec)
            bad[at] = bad[at - 1]
            knee_refused(bad, "record %d: not above record %d" % (at, at - 1))
            keep_refused(bad, [1], "record %d: not above record %d" % (at, at - 1))
    barcodes = [1, 4, 7, 10, 13, 4 ** bc_len - 1]
    for at in (0, 3, 5):
        bad = list(barcodes)
        bad[at] = 4 ** bc_len
        keep_refused(rec, bad, "entry %d:" % km.check_list(bad, bc_len))
        if at:
            bad = list(barcodes)
            bad[at] = bad[at - 1]
            keep_refused(rec, bad, "entry %d:" % at)
            bad[at] = 0
            keep_refused(rec, bad, "entry %d:" % at)
    for lens in ((0, 4), (4, 0), (17, 16), (32, 1)):
        knee_refused(rec, "barcode length", code=E.PA_ERR_UNSUPPORTED, lens=lens)
        keep_refused(rec, [1], "barcode length", code=E.PA_ERR_UNSUPPORTED, lens=lens)
    arr = kc.to_array(rec)
    n_rows, n_called, n_out = C.c_uint64(5), C.c_uint64(5), C.c_uint64(5)
    assert pa.lib().pa_bus_knee_records(None, arr.ctypes.data, 2 ** 31, bc_len, umi_len, None, None, 0, C.byref(n_rows), None, 0, C.byref(n_called), None) == E.PA_ERR_UNSUPPORTED
    assert n_rows.value == 0 and n_called.value == 0
    assert pa.lib().pa_bus_keep_records(None, arr.ctypes.data, 2 ** 31, bc_len, umi_len, None, 0, None, 0, C.byref(n_out), None) == E.PA_ERR_UNSUPPORTED and n_out.value == 0
    for call in (lambda: pa.lib().pa_bus_knee(None, None, None, 0, C.byref(n_rows), None, 0, C.byref(n_called), None), lambda: pa.lib().pa_bus_keep(None, None, 0, None)):
        with pytest.raises(pa.PaError) as e:
            pa.check(call())
        assert e.value.code == E.PA_ERR_INVALID_ARG
