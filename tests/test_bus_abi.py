"""The BUS entry points at the ABI's edges: integration/rust/src/amd_bus_ffi.rs (which cannot be compiled here) against the header,
prototype by prototype, struct and constant, with the comparison tools of tests/abi_sigs.py; pa_bus_record as ctypes and numpy see it
against the layout the header gives; the C client and the ctypes table name every entry point."""
import ctypes as C

import abi_sigs
import helpers

pa = helpers.pa
RUST = helpers.ROOT / "integration" / "rust" / "src" / "amd_bus_ffi.rs"
HEADER = helpers.ROOT / "include" / "pseudoaligner_amd.h"
ENTRY_POINTS = {"pa_bus_create", "pa_bus_add_device", "pa_bus_finish", "pa_bus_records", "pa_bus_ecs", "pa_bus_stats", "pa_bus_write", "pa_bus_destroy",
                "pa_write_bus"}


def test_rust_bus_binding_matches_the_header(monkeypatch):
    monkeypatch.setitem(abi_sigs.RUST_SCALARS, "PaBusRecord", "pa_bus_record")
    monkeypatch.setitem(abi_sigs.RUST_SCALARS, "PaBus", "pa_bus")
    header, rust = HEADER.read_text(), RUST.read_text()
    hp, rp = abi_sigs.header_prototypes(header), abi_sigs.rust_prototypes(rust)
    assert set(rp) == ENTRY_POINTS
    for name, sig in rp.items():
        assert hp[name] == sig, "%s: Rust says %s, the header %s" % (name, sig, hp[name])
    hs, rs = abi_sigs.header_structs(header), abi_sigs.rust_structs(rust)
    assert set(rs) == {"pa_bus_record"} and rs["pa_bus_record"] == hs["pa_bus_record"]
    assert [f for f, _ in hs["pa_bus_record"]] == ["barcode", "umi", "ec", "count", "flags", "pad"]
    hc, rc = abi_sigs.header_consts(header), abi_sigs.rust_consts(rust)
    assert rc == {"PA_BUS_STATS": 8} and hc["PA_BUS_STATS"] == 8 == pa._ffi.PA_BUS_STATS == len(pa._ffi.BUS_STAT_NAMES)
    # not vacuous: a drifted field order and a drifted argument are caught
    drift = rust.replace("pub ec: i32,\n    pub count: u32,", "pub count: u32,\n    pub ec: i32,")
    assert drift != rust and abi_sigs.rust_structs(drift)["pa_bus_record"] != hs["pa_bus_record"]
    drift = rust.replace("d_arena: *const u32, arena_len: u64, d_r1: *const u8", "d_arena: *const u32, d_r1: *const u8")
    assert drift != rust and abi_sigs.rust_prototypes(drift)["pa_bus_add_device"] != hp["pa_bus_add_device"]


def test_record_layout_as_python_sees_it(monkeypatch):
    monkeypatch.setitem(abi_sigs.C_SIZES, "int32_t", 4)
    offs, size = abi_sigs.layout(abi_sigs.header_structs(HEADER.read_text())["pa_bus_record"])
    assert size == 32 == C.sizeof(pa._ffi.BusRecord) == pa.BUS_RECORD_DTYPE.itemsize
    assert offs == dict(barcode=0, umi=8, ec=16, count=20, flags=24, pad=28)
    for f, off in offs.items():
        assert getattr(pa._ffi.BusRecord, f).offset == off == pa.BUS_RECORD_DTYPE.fields[f][1], f
    assert pa.BUS_RECORD_DTYPE.fields["ec"][0] == "<i4"


def test_c_client_and_ctypes_name_every_entry_point():
    src = (helpers.ROOT / "integration" / "c" / "abi_check.c").read_text()
    for name in ENTRY_POINTS:
        assert name + "(" in src and name in pa._ffi.SIGNATURES, name
    assert "LAYOUT_STRUCT(pa_bus_record)" in src and all("LAYOUT_FIELD(pa_bus_record, %s)" % f in src for f in ("barcode", "umi", "ec", "count", "flags", "pad"))
    amd = (helpers.ROOT / "integration" / "rust" / "src" / "amd.rs").read_text()
    assert "pub fn write_bus" in amd and "pa_write_bus(" in amd
