"""The BGZF entry points at the ABI's edges: integration/rust/src/amd_bgzf_ffi.rs (which cannot be compiled here) against the header,
prototype by prototype, struct and constants, with the comparison tools of tests/abi_sigs.py; the struct as ctypes and numpy see it against
what the C compiler laid out; without a GPU the device entry point refuses."""
import ctypes as C

import numpy as np
import pytest

import abi_sigs
import helpers

pa = helpers.pa
RUST = helpers.ROOT / "integration" / "rust" / "src" / "amd_bgzf_ffi.rs"
HEADER = helpers.ROOT / "include" / "pseudoaligner_amd.h"


def test_rust_bgzf_binding_matches_the_header(monkeypatch):
    monkeypatch.setitem(abi_sigs.RUST_SCALARS, "PaBgzfMember", "pa_bgzf_member")
    header, rust = HEADER.read_text(), RUST.read_text()
    hp, rp = abi_sigs.header_prototypes(header), abi_sigs.rust_prototypes(rust)
    assert set(rp) == {"pa_bgzf_scan", "pa_bgzf_inflate_device", "pa_inflate_status_name", "pa_process_reads_input_stats"}
    for name, sig in rp.items():
        assert hp[name] == sig, "%s: Rust says %s, the header %s" % (name, sig, hp[name])
    hs, rs = abi_sigs.header_structs(header), abi_sigs.rust_structs(rust)
    assert set(rs) == {"pa_bgzf_member"} and rs["pa_bgzf_member"] == hs["pa_bgzf_member"]
    hc, rc = abi_sigs.header_consts(header), abi_sigs.rust_consts(rust)
    assert len(rc) == 18 and all(hc.get(k) == v for k, v in rc.items()), {k: (v, hc.get(k)) for k, v in rc.items() if hc.get(k) != v}
    # the Python names of the statuses are the header's, in the header's order
    for code, name in enumerate(pa._ffi.INFLATE_STATUS_NAMES):
        assert hc["PA_INFLATE_" + name] == code
    assert len([k for k in hc if k.startswith("PA_INFLATE_")]) == len(pa._ffi.INFLATE_STATUS_NAMES)
    assert hc["PA_ERR_NOT_BGZF"] == pa._ffi.PA_ERR_NOT_BGZF
    # not vacuous: a drifted field order is caught
    drift = rust.replace("pub in_len: u32,\n    pub out_len: u32,", "pub out_len: u32,\n    pub in_len: u32,")
    assert drift != rust and abi_sigs.rust_structs(drift)["pa_bgzf_member"] != hs["pa_bgzf_member"]


def test_member_layout_as_python_sees_it(built):
    offs, size = abi_sigs.layout(abi_sigs.header_structs(HEADER.read_text())["pa_bgzf_member"])
    assert size == 40 == C.sizeof(pa._ffi.BgzfMember) == pa.BGZF_MEMBER_DTYPE.itemsize
    for f, off in offs.items():
        assert getattr(pa._ffi.BgzfMember, f).offset == off == pa.BGZF_MEMBER_DTYPE.fields[f][1], f
    assert pa.inflate_status_name(14) == "crc mismatch" and pa.inflate_status_name(99) == "unknown"


def test_inflate_without_a_gpu_refuses(built):
    if pa.lib().pa_device_count() > 0:
        pytest.skip("a GPU is present")
    import bgzf_cases as bc
    with pytest.raises(pa.PaError) as e:
        pa.bgzf_inflate(bc.bgzf(b"ACGT\n"))
    assert e.value.code == pa._ffi.PA_ERR_NO_DEVICE
