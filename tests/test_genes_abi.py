"""The gene counter at the ABI's edges: integration/rust/src/amd_genes_ffi.rs (which cannot be compiled here) against the header,
prototype by prototype, struct and constants, with the comparison tools of tests/abi_sigs.py; pa_genes_params as ctypes sees it; the
C client and the ctypes table name every entry point; the refusals that come before any device call."""
import ctypes as C

import numpy as np
import pytest

import abi_sigs
import genes_model as gm
import helpers

pa = helpers.pa
RUST = helpers.ROOT / "integration" / "rust" / "src" / "amd_genes_ffi.rs"
HEADER = helpers.ROOT / "include" / "pseudoaligner_amd.h"
ENTRY_POINTS = {"pa_genes_default_params", "pa_genes_create", "pa_genes_create_from_bus", "pa_genes_step", "pa_genes_run", "pa_genes_layout", "pa_genes_values",
                "pa_genes_cell_iters", "pa_genes_matrix", "pa_genes_stats", "pa_genes_write", "pa_genes_destroy", "pa_count_cells_em"}


def test_rust_genes_binding_matches_the_header(monkeypatch):
    for r, c in (("PaBusRecord", "pa_bus_record"), ("PaBus", "pa_bus"), ("PaGenes", "pa_genes"), ("PaGenesParams", "pa_genes_params")):
        monkeypatch.setitem(abi_sigs.RUST_SCALARS, r, c)
    header, rust = HEADER.read_text(), RUST.read_text()
    hp, rp = abi_sigs.header_prototypes(header), abi_sigs.rust_prototypes(rust)
    assert set(rp) == ENTRY_POINTS
    for name, sig in rp.items():
        assert hp[name] == sig, "%s: Rust says %s, the header %s" % (name, sig, hp[name])
    hs, rs = abi_sigs.header_structs(header), abi_sigs.rust_structs(rust)
    assert set(rs) == {"pa_genes_params"} and rs["pa_genes_params"] == hs["pa_genes_params"]
    assert [f for f, _ in hs["pa_genes_params"]] == ["alpha_limit", "alpha_change_limit", "alpha_change", "min_iters", "max_iters", "check_every", "mode", "reserved"]
    hc, rc = abi_sigs.header_consts(header), abi_sigs.rust_consts(rust)
    assert rc == {"PA_GENES_EM": 0, "PA_GENES_UNIQUE": 1, "PA_GENES_STATS": 16} and all(hc[k] == v for k, v in rc.items())
    assert pa._ffi.PA_GENES_STATS == 16 == len(pa._ffi.GENES_STAT_NAMES) and pa._ffi.GENES_MODES == {"em": hc["PA_GENES_EM"], "unique": hc["PA_GENES_UNIQUE"]}
    assert pa._ffi.GENES_STAT_NAMES[:12] == gm.STAT_NAMES
    # not vacuous: a drifted field order and a drifted argument are caught
    drift = rust.replace("pub check_every: u32,\n    pub mode: u32,", "pub mode: u32,\n    pub check_every: u32,")
    assert drift != rust and abi_sigs.rust_structs(drift)["pa_genes_params"] != hs["pa_genes_params"]
    drift = rust.replace("n_ecs: u32,\n", "n_ecs: u64,\n")
    assert drift != rust and abi_sigs.rust_prototypes(drift)["pa_genes_create"] != hp["pa_genes_create"]
    amd = (helpers.ROOT / "integration" / "rust" / "src" / "amd.rs").read_text()
    assert "pub fn count_cells_em" in amd and "pa_count_cells_em(idx, h," in amd


def test_params_layout_and_defaults(built):
    hs = abi_sigs.header_structs(HEADER.read_text())
    offs, size = abi_sigs.layout(hs["pa_genes_params"])
    P = pa._ffi.GenesParams
    assert C.sizeof(P) == size == 48
    for name, _ in P._fields_:
        assert getattr(P, name).offset == offs[name], name
    p = P()
    pa.lib().pa_genes_default_params(C.byref(p))
    q = pa._ffi.QuantParams()
    pa.lib().pa_quant_default_params(C.byref(q))
    for f in ("alpha_limit", "alpha_change_limit", "alpha_change", "min_iters", "max_iters", "check_every"):
        assert getattr(p, f) == getattr(q, f) == gm.DEFAULTS[f], f
    assert p.mode == pa._ffi.PA_GENES_EM and p.reserved == 0


def test_every_entry_point_is_named(built):
    src = (helpers.ROOT / "integration" / "c" / "abi_check.c").read_text()
    for fn in ENTRY_POINTS:
        assert fn + "(" in src and fn in pa._ffi.SIGNATURES, fn
    assert "LAYOUT_STRUCT(pa_genes_params)" in src and "LAYOUT_FIELD(pa_genes_params, mode)" in src


def _create(inp, **params):
    return pa.GeneCounter.from_arrays(None, *inp, **params)


def test_refusals_come_before_any_device_call(built):
    """every host argument is checked first: without a GPU a VALID call gets PA_ERR_NO_DEVICE, an invalid one PA_ERR_INVALID_ARG; with a GPU
    the valid call (no index handle) is refused for the null index"""
    E = pa._ffi
    no_gpu = pa.lib().pa_device_count() < 1
    inp = list(gm.directed([(1, [[[0]], [[0, 1]], [[1, 2], [1, 3]]]), (2, [[[2]], [[2, 3]]]), (3, [[[0, 1]]])], 4, bc_len=4, umi_len=4))
    n = len(inp[0])
    with pytest.raises(pa.PaError) as e:
        _create(inp)
    assert e.value.code == (E.PA_ERR_NO_DEVICE if no_gpu else E.PA_ERR_INVALID_ARG)

    def refused(changed, *needles, **params):
        with pytest.raises(pa.PaError) as e:
            _create(changed, **params)
        assert e.value.code == E.PA_ERR_INVALID_ARG, str(e.value)
        for s in needles:
            assert s in str(e.value), (s, str(e.value))

    for at in (0, n // 2, n - 1):                                  # each invalid-record kind at the first, a middle and the last record
        bad = [x.copy() if hasattr(x, "copy") else x for x in inp]
        bad[0]["ec"][at] = len(inp[1]) - 1                         # == n_ecs
        refused(bad, "record %d" % at, "ec")
        bad = [x.copy() if hasattr(x, "copy") else x for x in inp]
        bad[0]["ec"][at] = -1
        refused(bad, "record %d" % at)
        if at:
            bad = [x.copy() if hasattr(x, "copy") else x for x in inp]
            bad[0][at] = bad[0][at - 1]                            # equal to the record before: not STRICTLY ascending
            refused(bad, "record %d" % at)
            bad = [x.copy() if hasattr(x, "copy") else x for x in inp]
            bad[0]["barcode"][at] = 0                              # below the record before
            refused(bad, "record %d" % at)
    bad = list(inp)
    bad[3] = inp[3].copy()
    bad[3][5] = 4                                                  # tx_gene entry == num_genes
    refused(bad, "tx_gene[5]")
    for bc, umi in ((0, 4), (4, 0), (17, 16), (32, 1)):
        bad = list(inp)
        bad[5], bad[6] = bc, umi
        refused(bad, "barcode length")
    refused(inp, check_every=0)
    refused(inp, alpha_limit=float("nan"))
    refused(inp, alpha_change=-1.0)
    refused(inp, mode=2)
    with pytest.raises(TypeError):
        _create(inp, reserved=1)
    with pytest.raises(pa.PaError) as e:
        pa.GeneCounter.from_bus(None, inp[3], 4)
    assert e.value.code == E.PA_ERR_INVALID_ARG
