"""Single-cell UMI counting, CPU tier: the pure-Python model (tests/cells_model.py) on hand cases that pin the semantics of
include/pseudoaligner_amd.h, the new entry points exported and bound, argument checks that need no GPU, whitelist file errors."""
import ctypes as C
import gzip

import numpy as np
import pytest

import cells_model as cm
import helpers

pa = helpers.pa

WL = ["AAAA", "CCCC", "GGGG", "TTTT"]
TXG = [0, 1, 2]   # transcript t belongs to gene t


def run(reads, whitelist=WL, tx_gene=TXG, bc_len=4, umi_len=4):
    """reads: (R1, transcript ids of the R2's class or None for unmapped)"""
    mapping = [(ids is not None, ids or []) for _, ids in reads]
    return cm.count([r for r, _ in reads], mapping, tx_gene, whitelist, bc_len, umi_len)


def test_chain_is_corrected_one_step_not_transitively():
    # A(3) - B(2) - C(1), A-C at distance 2: B -> A, C -> B: two molecules
    a, b, c = "AAAA", "AAAC", "AACC"
    reads = [("CCCC" + a, [0])] * 3 + [("CCCC" + b, [0])] * 2 + [("CCCC" + c, [0])]
    matrix, st = run(reads)
    assert matrix == [(1, 0, 2)]
    assert st["umis_corrected"] == 2 and st["reads_counted"] == 6


def test_equal_counts_go_to_the_greater_umi():
    reads = [("AAAA" + "ACGT", [1])] * 2 + [("AAAA" + "ACGG", [1])] * 2
    matrix, st = run(reads)
    assert matrix == [(0, 1, 1)] and st["umis_corrected"] == 1   # ACGG moves to ACGT (T > G)


def test_gene_conflicts():
    # 3 versus 1: gene 0 keeps the molecule; 2 versus 2: nobody does
    reads = [("GGGG" + "TTTT", [0])] * 3 + [("GGGG" + "TTTT", [1])] + [("TTTT" + "CCCC", [0])] * 2 + [("TTTT" + "CCCC", [2])] * 2
    matrix, st = run(reads)
    assert matrix == [(2, 0, 1)]
    assert st["molecules_lost_to_conflicts"] == 3 and st["umis_in_matrix"] == 1


def test_barcode_rules():
    wl = ["AAAA", "AACC", "GGGG", "TTTT"]
    reads = [("AAAC" + "ACGT", [0]),   # one substitution from AAAA and from AACC: invalid
             ("GGGA" + "ACGT", [0]),   # one substitution from GGGG: corrected
             ("GNGG" + "ACGT", [0]),   # one N: corrected to GGGG
             ("GNGN" + "ACGT", [0]),   # two Ns: invalid
             ("ANAA" + "ACGT", [0]),   # one N, candidates AAAA only (ACAA, AGAA, ATAA are not whitelisted): corrected
             ("TTTT" + "ACNT", [0]),   # N in the UMI
             ("TTT", [0]),             # short R1
             ("TTTT" + "ACGT", None),  # unmapped
             ("TTTT" + "ACGT", [0, 1]),   # two genes
             ("TTTT" + "ACGT", [])]   # empty class
    matrix, st = run(reads, whitelist=wl)
    assert st["barcode_invalid"] == 3 and st["barcode_corrected"] == 3 and st["barcode_exact"] == 4
    assert st["umi_invalid"] == 1 and st["not_confidently_mapped"] == 3 and st["reads_counted"] == 3
    assert st["reads"] == st["barcode_invalid"] + st["umi_invalid"] + st["not_confidently_mapped"] + st["reads_counted"]
    assert matrix == [(0, 0, 1), (2, 0, 1)]


def test_umi_packing_is_string_order():
    umis = ["AAAA", "AAAC", "ACGT", "CAAA", "TTTT", "GTCA"]
    assert sorted(umis) == sorted(umis, key=cm.pack) and cm.pack("ACGT") == 0b00011011


def test_render_files():
    mtx, bcs, feats = cm.render([(1, 0, 2), (1, 2, 1), (3, 1, 5)], WL, ["g0", "g1", "g2"])
    assert mtx == "%%MatrixMarket matrix coordinate integer general\n3 2 3\n1 1 2\n3 1 1\n2 2 5\n"
    assert bcs == "CCCC\nTTTT\n" and feats.splitlines()[1] == "g1\tg1\tGene Expression"


def test_new_symbols_are_exported_and_bound(built):
    lib = pa.lib()
    for name in ("pa_cell_counter_create", "pa_cell_counter_add_device", "pa_cell_counter_finish", "pa_cell_counter_matrix",
                 "pa_cell_counter_stats", "pa_cell_counter_destroy", "pa_whitelist_load", "pa_count_cells"):
        assert hasattr(lib, name) and name in pa._ffi.SIGNATURES
    assert hasattr(pa, "CellCounter") and hasattr(pa.Pseudoaligner, "count_cells")


def test_argument_checks_need_no_gpu(built, small_index, tmp_path):
    host = small_index(24)
    tx_gene, names = host.genes()
    L = pa.lib()
    out = C.c_void_p()
    tg = np.ascontiguousarray(tx_gene, np.uint32)
    assert L.pa_cell_counter_create(None, host._h, tg.ctypes.data, len(names), b"ACGT", 1, 4, 4, C.byref(out)) == pa._ffi.PA_ERR_INVALID_ARG
    for bc_len, umi_len in ((0, 4), (17, 4), (4, 0), (4, 17)):
        assert L.pa_cell_counter_create(None, host._h, tg.ctypes.data, len(names), b"ACGT", 1, bc_len, umi_len, C.byref(out)) == pa._ffi.PA_ERR_INVALID_ARG
    assert L.pa_cell_counter_create(None, None, tg.ctypes.data, len(names), b"ACGT", 1, 4, 4, C.byref(out)) == pa._ffi.PA_ERR_INVALID_ARG
    assert L.pa_cell_counter_add_device(None, None, None, None, None, 0, None) == pa._ffi.PA_ERR_INVALID_ARG
    n = C.c_uint64()
    assert L.pa_cell_counter_finish(None, C.byref(n)) == pa._ffi.PA_ERR_INVALID_ARG
    assert L.pa_cell_counter_stats(None, None) == pa._ffi.PA_ERR_INVALID_ARG
    assert L.pa_count_cells(None, host._h, b"r1", b"r2", b"wl", 16, 12, str(tmp_path).encode(), 1, None) == pa._ffi.PA_ERR_INVALID_ARG
    assert L.pa_count_cells(None, host._h, b"r1", b"r2", b"wl", 16, 0, str(tmp_path).encode(), 1, None) == pa._ffi.PA_ERR_INVALID_ARG
    if L.pa_device_count() < 1:   # without a GPU the checks above are all there is: nothing reached a device call
        with pytest.raises(pa.PaError):
            pa.Pseudoaligner(host)


def test_whitelist_load(built, tmp_path):
    p = tmp_path / "wl.txt"
    p.write_bytes(b"ACGTAC\r\nTTTTTT\nGGCAAC\n")
    assert pa.load_whitelist(p, 6) == ["ACGTAC", "TTTTTT", "GGCAAC"]
    g = tmp_path / "wl.txt.gz"
    g.write_bytes(gzip.compress(b"ACGTAC\nTTTTTT\n"))
    assert pa.load_whitelist(g, 6) == ["ACGTAC", "TTTTTT"]
    for text, line in ((b"ACGTAC\nTTTTT\n", 2), (b"ACGTAC\nTTNTTT\n", 2), (b"ACGTAC\nGGGGGG\nACGTAC\n", 3), (b"ACGTAC\n\nGGGGGG\n", 2),
                       (b"acgtac\n", 1)):
        p.write_bytes(text)
        with pytest.raises(pa.PaError) as e:
            pa.load_whitelist(p, 6)
        assert e.value.code == pa._ffi.PA_ERR_FORMAT and ("line %d" % line) in str(e.value), str(e.value)
    with pytest.raises(pa.PaError) as e:
        pa.load_whitelist(tmp_path / "missing.txt", 6)
    assert e.value.code == -2
