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


# ---- the directed builder (cells_model.directed_case) and the named cases of tests/test_gpu_cells_edges.py: that each case has the
# property it claims is shown here, where no GPU is needed ----
def _decode(records, arena, ix):
    """records + arena -> [(mapped, transcript ids or "out of range")], read straight off the layout of pa_read_result"""
    off = ix["ec_offset"].astype(np.int64)
    out = []
    for r in records:
        mapped = bool(int(r["mismatches"]) >> 31)
        co, cl = int(r["class_off"]), int(r["class_len"])
        if co & 0x80000000:
            c = co & 0x7FFFFFFF
            ids = [int(t) for t in ix["ec_ids"][off[c]:off[c + 1]]] if c < ix["num_classes"] else "out of range"
            assert ids == "out of range" or len(ids) == cl
        else:
            ids = [int(t) for t in arena[co:co + cl]]
            if any(t >= ix["num_transcripts"] for t in ids):
                ids = "out of range"
        out.append((mapped, ids))
    return out


def test_directed_records_decode_to_their_mapping(small_index):
    ix = small_index(24).arrays()
    assert cm.RESULT_DTYPE == pa.RESULT_DTYPE and cm.CLASS_REF == pa.PA_CLASS_REF and cm.MAPPED_BIT == pa.PA_MAPPED_BIT
    nc, nt = int(ix["num_classes"]), int(ix["num_transcripts"])
    tx_gene = (np.arange(nt) // 40).astype(np.uint32)
    wl = ["ACGT", "TTGA"]
    molecules = [(0, 7, "AAAAC", 2), (1, nc - 1, "AAAAG", 1), (0, nc, "AAACC", 1), (0, 0x7FFFFFFF, "AAACG", 1), (1, [5, 9, 11], "CCCCA", 3),
                 (1, [nt], "CCCCG", 1), (1, [3, nt], "CCCCT", 1), (0, [], "TTTTA", 2), (0, None, "TTTTC", 1), (0, ("unmapped", [1, 2]), "TTTTG", 1),
                 (0, ("unmapped", 5), "TTTTT", 1), ("ACGN", 7, "AAAAC", 1), (1, 7, "", 2, "TTG")]
    r1, records, arena, mapping = cm.directed_case(molecules, ix, tx_gene, wl, seed=4)
    assert len(r1) == len(records) == len(mapping) == sum(m[3] for m in molecules) and arena.dtype == np.uint32 and len(arena) >= 1
    assert sorted(r1) == sorted(sum(([m[4] if len(m) > 4 else (m[0] if isinstance(m[0], str) else wl[m[0]]) + m[2]] * m[3] for m in molecules), []))
    decoded = _decode(records, arena, ix)
    several = 0
    for (mapped, ids), (m_mapped, m_ids) in zip(decoded, mapping):
        assert mapped == m_mapped
        if not mapped:
            assert m_ids == []
        elif ids == "out of range":   # the model is told "several genes"
            several += 1
            assert len({int(tx_gene[t]) for t in m_ids}) > 1 and cm.gene_of(True, m_ids, tx_gene) is None
        else:
            assert ids == m_ids
    assert several == 4
    # the same molecules, unshuffled: molecule order, and the records carry what the molecules say
    r1u, recu, arenau, mapu = cm.directed_case(molecules, ix, tx_gene, wl, shuffle=False)
    assert r1u[:3] == ["ACGTAAAAC", "ACGTAAAAC", "TTGAAAAAG"] and int(recu["class_off"][0]) == 0x80000007
    assert int(recu["class_len"][0]) == int(ix["ec_offset"][8] - ix["ec_offset"][7]) and int(recu["mismatches"][0]) >> 31 == 1
    with pytest.raises(ValueError):
        cm.directed_case([(0, nc, "AAAAA", 1)], ix, np.zeros(nt, np.uint32), wl)


def test_key_layout_follows_the_header():
    assert cm.key_layout(1, 1, 1) == dict(cell_bits=0, gene_bits=0, umi_bits=2, cell_shift=2, key_bits=2, end_bit=2, end_bit3=1, sentinel=3, sentinel3=1)
    lay = cm.key_layout(1, 0xFFFFFFFD, 16)
    assert (lay["cell_bits"], lay["gene_bits"], lay["cell_shift"], lay["key_bits"], lay["sentinel"]) == (0, 32, 64, 64, 2 ** 64 - 1)
    lay = cm.key_layout(4, 1 << 30, 16)
    assert (lay["cell_bits"], lay["gene_bits"], lay["key_bits"]) == (2, 30, 64) and cm.key_layout(4, 1 << 31, 16)["key_bits"] == 65
    assert cm.molecule_key(lay, 3, (1 << 30) - 1, "T" * 16) == 2 ** 64 - 1 and cm.molecule_key(lay, 1, 2, "AAAAAAAAAAAAAAAC") == (1 << 62) | (2 << 32) | 1
    assert cm.unpack(cm.pack("GATTACA"), 7) == "GATTACA" and cm.sub_at("ACGT", 3, 1) == "ACGA" and cm.hamming("ACGT", "ACCA") == 2


@pytest.mark.parametrize("name", list(cm.WIDTH_SHAPES))
def test_widths_cases_reach_their_edge(small_index, name):
    ix = small_index(24).arrays()
    case = cm.widths_case(name, ix)
    n_wl, bc_len, num_genes, umi_len = cm.WIDTH_SHAPES[name]
    assert len(case["whitelist"]) == n_wl == len(set(case["whitelist"])) and all(len(b) == bc_len for b in case["whitelist"])
    assert int(case["tx_gene"].max()) == num_genes - 1 and int(case["tx_gene"].min()) == 0
    lay = cm.key_layout(n_wl, num_genes, umi_len)
    assert lay["key_bits"] <= 64
    r1, records, arena, mapping = cm.directed_case(case["molecules"], ix, case["tx_gene"], case["whitelist"])
    matrix, st = cm.count(r1, mapping, case["tx_gene"], case["whitelist"], bc_len, umi_len)
    keys = {cm.molecule_key(lay, c, cm.gene_of(True, m[1] if not isinstance(m[1], int) else [cm.singleton_classes(ix)[0][1]], case["tx_gene"]), m[2])
            for m in case["molecules"] for c in [m[0]] if isinstance(c, int)}
    assert 0 in keys   # first cell, lowest gene, A..A
    assert max(keys) == cm.molecule_key(lay, n_wl - 1, num_genes - 1, "T" * umi_len)   # last cell, highest gene, T..T
    expect = {"key_2_bits": lay["key_bits"] == 2 and lay["end_bit3"] == 1 and lay["cell_bits"] + lay["gene_bits"] == 0,
              "cell_shift_64": lay["cell_shift"] == 64 and 0xFFFFFFFC in case["tx_gene"],
              "key_64_bits": lay["key_bits"] == 64 and max(keys) == 2 ** 64 - 1 and st["reads_counted"] > 0,
              "key_equals_sentinel": max(keys) == lay["sentinel"] and (n_wl - 1, num_genes - 1) in {(c, g) for c, g, _ in matrix},
              "no_power_of_two": all(v & (v - 1) for v in (n_wl, num_genes, umi_len)) and max(keys) < lay["sentinel"],
              "every_barcode_whitelisted": st["barcode_corrected"] == 0 and st["barcode_invalid"] == 1 and len({c for c, _, _ in matrix}) == 4}
    assert expect[name]
    assert {g for _, g, _ in matrix} == {0, num_genes - 1} and {0, n_wl - 1} <= {c for c, _, _ in matrix}


@pytest.mark.parametrize("survives", [False, True])
def test_sentinel_cases_collide(small_index, survives):
    ix = small_index(24).arrays()
    case = cm.sentinel_case(ix, survives)
    lay = cm.key_layout(len(case["whitelist"]), case["num_genes"], case["umi_len"])
    assert cm.molecule_key(lay, 3, 3, "TTTT") == lay["sentinel"] and ((3 << lay["gene_bits"]) | 3) == lay["sentinel3"]
    r1, records, arena, mapping = cm.directed_case(case["molecules"], ix, case["tx_gene"], case["whitelist"])
    matrix, st = cm.count(r1, mapping, case["tx_gene"], case["whitelist"], case["bc_len"], case["umi_len"])
    assert st["umi_invalid"] == 3 and st["not_confidently_mapped"] == 4 and st["molecules_lost_to_conflicts"] == 3
    assert (((3, 3, 1) in matrix) == survives) and (((3, 2, 1) in matrix) != survives)


def test_seam_case_segments(small_index):
    ix = small_index(24).arrays()
    case = cm.seam_case(ix)
    L = case["umi_len"]
    packed = {cell: {cm.pack(u): n for u, n in umis.items()} for cell, umis in case["segments"].items()}
    assert [len(packed[i]) for i in range(8)] == [1, 2, 63, 64, 65, 128, 129, 257] and (len(packed[8]), len(packed[9])) == (64, 65)
    for cell, umis in packed.items():
        if len(umis) >= 63:
            assert cm.segment_features(umis, L) >= cm.SEAM_FEATURES
    assert cm.segment_features(packed[1], L) == {"move_more", "move_first_base", "fewer_no_move"}
    assert all(cm.hamming(case["pad"], u) >= 2 for u in case["segments"][8]) and packed[8] == packed[3]
    m64, m65 = cm.umi_moves(packed[8], L), cm.umi_moves(packed[9], L)
    assert all(m65[u] == m64[u] for u in packed[8]) and sum(m64[u] != u for u in packed[8]) >= 4
    # the model's groups are these segments
    r1, records, arena, mapping = cm.directed_case(case["molecules"], ix, case["tx_gene"], case["whitelist"])
    matrix, st = cm.count(r1, mapping, case["tx_gene"], case["whitelist"], case["bc_len"], L)
    assert cm.largest_group == 257 and len(matrix) == 10 and st["reads_counted"] == st["reads"] == len(r1)
    assert st["umis_corrected"] == sum(v != u for umis in packed.values() for u, v in cm.umi_moves(umis, L).items())
    # the second gene's probes: on the tie's larger UMI (this gene's 6 reads beat its 4) and on b (x's 1 read ties its 1): in the eight
    # cells of 63 UMIs or more both probes and gene 0's molecule on b are lost, so gene 1 has no entry anywhere. A tie settled the other
    # way, or x moved on to c, would let a probe survive.
    assert [len(case["probes"][c]) for c in range(10)] == [0, 0] + [2] * 8 and case["probes"][8] == case["probes"][9] == case["probes"][3]
    for cell, pr in case["probes"].items():
        if pr:
            mv = cm.umi_moves(packed[cell], L)
            (big, n_big), (b, n_b) = [(cm.pack(u), n) for u, n in pr]
            assert sum(n for u, n in packed[cell].items() if mv[u] == big) == 6 > n_big == 4 and mv[big] == big
            assert sum(n for u, n in packed[cell].items() if mv[u] == b) == 1 == n_b and mv[b] != b
    assert {g for _, g, _ in matrix} == {0} and st["molecules_lost_to_conflicts"] == 3 * 8
    # a hand case of the feature finder: x(1) - b(4) - c(9) in a row
    assert cm.segment_features({cm.pack("AAAC"): 1, cm.pack("AAAA"): 4, cm.pack("CAAA"): 9}, 4) == {"move_more", "move_first_base", "move_last_base", "chain_one_step", "fewer_no_move"}


def test_stride_case_segments(small_index):
    ix = small_index(24).arrays()
    case = cm.stride_case(ix, 256)
    assert case["segs"] == 4 * 32 * 256 + 5000 and len(case["whitelist"]) * 4 >= case["segs"]
    groups = {}
    for cell, cls, umi, reads in case["molecules"]:
        groups.setdefault((cell, cls), {})[cm.pack(umi)] = reads
    assert len(groups) == case["segs"] and {len(g) for g in groups.values()} == {1, 2, 3}
    assert len(case["paired"]) == 100 + len([s for s in range(case["segs"] - 100) if s % 97 == 0])
    assert min(case["paired"][-100:]) >= 4 * 32 * 256   # the last hundred lie beyond one round of a 256-CU grid
    singles = [c for c, _ in cm.singleton_classes(ix)[:4]]
    for s in case["paired"]:
        g = groups[(s // 4, singles[s % 4])]
        assert len(g) == 2 and sum(v != u for u, v in cm.umi_moves(g, case["umi_len"]).items()) == 1
    assert 70000 < sum(m[3] for m in case["molecules"]) < 90000


def test_accumulator_growth_rule():
    assert cm.accumulator_growth([(4, 4)]) == (0, 0)
    assert cm.accumulator_growth([(4, 4), (3, 3)]) == (0, 1) and cm.accumulator_growth([(4, 4), (5, 5)]) == (1, 0)
    assert cm.accumulator_growth([(0, 0), (4, 2), (2, 2), (1, 1)]) == (0, 1)   # (distinct keys, not reads, fill it)
