"""The single-cell UMI counter (pa_cell_counter, csrc/barcode_counts.hip) at the edges its code has branches and arithmetic for, with no
aligner in the loop: the tests write the mapping's records themselves (cells_model.directed_case), so every (cell, gene, UMI, reads) is
chosen exactly. Every case equals the pure-Python model in the matrix and all ten stats, and first shows on the model's side alone that it
reaches the path it is named for. All integers: equality, no tolerance."""

import numpy as np
import pytest

import cells_model as cm
import helpers

pa = helpers.pa
pytestmark = pytest.mark.gpu

_cache = {}


def _setup():
    """the gencode_small index at K = 24 on the GPU: (host index, aligner, HostIndex.arrays())"""
    if "ix" not in _cache:
        host = pa.build_index(str(helpers.FASTA), 24, 8)
        _cache["ix"] = (host, pa.Pseudoaligner(host), host.arrays())
        assert cm.RESULT_DTYPE == pa.RESULT_DTYPE and cm.CLASS_REF == pa.PA_CLASS_REF and cm.MAPPED_BIT == pa.PA_MAPPED_BIT
    return _cache["ix"]


def _counter(case):
    host, al, _ = _setup()
    return pa.CellCounter(al, host, case["tx_gene"], case["num_genes"], case["whitelist"], case["bc_len"], case["umi_len"])


def _feed(counter, r1, records, arena):
    """one batch: the records, the arena and the R1 text (plus the 8 bytes of padding the other tests give it) uploaded as they are"""
    import torch
    if len(r1) == 0:
        counter.add_device(0, 0, 0, 0, 0)
        return
    text, off = pa.concat_reads(r1)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).cuda()
    d = [up(records), up(arena), up(np.concatenate([text, np.zeros(8, np.uint8)])), up(off)]
    torch.cuda.synchronize()
    counter.add_device(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), len(r1))


def _result(counter):
    cell, gene, umis = counter.matrix()
    return list(zip(cell.tolist(), gene.tolist(), umis.tolist())), counter.stats()


def _reads(case, seed=0):
    return cm.directed_case(case["molecules"], _setup()[2], case["tx_gene"], case["whitelist"], seed)


def _model(case, r1, mapping):
    want = cm.count(r1, mapping, case["tx_gene"], case["whitelist"], case["bc_len"], case["umi_len"])
    st = want[1]
    assert st["reads"] == st["barcode_invalid"] + st["umi_invalid"] + st["not_confidently_mapped"] + st["reads_counted"]
    return want


def _gpu(case, batches):
    """a fresh counter fed the batches [(r1, records, arena)] -> (matrix, stats)"""
    counter = _counter(case)
    for r1, records, arena in batches:
        _feed(counter, r1, records, arena)
    return _result(counter)


def _check(case, seed=0):
    r1, records, arena, mapping = _reads(case, seed)
    want = _model(case, r1, mapping)
    got = _gpu(case, [(r1, records, arena)])
    assert got[1] == want[1]
    assert got[0] == want[0]
    return want


# ---- widths of the key's fields ----
@pytest.mark.parametrize("name", list(cm.WIDTH_SHAPES))
def test_field_widths(name):
    case = cm.widths_case(name, _setup()[2])
    n_wl, bc_len, num_genes, umi_len = cm.WIDTH_SHAPES[name]
    lay = cm.key_layout(n_wl, num_genes, umi_len)
    tx_gene = case["tx_gene"]
    lo, hi = int(tx_gene.min()), int(tx_gene.max())
    assert hi == num_genes - 1 and lo == 0
    if name == "key_2_bits":
        assert lay["key_bits"] == 2 and lay["cell_bits"] + lay["gene_bits"] == 0 and lay["end_bit3"] == 1
    elif name == "cell_shift_64":
        assert lay["cell_shift"] == 64 and lay["key_bits"] == 64 and hi == 0xFFFFFFFC
    elif name == "key_64_bits":
        assert lay["key_bits"] == 64 and lay["cell_bits"] == 2 and lay["gene_bits"] == 30
    elif name == "key_equals_sentinel":
        assert cm.molecule_key(lay, n_wl - 1, hi, "T" * umi_len) == lay["sentinel"]
    elif name == "no_power_of_two":
        assert all(v & (v - 1) for v in (n_wl, num_genes, umi_len)) and lay["sentinel"] > cm.molecule_key(lay, n_wl - 1, hi, "T" * umi_len)
    want_m, want_s = _check(case)
    # both cells, both genes and the all-T UMI's key reach the matrix side (not only the dropped side)
    assert {c for c, _, _ in want_m} == {0, n_wl - 1} | ({65533, 16383} if name == "every_barcode_whitelisted" else set())
    assert {g for _, g, _ in want_m} == {lo, hi}
    assert want_s["reads_counted"] > 0 and want_s["umis_in_matrix"] > 0
    if name == "key_equals_sentinel":
        assert (n_wl - 1, hi) in {(c, g) for c, g, _ in want_m}
    if name == "every_barcode_whitelisted":   # no barcode can be corrected: a substitution is another cell, an N has four fillers
        assert want_s["barcode_corrected"] == 0 and want_s["barcode_invalid"] == 1 and want_s["barcode_exact"] == want_s["reads"] - 1


# ---- a valid key equal to the sentinel ----
@pytest.mark.parametrize("survives", [False, True])
def test_sentinel_collision(survives):
    case = cm.sentinel_case(_setup()[2], survives)
    lay = cm.key_layout(4, 4, 4)
    assert cm.molecule_key(lay, 3, 3, "TTTT") == lay["sentinel"] == 0xFFF and (3 << lay["gene_bits"] | 3) == lay["sentinel3"] == 0xF
    want_m, want_s = _check(case)
    assert want_s["umi_invalid"] > 0 and want_s["not_confidently_mapped"] > 0 and want_s["molecules_lost_to_conflicts"] >= 3
    cells_genes = {(c, g) for c, g, _ in want_m}
    if survives:
        assert (3, 3) in cells_genes and (3, 2) not in cells_genes
    else:
        assert (3, 3) not in cells_genes and (3, 2) in cells_genes


# ---- the seam between the lane-shuffle path (<= 64 UMIs) and the binary-search path ----
def test_segment_seam():
    case = cm.seam_case(_setup()[2])
    L = case["umi_len"]
    packed = {cell: {cm.pack(u): n for u, n in umis.items()} for cell, umis in case["segments"].items()}
    assert [len(packed[i]) for i in range(8)] == list(cm.SEAM_SIZES) and len(packed[8]) == 64 and len(packed[9]) == 65
    for cell, umis in packed.items():
        if len(umis) >= 63:
            assert cm.segment_features(umis, L) >= cm.SEAM_FEATURES, (cell, cm.SEAM_FEATURES - cm.segment_features(umis, L))
    # the same UMIs and counts as a 64-segment and inside a 65-segment: the same moves
    m64, m65 = cm.umi_moves(packed[8], L), cm.umi_moves(packed[9], L)
    pad = cm.pack(case["pad"])
    assert m65[pad] == pad and all(m65[u] == m64[u] for u in packed[8]) and any(m64[u] != u for u in packed[8])
    want_m, want_s = _check(case)
    assert cm.largest_group == 257
    # which UMI a move ends on shows through the second gene's probes (cells_model.seam_segment): all of them are lost, in the cells of
    # the lane-shuffle path and in those of the binary-search path alike
    assert {g for _, g, _ in want_m} == {0} and want_s["molecules_lost_to_conflicts"] == 3 * 8
    by_cell = {c: n for c, _, n in want_m}
    assert by_cell[9] == by_cell[8] + 1 == by_cell[3] + 1


# ---- more segments than the correction kernel has waves ----
def test_stride_loop():
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    case = cm.stride_case(_setup()[2], cus)
    r1, records, arena, mapping = _reads(case)
    want_m, want_s = _model(case, r1, mapping)
    waves = 32 * cus * 4   # the grid: at most 32 blocks per CU, 4 waves each
    assert case["segs"] == len(want_m) > waves and case["segs"] - 100 >= waves   # every segment is its own (cell, gene); the last 100 lie in the second round
    assert want_s["umis_corrected"] >= len(case["paired"]) >= 100 + case["segs"] // 97
    assert 70000 < len(r1) < 120000 * max(1, cus // 256)
    got = _gpu(case, [(r1, records, arena)])
    assert got[1] == want_s
    assert got[0] == want_m


# ---- degenerate batches, one counter each ----
def test_degenerate_batches():
    host, al, ix = _setup()
    L = pa.lib()
    singles = cm.singleton_classes(ix)[:3]
    tx_gene = np.zeros(ix["num_transcripts"], np.uint32)
    for g, (_, t) in enumerate(singles):
        tx_gene[t] = g
    cls = [c for c, _ in singles]
    case = dict(whitelist=["ACG", "CAT", "GGA", "TTC", "TAG"], bc_len=3, umi_len=6, num_genes=3, tx_gene=tx_gene)
    zero = dict.fromkeys(cm.STAT_NAMES, 0)
    build = lambda molecules, seed=0: cm.directed_case(molecules, ix, tx_gene, case["whitelist"], seed)
    model = lambda r1, mapping: _model(case, r1, mapping)

    # nothing added
    assert _gpu(case, []) == ([], zero)
    # a batch of no reads, null pointers
    assert _gpu(case, [([], None, None)]) == ([], zero)
    # a first batch in which every read drops (one of each fate), then a counting one
    dropped = build([("AAA", cls[0], "ACGTAC", 1), (0, cls[0], "ACNTAC", 1), (0, None, "ACGTAC", 1), (1, cls[1], "ACGTAC", 1, "CA")])
    counting = build([(0, cls[0], "ACGTAC", 2), (4, cls[2], "TTTTTT", 1)])
    want = model(dropped[0] + counting[0], dropped[3] + counting[3])
    assert model(dropped[0], dropped[3])[1]["reads_counted"] == 0 and want[1]["barcode_invalid"] == 2 and want[1]["umi_invalid"] == 1
    assert want[1]["not_confidently_mapped"] == 1 and want[1]["reads_counted"] == 3
    assert _gpu(case, [dropped[:3], counting[:3]]) == want
    # ... and a batch of dropped reads alone: an empty matrix
    assert _gpu(case, [dropped[:3]]) == model(dropped[0], dropped[3]) and model(dropped[0], dropped[3])[0] == []
    # one read
    one = build([(4, cls[2], "TTTTTT", 1)])
    assert model(one[0], one[3])[0] == [(4, 2, 1)]
    assert _gpu(case, [one[:3]]) == model(one[0], one[3])
    # twelve growing batches = the same reads in one batch. Every batch holds distinct molecules of one read; a molecule comes again
    # in the batch after its own, so equal keys meet across batches only.
    rng = np.random.default_rng(21)
    sizes = [1, 2, 3, 10, 12, 40, 45, 150, 160, 500, 520, 1600]
    batches, carry = [], []
    for j, size in enumerate(sizes):
        fresh = {("".join(cm.BASES[x] for x in rng.integers(0, 4, 6)), int(rng.integers(5)), int(rng.integers(3))) for _ in range(size)}
        mols = sorted(fresh | set(carry))
        batches.append(build([(cell, cls[g], umi, 1) for umi, cell, g in mols], seed=j))
        carry = mols[: len(mols) // 3]
    outgrown, doubled = cm.accumulator_growth([(len(b[0]), len(b[0])) for b in batches])
    assert outgrown >= 3 and doubled >= 1 and len(batches) == 12
    all_r1, all_map = sum((b[0] for b in batches), []), sum((b[3] for b in batches), [])
    want = model(all_r1, all_map)
    assert want[1]["umis_corrected"] > 0 and want[1]["molecules_lost_to_conflicts"] > 0
    assert _gpu(case, [b[:3] for b in batches]) == want
    # (one batch: the arenas are empty but for their padding word, the records hold class references only)
    assert all(len(b[2]) == 1 for b in batches)
    assert _gpu(case, [(all_r1, np.concatenate([b[1] for b in batches]), batches[0][2])]) == want
    # every molecule lost to a conflict: ties on every (cell, UMI)
    lost = build([(c, cls[g], umi, 2) for c, umi in ((0, "ACGTAC"), (3, "TTTTTT"), (4, "GATTAC")) for g in (0, 2)])
    want = model(lost[0], lost[3])
    assert want[0] == [] and want[1]["molecules_lost_to_conflicts"] == 6 and want[1]["reads_counted"] == 12
    assert _gpu(case, [lost[:3]]) == want
    # finish twice: the same count; a matrix buffer one entry too small
    counter = _counter(case)
    _feed(counter, *counting[:3])
    assert counter.finish() == counter.finish() == 2
    buf = [np.zeros(2, np.uint32) for _ in range(3)]
    assert L.pa_cell_counter_matrix(counter._h, buf[0].ctypes.data, buf[1].ctypes.data, buf[2].ctypes.data, 1) == pa._ffi.PA_ERR_BUFFER_TOO_SMALL
    assert L.pa_cell_counter_matrix(counter._h, buf[0].ctypes.data, buf[1].ctypes.data, buf[2].ctypes.data, 2) == pa._ffi.PA_OK
    assert list(zip(*(b.tolist() for b in buf))) == model(counting[0], counting[3])[0]
    assert counter.stats() == model(counting[0], counting[3])[1]


# ---- what read_gene makes of a record ----
def test_read_gene_edges():
    host, al, ix = _setup()
    num_classes, num_tx = int(ix["num_classes"]), int(ix["num_transcripts"])
    tx_gene = (np.arange(num_tx) // 40).astype(np.uint32)   # 40 neighbours to a gene
    num_genes = int(tx_gene.max()) + 1
    case = dict(whitelist=["ACGT", "TTGA"], bc_len=4, umi_len=5, num_genes=num_genes, tx_gene=tx_gene)
    one_gene = list(range(80, 120))
    assert len(one_gene) == 40 and len({int(tx_gene[t]) for t in one_gene}) == 1 and tx_gene[120] != tx_gene[119]
    molecules = [(0, num_classes, "AAAAC", 2),                       # a reference past the index's classes
                 (0, 0x7FFFFFFF, "AAAAG", 1),
                 (0, num_classes - 1, "AAATT", 1),                   # (the last class there is)
                 (1, [3, num_tx], "CCCCA", 1),                       # a list with an id that is no transcript
                 (1, [num_tx], "CCCCG", 1),
                 (1, one_gene, "GGGGA", 3),                          # 40 ids of one gene
                 (1, one_gene[:39] + [120], "GGGGC", 2),             # ... the last one alone of another gene
                 (1, [120] + one_gene[1:], "GGGGT", 1),              # ... the first one alone
                 (0, [], "TTTTA", 2),                                # mapped, empty class
                 (0, ("unmapped", one_gene), "TTTTC", 1),            # not mapped, a class all the same
                 (0, ("unmapped", 5), "TTTTG", 1),
                 (0, [num_tx - 1], "TTTTT", 1)]                      # (the last transcript there is)
    case["molecules"] = molecules
    r1, records, arena, mapping = _reads(case)
    assert (records["class_off"] == (cm.CLASS_REF | num_classes)).sum() == 2 and (records["class_off"] == 0xFFFFFFFF).sum() == 1
    assert ((records["class_len"] == 0) & (records["mismatches"] >= cm.MAPPED_BIT)).sum() == 2
    assert ((records["class_len"] == 40) & (records["mismatches"] < cm.MAPPED_BIT)).sum() == 1
    want_m, want_s = _check(case)
    last_class = ix["ec_ids"][int(ix["ec_offset"][num_classes - 1]):int(ix["ec_offset"][num_classes])]
    counted = 3 + 1 + (1 if len({int(tx_gene[t]) for t in last_class}) == 1 else 0)
    assert want_s["reads_counted"] == counted and want_s["not_confidently_mapped"] == len(r1) - counted
    assert (1, int(tx_gene[80]), 1) in want_m and (0, int(tx_gene[num_tx - 1])) in {(c, g) for c, g, _ in want_m}


# ---- the R1 text ----
def test_r1_text():
    host, al, ix = _setup()
    (c0, t0), (c1, t1) = cm.singleton_classes(ix)[:2]
    tx_gene = np.zeros(ix["num_transcripts"], np.uint32)
    tx_gene[t1] = 1
    # AACCA and AACCG differ in the last base alone: an N there has two fillers
    case = dict(whitelist=["ACGTA", "TTGAC", "AACCA", "AACCG", "GTGTG"], bc_len=5, umi_len=4, num_genes=2, tx_gene=tx_gene)
    molecules = [(0, c0, "ACGT", 1),
                 ("acgta", c0, "ACGT", 1),      # lower case is no base: five Ns
                 ("aCGTA", c0, "ACGT", 1),      # one lower-case base = one N at the first position: corrected
                 ("ACGTa", c0, "GGGG", 1),      # ... at the last
                 ("NCGTA", c0, "CCCC", 1), ("ACGTN", c1, "CCCC", 2),
                 ("AACCN", c0, "ACGT", 1),      # two fillers: invalid
                 ("NTGAN", c0, "ACGT", 1),      # two Ns: invalid
                 ("TTGAC", c1, "acgt", 1),      # a lower-case UMI: invalid UMI
                 ("TTGAC", c1, "ACGn", 1),
                 (1, c1, "", 1, "TTGACACG"),    # one byte short
                 (1, c1, "", 1, ""),            # empty
                 (4, c1, "", 2, "GTGTGTTTTAAAA"),   # (longer than barcode + UMI: the tail is not read)
                 (4, c1, "TTTA", 1)]
    case["molecules"] = molecules
    r1, records, arena, mapping = cm.directed_case(molecules, ix, tx_gene, case["whitelist"], shuffle=False)
    # the last record of the buffer is an R1 of exactly bc_len + umi_len bytes
    assert len(r1[-1]) == 9 and r1[-1] == "GTGTGTTTA"
    want = _model(case, r1, mapping)
    st = want[1]
    assert st["barcode_corrected"] == 5 and st["barcode_invalid"] == 5 and st["umi_invalid"] == 2 and st["reads_counted"] == 9
    # cell 0: gene 0 has ACGT, GGGG and one read of CCCC, which gene 1's two reads of CCCC take; cell 4: TTTA moves to TTTT
    assert want[0] == [(0, 0, 2), (0, 1, 1), (4, 1, 1)] and st["umis_corrected"] == 1 and st["molecules_lost_to_conflicts"] == 1
    got = _gpu(case, [(r1, records, arena)])
    assert got == want
