"""Designed inputs of the gene counter, one per shape its kernels can take (csrc/genes.hip): hand-written records through
genes_model.directed. Every case checks on the model's side that it reaches the shape it was built for (check(name, model))."""
import re
from pathlib import Path

import numpy as np

import genes_model as gm

# the thresholds of rust-pseudoaligner_amd/csrc/genes_state.hpp, restated (test_genes_model.py reads the source lines back)
GN_LANE_RECORDS = 4
GN_WAVE_CELLS = 4
GN_WAVE_MAX = 512
GN_LDS_CAP = 8192
MAX_BARCODE_16 = 4 ** 16 - 1


def thresholds_in_source():
    text = (Path(__file__).resolve().parent.parent / "rust-pseudoaligner_amd" / "csrc" / "genes_state.hpp").read_text()
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"constexpr uint32_t (GN_\w+) = (\d+);", text)}


def _long_molecule(n_records, common, first_extra):
    """n records whose gene sets all hold `common` and one gene of their own: the intersection is `common`"""
    return [list(common) + [first_extra + r] for r in range(n_records)]


def molecules_case():
    """molecules of 1, 2, 3, 63, 64, 65 and 257 records; intersections empty, a singleton, equal to one of the ecs, and a new multi set equal
    to another molecule's single-record set; barcode 0 and the largest barcode of 16 bases"""
    x = 100                                                       # genes from here on are the records' own extras
    c0 = [
        [[1]],                                                    # one record, one gene
        [[1, 2]],                                                 # one record, a multi set: a row {1, 2} by reference
        [[1, 2, 3], [1, 2, 4]],                                   # two records -> {1, 2}: a NEW list equal to the row above (must merge)
        [[5, 6], [7, 8]],                                         # empty: dropped
        [[5, 6], [6, 7], [6, 9]],                                 # three records -> the singleton {6}
        [[2, 3], [2, 3, 4]],                                      # equal to one of its ecs
        _long_molecule(63, [1, 2], x),                            # wave tier, merges with {1, 2}
        _long_molecule(64, [3], x + 300),                         # -> singleton {3}
        _long_molecule(65, [], x + 600),                          # -> empty
        _long_molecule(257, [10, 11, 12], x + 900),
        [[10, 11, 12]],
    ]
    c1 = [[[1]], [[1, 2], [2, 1]], [[4, 5], [4, 5], [4, 5]], _long_molecule(GN_LANE_RECORDS, [7, 8], x), _long_molecule(GN_LANE_RECORDS + 1, [7, 8], x)]
    return gm.directed([(0, c0), (12345, [[[5, 6], [7, 8]]]), (MAX_BARCODE_16, c1)], 1300)


def umi1_case():
    return gm.directed([(0, [[[1]], [[1, 2]], [[2, 3], [2, 4]], [[1, 2]]]), (3, [[[2]], [[1, 2], [1, 2, 3]]])], 8, bc_len=1, umi_len=1)


def run_ends_case():
    """molecule runs that end at records 255, 256, 257 and at the last record"""
    mols = [_long_molecule(255, [1, 2], 10), [[1]], [[1, 3]], [[2, 3], [2, 4], [2, 3, 4]]]
    return gm.directed([(7, mols)], 300)


def empty_case():
    return gm.directed([], 4)


def one_record_case():
    return gm.directed([(9, [[[1, 2]]])], 4)


def all_dropped_case():
    return gm.directed([(1, [[[1], [2]]]), (2, [[[1, 2], [3]], [[0], [3]]])], 4)


def chain_cell(size, first_gene=0, singles=(3, 0, 1)):
    """a cell of |E| + rows == size exactly (size >= 3): rows {g_k, g_k+1}, one more {g_0, g_2} for an even size; n_S and u vary"""
    R = (size - 1) // 2
    mols = []
    for k in range(R):
        mols += [[[first_gene + k, first_gene + k + 1]]] * (1 + k % 3)
    if size % 2 == 0:
        mols.append([[first_gene, first_gene + 2]])
    for k in range(R + 1):
        mols += [[[first_gene + k]]] * singles[k % len(singles)]
    return mols


def bins_case(sizes):
    return gm.directed([(10 + j, chain_cell(s)) for j, s in enumerate(sizes)], max(sizes) // 2 + 3, umi_len=12)


WAVE_EDGE = (GN_WAVE_MAX - 1, GN_WAVE_MAX, GN_WAVE_MAX + 1)
CAP_EDGE = (GN_LDS_CAP - 1, GN_LDS_CAP, GN_LDS_CAP + 1, 2 * GN_LDS_CAP)


def rows_case():
    """multi rows of 2, 3, 63, 64, 65, 256 and 257 genes in one cell; gene 0 only in multi rows, u = 0 for most"""
    lens = (2, 3, 63, 64, 65, 256, 257)
    mols = [[list(range(k, k + n))] for k, n in enumerate(lens)] + [[[1]], [[1]], [[300]]]
    return gm.directed([(5, mols)], 400)


def degrees_case():
    """genes of degree 1, 63, 64, 65, 256 and 257 in one cell: hub gene h in d rows {h, own partner}"""
    mols, nxt = [], 10
    for h, d in enumerate((1, 63, 64, 65, 256, 257)):
        for _ in range(d):
            mols.append([[h, nxt]])
            nxt += 1
        mols += [[[h]]] * (h % 3)
    return gm.directed([(5, mols)], nxt)


def all_multi_case():
    """every row multi (u = 0 everywhere)"""
    return gm.directed([(1, [[[0, 1]], [[1, 2]], [[0, 1, 2]], [[0, 1]]])], 3)


def many_cells_case(n_cells):
    """small cells of the wave bin: a ragged last block for n_cells % GN_WAVE_CELLS != 0"""
    cells = []
    for j in range(n_cells):
        a, b, c = j % 5, 5 + j % 3, 8 + j % 2
        cells.append((j * 3 + 1, [[[a, b]], [[a]], [[b, c]], [[b]] if j % 2 else [[a, b]]]))
    return gm.directed(cells, 10)


def stop_case():
    """a cell that meets the rule at min_iters while it still moves (a near-tie: 400 shared molecules, singleton rows 2 : 1, every change
    far below alpha_change: only a freeze keeps it at its 50th iterate) beside one that takes long: two genes share 400 molecules and only
    20 singleton molecules speak for gene 0, so gene 1 decays by 400 / 420 per iteration and keeps the change above alpha_change until it
    has fallen below alpha_change_limit, some 200 iterations later"""
    fast = [[[0]]] * 2 + [[[1]]] + [[[0, 1]]] * 400
    slow = [[[0, 1]]] * 400 + [[[0]]] * 20 + [[[2]]]
    return gm.directed([(1, fast), (2, slow)], 3)


def truncation_case():
    """gene 1 is starved by gene 0 and falls below any limit; u values to cut exactly at a limit of 2"""
    return gm.directed([(1, [[[0]]] * 30 + [[[0, 1]]] * 2 + [[[2]]] * 2 + [[[3]]])], 4)


CASES = {
    "molecules": molecules_case, "umi1": umi1_case, "run_ends": run_ends_case, "empty": empty_case, "one_record": one_record_case,
    "all_dropped": all_dropped_case, "rows": rows_case, "degrees": degrees_case, "all_multi": all_multi_case,
    "wave_edge": lambda: bins_case(WAVE_EDGE), "cap_edge": lambda: bins_case(CAP_EDGE), "one_cell": lambda: bins_case((9,)),
    "ragged": lambda: many_cells_case(3 * GN_WAVE_CELLS + 1), "stop": stop_case, "truncation": truncation_case,
}
# the cases whose cells take part in the step / 200-step / independence tests (all that have multi rows and are quick in the model)
EM_CASES = ("molecules", "umi1", "run_ends", "rows", "degrees", "all_multi", "wave_edge", "cap_edge", "one_cell", "ragged", "stop", "truncation")
_cache = {}


def case(name):
    if name not in _cache:
        _cache[name] = CASES[name]()
    return _cache[name]


def model(name, **params):
    key = (name, tuple(sorted(params.items())))
    if key not in _cache:
        _cache[key] = gm.Model(*case(name), **params)
    return _cache[key]


def check(name, m):
    """the shape the case was built for, on the model's side"""
    st, sizes = m.stats, sorted(c.size for c in m.cells)
    if name == "molecules":
        rec = case(name)[0]
        runs = Counter_runs(rec)
        assert {1, 2, 3, 63, 64, 65, 257, GN_LANE_RECORDS, GN_LANE_RECORDS + 1} <= set(runs)
        assert st["molecules_dropped"] == 3 and st["cells"] == 2 and m.barcodes.tolist() == [0, MAX_BARCODE_16]
        c0 = m.cells[0]
        assert dict(c0.multi)[(1, 2)] == 3 and dict(c0.multi)[(10, 11, 12)] == 2 and c0.u[6] == 1 and c0.u[3] == 1 and dict(c0.multi)[(2, 3)] == 1
    elif name == "umi1":
        assert st["cells"] == 2 and st["multi_gene_molecules"] >= 2
    elif name == "run_ends":
        rec = case(name)[0]
        ends = np.flatnonzero(np.append(rec["umi"][1:] != rec["umi"][:-1], True)) + 1
        assert {255, 256, 257, len(rec)} <= set(ends.tolist())
    elif name == "empty":
        assert st["records"] == 0 and st["cells"] == 0
    elif name == "one_record":
        assert st["records"] == 1 and st["multi_rows"] == 1
    elif name == "all_dropped":
        assert st["molecules"] == 3 and st["molecules_dropped"] == 3 and st["cells"] == 0
    elif name == "rows":
        assert {2, 3, 63, 64, 65, 256, 257} <= {len(s) for s, _ in m.cells[0].multi} and 0 not in m.cells[0].u
    elif name == "degrees":
        c = m.cells[0]
        assert np.diff(c.t_ptr)[:6].tolist() == [1, 63, 64, 65, 256, 257]
    elif name == "all_multi":
        assert not m.cells[0].u and st["unique_gene_molecules"] == 0
    elif name == "wave_edge":
        assert sizes == sorted(WAVE_EDGE)
    elif name == "cap_edge":
        assert sizes == sorted(CAP_EDGE)
    elif name == "one_cell":
        assert st["cells"] == 1 and st["cells_with_multi_rows"] == 1
    elif name == "ragged":
        assert st["cells_with_multi_rows"] % GN_WAVE_CELLS == 1 and st["cells_with_multi_rows"] > GN_WAVE_CELLS and max(sizes) <= GN_WAVE_MAX
    elif name == "stop":
        assert st["cells_with_multi_rows"] == 2
    elif name == "truncation":
        assert m.cells[0].u[2] == 2 and m.cells[0].u[3] == 1


def Counter_runs(rec):
    """lengths of the (barcode, UMI) runs"""
    head = np.append(True, (rec["umi"][1:] != rec["umi"][:-1]) | (rec["barcode"][1:] != rec["barcode"][:-1]))
    return np.diff(np.append(np.flatnonzero(head), len(rec))).tolist()


def batch_of(names, seed=5):
    """all cells of the named cases in one input: barcodes reassigned by a shuffle, so that every cell gets new neighbours. -> (input, [(name,
    barcode in its case, barcode in the batch)]); a barcode whose molecules are all dropped is no cell in either"""
    rng = np.random.RandomState(seed)
    parts = []
    for name in names:
        rec, off, ids, tx_gene, ng, _, _ = case(name)
        G = [tuple(int(t) for t in ids[int(off[e]):int(off[e + 1])]) for e in range(len(off) - 1)]
        for b in sorted(set(rec["barcode"].tolist())):
            parts.append((name, b, rec[rec["barcode"] == b], G))
    new_bc = rng.permutation(len(parts)) * 7 + 1
    ecs, rows, where = {}, [], []
    for (name, k, rec, G), b in zip(parts, new_bc):
        where.append((name, k, int(b)))
        for r in rec:
            tx = G[int(r["ec"])]
            ecs.setdefault(tx, None)
            rows.append((int(b), int(r["umi"]), tx, int(r["count"])))
    order = sorted(ecs)
    number = {tx: e for e, tx in enumerate(order)}
    out = np.zeros(len(rows), gm.BUS_RECORD_DTYPE)
    for i, (b, u, e, c) in enumerate(sorted((b, u, number[tx], c) for b, u, tx, c in rows)):
        out[i] = (b, u, e, c, 0, 0)
    ng = max(case(n)[4] for n in names)
    off = np.cumsum([0] + [len(tx) for tx in order]).astype(np.uint64)
    ids = np.array([t for tx in order for t in tx], np.uint32)
    return (out, off, ids, np.repeat(np.arange(ng, dtype=np.uint32), 2), ng, 16, 12), where
