"""The UMI correction's rule (include/pseudoaligner_amd.h, "UMI correction on BUS records") in plain Python, written from that text: molecules with
n(m) and S(m), the neighbours of a molecule inside its barcode, the one-step decision in both modes, the rewritten and re-collapsed records and
the 15 stats. Integers only (Python's, so nothing overflows)."""
import numpy as np

BUS_RECORD_DTYPE = np.dtype([("barcode", "<u8"), ("umi", "<u8"), ("ec", "<i4"), ("count", "<u4"), ("flags", "<u4"), ("pad", "<u4")])
GREATEST, DIRECTIONAL = 0, 1
MODES = {"greatest": GREATEST, "directional": DIRECTIONAL}
CLAMP = 2 ** 32 - 1
STAT_NAMES = ("records_in", "reads_in", "molecules_in", "barcodes", "molecules_inert", "molecules_with_hamming1", "molecules_with_neighbour", "molecules_moved",
              "molecules_moved_onto_moved", "records_rewritten", "reads_moved", "records_out", "molecules_out", "largest_barcode", "barcodes_hbm")
BASES = "ACGT"


def pack(s):
    """2 bits per base, A=0 C=1 G=2 T=3, first base most significant"""
    v = 0
    for ch in s:
        v = v * 4 + BASES.index(ch)
    return v


def unpack(v, length):
    return "".join(BASES[(int(v) >> (2 * (length - 1 - j))) & 3] for j in range(length))


def gene_sets(ec_offsets, ec_ids, tx_gene):
    """G(e): the distinct genes of every ec"""
    return [frozenset(int(tx_gene[t]) for t in ec_ids[int(ec_offsets[e]):int(ec_offsets[e + 1])]) for e in range(len(ec_offsets) - 1)]


def hamming1(u, v, umi_len):
    """u and v differ in exactly one of the umi_len bases"""
    return sum(((u >> (2 * j)) & 3) != ((v >> (2 * j)) & 3) for j in range(umi_len)) == 1


def substitutions(u, umi_len):
    """the 3 umi_len UMIs one substitution away from u"""
    return [u & ~(3 << (2 * j)) | (b << (2 * j)) for j in range(umi_len) for b in range(4) if b != (u >> (2 * j)) & 3]


class Molecule:
    def __init__(self, barcode, umi):
        self.barcode, self.umi, self.records, self.n, self.S, self.target = barcode, umi, [], 0, None, None

    def add(self, ec, count, G):
        self.records.append((ec, count))
        self.n += count
        self.S = G[ec] if self.S is None else self.S & G[ec]

    @property
    def inert(self):
        return not self.S


def molecules(records, G):
    """the maximal runs of equal (barcode, UMI), in record order"""
    out = []
    for b, u, e, c in zip(records["barcode"].tolist(), records["umi"].tolist(), records["ec"].tolist(), records["count"].tolist()):
        if not out or (out[-1].barcode, out[-1].umi) != (b, u):
            out.append(Molecule(b, u))
        out[-1].add(e, c, G)
    return out


def decide(m, cell, umi_len, mode):
    """(target, any Hamming-1 UMI present, any neighbour) of molecule m in its barcode `cell` = {umi: molecule}: one step on the input state"""
    if m.inert:
        return m, False, False
    present = [cell[v] for v in substitutions(m.umi, umi_len) if v in cell]
    neighbours = [v for v in present if not v.inert and m.S & v.S]
    eligible = [v for v in neighbours if mode == GREATEST or v.n >= 2 * m.n - 1]
    return max([m] + eligible, key=lambda x: (x.n, x.umi)), bool(present), bool(neighbours)


def correct(records, ec_offsets, ec_ids, tx_gene, umi_len, mode="greatest", lds_cap=None):
    """-> (the output records as an array, the stats as a dict). lds_cap: the molecule count above which a barcode takes the HBM variant (stats[14]
    is a fact about the implementation; without it the model reports 0)"""
    mode = MODES.get(mode, mode)
    assert mode in (GREATEST, DIRECTIONAL)
    records = np.asarray(records, BUS_RECORD_DTYPE)
    mols = molecules(records, gene_sets(ec_offsets, ec_ids, tx_gene))
    cells = {}
    for m in mols:
        cells.setdefault(m.barcode, {})[m.umi] = m
    h1 = nb = 0
    for m in mols:
        m.target, a, b = decide(m, cells[m.barcode], umi_len, mode)
        h1 += a
        nb += b
    moved = [m for m in mols if m.target is not m]
    out = {}
    for m in mols:
        for ec, count in m.records:
            key = (m.barcode, m.target.umi, ec)          # the target's UMI: targets are not followed
            out[key] = out.get(key, 0) + count
    rows = sorted(out)
    arr = np.zeros(len(rows), BUS_RECORD_DTYPE)
    for i, key in enumerate(rows):
        arr[i] = (key[0], key[1], key[2], min(out[key], CLAMP), 0, 0)
    sizes = [len(c) for c in cells.values()]
    stats = dict(zip(STAT_NAMES, (
        len(records), sum(m.n for m in mols), len(mols), len(cells), sum(m.inert for m in mols), h1, nb, len(moved), sum(m.target.target is not m.target for m in moved),
        sum(len(m.records) for m in moved), sum(m.n for m in moved), len(rows), len({k[:2] for k in rows}), max(sizes, default=0),
        sum(s > lds_cap for s in sizes) if lds_cap is not None else 0)))
    return arr, stats


def decide_brute(m, cell, umi_len, mode):
    """decide() by comparing m with every molecule of its barcode base by base"""
    if m.inert:
        return m
    best = m
    for v in cell.values():
        if v is m or v.inert or not hamming1(m.umi, v.umi, umi_len) or not (m.S & v.S):
            continue
        if mode == DIRECTIONAL and v.n < 2 * m.n - 1:
            continue
        if (v.n, v.umi) > (best.n, best.umi):
            best = v
    return best
