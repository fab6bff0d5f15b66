"""The gene counter's rules (include/pseudoaligner_amd.h, "cells x genes from BUS records") in plain numpy / Python, written from that
text: molecules, rows, the start point, one EM step in any float type, the stop rule per cell, truncation, the three files' text. Also
directed(): records, an ec table and tx_gene written by hand, with no aligner in the loop."""
from collections import Counter

import numpy as np

BUS_RECORD_DTYPE = np.dtype([("barcode", "<u8"), ("umi", "<u8"), ("ec", "<i4"), ("count", "<u4"), ("flags", "<u4"), ("pad", "<u4")])
DEFAULTS = dict(alpha_limit=1e-7, alpha_change_limit=1e-2, alpha_change=1e-2, min_iters=50, max_iters=10000, check_every=10, mode="em")
STAT_NAMES = ("records", "molecules", "molecules_dropped", "unique_gene_molecules", "multi_gene_molecules", "cells", "cells_with_multi_rows", "multi_rows",
              "multi_row_ids", "longest_multi_row", "largest_degree", "largest_cell")


def gene_sets(ec_offsets, ec_ids, tx_gene):
    """G(e): the ascending distinct genes of every ec"""
    return [tuple(sorted({int(tx_gene[t]) for t in ec_ids[int(ec_offsets[e]):int(ec_offsets[e + 1])]})) for e in range(len(ec_offsets) - 1)]


def molecules(records, G):
    """[(barcode, gene set)] of every molecule in record order; a dropped molecule has the empty set"""
    out = []
    i, n = 0, len(records)
    while i < n:
        j = i
        s = None
        while j < n and records["barcode"][j] == records["barcode"][i] and records["umi"][j] == records["umi"][i]:
            g = set(G[int(records["ec"][j])])
            s = g if s is None else s & g
            j += 1
        out.append((int(records["barcode"][i]), tuple(sorted(s))))
        i = j
    return out


class Cell:
    """one cell: u over all its genes, the multi rows in a fixed order, the incidence in local gene numbers of E"""

    def __init__(self, barcode, sets):
        self.barcode = barcode
        rows = Counter(sets)
        self.molecules = len(sets)
        self.u = {s[0]: n for s, n in rows.items() if len(s) == 1}
        self.multi = sorted((s, n) for s, n in rows.items() if len(s) >= 2)
        self.E = sorted({g for s, _ in self.multi for g in s})
        self.genes = sorted(set(self.u) | set(self.E))
        local = {g: k for k, g in enumerate(self.E)}
        self.row_n = np.array([n for _, n in self.multi], np.float64)
        self.row_ptr = np.cumsum([0] + [len(s) for s, _ in self.multi]).astype(np.int64)
        self.row_gene = np.array([local[g] for s, _ in self.multi for g in s], np.int64)
        row_of = np.repeat(np.arange(len(self.multi)), np.diff(self.row_ptr)) if self.multi else np.zeros(0, np.int64)
        order = np.argsort(self.row_gene, kind="stable")
        self.t_row = row_of[order]
        self.t_ptr = np.searchsorted(self.row_gene[order], np.arange(len(self.E) + 1)).astype(np.int64)
        self.u_E = np.array([self.u.get(g, 0) for g in self.E], np.float64)
        self.M = int(sum(n for _, n in self.multi))
        self.longest = max([len(s) for s, _ in self.multi], default=0)
        self.degree = int(np.max(np.diff(self.t_ptr))) if self.E else 0
        self.size = len(self.E) + len(self.multi) if self.multi else 0

    def start(self, mode="em"):
        if not self.multi:
            return self.u_E.copy()
        return self.u_E + float(self.M) / float(len(self.E)) if mode == "em" else self.u_E.copy()

    def step(self, alpha, dtype=np.float64):
        """one iteration over E in `dtype`"""
        a = np.asarray(alpha, dtype)
        if not self.multi:
            return a.copy()
        d = np.add.reduceat(a[self.row_gene], self.row_ptr[:-1])
        q = np.where(d > 0, self.row_n.astype(dtype) / np.where(d > 0, d, 1), dtype(0))
        s = np.add.reduceat(q[self.t_row], self.t_ptr[:-1])
        return self.u_E.astype(dtype) + a * s

    def run(self, alpha, par, dtype=np.float64):
        """the stop rule from alpha -> (final iterate before truncation, iterations, converged, smallest distance of a decision from its threshold)"""
        a = np.asarray(alpha, dtype)
        done, conv, margin = 0, False, np.inf
        if not self.multi or par["mode"] != "em":
            return a, 0, True, margin
        while done < par["max_iters"] and not conv:
            i = done + 1
            nxt = self.step(a, dtype)
            if (i >= par["min_iters"] and i % par["check_every"] == 0) or i == par["max_iters"]:
                big = nxt > par["alpha_change_limit"]
                rel = np.abs(nxt[big] - a[big]) / nxt[big]
                conv = not bool(np.any(rel > par["alpha_change"])) and i >= par["min_iters"]
                if rel.size:
                    margin = min(margin, float(np.min(np.abs(rel - par["alpha_change"]))))
                near = np.abs(nxt - par["alpha_change_limit"])
                margin = min(margin, float(np.min(near / par["alpha_change_limit"]))) if par["alpha_change_limit"] > 0 else margin
            a, done = nxt, i
        return a, done, conv, margin


def stop_rule_holds(prev, last, change_limit, change):
    big = last > change_limit
    return not bool(np.any(np.abs(last[big] - prev[big]) / last[big] > change))


class Model:
    def __init__(self, records, ec_offsets, ec_ids, tx_gene, num_genes, bc_len, umi_len, **params):
        self.par = dict(DEFAULTS, **params)
        self.num_genes, self.bc_len, self.umi_len = num_genes, bc_len, umi_len
        records = np.asarray(records, BUS_RECORD_DTYPE)
        self.G = gene_sets(ec_offsets, ec_ids, tx_gene)
        mols = molecules(records, self.G)
        kept = [(b, s) for b, s in mols if s]
        by_cell = {}
        for b, s in kept:
            by_cell.setdefault(b, []).append(s)
        self.cells = [Cell(b, by_cell[b]) for b in sorted(by_cell)]
        multi_cells = [c for c in self.cells if c.multi]
        self.stats = dict(zip(STAT_NAMES, (
            len(records), len(mols), len(mols) - len(kept), sum(len(s) == 1 for _, s in kept), sum(len(s) >= 2 for _, s in kept), len(self.cells), len(multi_cells),
            sum(len(c.multi) for c in self.cells), sum(int(c.row_ptr[-1]) for c in self.cells), max([c.longest for c in self.cells], default=0),
            max([c.degree for c in self.cells], default=0), max([c.size for c in self.cells], default=0))))
        self.barcodes = np.array([c.barcode for c in self.cells], np.uint64)
        self.cell = np.array([k for k, c in enumerate(self.cells) for _ in c.genes], np.uint32)
        self.gene = np.array([g for c in self.cells for g in c.genes], np.uint32)
        # where the genes of E lie in a cell's stretch of the value list
        self.base = np.cumsum([0] + [len(c.genes) for c in self.cells]).astype(np.int64)
        self.in_E = [np.searchsorted(c.genes, c.E).astype(np.int64) for c in self.cells]

    def _full(self, per_cell, dtype=np.float64):
        out = np.zeros(len(self.gene), dtype)
        for k, c in enumerate(self.cells):
            v = np.array([c.u.get(g, 0) for g in c.genes], dtype)
            if c.E:
                v[self.in_E[k]] = per_cell[k]
            out[self.base[k]:self.base[k + 1]] = v
        return out

    def _split(self, values, dtype=np.float64):
        values = np.asarray(values, dtype)
        return [values[self.base[k]:self.base[k + 1]][self.in_E[k]] for k in range(len(self.cells))]

    def start(self):
        """alpha over the (cell, gene) list self.cell / self.gene"""
        return self._full([c.start(self.par["mode"]) for c in self.cells])

    def step(self, values, dtype=np.float64):
        if self.par["mode"] != "em":
            return np.asarray(values, dtype).copy()
        return self._full([c.step(a, dtype) for c, a in zip(self.cells, self._split(values, dtype))], dtype)

    def iterate(self, n, dtype=np.float64):
        a = self._split(self.start(), dtype)
        if self.par["mode"] == "em":
            for _ in range(n):
                a = [c.step(x, dtype) for c, x in zip(self.cells, a)]
        return self._full(a, dtype)

    def iterate_per_cell(self, iters, dtype=np.float64):
        """cell k iterated iters[k] times from the start"""
        a = self._split(self.start(), dtype)
        for k, c in enumerate(self.cells):
            for _ in range(int(iters[k])):
                a[k] = c.step(a[k], dtype)
        return self._full(a, dtype)

    def run(self, values=None, dtype=np.float64):
        """-> (values after truncation, iterations per cell, converged per cell, the smallest margin of a stop decision)"""
        a = self._split(self.start() if values is None else values, dtype)
        res = [c.run(x, self.par, dtype) for c, x in zip(self.cells, a)]
        full = self._full([r[0] for r in res], dtype)
        full = np.where(full < self.par["alpha_limit"], dtype(0), full)
        return (full, np.array([r[1] for r in res], np.uint32), np.array([r[2] for r in res], bool), min([r[3] for r in res], default=np.inf))

    def unique_counter(self):
        """PA_GENES_UNIQUE by the plainest means: a Counter over the single-gene molecules"""
        return Counter((k, g) for k, c in enumerate(self.cells) for g, n in c.u.items() for _ in range(n))

    def matrix(self, values):
        keep = np.asarray(values) != 0
        return self.cell[keep], self.gene[keep], np.asarray(values, np.float64)[keep]


def decode_barcode(bc, bc_len):
    return "".join("ACGT"[(int(bc) >> (2 * (bc_len - 1 - j))) & 3] for j in range(bc_len))


def f64_text(v):
    """shortest digits that read back as the same double, fixed notation"""
    s = np.format_float_positional(np.float64(v), unique=True, trim="-")
    return s


def matrix_text(num_genes, n_cells, cell, gene, value):
    lines = ["%%MatrixMarket matrix coordinate real general", "%d %d %d" % (num_genes, n_cells, len(value))]
    lines += ["%d %d %s" % (int(g) + 1, int(c) + 1, f64_text(v)) for c, g, v in zip(cell, gene, value)]
    return "\n".join(lines) + "\n"


def barcodes_text(barcodes, bc_len):
    return "".join(decode_barcode(b, bc_len) + "\n" for b in barcodes)


def features_text(gene_names):
    return "".join("%s\t%s\tGene Expression\n" % (g, g) for g in gene_names)


def directed(cells, num_genes, bc_len=16, umi_len=12):
    """cells: [(barcode, [molecule, ...])], a molecule = [record, ...] (or (umi, [record, ...])), a record = the genes of its ec. Gene g has
    the transcripts 2g and 2g + 1; the k-th record of one molecule with the same genes takes another transcript choice (2g; 2g + 1; both), so
    that its ec differs. -> (records, ec_offsets, ec_ids, tx_gene, num_genes, bc_len, umi_len)"""
    tx_gene = np.repeat(np.arange(num_genes, dtype=np.uint32), 2)
    ecs, recs = {}, []
    for barcode, mols in cells:
        for m, mol in enumerate(mols):
            umi, mol = mol if isinstance(mol, tuple) else (m, mol)
            seen = Counter()
            for genes in mol:
                key = tuple(sorted(genes))
                k = seen[key]
                seen[key] += 1
                assert k < 3, "at most three records of one molecule with the same genes"
                tx = tuple(sorted([2 * g for g in key] if k == 0 else [2 * g + 1 for g in key] if k == 1 else [t for g in key for t in (2 * g, 2 * g + 1)]))
                recs.append((barcode, umi, tx))
                ecs.setdefault(tx, None)
    order = sorted(ecs)
    number = {tx: e for e, tx in enumerate(order)}
    out = np.zeros(len(recs), BUS_RECORD_DTYPE)
    for i, (b, u, tx) in enumerate(sorted((b, u, number[tx]) for b, u, tx in recs)):
        out[i] = (b, u, tx, 1 + i % 3, 0, 0)
    off = np.cumsum([0] + [len(tx) for tx in order]).astype(np.uint64)
    ids = np.array([t for tx in order for t in tx], np.uint32)
    return out, off, ids, tx_gene, num_genes, bc_len, umi_len
