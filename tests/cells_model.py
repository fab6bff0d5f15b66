"""Pure-Python model of the single-cell UMI counting semantics (include/pseudoaligner_amd.h, pa_cell_counter / pa_count_cells),
written from the rules alone: what the GPU counter's matrix, stats and output files must equal exactly. It also makes the paired
test data (whitelist, R1 with injected faults, R2 cut from transcripts) the GPU tests feed both sides with."""
from __future__ import annotations

from collections import Counter, defaultdict

import numpy as np

BASES = "ACGT"
CODE = {b: i for i, b in enumerate(BASES)}
STAT_NAMES = ("reads", "barcode_exact", "barcode_corrected", "barcode_invalid", "umi_invalid", "not_confidently_mapped", "reads_counted",
              "umis_corrected", "molecules_lost_to_conflicts", "umis_in_matrix")


def pack(seq: str) -> int:
    """2 bits per base, first base most significant (integer order = string order under A < C < G < T)"""
    v = 0
    for ch in seq:
        v = v * 4 + CODE[ch]
    return v


def correct_barcode(bc: str, wl_line: dict):
    """-> (cell, "exact" | "corrected") or (None, "invalid"): the unique 1-mismatch neighbour rule"""
    n_pos = [i for i, ch in enumerate(bc) if ch not in CODE]
    if not n_pos and bc in wl_line:
        return wl_line[bc], "exact"
    if len(n_pos) > 1:
        return None, "invalid"
    positions = n_pos if n_pos else range(len(bc))
    hits = set()
    for i in positions:
        for b in BASES:
            if b != bc[i]:
                cand = bc[:i] + b + bc[i + 1:]
                if cand in wl_line:
                    hits.add(wl_line[cand])
    return (hits.pop(), "corrected") if len(hits) == 1 else (None, "invalid")


def gene_of(mapped: bool, class_ids, tx_gene):
    """the gene of a confidently mapped read, else None"""
    if not mapped or len(class_ids) == 0:
        return None
    genes = {int(tx_gene[t]) for t in class_ids}
    return genes.pop() if len(genes) == 1 else None


def neighbours(u: int, umi_len: int):
    for pos in range(umi_len):
        sh = 2 * pos
        cur = (u >> sh) & 3
        for b in range(4):
            if b != cur:
                yield (u & ~(3 << sh)) | (b << sh)


largest_group = 0   # UMIs of the largest (cell, gene) group of the last count() call


def count(r1s, mapping, tx_gene, whitelist, bc_len: int, umi_len: int):
    """r1s: R1 strings; mapping: per read (mapped, class ids) of its R2; whitelist: barcodes (line i = cell i).
    -> (matrix [(cell, gene, umis)] sorted by (cell, gene), stats dict)"""
    wl_line = {b: i for i, b in enumerate(whitelist)}
    st = dict.fromkeys(STAT_NAMES, 0)
    reads = Counter()
    for r1, (mapped, ids) in zip(r1s, mapping):
        st["reads"] += 1
        if len(r1) < bc_len + umi_len:
            st["barcode_invalid"] += 1
            continue
        cell, kind = correct_barcode(r1[:bc_len], wl_line)
        if cell is None:
            st["barcode_invalid"] += 1
            continue
        st["barcode_exact" if kind == "exact" else "barcode_corrected"] += 1
        umi = r1[bc_len:bc_len + umi_len]
        if any(ch not in CODE for ch in umi):
            st["umi_invalid"] += 1
            continue
        g = gene_of(mapped, ids, tx_gene)
        if g is None:
            st["not_confidently_mapped"] += 1
            continue
        st["reads_counted"] += 1
        reads[(cell, g, pack(umi))] += 1
    # UMI correction inside (cell, gene): one step to the greatest of {u} + present neighbours under (reads, UMI value)
    groups = defaultdict(dict)
    for (c, g, u), n in reads.items():
        groups[(c, g)][u] = n
    global largest_group
    largest_group = max((len(v) for v in groups.values()), default=0)
    molecules = Counter()
    for (c, g), umis in groups.items():
        for u, n in umis.items():
            best = (n, u)
            for v in neighbours(u, umi_len):
                if v in umis:
                    best = max(best, (umis[v], v))
            if best[1] != u:
                st["umis_corrected"] += 1
            molecules[(c, g, best[1])] += n
    # gene conflicts per (cell, UMI): strictly the most reads keeps it
    by_cu = defaultdict(list)
    for (c, g, u), n in molecules.items():
        by_cu[(c, u)].append((g, n))
    kept = Counter()
    for (c, u), lst in by_cu.items():
        for g, n in lst:
            other = max((m for h, m in lst if h != g), default=0)
            if n > other:
                kept[(c, g)] += 1
            else:
                st["molecules_lost_to_conflicts"] += 1
    matrix = sorted((c, g, n) for (c, g), n in kept.items())
    st["umis_in_matrix"] = sum(n for _, _, n in matrix)
    return matrix, st


def render(matrix, whitelist, gene_names):
    """(matrix.mtx, barcodes.tsv, features.tsv) text as pa_count_cells writes them"""
    cells = sorted({c for c, _, _ in matrix})
    col = {c: j + 1 for j, c in enumerate(cells)}
    mtx = "%%%%MatrixMarket matrix coordinate integer general\n%d %d %d\n" % (len(gene_names), len(cells), len(matrix))
    mtx += "".join("%d %d %d\n" % (g + 1, col[c], n) for c, g, n in matrix)
    barcodes = "".join(whitelist[c] + "\n" for c in cells)
    features = "".join("%s\t%s\tGene Expression\n" % (n, n) for n in gene_names)
    return mtx, barcodes, features


def _sub(rng, s: str, i: int) -> str:
    return s[:i] + BASES[(CODE[s[i]] + 1 + int(rng.integers(3))) % 4] + s[i + 1:]


def make_case(seed: int, transcripts, tx_gene, bc_len: int, umi_len: int, n_whitelist=2000, n_cells=300, read_len=90, big_segment=0):
    """Paired reads of a synthetic 10x run: -> dict(whitelist, r1, r2). Molecules of 1-8 reads, R2 cut from the molecule's transcript
    with 0-1 % substitutions; R1 faults: barcode substitutions (some constructed to have two whitelist neighbours), Ns in barcodes and
    UMIs, UMI substitutions, short R1s, UMIs shared across genes of a cell. big_segment > 0: one (cell, transcript) with that many UMIs."""
    rng = np.random.default_rng(seed)
    wl = set()
    whitelist = []
    while len(whitelist) < n_whitelist - 40:
        b = "".join(BASES[x] for x in rng.integers(0, 4, bc_len))
        if b not in wl:
            wl.add(b)
            whitelist.append(b)
    ambiguous = []   # Z at distance 1 from two whitelist barcodes A and B (A, B at distance 2)
    for a in whitelist[:20]:
        i, j = sorted(rng.choice(bc_len, 2, replace=False).tolist())
        b = _sub(rng, _sub(rng, a, i), j)
        z = a[:i] + b[i] + a[i + 1:]
        if b not in wl and z not in wl:
            wl.add(b)
            whitelist.append(b)
            ambiguous.append(z)
    order = rng.permutation(len(whitelist))
    whitelist = [whitelist[i] for i in order]
    usable = [t for t, s in enumerate(transcripts) if len(s) >= read_len + 10]
    cells = rng.choice(len(whitelist), n_cells, replace=False)
    r1, r2 = [], []
    rand_umi = lambda: "".join(BASES[x] for x in rng.integers(0, 4, umi_len))

    def emit(cell_bc, umi, t, n_reads):
        s = transcripts[t]
        for _ in range(n_reads):
            p = int(rng.integers(0, len(s) - read_len + 1))
            seq = list(s[p:p + read_len])
            for i in np.nonzero(rng.random(read_len) < rng.uniform(0, 0.01))[0]:
                seq[i] = BASES[(CODE.get(seq[i], 0) + 1 + int(rng.integers(3))) % 4]
            bc, u = cell_bc, umi
            x = rng.random()
            if x < 0.05:
                bc = _sub(rng, bc, int(rng.integers(bc_len)))
            elif x < 0.08:
                i = int(rng.integers(bc_len))
                bc = bc[:i] + "N" + bc[i + 1:]
            elif x < 0.09:
                i, j = rng.choice(bc_len, 2, replace=False)
                bc = "".join("N" if k in (i, j) else ch for k, ch in enumerate(bc))
            elif x < 0.10 and ambiguous:
                bc = ambiguous[int(rng.integers(len(ambiguous)))]
            y = rng.random()
            if y < 0.06:
                u = _sub(rng, u, int(rng.integers(umi_len)))
            elif y < 0.08:
                i = int(rng.integers(umi_len))
                u = u[:i] + "N" + u[i + 1:]
            tail = "".join(BASES[v] for v in rng.integers(0, 4, int(rng.integers(0, 12))))
            read1 = bc + u + tail
            if rng.random() < 0.01:
                read1 = read1[: int(rng.integers(0, bc_len + umi_len))]
            r1.append(read1)
            r2.append("".join(seq))

    for c in cells:
        umis = []
        for _ in range(int(rng.integers(1, 14))):
            t = usable[int(rng.integers(len(usable)))]
            u = umis[int(rng.integers(len(umis)))] if umis and rng.random() < 0.08 else rand_umi()   # shared across genes
            umis.append(u)
            emit(whitelist[c], u, t, int(rng.integers(1, 9)))
    if big_segment:
        c = whitelist[cells[0]]
        t = usable[0]
        base = rand_umi()
        seen = set()
        for k in range(big_segment):
            u = base if k == 0 else _sub(rng, base, int(rng.integers(umi_len))) if k % 3 else rand_umi()
            if u in seen:
                u = rand_umi()
            seen.add(u)
            emit(c, u, t, int(rng.integers(1, 5)))
    perm = rng.permutation(len(r1))
    return dict(whitelist=whitelist, r1=[r1[i] for i in perm], r2=[r2[i] for i in perm])


def model_from_oracle(oracle, case, tx_gene, bc_len, umi_len, nthreads=8):
    """the model's matrix + stats for a case, with every R2 mapped by the independent oracle"""
    res, coff, cids, _ = oracle.map_reads(case["r2"], 2, nthreads)
    mapping = [(bool(res["mapped"][i]), cids[int(coff[i]):int(coff[i + 1])]) for i in range(len(case["r2"]))]
    return count(case["r1"], mapping, tx_gene, case["whitelist"], bc_len, umi_len)
