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


# ---- directed cases (tests/test_gpu_cells_edges.py): the mapping's records written by hand, no aligner in the loop ----
RESULT_DTYPE = np.dtype([("coverage", "<u4"), ("mismatches", "<u4"), ("class_off", "<u4"), ("class_len", "<u4")])   # pa_read_result
MAPPED_BIT = 0x80000000   # PA_MAPPED_BIT (mismatches)
CLASS_REF = 0x80000000    # PA_CLASS_REF (class_off)


def unpack(v: int, n: int) -> str:
    return "".join(BASES[(v >> (2 * (n - 1 - i))) & 3] for i in range(n))


def sub_at(s: str, i: int, k: int = 1) -> str:
    """s with base i replaced by the k-th next base (k = 1..3): a Hamming-1 neighbour"""
    return s[:i] + BASES[(CODE[s[i]] + k) % 4] + s[i + 1:]


def hamming(a: str, b: str) -> int:
    return sum(x != y for x, y in zip(a, b))


def key_layout(n_whitelist: int, num_genes: int, umi_len: int) -> dict:
    """the molecule key's fields as include/pseudoaligner_amd.h lays them out (cell | gene | UMI, widths bits(n_whitelist - 1),
    bits(num_genes - 1), 2 umi_len) and the values the counter derives from them: the bits its sorts look at (a radix sort wants at
    least one) and the all-ones keys it gives to dropped reads (sentinel) and to molecules lost to a conflict (sentinel3, over cell | gene)"""
    cell_bits, gene_bits, umi_bits = (n_whitelist - 1).bit_length(), (num_genes - 1).bit_length(), 2 * umi_len
    key_bits = cell_bits + gene_bits + umi_bits
    end_bit, end_bit3 = max(1, key_bits), max(1, cell_bits + gene_bits)
    return dict(cell_bits=cell_bits, gene_bits=gene_bits, umi_bits=umi_bits, cell_shift=gene_bits + umi_bits, key_bits=key_bits, end_bit=end_bit,
                end_bit3=end_bit3, sentinel=(1 << end_bit) - 1, sentinel3=(1 << end_bit3) - 1)


def molecule_key(lay: dict, cell: int, gene: int, umi: str) -> int:
    return (cell << lay["cell_shift"]) | (gene << lay["umi_bits"]) | pack(umi)


def singleton_classes(index: dict):
    """[(class, its one transcript)] of a host index's arrays()"""
    off = np.asarray(index["ec_offset"]).astype(np.int64)
    return [(int(c), int(index["ec_ids"][off[c]])) for c in np.flatnonzero(off[1:] - off[:-1] == 1)]


def directed_case(molecules, index: dict, tx_gene, whitelist, seed: int = 0, shuffle: bool = True):
    """Reads that realise a list of molecules exactly. A molecule is (cell, cls, umi, reads[, r1]):
      cell   a whitelist line, or a str: the barcode's text as it stands in R1 (lower case, N, a substitution)
      cls    int c: the class goes by reference (class_off = PA_CLASS_REF | c, class_len = the length of index class c);
             a list of transcript ids: it goes into the arena (class_off = its offset, class_len = its length, [] included);
             ("unmapped", either of the two): the same record with PA_MAPPED_BIT clear; None: an unmapped record with no class
      umi    the UMI's text (any byte)
      reads  how many reads
      r1     the whole R1 text in place of barcode + umi (a short or empty R1)
    index: HostIndex.arrays() of the index the counter is created with (its classes' transcript lists are what a reference means).
    -> (r1 strings, records [n] RESULT_DTYPE, arena uint32 (never empty), mapping [(mapped, transcript ids)] for count()).
    A reference to a class the index does not have (c >= num_classes) or a list with an id that is no transcript (>= num_transcripts)
    names no transcripts of ONE gene, and include/pseudoaligner_amd.h:423-424 counts a read only when its class is non-empty and
    its "transcripts (tx_gene) all belong to one gene; everything else drops": the mapping then carries two transcripts of
    different genes of tx_gene, which is how count() is told "several genes"."""
    rng = np.random.default_rng(seed)
    off = np.asarray(index["ec_offset"]).astype(np.int64)
    ec_ids, num_classes, num_tx = index["ec_ids"], int(index["num_classes"]), int(index["num_transcripts"])
    several = None

    def several_genes():
        nonlocal several
        if several is None:
            other = [t for t in range(len(tx_gene)) if int(tx_gene[t]) != int(tx_gene[0])]
            if not other:
                raise ValueError("an out-of-range class needs a tx_gene of at least two genes")
            several = [0, other[0]]
        return several

    arena, arena_at = [0], {}   # (word 0 is padding: no list starts there, and the arena is never empty)
    r1s, recs, mapping = [], [], []
    for mol in molecules:
        cell, cls, umi, reads = mol[:4]
        text = mol[4] if len(mol) > 4 else (whitelist[cell] if isinstance(cell, (int, np.integer)) else cell) + umi
        mapped = True
        if cls is None:
            mapped, cls = False, []
        elif isinstance(cls, tuple) and len(cls) == 2 and cls[0] == "unmapped":
            mapped, cls = False, cls[1]
        if isinstance(cls, (int, np.integer)):
            c = int(cls)
            ids = [int(t) for t in ec_ids[off[c]:off[c + 1]]] if c < num_classes else several_genes()
            class_off, class_len = CLASS_REF | c, len(ids) if c < num_classes else 1
        else:
            ids = [int(t) for t in cls]
            if tuple(ids) not in arena_at:
                arena_at[tuple(ids)] = len(arena)
                arena.extend(ids)
            class_off, class_len = arena_at[tuple(ids)], len(ids)
            if any(t >= num_tx for t in ids):
                ids = several_genes()
        for _ in range(reads):
            r1s.append(text)
            recs.append((40 + len(recs) % 50, (MAPPED_BIT if mapped else 0) | (len(recs) % 3), class_off, class_len))
            mapping.append((mapped, ids if mapped else []))
    order = rng.permutation(len(r1s)) if shuffle else np.arange(len(r1s))
    records = np.array(recs, RESULT_DTYPE)[order] if recs else np.zeros(0, RESULT_DTYPE)
    return [r1s[i] for i in order], records, np.array(arena, np.uint32), [mapping[i] for i in order]


def umi_moves(umis: dict, umi_len: int) -> dict:
    """{u: where u moves} inside one (cell, gene) group {packed UMI: reads}: the rule of count(), for the tests' own assertions"""
    out = {}
    for u, n in umis.items():
        best = (n, u)
        for v in neighbours(u, umi_len):
            if v in umis:
                best = max(best, (umis[v], v))
        out[u] = best[1]
    return out


def segment_features(umis: dict, umi_len: int) -> set:
    """which of the correction rule's situations a (cell, gene) group {packed UMI: reads} holds"""
    mv = umi_moves(umis, umi_len)
    top, low = 3 << (2 * (umi_len - 1)), 3
    found = set()
    for u, n in umis.items():
        nb = [v for v in neighbours(u, umi_len) if v in umis]
        if mv[u] != u and umis[mv[u]] > n:
            found.add("move_more")
            found.add("move_first_base" if (u ^ mv[u]) & top else "move_last_base" if (u ^ mv[u]) & low else "move_inner_base")
        if mv[u] != u and umis[mv[u]] == n:
            found.add("tie_larger_wins")
        if mv[u] == u and any(umis[v] == n and v < u for v in nb):
            found.add("tie_keeps_own")
        if mv[u] == u and nb and all(umis[v] < n for v in nb):
            found.add("fewer_no_move")
        if mv[u] != u and mv[mv[u]] != mv[u]:
            found.add("chain_one_step")
    return found


SEAM_FEATURES = {"move_more", "move_first_base", "move_last_base", "tie_larger_wins", "tie_keeps_own", "fewer_no_move", "chain_one_step"}
SEAM_SIZES = (1, 2, 63, 64, 65, 128, 129, 257)


def seam_segment(rng, size: int, umi_len: int) -> dict:
    """{UMI text: reads} of exactly `size` UMIs: three motifs around bases of their own — a (5 reads) with its first-base neighbour
    (2: moves to a, which itself meets only fewer reads); c (9), its last-base neighbour b (4) and b's first-base neighbour x (1):
    x -> b -> c, x stops at b; t and its last-base neighbour, 3 reads each: the smaller moves, the larger stays — then random UMIs
    of 1..4 reads. size 1 is a alone, size 2 a and its neighbour.
    -> (the UMIs, probes): which UMI a move ends on does not show in a count of distinct UMIs, so a second gene puts a molecule on the two
    UMIs where it matters — 4 reads on the larger of the tie (it holds 6 of this gene after the move: the second gene loses; had the
    larger moved to the smaller, it would survive) and 1 read on b (which holds x's 1 read after b's own 4 moved on to c: a tie, both lost;
    had x gone on to c, the second gene would survive)."""
    rnd = lambda: "".join(BASES[x] for x in rng.integers(0, 4, umi_len))
    a, c, t = rnd(), rnd(), rnd()
    b = sub_at(c, umi_len - 1)
    motif = [(a, 5), (sub_at(a, 0), 2), (c, 9), (b, 4), (sub_at(b, 0, 2), 1), (t, 3), (sub_at(t, umi_len - 1, 2), 3)]
    umis = dict(motif[:size] if size < len(motif) else motif)
    assert len(umis) == min(size, len(motif))
    while len(umis) < size:
        umis.setdefault(rnd(), int(rng.integers(1, 5)))
    t2 = sub_at(t, umi_len - 1, 2)
    return umis, ([(max(t, t2, key=pack), 4), (b, 1)] if size >= len(motif) else [])


def seam_case(index: dict, umi_len: int = 12, seed: int = 3) -> dict:
    """one (cell, gene) segment of each SEAM_SIZES size in cells 0.. of a 16-barcode whitelist, then the 64-UMI segment of cell 3 again
    in cell 8 and once more in cell 9 with one more UMI at distance >= 2 from all of them (a 65-segment: the other code path). Gene 0 holds
    the segments, gene 1 the probes of seam_segment in every cell of 63 UMIs or more."""
    rng = np.random.default_rng(seed)
    whitelist = [a + b for a in BASES for b in BASES]
    (cls, t0), (cls_b, t_b) = singleton_classes(index)[:2]
    tx_gene = np.zeros(int(index["num_transcripts"]), np.uint32)
    tx_gene[t_b] = 1
    built = {i: seam_segment(rng, s, umi_len) for i, s in enumerate(SEAM_SIZES)}
    segments, probes = {i: v[0] for i, v in built.items()}, {i: v[1] for i, v in built.items()}
    shared = segments[SEAM_SIZES.index(64)]
    probes[8] = probes[9] = probes[SEAM_SIZES.index(64)]
    while True:
        pad = "".join(BASES[x] for x in rng.integers(0, 4, umi_len))
        if all(hamming(pad, u) >= 2 for u in shared):
            break
    segments[8] = dict(shared)
    segments[9] = dict(shared, **{pad: 2})
    molecules = [(cell, cls if j % 2 else [t0], u, n) for cell, umis in segments.items() for j, (u, n) in enumerate(umis.items())]
    molecules += [(cell, cls_b, u, n) for cell, pr in probes.items() for u, n in pr]
    return dict(whitelist=whitelist, bc_len=2, umi_len=umi_len, num_genes=2, tx_gene=tx_gene, molecules=molecules, segments=segments, probes=probes, pad=pad)


def stride_case(index: dict, cus: int, umi_len: int = 10, seed: int = 5) -> dict:
    """4 * 32 * cus + 5000 (cell, gene) segments of 1..3 UMIs, one read each: more than the correction kernel's grid of 32 * cus blocks of
    4 waves has waves, so its loop over segments goes round again. Every 97th segment and each of the last 100 holds a Hamming-1 pair of
    2 and 1 reads (one move each). Four genes by four class references; cell = segment // 4."""
    rng = np.random.default_rng(seed)
    segs = 4 * 32 * cus + 5000
    singles = singleton_classes(index)[:4]
    tx_gene = np.zeros(int(index["num_transcripts"]), np.uint32)
    for g, (_, t) in enumerate(singles):
        tx_gene[t] = g
    # (transcripts outside the four classes stay in gene 0; the class references alone decide a read's gene here)
    bc_len = 1
    while 4 ** bc_len * 4 < segs:
        bc_len += 1
    whitelist = [unpack(i, bc_len) for i in range(4 ** bc_len)]
    codes = rng.integers(0, 4, (segs, 3, umi_len))
    molecules, paired = [], []
    for s in range(segs):
        cell, cls = s // 4, singles[s % 4][0]
        u = ["".join(BASES[x] for x in codes[s, j]) for j in range(3)]
        if s % 97 == 0 or s >= segs - 100:
            paired.append(s)
            molecules += [(cell, cls, u[0], 2), (cell, cls, sub_at(u[0], s % umi_len, 1 + s % 3), 1)]
        else:
            molecules += [(cell, cls, x, 1) for x in dict.fromkeys(u[: 1 + s % 3])]
    return dict(whitelist=whitelist, bc_len=bc_len, umi_len=umi_len, num_genes=4, tx_gene=tx_gene, molecules=molecules, segs=segs, paired=paired)


WIDTH_SHAPES = {   # name: (whitelist size, bc_len, num_genes, umi_len)
    "key_2_bits": (1, 1, 1, 1),
    "cell_shift_64": (1, 3, 0xFFFFFFFD, 16),
    "key_64_bits": (4, 1, 1 << 30, 16),
    "key_equals_sentinel": (4, 2, 4, 4),
    "no_power_of_two": (5, 3, 3, 5),
    "every_barcode_whitelisted": (1 << 16, 8, 2, 12),
}


def widths_case(name: str, index: dict, seed: int = 9) -> dict:
    """molecules in the first and the last cell, of the lowest and the highest gene of tx_gene (the lowest by class reference, the highest
    by an id list), with UMIs A..A, T..T (on both genes: a conflict that the larger count wins, or nobody) and two random ones, 1..4
    reads each"""
    n_wl, bc_len, num_genes, umi_len = WIDTH_SHAPES[name]
    rng = np.random.default_rng(seed)
    if n_wl == 4 ** bc_len:
        whitelist = [unpack(i, bc_len) for i in range(n_wl)]
    else:
        whitelist = [unpack(int(i), bc_len) for i in sorted(rng.choice(4 ** bc_len, n_wl, replace=False).tolist())]
    (c_lo, t_lo), (c_hi, t_hi) = singleton_classes(index)[:2]
    tx_gene = np.zeros(int(index["num_transcripts"]), np.uint32)
    if num_genes > 2:   # a gene in the middle too, on transcripts no molecule names
        tx_gene[2::7] = (num_genes - 1) // 2
        tx_gene[t_lo] = 0
    tx_gene[t_hi] = num_genes - 1
    umis = ["A" * umi_len, "T" * umi_len] + ["".join(BASES[x] for x in rng.integers(0, 4, umi_len)) for _ in range(2)]
    molecules = []
    for cell in sorted({0, n_wl - 1}):
        for gene_cls in ((c_lo, [t_hi]) if num_genes > 1 else (c_lo, [t_lo])):
            own = ["".join(BASES[x] for x in rng.integers(0, 4, umi_len)) for _ in range(2)]   # (the two random ones: this gene's alone)
            for u in dict.fromkeys(umis[:2] + own):
                molecules.append((cell, gene_cls, u, int(rng.integers(1, 5))))
    if name == "key_equals_sentinel":   # the all-ones key is the strict winner of its (cell, UMI), so it reaches the matrix
        molecules = [m for m in molecules if not (m[0] == n_wl - 1 and m[2] == "T" * umi_len)]
        molecules += [(n_wl - 1, [t_hi], "T" * umi_len, 4), (n_wl - 1, c_lo, "T" * umi_len, 1)]
    if name == "every_barcode_whitelisted":   # a substitution is another cell's exact barcode; an N has four fillers
        bc = whitelist[n_wl - 1]
        molecules += [(sub_at(bc, 0), c_lo, umis[2], 2), (sub_at(bc, bc_len - 1, 2), [t_hi], umis[3], 1), (bc[:3] + "N" + bc[4:], c_lo, umis[2], 1)]
    return dict(whitelist=whitelist, bc_len=bc_len, umi_len=umi_len, num_genes=num_genes, tx_gene=tx_gene, molecules=molecules)


def sentinel_case(index: dict, survives: bool) -> dict:
    """the 4 / 4 / 4 shape (4 cells, 4 genes, 4-base UMIs: every field a power of two), where (cell 3, gene 3, TTTT) is a valid key of all
    ones = the key dropped reads get, and (cell 3, gene 3) the all-ones key of molecules lost to a conflict. survives False: gene 3 has
    3 reads on (cell 3, TTTT) and gene 2 has 5, so (3, 3) is lost and (3, 2) is kept; True: 5 against 3, (3, 3) is kept beside lost
    molecules. Both with reads dropped for their UMI and for their mapping in the same batch."""
    singles = singleton_classes(index)[:4]
    tx_gene = np.zeros(int(index["num_transcripts"]), np.uint32)
    for g, (_, t) in enumerate(singles):
        tx_gene[t] = g
    cls = [c for c, _ in singles]
    t3 = singles[3][1]
    a, b = (5, 3) if survives else (3, 5)
    molecules = [(3, [t3], "TTTT", a), (3, cls[2], "TTTT", b),
                 (0, cls[0], "ACGT", 2), (0, cls[1], "ACGT", 2),     # a tie: both lost
                 (1, cls[3], "TTTT", 1), (1, cls[3], "AAAA", 2), (2, cls[0], "GGCA", 1),
                 (3, cls[3], "TTNT", 2), (0, cls[1], "NNNN", 1),     # dropped: UMI
                 (3, None, "TTTT", 2), (3, ("unmapped", cls[3]), "TTTT", 1), (2, [singles[0][1], singles[1][1]], "TTTT", 1)]   # dropped: mapping
    return dict(whitelist=["AA", "CC", "GG", "TT"], bc_len=2, umi_len=4, num_genes=4, tx_gene=tx_gene, molecules=molecules)


def accumulator_growth(batches):
    """the counter's accumulator over batches of (reads counted, distinct keys): it is grown when acc_n + counted exceeds its size, to
    max(acc_n + counted, 2 size). -> (times the need outgrew the doubling of a non-empty accumulator, times the doubling was enough)"""
    size = acc_n = outgrown = doubled = 0
    for counted, runs in batches:
        if counted and acc_n + counted > size:
            if size:
                if acc_n + counted > 2 * size:
                    outgrown += 1
                else:
                    doubled += 1
            size = max(acc_n + counted, 2 * size)
        acc_n += runs
    return outgrown, doubled
