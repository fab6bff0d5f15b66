"""Designed inputs of the UMI correction, one per rule and per shape its kernels can take (csrc/bus_umi.hip): hand-written records with no aligner in
the loop. build(): cells = [(barcode, [(umi, [record, ...]), ...])], a record = (genes, count) or (genes, count, variant). Gene g has the transcripts
2g and 2g + 1; variant 0 takes 2g of every gene, 1 takes 2g + 1, 2 both, so that records of one molecule with the same genes get different ecs."""
import re
from pathlib import Path

import numpy as np

import umi_model as um

# the thresholds of rust-pseudoaligner_amd/csrc/bus_umi_state.hpp, restated (test_umi_model.py reads the source lines back)
UM_LANE_MAX = 64
UM_LDS_CAP = 8192
BIG = 2 ** 32 - 1


def thresholds_in_source():
    text = (Path(__file__).resolve().parent.parent / "rust-pseudoaligner_amd" / "csrc" / "bus_umi_state.hpp").read_text()
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"constexpr uint32_t (UM_\w+) = (\d+);", text)}


def _tx(genes, variant):
    genes = sorted(genes)
    return tuple(sorted([2 * g for g in genes] if variant == 0 else [2 * g + 1 for g in genes] if variant == 1 else [t for g in genes for t in (2 * g, 2 * g + 1)]))


def build(cells, num_genes, bc_len, umi_len):
    """-> (records, ec_offsets, ec_ids, tx_gene, num_genes, bc_len, umi_len); barcodes and UMIs are strings of bases or packed values"""
    val = lambda x: um.pack(x) if isinstance(x, str) else int(x)
    rows = []
    for barcode, mols in cells:
        for umi, recs in mols:
            for r in recs:
                rows.append((val(barcode), val(umi), _tx(r[0], r[2] if len(r) > 2 else 0), r[1]))
    order = sorted({r[2] for r in rows})
    number = {tx: e for e, tx in enumerate(order)}
    rows = sorted((b, u, number[tx], c) for b, u, tx, c in rows)
    assert len({r[:3] for r in rows}) == len(rows), "two records of one (barcode, UMI, ec)"
    rec = np.zeros(len(rows), um.BUS_RECORD_DTYPE)
    for i, (b, u, e, c) in enumerate(rows):
        rec[i] = (b, u, e, c, 0, 0)
    off = np.cumsum([0] + [len(tx) for tx in order]).astype(np.uint64)
    ids = np.array([t for tx in order for t in tx], np.uint32)
    return rec, off, ids, np.repeat(np.arange(num_genes, dtype=np.uint32), 2), num_genes, bc_len, umi_len


def ec_of(case, genes, variant=0):
    """the ec number that build() gave the record (genes, variant)"""
    _, off, ids, *_ = case
    want = list(_tx(genes, variant))
    return [e for e in range(len(off) - 1) if ids[int(off[e]):int(off[e + 1])].tolist() == want][0]


def expect(case, rows):
    """expected output records written out: [(barcode, umi, (genes, variant), count)]"""
    out = sorted((um.pack(b), um.pack(u), ec_of(case, *g), c) for b, u, g, c in rows)
    return np.array([(b, u, e, c, 0, 0) for b, u, e, c in out], um.BUS_RECORD_DTYPE)


G1 = ([1], 0)
# ---- the hand cases: name -> (cells, expected records or None for "the input", a few stats that must hold) ----
HAND = {
    "one_neighbour": ([("ACGT", [("AAAA", [([1], 5)]), ("AAAC", [([1], 1)])])],
                      [("ACGT", "AAAA", G1, 6)], dict(molecules_moved=1, records_out=1, molecules_out=1, reads_moved=1)),
    "tie_broken_by_umi": ([("ACGT", [("AAAC", [([1], 3)]), ("AAAG", [([1], 3)])])],
                          [("ACGT", "AAAG", G1, 6)], dict(molecules_moved=1, molecules_with_neighbour=2)),
    "greater_of_two": ([("ACGT", [("AAAA", [([1], 1)]), ("CAAA", [([1], 4)]), ("AAAG", [([1], 7)])])],
                       [("ACGT", "AAAG", G1, 8), ("ACGT", "CAAA", G1, 4)], dict(molecules_moved=1, molecules_with_neighbour=3)),
    "chain_not_transitive": ([("ACGT", [("AAAA", [([1], 1)]), ("AAAC", [([1], 2)]), ("AACC", [([1], 5)])])],
                             [("ACGT", "AAAC", G1, 1), ("ACGT", "AACC", G1, 7)], dict(molecules_moved=2, molecules_moved_onto_moved=1, molecules_out=2)),
    "genes_do_not_meet": ([("ACGT", [("AAAA", [([1], 5)]), ("AAAC", [([2], 1)])])],
                          None, dict(molecules_with_hamming1=2, molecules_with_neighbour=0, molecules_moved=0)),
    "inert_in_between": ([("ACGT", [("AAAA", [([1], 1)]), ("AAAC", [([1], 9), ([2], 9)]), ("AACC", [([1], 5)])])],
                         None, dict(molecules_inert=1, molecules_with_hamming1=2, molecules_with_neighbour=0, molecules_moved=0)),
    "two_barcodes": ([("ACGT", [("AAAA", [([1], 5)])]), ("ACGG", [("AAAC", [([1], 1)])]), ("TTTT", [("AAAA", [([1], 5)]), ("AAAC", [([1], 1)])])],
                     [("ACGT", "AAAA", G1, 5), ("ACGG", "AAAC", G1, 1), ("TTTT", "AAAA", G1, 6)], dict(molecules_moved=1, barcodes=3, molecules_with_hamming1=2)),
    "clamped_sum": ([("ACGT", [("AAAA", [([1, 2], BIG), ([1], 10)]), ("AAAC", [([1, 2], 5), ([1, 3], 1)])])],
                    [("ACGT", "AAAA", ([1, 2], 0), BIG), ("ACGT", "AAAA", ([1], 0), 10), ("ACGT", "AAAA", ([1, 3], 0), 1)],
                    dict(molecules_moved=1, records_rewritten=2, reads_moved=6, records_out=3, reads_in=BIG + 16)),
    "n_beyond_32_bits": ([("ACGT", [("AAAA", [([1, 2], BIG), ([1, 3], BIG)]), ("AAAC", [([1], BIG)])])],
                         [("ACGT", "AAAA", ([1, 2], 0), BIG), ("ACGT", "AAAA", ([1, 3], 0), BIG), ("ACGT", "AAAA", ([1], 0), BIG)],
                         dict(molecules_moved=1, reads_moved=BIG, reads_in=3 * BIG)),
    "nothing_moves": ([("ACGT", [("AAAA", [([1], 5), ([1, 2], 1)]), ("CCCC", [([1], 1)]), ("GGTT", [([2, 3], 2)])]), ("TTTT", [("AAAA", [([1], 2)])])],
                      None, dict(molecules_moved=0, molecules_with_hamming1=0, records_out=5)),
}


def hand(name):
    cells, want, st = HAND[name]
    case = build(cells, 4, 4, 4)
    return case, (case[0] if want is None else expect(case, want)), st


def _split(total):
    """records of one molecule whose counts sum to total (each at most 2^32 - 1)"""
    return [([1], total)] if total <= BIG else [([1, 2], total // 2), ([1, 3], total - total // 2)]


def directional_case():
    """n(v) = 2 n(u) - 2, 2 n(u) - 1 and 2 n(u) at n(u) = 1 and at n(u) = 3 * 10^9, one barcode each; u = ACGA, v = ACGT (the greater UMI).
    -> (case, {mode: the UMIs left in every barcode}), the expectation written out from the rule: at n(u) = 1 the first v has n = 0 and moves
    onto u itself; n(v) = 1 ties with u and the UMI value decides for v; the large u stays in DIRECTIONAL mode only below 2 n(u) - 1"""
    cells = [(j, [("ACGA", _split(nu)), ("ACGT", _split(nv))]) for j, (nu, nv) in enumerate([(n, 2 * n + d) for n in (1, 3_000_000_000) for d in (-2, -1, 0)])]
    u, v = um.pack("ACGA"), um.pack("ACGT")
    left = {"directional": [{u}, {v}, {v}, {u, v}, {v}, {v}], "greatest": [{u}, {v}, {v}, {v}, {v}, {v}]}
    return build(cells, 4, 4, 4), left


def widths_cases():
    """umi_len 1 (every other UMI is a neighbour), 16 (the u32 word is full), 17 (the first u64 width), (bc_len, umi_len) = (1, 31) and (16, 16) with an
    all-T barcode and UMI, a substitution at the first and at the last base"""
    out = {"umi_len_1": build([("ACGT", [("A", [([1], 2)]), ("C", [([1], 2)]), ("G", [([2], 9)]), ("T", [([1], 1)])])], 4, 4, 1)}
    for name, bc_len, umi_len in (("umi_len_16", 16, 16), ("umi_len_17", 15, 17), ("umi_len_31", 1, 31)):
        t = "T" * umi_len
        mols = [(t, [([1], 7)]), ("A" + t[1:], [([1], 1)]), (t[:-1] + "G", [([1], 2)]), ("C" + t[1:-1] + "C", [([1], 1)]),        # first base, last base, two bases
                ("G" * umi_len, [([1], 3)]), ("G" * (umi_len - 1) + "A", [([2], 9)]), ("C" + "G" * (umi_len - 1), [([1, 2], 4)])]
        out[name] = build([("T" * bc_len, mols), ("A" * bc_len, mols[:3])], 4, bc_len, umi_len)
    return out


def bin_barcode(k, umi_len, seed):
    """one barcode of exactly k molecules: UMIs drawn sparsely, with planted Hamming-1 partners of the first and of the last molecule (last base) and
    pairs that differ in their first base (far apart in the sorted order)"""
    rng = np.random.RandomState(seed)
    top, extra = 4 ** umi_len, min(k // 4, 40)
    draw = lambda: int(rng.randint(8, top - 8, dtype=np.int64))
    umis = set()
    while len(umis) < k - 4 - extra:
        umis.add(draw())
    for u in sorted(umis):                                           # first-base partners of some
        partner = u ^ (int(rng.randint(1, 4)) << (2 * (umi_len - 1)))
        if 8 <= partner < top - 8 and len(umis) < k - 4:
            umis.add(partner)
    while len(umis) < k - 4:
        umis.add(draw())
    umis = sorted(umis | {4, 5, top - 2, top - 1})                   # first and second, last and the one before: one last-base substitution apart
    assert len(umis) == k and umis[:2] == [4, 5] and umis[-2:] == [top - 2, top - 1]
    return [(u, [([1 + (i % 7 == 3)], 1 + i % 3)] if i % 11 else [([1, 2], 2), ([1, 3], 1 + i % 2)]) for i, u in enumerate(umis)]


BIN_SIZES = (UM_LANE_MAX, UM_LANE_MAX + 1, UM_LDS_CAP, UM_LDS_CAP + 1)


def bins_case(umi_len):
    """one barcode of each edge size, for the u32 word (umi_len 16) or the u64 word (17)"""
    bc_len = 32 - umi_len if umi_len > 16 else 12
    return build([(100 + j, bin_barcode(k, umi_len, 7 + j)) for j, k in enumerate(BIN_SIZES)], 4, bc_len, umi_len)


def random_case(seed):
    """about 2 000 records, umi_len 4 - 5 (neighbours are dense), 3 - 40 barcodes, multi-gene ecs"""
    rng = np.random.RandomState(seed)
    umi_len, n_bc, num_genes = int(rng.randint(4, 6)), int(rng.randint(3, 41)), 6
    cells = {}
    while sum(len(r) for c in cells.values() for r in c.values()) < 2000:
        b, u = int(rng.randint(0, n_bc)) * 3, int(rng.randint(0, 4 ** umi_len))
        recs = cells.setdefault(b, {}).setdefault(u, {})
        genes = tuple(sorted(set(rng.randint(0, num_genes, int(rng.choice([1, 1, 1, 2, 3]))).tolist())))
        recs[(genes, int(rng.randint(0, 3)))] = int(rng.choice([1, 1, 2, 3, 10]))
    return build([(b, [(u, [(g, c, v) for (g, v), c in recs.items()]) for u, recs in mols.items()]) for b, mols in cells.items()], num_genes, 8, umi_len)


_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def model(key, case, mode):
    """the model's answer for a case, computed once and left unchanged"""
    return cached(("model", key, mode), lambda: um.correct(case[0], case[1], case[2], case[3], case[6], mode, lds_cap=UM_LDS_CAP))


def one_barcode(case, barcode):
    """the records of one barcode as a case of their own (same tables)"""
    rec = case[0]
    return (rec[rec["barcode"] == barcode],) + tuple(case[1:])


def rows_of(case, rec):
    """records as (barcode, umi, the ec's transcripts, count): comparable between cases whose ecs are numbered differently"""
    _, off, ids, *_ = case
    return [(int(r["barcode"]), int(r["umi"]), tuple(ids[int(off[r["ec"]]):int(off[r["ec"] + 1])].tolist()), int(r["count"])) for r in rec]


def hand_batch(seed=4):
    """every barcode of every hand case in one input, renumbered by a shuffle -> (case, [(name, barcode in its case, barcode in the batch)])"""
    parts = [(name, bc, mols) for name in sorted(HAND) for bc, mols in HAND[name][0]]
    new = np.random.RandomState(seed).permutation(len(parts)) * 5 + 2
    return build([(int(b), mols) for (_, _, mols), b in zip(parts, new)], 4, 4, 4), [(name, um.pack(bc), int(b)) for (name, bc, _), b in zip(parts, new)]


def with_umi_errors(pairs, bc_len, umi_len, rate, seed):
    """paired test data (dict r1, r2, ...) with a copy of `rate` of the pairs whose UMI carries one substitution, the same R2; shuffled again"""
    rng = np.random.default_rng(seed)
    r1, r2 = list(pairs["r1"]), list(pairs["r2"])
    for i in np.flatnonzero(rng.random(len(r1)) < rate).tolist():
        at = bc_len + int(rng.integers(umi_len))
        base = um.BASES[(um.BASES.index(r1[i][at]) + 1 + int(rng.integers(3))) % 4]
        r1.append(r1[i][:at] + base + r1[i][at + 1:])
        r2.append(r2[i])
    order = rng.permutation(len(r1))
    return dict(pairs, r1=[r1[i] for i in order], r2=[r2[i] for i in order])
