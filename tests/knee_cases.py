"""Hand-made cases and sized generators of the cell calling on BUS records (pa_bus_knee, pa_bus_keep) for tests/test_knee_model.py,
tests/test_knee_host.py and tests/test_gpu_knee*.py, with the constants of csrc/bus_knee.hip restated (test_knee_model.py reads them back from
the source lines). A case is a list of records [(barcode, umi, ec, count)] strictly ascending; what must come out is tests/knee_model.py's
answer, and for the hand cases it is also written out here. Every case that is decided by PA_KNEE_CURVE passes clear_knee() when it is made: a
condition on the inputs, so that an ulp of log10 cannot decide a test."""
from __future__ import annotations

import numpy as np

import knee_model as km
from bus_model import RECORD_DTYPE

# ---- restated from the sources ----
BLOCK = 256              # KNEE_BLOCK
ITEMS = 8                # KNEE_ITEMS
TILE = BLOCK * ITEMS     # KNEE_TILE
MAX_GRID = 1024          # KNEE_MAX_GRID
ROW_DTYPE = np.dtype([("barcode", "<u8"), ("reads", "<u8"), ("records", "<u4"), ("umis", "<u4"), ("rank", "<u4"), ("called", "<u4")])   # pa_bus_barcode_row


def to_array(records) -> np.ndarray:
    arr = np.zeros(len(records), RECORD_DTYPE)
    if len(records):
        cols = list(zip(*records))
        arr["barcode"], arr["umi"], arr["ec"], arr["count"] = (np.array(c, dtype=object).astype(t) for c, t in zip(cols, (np.uint64, np.uint64, np.int32, np.uint32)))
    return arr


def from_array(arr):
    assert not arr["flags"].any() and not arr["pad"].any()
    return list(zip(arr["barcode"].tolist(), arr["umi"].tolist(), arr["ec"].tolist(), arr["count"].tolist()))


def rows_from_array(arr):
    return [tuple(int(x) for x in r) for r in arr.tolist()]


def clear_knee(v, R, lower) -> bool:
    """the condition of the generated PA_KNEE_CURVE cases: with L >= 3 points the best score is ahead of the second best by more than 1e-9 of
    its size, or (a curve without a shoulder) every inner score is below zero by more than 1e-9 of the largest size. (The two end scores are
    exact zeros: 0 * dx - 0 * dy and dy * dx - dx * dy.)"""
    L = sum(1 for x in v if x >= lower)
    if L <= 2:
        return True
    s = km.scores(v, R, L)
    assert s[0] == 0.0 and s[L - 1] == 0.0
    inner = sorted(s[1:L - 1], reverse=True)
    best, second = inner[0], max(inner[1] if len(inner) > 1 else 0.0, 0.0)
    if best > 0:
        return best - second > 1e-9 * best
    return best < 0 and -best > 1e-9 * max(abs(x) for x in s)


def assert_clear(records, lower):
    v, R = km.curve(km.table(records))
    assert clear_knee(v, R, lower), (v[:8], R[:8])
    return records


def from_umis(umis, barcodes=None, records_per_molecule=1, count=1):
    """one barcode per entry of `umis` (barcode i = barcodes[i], default 3 i + 1) with that many molecules of `records_per_molecule` records each"""
    rec = []
    for i, m in enumerate(umis):
        b = barcodes[i] if barcodes is not None else 3 * i + 1
        for u in range(m):
            for e in range(records_per_molecule):
                rec.append((b, u, e, count))
    return rec


def from_heads(n, barcode_heads, molecule_heads, first_barcode=5, barcode_step=3, count=lambda i: 1 + (i * 7) % 5):
    """n records laid out by position: a new barcode begins at every index of barcode_heads (and at 0), a new molecule at every index of
    molecule_heads (and at every barcode head); inside a molecule the ec counts up"""
    bh, mh = set(barcode_heads) | {0}, set(molecule_heads)
    rec, b, u, e = [], first_barcode - barcode_step, 0, 0
    for i in range(n):
        if i in bh:
            b, u, e = b + barcode_step, 0, 0
        elif i in mh:
            u, e = u + 1, 0
        else:
            e += 1
        rec.append((b, u, e, count(i)))
    return rec


# ---- hand cases: name -> (umis per barcode, params, what must come out) ----
SHOULDER = [100, 99, 98, 97, 96] + [3] * 10 + [2] * 10 + [1] * 20
FLAT = [50] * 4 + [1] * 30
HAND = {
    "shoulder_divisor_1": (SHOULDER, dict(lower=1, divisor=1), dict(L=8, knee=96, t=96, called=5)),
    "shoulder_divisor_10": (SHOULDER, dict(lower=1, divisor=10), dict(L=8, knee=96, t=10, called=5)),
    "flat_lower_1": (FLAT, dict(lower=1, divisor=1), dict(L=2, knee=1, t=1, called=34)),
    "flat_lower_2": (FLAT, dict(lower=2, divisor=1), dict(L=1, knee=50, t=50, called=4)),
    "flat_lower_51": (FLAT, dict(lower=51, divisor=1), dict(L=0, knee=None, t=51, called=0)),
    # PA_KNEE_EXPECTED: 12 barcodes of 120, 110, .., 10 molecules. expected_cells 3000: r = 30, lowered to 11: m = 10, t = 1. 99: r = 0: m = 120, t = 12
    "expected_beyond_the_rows": (list(range(120, 0, -10)), dict(mode="expected", expected_cells=3000), dict(L=0, knee=None, t=1, called=12)),
    "expected_rank_0": (list(range(120, 0, -10)), dict(mode="expected", expected_cells=99), dict(L=0, knee=None, t=12, called=11)),
    "expected_rank_3": (list(range(120, 0, -10)), dict(mode="expected", expected_cells=399), dict(L=0, knee=None, t=9, called=12)),
    "min_umis_3": (SHOULDER, dict(mode="min", min_umis=3), dict(L=0, knee=None, t=3, called=15)),
}
SHOULDER_SCORES = (1.3686, 1.1823)     # the best (at 96) and the runner-up, to four places


def cells_and_ambient(seed, n_cells, n_ambient, cell_umis=(200, 400), ambient_umis=(1, 5), records_per_molecule=(1, 3), bc_len=12, umi_len=10, lower=10):
    """a library in small: n_cells barcodes with many molecules, n_ambient with few, at random barcode values; every molecule 1 .. 3 records with
    counts 1 .. 4. Redrawn (seed + 1000, ...) until the curve has a clear knee"""
    for attempt in range(20):
        rng = np.random.default_rng(seed + 1000 * attempt)
        barcodes = sorted(int(x) for x in rng.choice(4 ** bc_len, n_cells + n_ambient, replace=False))
        is_cell = set(int(x) for x in rng.choice(n_cells + n_ambient, n_cells, replace=False))
        rec = []
        for i, b in enumerate(barcodes):
            lo, hi = cell_umis if i in is_cell else ambient_umis
            m = int(rng.integers(lo, hi + 1))
            for u in sorted(int(x) for x in rng.choice(4 ** umi_len, m, replace=False)):
                k = int(rng.integers(records_per_molecule[0], records_per_molecule[1] + 1))
                for e in sorted(int(x) for x in rng.choice(40, k, replace=False)):
                    rec.append((b, u, e, int(rng.integers(1, 5))))
        v, R = km.curve(km.table(rec))
        if clear_knee(v, R, lower):
            return rec, bc_len, umi_len
    raise AssertionError("no clear knee in 20 draws")


def make_pairs_case(seed, transcripts, bc_len, umi_len, n_cells=30, molecules_per_cell=(90, 160), n_ambient=300, n_extra=500, read_len=90, one_sub=0.01):
    """the paired test data of tests/test_gpu_knee.py -> dict(r1, r2, cells [str], whitelist [str]): n_cells barcodes with many molecules of
    1 .. 3 reads, n_ambient barcodes with 1 .. 3 molecules, one_sub of all R1s with one barcode substitution; the pairs shuffled. The whitelist
    lists POSSIBLE barcodes: the cells, the ambient ones and n_extra others"""
    rng = np.random.default_rng(seed)
    rand = lambda n: "".join(km.BASES[x] for x in rng.integers(0, 4, n))
    names = sorted({rand(bc_len) for _ in range(n_cells + n_ambient + n_extra)})
    names = [names[i] for i in rng.permutation(len(names))]
    cells, ambient, extra = names[:n_cells], names[n_cells:n_cells + n_ambient], names[n_cells + n_ambient:]
    usable = [t for t, s in enumerate(transcripts) if len(s) >= read_len + 10]
    pairs = []
    for group, (lo, hi) in ((cells, molecules_per_cell), (ambient, (1, 3))):
        for bc0 in group:
            for _ in range(int(rng.integers(lo, hi + 1))):
                umi = rand(umi_len)
                s = transcripts[usable[int(rng.integers(len(usable)))]]
                for _ in range(int(rng.integers(1, 4))):
                    p = int(rng.integers(0, len(s) - read_len + 1))
                    bc = bc0
                    if rng.random() < one_sub:
                        i = int(rng.integers(bc_len))
                        bc = bc[:i] + km.BASES[(km.BASES.index(bc[i]) + 1 + int(rng.integers(3))) % 4] + bc[i + 1:]
                    pairs.append((bc + umi + rand(int(rng.integers(0, 6))), s[p:p + read_len]))
    pairs = [pairs[i] for i in rng.permutation(len(pairs))]
    return dict(r1=[p[0] for p in pairs], r2=[p[1] for p in pairs], cells=sorted(cells), whitelist=sorted(names))


def strided_case(extra=5):
    """MAX_GRID * TILE + extra records as arrays (too many for tuples): runs of 1 .. 3000 records per barcode, molecules of 1 .. 4 records; a
    barcode and a molecule begin exactly at the first record of the second grid stride. -> (records array, the model's table)"""
    n = MAX_GRID * TILE + extra
    rng = np.random.default_rng(77)
    cuts = np.unique(np.concatenate([[0, MAX_GRID * TILE], rng.choice(n, n // 1500, replace=False)]))
    bh = np.zeros(n, bool)
    bh[cuts] = True
    mh = bh | (rng.integers(0, 3, n) == 0)
    idx = np.arange(n)
    b_id = np.cumsum(bh) - 1
    m_start = np.maximum.accumulate(np.where(mh, idx, 0))
    b_start = np.maximum.accumulate(np.where(bh, idx, 0))
    m_id = np.cumsum(mh) - 1
    arr = np.zeros(n, RECORD_DTYPE)
    arr["barcode"] = 7 + 5 * b_id.astype(np.uint64)
    arr["umi"] = (m_id - m_id[b_start]).astype(np.uint64)
    arr["ec"] = (idx - m_start).astype(np.int32)
    arr["count"] = (1 + idx % 3).astype(np.uint32)
    tab = km.table(zip(arr["barcode"].tolist(), arr["umi"].tolist(), arr["ec"].tolist(), arr["count"].tolist()))
    return arr, tab
