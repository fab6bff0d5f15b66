"""Pure-Python model of the cell calling on BUS records (include/pseudoaligner_amd.h, pa_bus_knee / pa_bus_keep), written from the rules of that
section alone: the barcode table, the rank, the curve, the three threshold rules (math.log10, plain float arithmetic), the called list, the ten
stats, the pure filter with its seven stats and the text of barcode_ranks.tsv — what the GPU stage must equal exactly."""
from __future__ import annotations

import math
from collections import Counter

CURVE, EXPECTED, MIN = 0, 1, 2
MODES = {"curve": CURVE, "expected": EXPECTED, "min": MIN}
DEFAULTS = dict(mode=CURVE, lower=10, divisor=10, expected_cells=3000, min_umis=1)
STAT_NAMES = ("records", "reads", "molecules", "barcodes", "distinct_values", "values_above_lower", "threshold", "barcodes_called", "molecules_called", "reads_called")
KEEP_STAT_NAMES = ("records_in", "reads_in", "barcodes_in", "barcodes_kept", "records_out", "reads_out", "listed_absent")
TSV_HEADER = "barcode\trecords\tumis\treads\trank\tcalled\n"
BASES = "ACGT"


def params(**given):
    p = dict(DEFAULTS)
    for k, v in given.items():
        assert k in p, k
        p[k] = MODES[v] if k == "mode" and isinstance(v, str) else v
    return p


def table(records):
    """records [(barcode, umi, ec, count)] strictly ascending -> rows [[barcode, records, umis, reads]] in ascending barcode order"""
    rows = []
    last = None
    for b, u, _, n in records:
        if not rows or rows[-1][0] != b:
            rows.append([b, 0, 0, 0])
            last = None
        row = rows[-1]
        row[1] += 1
        row[3] += n
        if u != last:
            row[2] += 1
            last = u
    return rows


def ranks(rows):
    """rank[i] of row i: its 0-based position in the order (umis descending, barcode ascending)"""
    order = sorted(range(len(rows)), key=lambda i: (-rows[i][2], rows[i][0]))
    out = [0] * len(rows)
    for r, i in enumerate(order):
        out[i] = r
    return out


def curve(rows):
    """(v, R): the distinct umis values, descending; R[j] = the barcodes with umis >= v[j]"""
    c = Counter(r[2] for r in rows)
    v = sorted(c, reverse=True)
    R, acc = [], 0
    for x in v:
        acc += c[x]
        R.append(acc)
    return v, R


def scores(v, R, L):
    """PA_KNEE_CURVE's s_j over the first L points (L >= 3), each product and difference one float operation, as written in the header"""
    x0, y0 = math.log10(R[0]), math.log10(v[0])
    dx, dy = math.log10(R[L - 1]) - x0, math.log10(v[L - 1]) - y0
    return [(math.log10(v[j]) - y0) * dx - (math.log10(R[j]) - x0) * dy for j in range(L)]


def knee_index(v, R, L):
    if L <= 2:
        return L - 1
    s = scores(v, R, L)
    k = max(range(L), key=lambda j: (s[j], -j))     # the smallest j with the greatest s_j
    return k if s[k] > 0 else L - 1


def threshold(p, v, R):
    """-> (t, L); L = 0 outside PA_KNEE_CURVE"""
    if p["mode"] == MIN:
        return p["min_umis"], 0
    if p["mode"] == EXPECTED:
        if not v:
            return 1, 0
        B = R[-1]
        r = min(p["expected_cells"] // 100, B - 1)
        m = next(v[j] for j in range(len(v)) if R[j] > r)
        return (m + 9) // 10, 0
    assert p["mode"] == CURVE
    L = sum(1 for x in v if x >= p["lower"])
    if L == 0:
        return p["lower"], 0
    k = knee_index(v, R, L)
    return max(p["lower"], (v[k] + p["divisor"] - 1) // p["divisor"]), L


def knee(records, **given):
    """-> (rows [(barcode, reads, records, umis, rank, called)] in the field order of pa_bus_barcode_row, called barcodes ascending, stats dict)"""
    return knee_of_table(table(records), len(records), **given)


def knee_of_table(tab, n_records, **given):
    """knee() behind the table: tab as table() gives it"""
    p = params(**given)
    rk = ranks(tab)
    v, R = curve(tab)
    t, L = threshold(p, v, R)
    rows = [(b, reads, nrec, umis, rk[i], 1 if umis >= t else 0) for i, (b, nrec, umis, reads) in enumerate(tab)]
    called = [r[0] for r in rows if r[5]]
    st = dict(zip(STAT_NAMES, (n_records, sum(r[1] for r in rows), sum(r[3] for r in rows), len(rows), len(v), L, t, len(called),
                               sum(r[3] for r in rows if r[5]), sum(r[1] for r in rows if r[5]))))
    assert st["barcodes_called"] <= st["barcodes"] and st["molecules_called"] <= st["molecules"] and st["reads_called"] <= st["reads"]
    return rows, called, st


def check_list(barcodes, bc_len):
    """None for a valid list, else the entry the refusal names: the first that is >= 4^bc_len or not above the one before it"""
    for i, b in enumerate(barcodes):
        if b >= 4 ** bc_len or (i and barcodes[i - 1] >= b):
            return i
    return None


def keep(records, barcodes):
    """-> (records out, stats dict)"""
    listed = set(barcodes)
    out = [r for r in records if r[0] in listed]
    present = {r[0] for r in records}
    st = dict(zip(KEEP_STAT_NAMES, (len(records), sum(r[3] for r in records), len(present), len(present & listed), len(out), sum(r[3] for r in out),
                                    len(listed - present))))
    return out, st


def unpack(value, bc_len):
    return "".join(BASES[(value >> (2 * (bc_len - 1 - j))) & 3] for j in range(bc_len))


def ranks_tsv(rows, bc_len):
    return TSV_HEADER + "".join("%s\t%d\t%d\t%d\t%d\t%d\n" % (unpack(b, bc_len), nrec, umis, reads, rank, called) for b, reads, nrec, umis, rank, called in rows)
