"""Pure-Python model of the BUS barcode correction (include/pseudoaligner_amd.h, pa_bus_correct), written from the rules of that section
alone: the whitelist as a dict, the rule per distinct barcode (exact, corrected, none, ambiguous; the first that applies), the rewrite,
the sort, the merge of equal (barcode, UMI, ec) with the count clamped at 2^32 - 1, and all thirteen stats — what the GPU stage must
equal exactly."""
from __future__ import annotations

from collections import Counter

BASES = "ACGT"
CODE = {b: i for i, b in enumerate(BASES)}
COUNT_MAX = 0xFFFFFFFF
STAT_NAMES = ("records_in", "reads_in", "barcodes_in", "barcodes_exact", "barcodes_corrected", "barcodes_none", "barcodes_ambiguous", "records_exact",
              "records_corrected", "records_dropped", "reads_dropped", "records_out", "barcodes_out")
EXACT, CORRECTED, NONE, AMBIGUOUS = "exact", "corrected", "none", "ambiguous"


def pack(seq: str) -> int:
    """2 bits per base, A=0 C=1 G=2 T=3, first base most significant; a byte that is no base raises KeyError"""
    v = 0
    for ch in seq:
        v = v * 4 + CODE[ch]
    return v


def unpack(value: int, bc_len: int) -> str:
    return "".join(BASES[(value >> (2 * (bc_len - 1 - j))) & 3] for j in range(bc_len))


def check_whitelist(whitelist, bc_len: int):
    """None for a valid whitelist, else the entry the refusal names (a value >= 4^bc_len: its index; a duplicate: the smaller index)"""
    first_of = {}
    named = []
    for i, w in enumerate(whitelist):
        if w >= 4 ** bc_len:
            return i
        if w in first_of:
            named.append(first_of[w])
        first_of.setdefault(w, i)
    return min(named) if named else None


def neighbours(barcode: int, bc_len: int):
    """the 3 bc_len single substitutions"""
    for p in range(bc_len):
        old = (barcode >> (2 * p)) & 3
        for b in range(4):
            if b != old:
                yield barcode + ((b - old) << (2 * p))


def decide(barcode: int, whitelist: dict, bc_len: int):
    """-> (kind, target | None)"""
    if barcode in whitelist:
        return EXACT, barcode
    hits = [c for c in neighbours(barcode, bc_len) if c in whitelist]
    if len(hits) == 1:
        return CORRECTED, hits[0]
    return (NONE if not hits else AMBIGUOUS), None


def correct(records, whitelist, bc_len: int, umi_len: int):
    """records: [(barcode, umi, ec, count)] strictly ascending; whitelist: packed values in any order
    -> (records out [(barcode, umi, ec, count)] strictly ascending, stats dict, {barcode: (kind, target)})"""
    wl = {int(w): True for w in whitelist}
    st = dict.fromkeys(STAT_NAMES, 0)
    decided = {}
    merged = Counter()
    for b, u, ec, n in records:
        if b not in decided:
            decided[b] = decide(b, wl, bc_len)
            st["barcodes_in"] += 1
            st["barcodes_" + decided[b][0]] += 1
        kind, target = decided[b]
        st["records_in"] += 1
        st["reads_in"] += n
        if target is None:
            st["records_dropped"] += 1
            st["reads_dropped"] += n
            continue
        st["records_" + kind] += 1
        merged[(target, u, ec)] += n
    out = sorted((b, u, ec, min(n, COUNT_MAX)) for (b, u, ec), n in merged.items())
    st["records_out"] = len(out)
    st["barcodes_out"] = len({r[0] for r in out})
    assert st["barcodes_in"] == st["barcodes_exact"] + st["barcodes_corrected"] + st["barcodes_none"] + st["barcodes_ambiguous"]
    assert st["records_in"] == st["records_exact"] + st["records_corrected"] + st["records_dropped"] and st["records_out"] <= st["records_exact"] + st["records_corrected"]
    return out, st, decided
