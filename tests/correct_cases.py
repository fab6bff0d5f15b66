"""Hand-made cases of the BUS barcode correction (pa_bus_correct) for tests/test_correct_model.py and tests/test_gpu_correct*.py, the constants of
csrc/bus_correct.hip / bus_correct_host.cpp restated (the hash, the capacity rule, the group width: test_correct_model.py reads them back from
the source lines), and the generator of the paired test data with barcode errors. A case is (records [(barcode, umi, ec, count)] strictly
ascending, whitelist [packed], bc_len, umi_len); what must come out is tests/correct_model.py's answer, and for the small cases also written
out here."""
from __future__ import annotations

import numpy as np

import correct_model as cm
from bus_model import RECORD_DTYPE

# ---- restated from the sources ----
BLOCK = 256            # CORRECT_BLOCK
GROUP = 16             # CORRECT_GROUP: lanes per missed barcode
MAX_ROUNDS = 6         # CORRECT_MAX_ROUNDS
GROUPS_PER_WAVE = 64 // GROUP
GROUPS_PER_BLOCK = BLOCK // GROUP
M64 = (1 << 64) - 1


def mix64(x: int) -> int:
    """pa_mix64: murmur3 fmix64"""
    x ^= x >> 33
    x = (x * 0xff51afd7ed558ccd) & M64
    x ^= x >> 33
    x = (x * 0xc4ceb9fe1a85ec53) & M64
    x ^= x >> 33
    return x


def capacity(n_whitelist: int) -> int:
    """the power of two >= 2 n_whitelist (at least 2)"""
    cap = 2
    while cap < 2 * n_whitelist:
        cap <<= 1
    return cap


def home(barcode: int, cap: int) -> int:
    return mix64(barcode) & (cap - 1)


def to_array(records) -> np.ndarray:
    arr = np.zeros(len(records), RECORD_DTYPE)
    for i, (b, u, ec, n) in enumerate(records):
        arr[i] = (b, u, ec, n, 0, 0)
    return arr


def from_array(arr):
    assert not arr["flags"].any() and not arr["pad"].any()
    return list(zip(arr["barcode"].tolist(), arr["umi"].tolist(), arr["ec"].tolist(), arr["count"].tolist()))


def sub(barcode: int, bc_len: int, pos_from_first: int, k: int = 1) -> int:
    """the barcode with the base at `pos_from_first` moved k steps round A C G T"""
    shift = 2 * (bc_len - 1 - pos_from_first)
    old = (barcode >> shift) & 3
    return barcode + ((((old + k) & 3) - old) << shift)


P = cm.pack

# ---- the hand cases with their answers written out: name -> (records, whitelist, bc_len, umi_len, records out, {barcode: kind}) ----
HAND = {}

# bc_len = 1: every barcode neighbours every other. Whitelist {A}: C, G, T are all corrected to A, and all four land on one record
HAND["one_base_all_corrected"] = ([(0, 1, 5, 1), (1, 1, 5, 2), (2, 1, 5, 3), (3, 1, 5, 4), (3, 2, 5, 1)], [0], 1, 2,
                                  [(0, 1, 5, 10), (0, 2, 5, 1)], {0: "exact", 1: "corrected", 2: "corrected", 3: "corrected"})
# whitelist {A, C}: G and T have two neighbours
HAND["one_base_ambiguous"] = ([(0, 1, 5, 1), (1, 1, 5, 2), (2, 1, 5, 3), (3, 1, 5, 4)], [1, 0], 1, 2,
                              [(0, 1, 5, 1), (1, 1, 5, 2)], {0: "exact", 1: "exact", 2: "ambiguous", 3: "ambiguous"})
# exact wins over a whitelisted neighbour; midway between two at distance 2: ambiguous; distance 2 from everything: none
_A, _B = P("ACGTAC"), P("ACGTAG")             # both whitelisted, one apart
_C, _D = P("TTTTTT"), P("TTTTGG")             # both whitelisted, two apart; TTTTGT and TTTTTG lie midway
HAND["exact_wins_midway_far"] = ([(_A, 0, 1, 1), (_B, 0, 1, 1), (P("CCGGAA"), 0, 1, 7), (P("TTTTGT"), 0, 1, 1), (P("TTTTTG"), 3, 1, 1)], [_D, _A, _C, _B], 6, 4,
                                 [(_A, 0, 1, 1), (_B, 0, 1, 1)],
                                 {_A: "exact", _B: "exact", P("CCGGAA"): "none", P("TTTTGT"): "ambiguous", P("TTTTTG"): "ambiguous"})
# merges: two and three sources on one target with equal (UMI, ec), the clamp, a merge with the target's own record, equal UMI but
# different ec stays two records
_T = P("GATTACA")
_S = [sub(_T, 7, 0), sub(_T, 7, 3, 2), sub(_T, 7, 6, 3)]          # three sources, all one away from _T
_U = P("CCCCCCC")
_V = [sub(_U, 7, 1), sub(_U, 7, 5)]
_merge_in = sorted([(_S[0], 1, 4, 2), (_S[1], 1, 4, 3), (_S[2], 1, 4, 5),          # three sources, no own record
                    (_S[0], 2, 4, 0xFFFFFFFF), (_S[1], 2, 4, 1),                   # 0xFFFFFFFF + 1 clamps
                    (_S[0], 3, 4, 0x80000000), (_S[2], 3, 4, 0x80000000),          # 0x80000000 + 0x80000000 clamps
                    (_T, 5, 4, 10), (_S[1], 5, 4, 1),                              # with the target's own record
                    (_T, 6, 4, 1), (_S[2], 6, 9, 1),                               # equal UMI, different ec: two records
                    (_V[0], 0, 0, 1), (_V[1], 0, 0, 1)])                           # two sources
HAND["merges"] = (_merge_in, [_U, _T], 7, 3,
                  sorted([(_T, 1, 4, 10), (_T, 2, 4, 0xFFFFFFFF), (_T, 3, 4, 0xFFFFFFFF), (_T, 5, 4, 11), (_T, 6, 4, 1), (_T, 6, 9, 1), (_U, 0, 0, 2)]),
                  {_T: "exact", _S[0]: "corrected", _S[1]: "corrected", _S[2]: "corrected", _V[0]: "corrected", _V[1]: "corrected"})
# a corrected barcode that lands before the first and after the last other barcode
_LO, _HI, _MID = P("AAAAC"), P("TTTTG"), P("CGCGC")
HAND["lands_at_the_ends"] = (sorted([(P("TAAAC"), 0, 0, 1), (_MID, 0, 0, 1), (P("ATTTG"), 0, 0, 1)]), [_MID, _HI, _LO], 5, 5,
                             [(_LO, 0, 0, 1), (_MID, 0, 0, 1), (_HI, 0, 0, 1)], {P("TAAAC"): "corrected", _MID: "exact", P("ATTTG"): "corrected"})
# every record dropped; a whitelist of one
HAND["all_dropped"] = ([(P("ACAC"), 0, 0, 1), (P("GTGT"), 1, 2, 3)], [P("TTTT")], 4, 4, [], {P("ACAC"): "none", P("GTGT"): "none"})
HAND["no_records"] = ([], [P("TTTT")], 4, 4, [], {})


def long_barcode_case(bc_len: int, umi_len: int):
    """the substitution at the first and at the last base of a long barcode (shifts 2 (bc_len - 1) and 0), and one in the middle"""
    rng = np.random.default_rng(bc_len)
    wl = [int("".join(str(x) for x in rng.integers(0, 4, bc_len)), 4) for _ in range(5)]
    rec = sorted([(sub(wl[0], bc_len, 0, 1), 1, 0, 1), (sub(wl[1], bc_len, bc_len - 1, 2), 1, 0, 2), (sub(wl[2], bc_len, bc_len // 2, 3), 1, 0, 3), (wl[3], 1, 0, 4),
                  (sub(sub(wl[4], bc_len, 0), bc_len, bc_len - 1), 1, 0, 5)])
    return rec, wl, bc_len, umi_len


def wrap_whitelist(bc_len: int = 8, n: int = 5):
    """a whitelist of n whose table (capacity(n) slots) has two keys at home in the LAST slot and one at home in slot 0: whichever of the two
    arrives second is displaced past the end, to slot 0 or further"""
    cap = capacity(n)
    last = [v for v in range(4 ** bc_len) if home(v, cap) == cap - 1][:2]
    zero = [v for v in range(4 ** bc_len) if home(v, cap) == 0][:1]
    rest = [v for v in range(4 ** bc_len) if home(v, cap) not in (0, 1, cap - 1)][:n - 3]
    return last + zero + rest, cap


def wrap_case():
    wl, cap = wrap_whitelist()
    rec = sorted({(b, 0, 0, 1) for w in wl for b in (w, sub(w, 8, 2), sub(w, 8, 7, 2))} | {(sub(sub(wl[0], 8, 0), 8, 1), 0, 0, 1)})
    return rec, wl, 8, 6


def sized_case(seed: int, n_exact: int, n_corrected: int, n_other: int, bc_len: int = 12, umi_len: int = 5, n_whitelist: int = 300):
    """n_exact whitelisted barcodes, n_corrected one substitution away from exactly one whitelisted barcode, n_other random ones (none, or by
    chance anything): the distinct barcodes of the input number n_exact + n_corrected + n_other and the miss list n_corrected + n_other.
    One to three records each; few UMIs and ecs, so that corrected records meet the target's own"""
    rng = np.random.default_rng(seed)
    wl = sorted({int(x) for x in rng.integers(0, 4 ** bc_len, n_whitelist * 2)})
    wl = [wl[i] for i in rng.permutation(len(wl))[:n_whitelist]]
    wl_set = set(wl)
    chosen = set(wl[:n_exact])
    assert len(chosen) == n_exact
    while len(chosen) < n_exact + n_corrected:
        w = wl[int(rng.integers(len(wl)))]
        c = sub(w, bc_len, int(rng.integers(bc_len)), int(rng.integers(1, 4)))
        if c not in wl_set and cm.decide(c, wl_set, bc_len)[0] == "corrected":
            chosen.add(c)
    while len(chosen) < n_exact + n_corrected + n_other:
        c = int(rng.integers(0, 4 ** bc_len))
        if c not in wl_set:
            chosen.add(c)
    rec = set()
    for b in chosen:
        for _ in range(int(rng.integers(1, 4))):
            rec.add((b, int(rng.integers(3)), int(rng.integers(2))))
    rec = sorted(rec)
    return [(b, u, ec, int(rng.integers(1, 5))) for b, u, ec in rec], wl, bc_len, umi_len


# ---- the paired test data of tests/test_gpu_correct.py: bus_model.make_case's shape with barcode errors and a whitelist ----
def make_pairs_case(seed: int, transcripts, bc_len: int, umi_len: int, n_pairs: int = 20000, n_cells: int = 150, n_extra: int = 2000, read_len: int = 90,
                    one_sub: float = 0.08, two_subs: float = 0.01):
    """-> dict(r1, r2, whitelist [str]): whitelist = the n_cells true cells + n_extra random barcodes, shuffled; one_sub of the R1s get one
    barcode substitution, two_subs two"""
    rng = np.random.default_rng(seed)
    rand = lambda n: "".join(cm.BASES[x] for x in rng.integers(0, 4, n))
    cells = sorted({rand(bc_len) for _ in range(n_cells)})
    extra = sorted({rand(bc_len) for _ in range(n_extra)} - set(cells))
    whitelist = cells + extra
    whitelist = [whitelist[i] for i in rng.permutation(len(whitelist))]
    usable = [t for t, s in enumerate(transcripts) if len(s) >= read_len + 10]
    r1, r2 = [], []
    while len(r1) < n_pairs:
        cell, umi = cells[int(rng.integers(len(cells)))], rand(umi_len)
        s = transcripts[usable[int(rng.integers(len(usable)))]]
        for _ in range(int(rng.integers(1, 6))):
            p = int(rng.integers(0, len(s) - read_len + 1))
            seq = rand(read_len) if rng.random() < 0.05 else s[p:p + read_len]
            bc = cell
            y = rng.random()
            for _ in range(1 if y < one_sub else 2 if y < one_sub + two_subs else 0):
                i = int(rng.integers(bc_len))
                bc = bc[:i] + cm.BASES[(cm.CODE[bc[i]] + 1 + int(rng.integers(3))) % 4] + bc[i + 1:]
            r1.append(bc + umi + rand(int(rng.integers(0, 6))))
            r2.append(seq)
    return dict(r1=r1[:n_pairs], r2=r2[:n_pairs], whitelist=whitelist)
