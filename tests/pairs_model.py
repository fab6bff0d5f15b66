"""The model of the paired-end stage, written from the rules in include/pseudoaligner_amd.h ("paired-end reads"), not from the stage (the rule of csrc/pairs.hip over the skeleton of csrc/pair_stage.hpp):

  * reverse complement on packed 2-bit codes (numpy);
  * the pair rule over two mates' results — from the oracle (an id list, coverage, mismatches or None per mate) or from device-format
    records the tests write by hand;
  * the dense table and the novel records of the pair results, through helpers.counts_reference / novel_reference;
  * the stats vector;
  * a seeded pair simulator: a fragment drawn from a transcript, mate 1 = its first L bases, mate 2 = the reverse complement of its last
    L bases, optional substitutions.
All integers: the tests compare with equality."""
import numpy as np

import helpers

pa = helpers.pa
RESULT_DTYPE = np.dtype([("coverage", "<u4"), ("mismatches", "<u4"), ("class_off", "<u4"), ("class_len", "<u4")])
MAPPED_BIT = 0x80000000
CLASS_REF = 0x80000000
UNFIT = 0x7FFFFFFF
STAT_NAMES = ("pairs", "both_mapped", "mate1_only", "mate2_only", "neither", "both_mapped_empty", "by_reference", "in_arena")
ORIENT = {"fr": (False, True), "rf": (True, False), "ff": (False, False)}   # which mates are reverse-complemented


# ---- reverse complement ----
def revcomp_codes(codes):
    """base j of the output = 3 - base len - 1 - j of the input"""
    return (3 - np.asarray(codes, np.uint8)[::-1]).astype(np.uint8)


def revcomp_packed(words, length):
    """packed words (base j in bits 2 (j % 32) of word j / 32) -> ceil(length / 32) packed words, zero beyond `length`"""
    out = helpers.pack_bases(revcomp_codes(helpers.unpack_bases(words, length)))
    return out[: (length + 31) // 32]


def revcomp_tiles(tiles, lens, wpr):
    """the tile layout (tiles[(t * wpr + w) * 64 + r]) -> the same layout, every read reverse-complemented"""
    n = len(lens)
    t3 = np.asarray(tiles, np.uint64).reshape(-1, wpr, 64)
    out = np.zeros_like(t3)
    for i in range(n):
        w = revcomp_packed(t3[i >> 6, :, i & 63], int(lens[i]))
        out[i >> 6, : len(w), i & 63] = w
    return out.reshape(-1)


def tile_bases(tiles, lens, wpr):
    """codes of every read of a tile buffer (list of uint8 arrays) and whether every bit beyond a read's length is zero"""
    t3 = np.asarray(tiles, np.uint64).reshape(-1, wpr, 64)
    bases, clean = [], True
    for i in range(len(lens)):
        w = t3[i >> 6, :, i & 63]
        n = int(lens[i])
        bases.append(helpers.unpack_bases(w, n))
        full, rem = n >> 5, n & 31
        if rem:
            clean &= int(w[full]) >> (2 * rem) == 0
            full += 1
        clean &= not w[full:].any()
    return bases, clean


_COMP = str.maketrans("ACGTacgt", "TGCAtgca")


def revcomp_text(s):
    """the same on text, for reads the encoder has not seen yet: an N stays an N here and becomes A then T / A by where it is encoded —
    so the model orients PACKED reads, never text, when a read may hold one (simulated reads hold none)"""
    return s.translate(_COMP)[::-1]


# ---- the pair rule ----
def pair_rule(m1, m2):
    """mate = None | (sorted id list, coverage, mismatches) -> the pair's, by the table of the header"""
    if m1 is None and m2 is None:
        return None
    if m1 is None or m2 is None:
        ids, cov, mm = m1 if m2 is None else m2
        return list(ids), cov, mm
    s2 = set(m2[0])
    return [t for t in m1[0] if t in s2], m1[1] + m2[1], m1[2] + m2[2]


def mates_from_oracle(o_res, coff, ids):
    coff = np.asarray(coff, np.int64)
    return [None if not o_res["mapped"][i] else (ids[coff[i]:coff[i + 1]].tolist(), int(o_res["coverage"][i]), int(o_res["mismatches"][i]))
            for i in range(len(o_res))]


def mates_from_records(records, arena, arrays):
    """device-format records (class by reference or in `arena`) -> mates"""
    off = arrays["ec_offset"].astype(np.int64)
    out = []
    for r in records:
        if not (int(r["mismatches"]) & MAPPED_BIT):
            out.append(None)
            continue
        n, o = int(r["class_len"]), int(r["class_off"])
        if n == 0:
            ids = []
        elif o & CLASS_REF:
            c = o & 0x7FFFFFFF
            ids = arrays["ec_ids"][off[c]:off[c + 1]].tolist()
            assert len(ids) == n, "a record by reference carries its class's length"
        else:
            ids = np.asarray(arena)[o:o + n].tolist()
        out.append((ids, int(r["coverage"]), int(r["mismatches"]) & 0x7FFFFFFF))
    return out


def combine(mates1, mates2):
    """-> (results RESULT_DTYPE with class_off = the CSR offset, class_offsets[n + 1], class_ids, stats dict)"""
    n = len(mates1)
    assert len(mates2) == n
    res = np.zeros(n, RESULT_DTYPE)
    coff = np.zeros(n + 1, np.uint64)
    ids_all = []
    st = dict.fromkeys(STAT_NAMES, 0)
    st["pairs"] = n
    for i, (a, b) in enumerate(zip(mates1, mates2)):
        st["both_mapped" if a is not None and b is not None else "mate1_only" if a is not None else "mate2_only" if b is not None else "neither"] += 1
        r = pair_rule(a, b)
        if r is not None:
            ids, cov, mm = r
            assert ids == sorted(set(ids))
            res[i] = (cov, mm | MAPPED_BIT, len(ids_all), len(ids))
            ids_all.extend(ids)
            if a is not None and b is not None and not ids:
                st["both_mapped_empty"] += 1
        coff[i + 1] = len(ids_all)
    return res, coff, np.array(ids_all, np.uint32), st


def check_stats(stats, results):
    """the two identities of the header, and by_reference + in_arena against the records"""
    assert stats["pairs"] == stats["both_mapped"] + stats["mate1_only"] + stats["mate2_only"] + stats["neither"]
    mapped = (results["mismatches"] >> 31).astype(bool)
    empty = int((mapped & (results["class_len"] == 0)).sum())
    assert stats["by_reference"] + stats["in_arena"] == stats["pairs"] - stats["neither"] - empty


def table_and_novel(res, coff, ids, host):
    return helpers.counts_reference(res, coff, ids, host), helpers.novel_reference(res, coff, ids, host)


def fates(res, coff, ids, mates1, mates2, host):
    """which of the fates a batch reaches, on the model's side: {"subset_class", "novel", "empty", "mate1_only", "mate2_only", "neither"}"""
    a = host.arrays()
    off = a["ec_offset"].astype(np.int64)
    known = {tuple(a["ec_ids"][off[c]:off[c + 1]].tolist()) for c in range(a["num_classes"])}
    out = set()
    coff = np.asarray(coff, np.int64)
    for i, (x, y) in enumerate(zip(mates1, mates2)):
        if x is None and y is None:
            out.add("neither")
        elif y is None:
            out.add("mate1_only")
        elif x is None:
            out.add("mate2_only")
        else:
            got = tuple(ids[coff[i]:coff[i + 1]].tolist())
            if not got:
                out.add("empty")
            elif len(got) < len(x[0]) and len(got) < len(y[0]):
                out.add("subset_class" if got in known else "novel")
    return out


ALL_FATES = {"subset_class", "novel", "empty", "mate1_only", "mate2_only", "neither"}


# ---- reads ----
def transcripts_text(host):
    packed, tx_start = host.transcripts()
    codes = helpers.unpack_bases(packed, int(tx_start[-1]))
    lut = np.frombuffer(b"ACGT", np.uint8)
    text = lut[codes].tobytes().decode()
    return [text[int(tx_start[t]):int(tx_start[t + 1])] for t in range(len(tx_start) - 1)]


def simulate_pairs(txs, n, seed, frag_lo=100, frag_hi=400, mate_len=75, sub_rate=0.0, orient="fr", junk_every=0, chimera_every=0):
    """n pairs -> (mates 1, mates 2, transcript of every pair; -1: a junk mate). The fragment's start and length (frag_lo..frag_hi, cut to
    the transcript) are drawn from a transcript drawn uniformly among those of at least mate_len bases; "fr": mate 1 = the first mate_len
    bases, mate 2 = the reverse complement of the last mate_len; "rf": the two the other way round; "ff": mate 2 = the last mate_len bases as
    they are. junk_every = j > 0: in pair i with i % j == 0 mate 1, with i % j == 1 mate 2 and with i % j == 2 both are random bases.
    chimera_every = c > 0: in pair i with i % c == 3 mate 2 comes from a fragment of another transcript (src stays mate 1's)."""
    rng = np.random.default_rng(seed)
    ok = [t for t, s in enumerate(txs) if len(s) >= mate_len]
    r1, r2, src = [], [], []

    def mutate(s):
        if sub_rate <= 0:
            return s
        b = bytearray(s.encode())
        for j in np.flatnonzero(rng.random(len(b)) < sub_rate):
            b[j] = ord("ACGT"[("ACGT".index(chr(b[j])) + int(rng.integers(1, 4))) % 4])
        return b.decode()

    def junk():
        return "".join("ACGT"[x] for x in rng.integers(0, 4, mate_len))

    for i in range(n):
        t = ok[int(rng.integers(len(ok)))]
        s = txs[t]
        flen = min(len(s), int(rng.integers(frag_lo, frag_hi + 1)))
        flen = max(flen, mate_len)
        start = int(rng.integers(0, len(s) - flen + 1))
        frag = s[start:start + flen]
        a, b = mutate(frag[:mate_len]), mutate(frag[-mate_len:])
        if chimera_every and i % chimera_every == 3:
            s2 = txs[ok[int(rng.integers(len(ok)))]]
            st2 = int(rng.integers(0, len(s2) - mate_len + 1))
            b = mutate(s2[st2:st2 + mate_len])
        if orient == "fr":
            m1, m2 = a, revcomp_text(b)
        elif orient == "rf":
            m1, m2 = revcomp_text(a), b
        else:
            m1, m2 = a, b
        if junk_every and i % junk_every == 0:
            m1 = junk()
        elif junk_every and i % junk_every == 1:
            m2 = junk()
        elif junk_every and i % junk_every == 2:
            m1, m2 = junk(), junk()
        r1.append(m1)
        r2.append(m2)
        src.append(t)
    return r1, r2, np.array(src, np.int64)


def model_pairs(host, reads1, reads2, orient="fr", allowed=2):
    """the whole model on text mates: pack (the checker's packer), orient the packed reads, oracle per mate, pair rule.
    -> (results, class_offsets, class_ids, stats, mates1, mates2)"""
    oracle = helpers.Oracle(host)
    mates = []
    for reads, rc in zip((reads1, reads2), ORIENT[orient]):
        tiles, lens, wpr = helpers.pack_reads_tiles(reads)
        if rc:
            tiles = revcomp_tiles(tiles, lens, wpr)
        o_res, coff, ids, _ = oracle.map_tiles(tiles, lens, wpr, allowed, 4)
        mates.append(mates_from_oracle(o_res, coff, ids))
    res, coff, ids, st = combine(mates[0], mates[1])
    return res, coff, ids, st, mates[0], mates[1]
