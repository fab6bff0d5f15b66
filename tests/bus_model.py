"""Pure-Python model of the BUS output (include/pseudoaligner_amd.h, pa_bus / pa_write_bus), written from the rules of that section alone:
the six fates in their order, the ec numbering, the sorted collapsed records and all eight stats — what the GPU writer must equal
exactly — plus an independent reader and writer of the three files (struct for the BUS v1 layout) and the builder of the directed cases
(records and arenas written by hand, no aligner in the loop). No copy of bustools or kallisto exists where this runs: conformance with
the format is argued from its description, and this reader / writer is the second implementation the bytes are compared with."""
from __future__ import annotations

import struct
from collections import Counter

import numpy as np

BASES = "ACGT"
CODE = {b: i for i, b in enumerate(BASES)}
STAT_NAMES = ("reads", "r1_short", "barcode_n", "umi_n", "unmapped", "bad_class", "recorded", "records")
BAD = "bad"   # in a mapping: a class the record cannot name (a reference past the index's classes, a range outside the arena)

RESULT_DTYPE = np.dtype([("coverage", "<u4"), ("mismatches", "<u4"), ("class_off", "<u4"), ("class_len", "<u4")])   # pa_read_result
RECORD_DTYPE = np.dtype([("barcode", "<u8"), ("umi", "<u8"), ("ec", "<i4"), ("count", "<u4"), ("flags", "<u4"), ("pad", "<u4")])   # pa_bus_record
MAPPED_BIT = 0x80000000   # PA_MAPPED_BIT (mismatches)
CLASS_REF = 0x80000000    # PA_CLASS_REF (class_off)
COUNT_MAX = 0xFFFFFFFF


def pack(seq: str) -> int:
    """2 bits per base, A=0 C=1 G=2 T=3, first base most significant"""
    v = 0
    for ch in seq:
        v = v * 4 + CODE[ch]
    return v


def fate(r1: str, mapped: bool, ids, num_tx: int, bc_len: int, umi_len: int) -> str:
    """the first rule that applies"""
    if len(r1) < bc_len + umi_len:
        return "r1_short"
    if any(ch not in CODE for ch in r1[:bc_len]):
        return "barcode_n"
    if any(ch not in CODE for ch in r1[bc_len:bc_len + umi_len]):
        return "umi_n"
    if not mapped or (not isinstance(ids, str) and len(ids) == 0):
        return "unmapped"
    if isinstance(ids, str) or any(int(t) >= num_tx for t in ids) or any(int(a) >= int(b) for a, b in zip(ids[:-1], ids[1:])):
        return "bad_class"
    return "recorded"


def index_classes(index: dict):
    """the id lists of a host index's classes (HostIndex.arrays())"""
    off = np.asarray(index["ec_offset"]).astype(np.int64)
    ids = np.asarray(index["ec_ids"])
    return [tuple(int(t) for t in ids[off[c]:off[c + 1]]) for c in range(int(index["num_classes"]))]


def number_ecs(num_tx: int, classes, recorded_lists):
    """-> (ec of every id tuple that can be recorded, the table [ids of ec 0, ids of ec 1, ...]): t < T is {t}; T + j the j-th index
    class of two ids or more in class-id order; then the recorded lists of two ids or more that equal no index class, lexicographically"""
    table = [(t,) for t in range(num_tx)]
    ec_of = {}
    for c in classes:
        if len(c) >= 2:
            ec_of.setdefault(tuple(c), len(table))
            table.append(tuple(c))
    novel = sorted({tuple(l) for l in recorded_lists if len(l) >= 2 and tuple(l) not in ec_of})   # tuple order = lexicographic order
    for l in novel:
        ec_of[l] = len(table)
        table.append(l)
    return ec_of, table, novel


def model(r1s, mapping, num_tx: int, classes, bc_len: int, umi_len: int):
    """r1s: R1 strings; mapping: per read (mapped, ids of its R2's class | BAD); classes: index_classes().
    -> (records [(barcode, umi, ec, count)] sorted, ec table [tuple of ids], stats dict, fates [str per read])"""
    st = dict.fromkeys(STAT_NAMES, 0)
    fates, kept = [], []
    for r1, (mapped, ids) in zip(r1s, mapping):
        f = fate(r1, mapped, ids, num_tx, bc_len, umi_len)
        st["reads"] += 1
        st[f] += 1
        fates.append(f)
        if f == "recorded":
            kept.append((pack(r1[:bc_len]), pack(r1[bc_len:bc_len + umi_len]), tuple(int(t) for t in ids)))
    ec_of, table, _ = number_ecs(num_tx, classes, [k[2] for k in kept])
    reads = Counter((b, u, ids[0] if len(ids) == 1 else ec_of[ids]) for b, u, ids in kept)
    records = sorted((b, u, ec, min(n, COUNT_MAX)) for (b, u, ec), n in reads.items())
    st["records"] = len(records)
    assert st["reads"] == sum(st[k] for k in STAT_NAMES[1:7])
    return records, table, st, fates


# ---- the three files ----
def bus_bytes(records, bc_len: int, umi_len: int, text: bytes = b"") -> bytes:
    """a BUS v1 file: "BUS\\0", u32 version = 1, u32 bclen, u32 umilen, u32 tlen, the text, then 32 bytes per record:
    u64 barcode, u64 umi, i32 ec, u32 count, u32 flags = 0, u32 pad = 0 — all little-endian"""
    out = [b"BUS\0", struct.pack("<IIII", 1, bc_len, umi_len, len(text)), text]
    for b, u, ec, n in records:
        out.append(struct.pack("<QQiIII", b, u, ec, n, 0, 0))
    return b"".join(out)


def read_bus(data: bytes):
    """-> (bc_len, umi_len, text, [(barcode, umi, ec, count)]); the magic, the version, flags = pad = 0 and the length are checked"""
    assert data[:4] == b"BUS\0", data[:4]
    version, bc_len, umi_len, tlen = struct.unpack_from("<IIII", data, 4)
    assert version == 1
    text = data[20:20 + tlen]
    body = data[20 + tlen:]
    assert len(body) % 32 == 0
    records = []
    for off in range(0, len(body), 32):
        b, u, ec, n, flags, pad = struct.unpack_from("<QQiIII", body, off)
        assert flags == 0 and pad == 0
        records.append((b, u, ec, n))
    return bc_len, umi_len, text, records


def matrix_ec_text(table) -> str:
    return "".join("%d\t%s\n" % (ec, ",".join(str(t) for t in ids)) for ec, ids in enumerate(table))


def read_matrix_ec(text: str):
    table = []
    for j, line in enumerate(text.splitlines()):
        ec, ids = line.split("\t")
        assert int(ec) == j
        table.append(tuple(int(t) for t in ids.split(",")))
    return table


def transcripts_text(names) -> str:
    return "".join(n + "\n" for n in names)


def table_from_csr(offsets, ids):
    offsets = [int(x) for x in offsets]
    return [tuple(int(t) for t in ids[a:b]) for a, b in zip(offsets[:-1], offsets[1:])]


def records_from_array(arr):
    """pa_bus_record array -> [(barcode, umi, ec, count)], flags = pad = 0 checked"""
    assert not arr["flags"].any() and not arr["pad"].any()
    return list(zip(arr["barcode"].tolist(), arr["umi"].tolist(), arr["ec"].tolist(), arr["count"].tolist()))


# ---- directed cases: the mapping's records written by hand ----
def singleton_classes(index: dict):
    """[(class, its one transcript)]"""
    return [(c, ids[0]) for c, ids in enumerate(index_classes(index)) if len(ids) == 1]


def multi_classes(index: dict):
    """[(class, its ids, j = its rank among the classes of two ids or more)]"""
    out = []
    for c, ids in enumerate(index_classes(index)):
        if len(ids) >= 2:
            out.append((c, ids, len(out)))
    return out


def directed(reads, index: dict, seed: int = 0, shuffle: bool = True, pad: int = 1):
    """reads: [(r1 text, cls, how many reads)] with cls one of
      int c                      by reference: class_off = PA_CLASS_REF | c, class_len = the length of index class c (1 past the index)
      list of ids                in the arena, one copy per distinct content
      ("fresh", ids)             in the arena at an offset of its own
      ("unmapped", int | list)   the same record with PA_MAPPED_BIT clear
      None                       an unmapped record without a class
      ("raw", off, len)          class_off / class_len as given (a range the arena does not hold)
    `pad` words of padding lead the arena (a list's offset moves with it).
    -> (r1 strings, records RESULT_DTYPE, arena uint32 (never empty), mapping [(mapped, ids | BAD)])"""
    rng = np.random.default_rng(seed)
    classes = index_classes(index)
    arena, arena_at = [0xDEADBEEF] * max(pad, 1), {}
    r1s, recs, mapping = [], [], []

    def put(ids, fresh):
        if fresh or tuple(ids) not in arena_at:
            arena_at[tuple(ids)] = len(arena)
            arena.extend(ids)
        return arena_at[tuple(ids)]

    for text, cls, count in reads:
        mapped = True
        if cls is None:
            mapped, cls = False, []
        elif isinstance(cls, tuple) and cls[0] == "unmapped":
            mapped, cls = False, cls[1]
        if isinstance(cls, (int, np.integer)):
            c = int(cls)
            ids = list(classes[c]) if c < len(classes) else BAD
            class_off, class_len = CLASS_REF | c, len(ids) if c < len(classes) else 1
        elif isinstance(cls, tuple) and cls[0] == "raw":
            ids, class_off, class_len = BAD, int(cls[1]), int(cls[2])
        else:
            fresh = isinstance(cls, tuple) and cls[0] == "fresh"
            ids = [int(t) for t in (cls[1] if fresh else cls)]
            class_off, class_len = (put(ids, fresh) if ids else 0), len(ids)
        for _ in range(count):
            r1s.append(text)
            recs.append((40 + len(recs) % 50, (MAPPED_BIT if mapped else 0) | (len(recs) % 3), class_off, class_len))
            mapping.append((mapped, ids))
    order = rng.permutation(len(r1s)) if shuffle else np.arange(len(r1s))
    records = np.array(recs, RESULT_DTYPE)[order] if recs else np.zeros(0, RESULT_DTYPE)
    return [r1s[i] for i in order], records, np.array(arena, np.uint32), [mapping[i] for i in order]


# ---- the paired test data of tests/test_gpu_bus.py ----
def make_case(seed: int, transcripts, bc_len: int, umi_len: int, n_pairs: int = 20000, n_cells: int = 150, read_len: int = 90):
    """-> dict(r1, r2): R2 cut from transcripts (some with substitutions, some random), R1 = barcode + UMI + a tail of 0..11 bases
    with injected Ns, lower-case bytes and short reads. Few cells and short molecule lists, so that (barcode, UMI, ec) repeat."""
    rng = np.random.default_rng(seed)
    rand = lambda n: "".join(BASES[x] for x in rng.integers(0, 4, n))
    cells = [rand(bc_len) for _ in range(n_cells)]
    usable = [t for t, s in enumerate(transcripts) if len(s) >= read_len + 10]
    r1, r2 = [], []
    while len(r1) < n_pairs:
        cell, umi = cells[int(rng.integers(n_cells))], rand(umi_len)
        t = usable[int(rng.integers(len(usable)))]
        s = transcripts[t]
        for _ in range(int(rng.integers(1, 6))):
            x = rng.random()
            if x < 0.1:
                seq = rand(read_len)
            else:
                p = int(rng.integers(0, len(s) - read_len + 1))
                seq = list(s[p:p + read_len])
                if x < 0.4:
                    for i in np.flatnonzero(rng.random(read_len) < 0.01):
                        seq[i] = BASES[(CODE.get(seq[i], 0) + 1 + int(rng.integers(3))) % 4]
                seq = "".join(seq)
            text = cell + umi + rand(int(rng.integers(0, 12)))
            y = rng.random()
            if y < 0.03:
                i = int(rng.integers(bc_len + umi_len))
                text = text[:i] + "N" + text[i + 1:]
            elif y < 0.04:
                i = int(rng.integers(bc_len + umi_len))
                text = text[:i] + text[i].lower() + text[i + 1:]
            elif y < 0.06:
                text = text[:int(rng.integers(0, bc_len + umi_len))]
            r1.append(text)
            r2.append(seq)
    return dict(r1=r1[:n_pairs], r2=r2[:n_pairs])


def mapping_from_oracle(oracle, r2, nthreads: int = 8):
    res, coff, cids, _ = oracle.map_reads(r2, 2, nthreads)
    return [(bool(res["mapped"][i]), [int(t) for t in cids[int(coff[i]):int(coff[i + 1])]]) for i in range(len(r2))]
