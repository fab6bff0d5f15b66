"""A model of the compact records (pa_results_compact_device), written from the text of include/pseudoaligner_amd.h and from nothing else: plain Python
integers, one record at a time, no scan and none of the kernel's arithmetic.

A launch's record is pa_read_result {coverage, mismatches (bit 31: mapped), class_off (bit 31: PA_CLASS_REF), class_len}; its class is
  unmapped   bit 31 of mismatches clear: whatever the class fields hold means nothing
  empty      mapped, class_len == 0 (whatever class_off holds, the REF bit included)
  by ref     mapped, class_len != 0, PA_CLASS_REF set: index class class_off & 0x7FFFFFFF
  packed     mapped, class_len != 0, no REF bit, class_off + class_len <= arena_cap: the ids are arena[class_off : class_off + class_len]
  lost       mapped, class_len != 0, no REF bit, the ids do not lie inside the launch's arena
and the 8-byte record says
  bits 0..13 coverage | bits 14..27 mismatches | bit 28 mapped | bit 29 BY_REF | bit 30 PACKED | bit 31 nothing | bits 32..63 `hi`
  hi = the index class (by ref) | the word offset of the record's {length, ids...} entry in the packed stream of the launch, modulo 2^32 (packed) | 0
  neither class bit: empty or unmapped; both: lost (no entry, no room taken in the stream).
Entries follow each other in READ order; one that would end beyond packed_cap is not written (offsets are monotone: none behind it is either);
`need` counts every entry, written or not."""
import numpy as np

MAPPED_BIT = 0x80000000
CLASS_REF = 0x80000000
COMPACT_MAPPED, COMPACT_BY_REF, COMPACT_PACKED = 0x10000000, 0x20000000, 0x40000000
FIELD_BITS = 14
FIELD_MAX = (1 << FIELD_BITS) - 1          # PA_COMPACT_MAX_READ_LEN
RESULT_DTYPE = np.dtype([("coverage", "<u4"), ("mismatches", "<u4"), ("class_off", "<u4"), ("class_len", "<u4")])
KINDS = ("unmapped", "empty", "by_ref", "packed", "lost")


def kind(rec, arena_cap):
    """which of the five kinds a pa_read_result record is"""
    mm, off, ln = int(rec["mismatches"]), int(rec["class_off"]), int(rec["class_len"])
    if not mm & MAPPED_BIT:
        return "unmapped"
    if ln == 0:
        return "empty"
    if off & CLASS_REF:
        return "by_ref"
    return "packed" if off + ln <= int(arena_cap) else "lost"      # (Python integers: the sum does not wrap)


def compact(results, arena, arena_cap, packed_cap):
    """-> (compact u64[n], packed u32[min(need, packed_cap)], written bool[the same]: the words that must have been written, need)"""
    results = np.asarray(results, RESULT_DTYPE).reshape(-1)
    arena = np.asarray(arena, np.uint32).reshape(-1)
    arena_cap, packed_cap = int(arena_cap), int(packed_cap)
    n = len(results)
    out = np.zeros(n, np.uint64)
    entries = []                                                    # (word offset, ids) of every packed record, in read order
    need = 0
    for i in range(n):
        r = results[i]
        k = kind(r, arena_cap)
        lo = (int(r["coverage"]) & FIELD_MAX) | ((int(r["mismatches"]) & FIELD_MAX) << FIELD_BITS)
        hi = 0
        if k != "unmapped":
            lo |= COMPACT_MAPPED
        if k == "by_ref":
            lo |= COMPACT_BY_REF
            hi = int(r["class_off"]) & ~CLASS_REF & 0xFFFFFFFF
        elif k == "packed":
            lo |= COMPACT_PACKED
            hi = need & 0xFFFFFFFF
            off, ln = int(r["class_off"]), int(r["class_len"])
            assert off + ln <= len(arena), "a packed record must lie inside the arena that is really there"
            entries.append((need, arena[off:off + ln].copy()))
            need += 1 + ln
        elif k == "lost":
            lo |= COMPACT_BY_REF | COMPACT_PACKED
        out[i] = lo | (hi << 32)
    m = min(need, packed_cap)
    packed, written = np.zeros(m, np.uint32), np.zeros(m, bool)
    for at, ids in entries:
        if at + 1 + len(ids) <= packed_cap:
            packed[at] = len(ids)
            packed[at + 1:at + 1 + len(ids)] = ids
            written[at:at + 1 + len(ids)] = True
    return out, packed, written, need


def fields(record):
    """one 8-byte record -> dict(coverage, mismatches, mapped, by_ref, packed, bit31, hi)"""
    v = int(record)
    lo = v & 0xFFFFFFFF
    return dict(coverage=lo & FIELD_MAX, mismatches=(lo >> FIELD_BITS) & FIELD_MAX, mapped=bool(lo & COMPACT_MAPPED), by_ref=bool(lo & COMPACT_BY_REF),
                packed=bool(lo & COMPACT_PACKED), bit31=bool(lo & 0x80000000), hi=v >> 32)


def class_table(index_arrays):
    """{ids of an index class: its number} of the flat index"""
    off = index_arrays["ec_offset"].astype(np.int64)
    ids = index_arrays["ec_ids"]
    return {tuple(ids[off[c]:off[c + 1]].tolist()): c for c in range(int(index_arrays["num_classes"]))}


def records_of(mapped, coverage, mismatches, classes, table, junk=3):
    """what a launch writes for reads with these answers -> (records, arena, arena_cap): a class that is an index class goes by reference, any other
    one into the arena (with `junk` words of padding in front of each: offset 0 is nothing special), an empty one nowhere"""
    n = len(classes)
    rec = np.zeros(n, RESULT_DTYPE)
    arena = []
    for i in range(n):
        if not mapped[i]:
            continue
        ids = tuple(int(x) for x in classes[i])
        rec[i]["coverage"], rec[i]["mismatches"], rec[i]["class_len"] = int(coverage[i]), int(mismatches[i]) | MAPPED_BIT, len(ids)
        if not ids:
            continue
        c = table.get(ids)
        if c is not None:
            rec[i]["class_off"] = CLASS_REF | c
        else:
            arena += [0xEEEE0000 + j for j in range(junk)]
            rec[i]["class_off"] = len(arena)
            arena += list(ids)
    arena = np.array(arena + [0xEEEE0000], np.uint32)
    return rec, arena, len(arena)


def host_batch(mapped, coverage, mismatches, coff, ids, index_arrays, chunk):
    """what the host-to-host entry returns for a batch with these answers, mapped in chunks of `chunk` reads: every chunk is a launch of its own (`hi` of
    its packed records restarts at 0), the packed streams of the chunks follow each other -> (compact u64[n], packed u32[words], words of every chunk)"""
    table = class_table(index_arrays)
    n = len(mapped)
    coff = np.asarray(coff, np.int64)
    out, streams, words = [], [], []
    for lo in range(0, n, chunk):
        hi = min(n, lo + chunk)
        classes = [ids[coff[i]:coff[i + 1]] for i in range(lo, hi)]
        rec, arena, cap = records_of(mapped[lo:hi], coverage[lo:hi], mismatches[lo:hi], classes, table)
        c, p, w, need = compact(rec, arena, cap, 1 << 40)
        assert w.all() and need == len(p)
        out.append(c); streams.append(p); words.append(need)
    cat = lambda parts, dt: np.concatenate(parts).astype(dt) if parts else np.zeros(0, dt)
    return cat(out, np.uint64), cat(streams, np.uint32), words
