"""Model of the overflow table of novel classes (csrc/collective.hip: pa_overflow_insert_kernel, pa_overflow_export_kernel) in plain Python and
numpy; no product code. What the table must hold after any sequence of inserts is a Counter over id tuples; what fetch must return is that
Counter serialised canonically. Besides that the model knows where a list starts its probe walk (list hash, start slot, sizing rule), so that
tests/test_gpu_overflow_edges.py can DESIGN lists that share a start slot, wrap through slot 0, or share their whole 64-bit key."""
from collections import Counter

import numpy as np

M64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15
SEED = 0x243F6A8885A308D3
MIN_CAP = 1024
META_WORDS = 6                    # per slot: pool offset, length, count low, count high, ready, pad
STATUS_TABLE_FULL, STATUS_POOL_FULL, STATUS_LIST_FULL, STATUS_EXPORT_FULL = 1, 2, 4, 8
PAIR_IDS = 600                    # the designers search the two-id lists (a, b), a < b < PAIR_IDS


def fmix64(x):
    """murmur3's finaliser (pa_mix64)"""
    x &= M64
    x ^= x >> 33
    x = x * 0xFF51AFD7ED558CCD & M64
    x ^= x >> 33
    x = x * 0xC4CEB9FE1A85EC53 & M64
    x ^= x >> 33
    return x


def list_hash(ids):
    h = SEED ^ len(ids)
    for i in ids:
        h = (fmix64(h ^ int(i)) + GOLDEN) & M64
    return h


def key_of(ids):
    """what the table stores in keys[slot]: the list hash with bit 63 forced (0 = a free slot)"""
    return list_hash(ids) | 1 << 63


def start_slot(h, cap):
    return ((h | 1 << 63) * GOLDEN & M64) >> 20 & (cap - 1)


def slot_of(ids, cap=MIN_CAP):
    return start_slot(list_hash(ids), cap)


def table_cap(max_classes):
    """slots of a table made for max_classes distinct classes: load <= 0.5, at least 1024"""
    cap = MIN_CAP
    while cap < 2 * max_classes:
        cap <<= 1
    return cap


# ---- the serialised form: [records, words, {len, count lo, count hi, ids ...} ...], lexicographic by id list ----
def serialise(table):
    w = [0, 0]
    for ids in sorted(table):
        c = int(table[ids])
        assert 0 < c < 1 << 64 and len(ids) > 0
        w += [len(ids), c & 0xFFFFFFFF, c >> 32]
        w += [int(i) for i in ids]
    w[0], w[1] = len(table), len(w)
    return np.array(w, dtype=np.uint32)


def parse(words):
    words = [int(x) for x in words]
    assert len(words) >= 2 and words[1] == len(words), "header: %r for %d words" % (words[:2], len(words))
    out, p = Counter(), 2
    for _ in range(words[0]):
        assert p + 3 <= len(words), "record at word %d starts beyond the end" % p
        n = words[p]
        ids = tuple(words[p + 3:p + 3 + n])
        assert len(ids) == n and ids not in out, "record at word %d" % p
        out[ids] = words[p + 1] | words[p + 2] << 32
        p += 3 + n
    assert p == len(words), "records end at word %d of %d" % (p, len(words))
    return out


# ---- numpy forms of the hash, for the designers ----
def _fmix64_np(x):
    x = x ^ (x >> np.uint64(33))
    x = x * np.uint64(0xFF51AFD7ED558CCD)
    x = x ^ (x >> np.uint64(33))
    x = x * np.uint64(0xC4CEB9FE1A85EC53)
    return x ^ (x >> np.uint64(33))


def _step_np(h, ids):
    with np.errstate(over="ignore"):
        return _fmix64_np(h ^ ids.astype(np.uint64)) + np.uint64(GOLDEN)


_pairs = None


def pair_lists():
    """every two-id list (a, b), a < b < PAIR_IDS, with its hash: (a[], b[], h[])"""
    global _pairs
    if _pairs is None:
        a, b = np.triu_indices(PAIR_IDS, 1)
        h1 = _step_np(np.uint64(SEED ^ 2), a)
        _pairs = (a, b, _step_np(h1, b))
    return _pairs


def pair_slots(cap=MIN_CAP):
    a, b, h = pair_lists()
    with np.errstate(over="ignore"):
        return ((h | np.uint64(1 << 63)) * np.uint64(GOLDEN) >> np.uint64(20) & np.uint64(cap - 1)).astype(np.int64)


def lists_for_slot(slot, count, cap=MIN_CAP):
    """the first `count` two-id lists (in (a, b) order) whose probe walk starts at `slot` of a table of `cap` slots"""
    a, b, _ = pair_lists()
    at = np.flatnonzero(pair_slots(cap) == slot)[:count]
    assert len(at) == count, "only %d two-id lists start at slot %d of %d" % (len(at), slot, cap)
    return [(int(a[i]), int(b[i])) for i in at]


def near_lists_for_slot(slot, cap=MIN_CAP):
    """two-id lists that start at `slot` and are as alike as lists of one start slot can be: -> (same first id: (a, b), (a, b')),
    (same last id: (a, b), (a', b)); None where the slot has no such pair"""
    a, b, _ = pair_lists()
    at = np.flatnonzero(pair_slots(cap) == slot)
    by_first, by_last, first, last = {}, {}, None, None
    for i in at:
        x, y = int(a[i]), int(b[i])
        if first is None and x in by_first:
            first = ((x, by_first[x]), (x, y))
        if last is None and y in by_last:
            last = ((by_last[y], y), (x, y))
        by_first.setdefault(x, y)
        by_last.setdefault(y, x)
    return first, last


def longer_list_for_slot(prefix, slot, cap=MIN_CAP, limit=1 << 16):
    """prefix + (c,) with the smallest c > prefix[-1] that starts at `slot`"""
    for c in range(prefix[-1] + 1, prefix[-1] + 1 + limit):
        if slot_of(prefix + (c,), cap) == slot:
            return prefix + (c,)
    raise AssertionError("no extension of %r starts at slot %d" % (prefix, slot))


def chain_slots(lists, cap=MIN_CAP):
    """slots the distinct `lists` end up in when they are inserted one after the other, in this order, into an empty table"""
    taken, out = set(), []
    for ids in lists:
        s = slot_of(ids, cap)
        while s in taken:
            s = (s + 1) & (cap - 1)
        taken.add(s)
        out.append(s)
    return out


def colliding_lists(prefix=(), tail=(), n_first=1 << 18):
    """Two DIFFERENT lists of one length with the SAME 64-bit hash, hence the same key and start slot in a table of any size: the one case
    in which the table's content comparison decides (a key that differs ends the comparison before it starts). The lists are
    prefix + (a, b) + tail and prefix + (a', b') + tail. With h the state behind the prefix, the state behind a is h1(a) = fmix64(h ^ a) +
    golden and b enters as h1 ^ b, so the two collide behind b — and then behind any common tail — exactly when h1(a) ^ b == h1(a') ^ b'.
    That needs the high words of h1(a) and h1(a') equal (ids are 32 bits): a birthday search over n_first values of a; then
    b' = b ^ low32(h1(a) ^ h1(a')). No two lists that differ in ONE position collide: every step is a bijection of the state.
    (a, b) and (a', b') ascending where the search allows it: -> (prefix + (a, b) + tail, prefix + (a', b') + tail)"""
    h = SEED ^ (len(prefix) + 2 + len(tail))
    for i in prefix:
        h = (fmix64(h ^ int(i)) + GOLDEN) & M64
    a = np.arange(n_first, dtype=np.uint64)
    h1 = _step_np(np.uint64(h), a)
    hi = h1 >> np.uint64(32)
    order = np.argsort(hi, kind="stable")
    same = np.flatnonzero(hi[order][1:] == hi[order][:-1])
    assert len(same), "no two of the first %d ids share the high word of their state" % n_first
    best = None
    for j in same:
        x, y = int(order[j]), int(order[j + 1])
        d = int(h1[x] ^ h1[y])
        assert d >> 32 == 0 and d != 0
        b = 0xFFFFFFFE & ~d if d >> 31 == 0 else 0xFFFFFFFE    # b and b ^ d both above every first id when d's top bit is clear
        pair = (tuple(prefix) + (x, b) + tuple(tail), tuple(prefix) + (y, b ^ d) + tuple(tail))
        if d >> 31 == 0:
            return pair
        best = best or pair
    return best
