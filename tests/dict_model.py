"""The k-mer dictionary's two bucketed formats read back in numpy, from the text of csrc/device_layout.hpp (not from the builders' dict_slots.hpp):

  k <= 32   16-byte slots {key_lo, key_hi, handle, off | ~flags << 24}, four to a 64-byte bucket. bucket = mulhi32(x, nbuckets), home slot
            j = x & 3, x = the 32-bit mix of pa_bucket_home. A key lies in its home slot, or in slot (j + 1 + i) & 3 of the bucket (flag i of slot j
            says so), or went on to the next bucket (flag 3 of slot j), where the same rule applies to slot j of that bucket.
  k > 32    lines of two entries {key word 0..3, handle, off, -, -}. bucket = mulhi32(pa_mix128(lo, hi) >> 32, nbuckets), linear probing over lines,
            a line with a free entry ends the probe sequence.

Both lookups follow at most DICT_MAX_PROBES = 15 buckets beyond the first, as the mapping kernel does. `lookup` answers for one k-mer, `lookup_many` for
arrays of them, `audit` checks a whole table and says where its keys lie. A table is the u64 (or u32, or byte) array the library's test surface returns;
a k-mer is a Python int (base j in bits 2 j, 2 j + 1), arrays of k-mers are two u64 arrays (low word, high word; the high word is 0 for k <= 32)."""
import numpy as np

EMPTY = 0xFFFFFFFF
MAX_PROBES = 15                 # DICT_MAX_PROBES
SLOT_LOAD, LINE_LOAD = 0.25, 1.0 / 3.0   # the loads the library ships (DICT_LOAD; k > 32: load <= 1/3)
_U32, _U64 = np.uint32, np.uint64
HOME, NAMED0, ON = 0, 1, 4      # codes of `where`: 0 home slot, 1 + i named slot i, ON - 1 + d: d >= 1 buckets on


def slots_per_bucket(k):
    return 4 if k <= 32 else 2


def shipped_load(k):
    return SLOT_LOAD if k <= 32 else LINE_LOAD


def first_sizing(num_kmers, k, load):
    """the buckets the builders begin with: nk / (slots x load) + 1 (a retry multiplies the load by 0.75)"""
    return max(1, int(num_kmers / (slots_per_bucket(k) * load)) + 1)


def where_name(w):
    w = int(w)
    return "home slot" if w == HOME else "named slot %d" % (w - NAMED0) if w < ON else "%d buckets on" % (w - ON + 1)


def words(table, nbuckets):
    t = np.ascontiguousarray(table).view(_U32)
    assert t.size == 16 * nbuckets, "a table of %d words is not %d buckets of 64 bytes" % (t.size, nbuckets)
    return t.reshape(nbuckets, 16)


def _mix64(x):   # murmur3 fmix64 on u64 arrays
    x = x ^ (x >> _U64(33))
    x = x * _U64(0xff51afd7ed558ccd)
    x = x ^ (x >> _U64(33))
    x = x * _U64(0xc4ceb9fe1a85ec53)
    return x ^ (x >> _U64(33))


def pa_mix128(lo, hi):
    lo, hi = np.atleast_1d(np.asarray(lo, _U64)), np.atleast_1d(np.asarray(hi, _U64))
    return _mix64(lo ^ (_mix64(hi) * _U64(0x9e3779b97f4a7c15)))


def mulhi32(x, n):
    return ((np.asarray(x, _U64) & _U64(EMPTY)) * _U64(n)) >> _U64(32)


def pa_bucket_home(lo, nbuckets):
    """k <= 32: (bucket, home slot) of the k-mers in the u64 array lo"""
    lo = np.atleast_1d(np.asarray(lo, _U64))
    x = (lo & _U64(EMPTY)).astype(_U32) * _U32(0x9E3779B1) + (lo >> _U64(32)).astype(_U32) * _U32(0x85EBCA77)
    x = x ^ (x >> _U32(15))
    x = x * _U32(0x2C1B3C6D)
    x = x ^ (x >> _U32(13))
    return mulhi32(x, nbuckets).astype(np.int64), (x & _U32(3)).astype(np.int64)


def bucket_of(lo, hi, nbuckets, k):
    """(bucket, home slot) under either format (k > 32: no home slot, 0)"""
    if k <= 32:
        return pa_bucket_home(lo, nbuckets)
    b = mulhi32(pa_mix128(lo, hi) >> _U64(32), nbuckets).astype(np.int64)
    return b, np.zeros(len(b), np.int64)


def split(kmer):
    return np.array([kmer & 0xFFFFFFFFFFFFFFFF], _U64), np.array([kmer >> 64], _U64)


def kmer_string(lo, hi, k):
    v = int(lo) | (int(hi) << 64)
    return "".join("ACGT"[(v >> (2 * j)) & 3] for j in range(k))


def kmer_of_string(s):
    return sum("ACGT".index(c) << (2 * j) for j, c in enumerate(s))


def _slot_hit(T, b, slot, lo, hi):
    """do the slots (b, slot) hold the keys? -> (hit, handle, off, flags of the slot)"""
    rows = T[b]
    col = 4 * slot
    idx = np.arange(len(b))
    w0, w1, w2, w3 = rows[idx, col], rows[idx, col + 1], rows[idx, col + 2], rows[idx, col + 3]
    hit = (w2 != EMPTY) & (w0 == (lo & _U64(EMPTY)).astype(_U32)) & (w1 == (lo >> _U64(32)).astype(_U32))
    return hit, w2, w3 & _U32(0xFFFFFF), (~w3 >> _U32(24)) & _U32(15)


def lookup_many(table, nbuckets, k, lo, hi=None, wrap=True):
    """-> (found, handle, off, buckets beyond home, where) for the k-mers (lo, hi). wrap=False is the negative control of tests/test_dict_model.py: a
    probe that runs off the table's end stops there"""
    T = words(table, nbuckets)
    lo = np.atleast_1d(np.asarray(lo, _U64))
    hi = np.zeros(len(lo), _U64) if hi is None else np.atleast_1d(np.asarray(hi, _U64))
    n = len(lo)
    found, handle, off = np.zeros(n, bool), np.full(n, EMPTY, _U32), np.zeros(n, _U32)
    dist, where = np.zeros(n, np.int64), np.zeros(n, np.int64)
    b0, home = bucket_of(lo, hi, nbuckets, k)
    active = np.arange(n)
    for d in range(MAX_PROBES + 1):
        if not len(active):
            break
        b = b0[active] + d
        if wrap:
            b = np.where(b >= nbuckets, b - nbuckets, b)
        else:
            active, b = active[b < nbuckets], b[b < nbuckets]
        al, ah = lo[active], hi[active]
        go_on = np.zeros(len(active), bool)
        if k <= 32:
            j = home[active]
            hit, h, o, flags = _slot_hit(T, b, j, al, ah)
            w = np.full(len(active), HOME if d == 0 else ON - 1 + d, np.int64)
            for i in range(3):   # the slots the home slot names
                named = ~hit & ((flags >> _U32(i)) & _U32(1)).astype(bool)
                if named.any():
                    hit2, h2, o2, _ = _slot_hit(T, b, (j + 1 + i) & 3, al, ah)
                    take = named & hit2
                    h, o = np.where(take, h2, h), np.where(take, o2, o)
                    if d == 0:
                        w = np.where(take, NAMED0 + i, w)
                    hit = hit | take
            go_on = ~hit & ((flags & _U32(8)) != 0)
        else:
            rows = T[b]
            hit, h, o = np.zeros(len(active), bool), np.full(len(active), EMPTY, _U32), np.zeros(len(active), _U32)
            full = np.ones(len(active), bool)
            key = [(al & _U64(EMPTY)).astype(_U32), (al >> _U64(32)).astype(_U32), (ah & _U64(EMPTY)).astype(_U32), (ah >> _U64(32)).astype(_U32)]
            for i in range(2):
                occupied = rows[:, 8 * i + 4] != EMPTY
                same = occupied & ~hit
                for t in range(4):
                    same &= rows[:, 8 * i + t] == key[t]
                h, o = np.where(same, rows[:, 8 * i + 4], h), np.where(same, rows[:, 8 * i + 5], o)
                hit |= same
                full &= occupied
            w = np.full(len(active), HOME if d == 0 else ON - 1 + d, np.int64)
            go_on = ~hit & full
        at = active[hit]
        found[at], handle[at], off[at], dist[at], where[at] = True, h[hit], o[hit], d, w[hit]
        active = active[go_on]
    return found, handle, off, dist, where


def lookup(table, nbuckets, k, kmer, wrap=True):
    """one k-mer (a Python int) -> (handle, off, buckets beyond home, where) or None; where is "home slot", "named slot i" or "d buckets on" """
    lo, hi = split(kmer)
    found, handle, off, dist, where = lookup_many(table, nbuckets, k, lo, hi, wrap)
    return (int(handle[0]), int(off[0]), int(dist[0]), where_name(where[0])) if found[0] else None


def keys_of(table, nbuckets, k):
    """every occupied slot (k > 32: entry): (lo, hi, handle, off, bucket, slot)"""
    T = words(table, nbuckets)
    per, hw = (4, 2) if k <= 32 else (8, 4)            # words per slot / entry, the handle's word in it
    E = T.reshape(nbuckets, 16 // per, per)
    c, t = np.nonzero(E[:, :, hw] != EMPTY)
    e = E[c, t].astype(_U64)
    lo = e[:, 0] | (e[:, 1] << _U64(32))
    if k <= 32:
        return lo, np.zeros(len(lo), _U64), E[c, t, 2], E[c, t, 3] & _U32(0xFFFFFF), c, t
    return lo, e[:, 2] | (e[:, 3] << _U64(32)), E[c, t, 4], E[c, t, 5], c, t


def audit(table, nbuckets, k, samples=0, wrap=True):
    """Checks the table (AssertionError with the first offender) and returns what it holds:
      keys_per_bucket  int array [nbuckets]
      placements       {"home": n, "named": [n0, n1, n2], "on": {d: n for d >= 1}}
      wrapped          keys in a bucket whose index is below their home bucket's
      samples          {where or "wrapped": up to `samples` k-mers as strings}
      lo, hi, handle, off, where, dist   the keys, sorted by (hi, lo)"""
    T = words(table, nbuckets)
    lo, hi, handle, off, c, t = keys_of(table, nbuckets, k)
    n = len(lo)
    order = np.lexsort((lo, hi))
    lo, hi, handle, off, c, t = (a[order] for a in (lo, hi, handle, off, c, t))
    if n > 1:
        dup = np.nonzero((lo[1:] == lo[:-1]) & (hi[1:] == hi[:-1]))[0]
        assert not len(dup), "the key %s occurs twice" % kmer_string(lo[dup[0]], hi[dup[0]], k)
    if k < 32:
        assert not (lo >> _U64(2 * k)).any(), "a key has bits beyond its %d bases" % k
    elif 32 < k < 64:
        assert not (hi >> _U64(2 * (k - 32))).any(), "a key has bits beyond its %d bases" % k
    b, j = bucket_of(lo, hi, nbuckets, k)
    d = (c - b) % nbuckets
    far = np.nonzero(d > MAX_PROBES)[0]
    assert not len(far), "the key %s lies %d buckets from its home" % (kmer_string(lo[far[0]], hi[far[0]], k), d[far[0]])
    found, fh, fo, fd, where = lookup_many(table, nbuckets, k, lo, hi, wrap)
    bad = np.nonzero(~found | (fh != handle) | (fo != off) | (fd != d))[0]
    assert not len(bad), "the key %s of bucket %d is not found again by the lookup" % (kmer_string(lo[bad[0]], hi[bad[0]], k), c[bad[0]])
    if k <= 32:
        # the flags the placements imply: slot j of the key's last bucket names slot t when t != j; slot j of every bucket before it says "overflowed"
        need = np.zeros((nbuckets, 4), np.uint8)
        named = t != j
        np.bitwise_or.at(need, (c[named], j[named]), (1 << ((t[named] - j[named] - 1) & 3)).astype(np.uint8))
        for e in range(int(d.max()) if n else 0):
            m = d > e
            np.bitwise_or.at(need, ((b[m] + e) % nbuckets, j[m]), np.uint8(8))
        have = ((~T[:, 3::4] >> _U32(24)) & _U32(15)).astype(np.uint8)
        diff = np.argwhere(need != have)
        assert not len(diff), "slot %d of bucket %d has flags %x, its keys imply %x" % (
            diff[0][1], diff[0][0], have[tuple(diff[0])], need[tuple(diff[0])])
        expect_where = np.where(d > 0, ON - 1 + d, np.where(named, NAMED0 + ((t - j - 1) & 3), HOME))
    else:
        # a line with a free entry ends the probe sequence: every line a key went past is full
        full = (T[:, 4] != EMPTY) & (T[:, 12] != EMPTY)
        for e in range(int(d.max()) if n else 0):
            m = d > e
            assert full[(b[m] + e) % nbuckets].all(), "a key lies behind a line with a free entry"
        expect_where = np.where(d > 0, ON - 1 + d, HOME)
    assert np.array_equal(where, expect_where), "the lookup names another place than the one the key lies in"
    wrapped = c < b
    out_samples = {}
    if samples:
        for w in np.unique(where).tolist():
            idx = np.nonzero(where == w)[0]
            out_samples[where_name(w)] = [kmer_string(lo[i], hi[i], k) for i in idx[:: max(1, len(idx) // samples)][:samples]]
        idx = np.nonzero(wrapped)[0]
        out_samples["wrapped"] = [kmer_string(lo[i], hi[i], k) for i in idx[:samples]]
    on = {int(x): int(np.count_nonzero(d == x)) for x in np.unique(d[d > 0]).tolist()}
    return dict(keys_per_bucket=np.bincount(c, minlength=nbuckets), wrapped=int(np.count_nonzero(wrapped)), samples=out_samples,
                placements=dict(home=int(np.count_nonzero(where == HOME)), named=[int(np.count_nonzero(where == NAMED0 + i)) for i in range(3)], on=on),
                lo=lo, hi=hi, handle=handle, off=off, where=where, dist=d)


def expected_keys_per_bucket(lo, hi, nbuckets, k):
    """How full every bucket of a table of these keys is, whoever came first. The builders place every key that can have it in its home slot (k <= 32),
    then the others in any free slot of their bucket, else of the next one: linear probing over buckets of four (k > 32: two) places. Which key lies
    where depends on the order of insertion; how many keys move on from a bucket to the next does not."""
    cap = slots_per_bucket(k)
    b, j = bucket_of(lo, hi, nbuckets, k)
    occ = np.zeros(nbuckets, np.int64)
    if k <= 32:
        np.add.at(occ, np.unique(b * 4 + j) >> 2, 1)          # pass 1: one key per home slot that any key has
    rest = (np.bincount(b, minlength=nbuckets) - occ).tolist()
    occ = occ.tolist()
    carry, lap = 0, 0
    while lap == 0 or carry:
        assert lap < 3, "more keys than places"
        for i in range(nbuckets):
            incoming = carry + (rest[i] if lap == 0 else 0)
            if incoming:
                placed = min(cap - occ[i], incoming)
                occ[i] += placed
                carry = incoming - placed
            if lap and not carry:
                break
        lap += 1
    return np.array(occ, np.int64)


def summary(a):
    """the counts of an audit, without its arrays (what a child process prints)"""
    p = a["placements"]
    return dict(keys=int(len(a["lo"])), home=p["home"], named=p["named"], on={str(d): n for d, n in p["on"].items()}, wrapped=a["wrapped"],
                max_keys_per_bucket=int(a["keys_per_bucket"].max()) if len(a["keys_per_bucket"]) else 0)


def shares(a):
    """home / named / further-bucket shares of an audit's keys (device_layout.hpp quotes 88 % home at load 0.25 and 78 % at 0.5)"""
    p, n = a["placements"], max(1, len(a["lo"]))
    return p["home"] / n, sum(p["named"]) / n, sum(p["on"].values()) / n


def index_kmers(arrays):
    """every k-mer of a host index's graph, node by node, from node_seq / node_start / node_len -> (lo, hi)"""
    k = int(arrays["k"])
    w = np.concatenate([np.asarray(arrays["node_seq"], _U64), np.zeros(2, _U64)])
    start, length = np.asarray(arrays["node_start"], np.int64), np.asarray(arrays["node_len"], np.int64)
    count = np.maximum(length - k + 1, 0)
    node = np.repeat(np.arange(len(length)), count)
    pos = start[node] + (np.arange(int(count.sum())) - np.repeat(np.cumsum(count) - count, count))

    def window(p, bases):   # `bases` <= 32 bases from position p
        i, s = p >> 5, ((p & 31) * 2).astype(_U64)
        v = (w[i] >> s) | np.where(s != 0, w[i + 1] << ((_U64(64) - s) & _U64(63)), _U64(0))
        return v if bases >= 32 else v & _U64((1 << (2 * bases)) - 1)

    if k <= 32:
        return window(pos, k), np.zeros(len(pos), _U64)
    return window(pos, 32), window(pos + 32, k - 32)
