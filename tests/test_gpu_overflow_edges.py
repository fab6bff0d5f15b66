"""The overflow table of novel classes (csrc/collective.hip: pa_overflow_insert_kernel, pa_overflow_export_kernel, export_locked) at its probe
and capacity edges, driven through tests/overflow/overflow_probe.hip exactly as a map launch drives it: a list of {arena offset, length}, a
counter, pa::overflow_after_map on one stream. The lists are DESIGNED with tests/overflow_model.py (start slots, chains, wraps through slot
0, lists that share their whole 64-bit key) and the dump proves that a case reached the slots it was designed for. Every comparison is
exact, against the model's Counter serialised by the model. A HIP error ends the session: nothing more is started on a GPU that may have
faulted.

What the table's own text settles and these tests rely on: a list of another KEY is never compared, so only lists that share all 64 bits of
their hash reach the content comparison (om.colliding_lists makes them); an entry is claimed by one CAS and published behind a ready flag, so
one content has one entry however many lanes bring it at once, and the pool holds every distinct list exactly once."""
import ctypes as C
import threading
from collections import Counter

import numpy as np
import pytest

import helpers
import overflow_model as om

pytestmark = pytest.mark.gpu
pa = helpers.pa
ARENA_FULL, ERR_HIP = pa._ffi.PA_ERR_ARENA_FULL, -5   # PA_ERR_HIP of include/pseudoaligner_amd.h
LAUNCH = 1 << 18   # lanes of one insert launch (1024 blocks of 256): that many entries are handled one per lane


@pytest.fixture(scope="module")
def L():
    if pa.lib().pa_device_count() < 1:
        raise RuntimeError("the gpu tier needs a GPU")
    return helpers.overflow_lib()


def ok(rc, what):
    """a pa_status of the probe: a HIP error ends the session, any other failure is a PaError with the library's message"""
    if rc == ERR_HIP:
        pytest.exit("overflow table, %s: %s" % (what, (pa.lib().pa_last_error() or b"").decode("utf-8", "replace")), returncode=3)
    pa._ffi.check(rc)


def pack(lists, share=True):
    """id tuples (repeats allowed) -> (arena u32[], entries u32[n, 2] = {offset, length}); share: a content lies in the arena once and all its
    entries point there, else every entry has ids of its own"""
    at, words, entries = {}, [], []
    for ids in lists:
        if not share or ids not in at:
            at[ids] = len(words)
            words += ids
        entries.append((at[ids], len(ids)))
    return np.array(words, np.uint32), np.array(entries, np.uint32).reshape(-1, 2)


class Table:
    def __init__(self, L, max_classes, max_ids):
        self.L, self._h = L, C.c_void_p()
        ok(L.pa_overflow_create(0, max_classes, max_ids, C.byref(self._h)), "create")

    def insert_entries(self, arena, entries, ctr=None, novel_cap=None, stream=None, checked=True):
        arena, entries = np.ascontiguousarray(arena, np.uint32), np.ascontiguousarray(entries, np.uint32)
        n = len(entries)
        rc = self.L.ovp_insert(self._h, arena.ctypes.data, len(arena), entries.ctypes.data, n, n if ctr is None else ctr, n if novel_cap is None else novel_cap, stream)
        if checked:
            ok(rc, "insert")
        return rc

    def insert(self, lists, share=True, **kw):
        return self.insert_entries(*pack(lists, share), **kw)

    def _words(self, rc, w, n):
        ok(rc, "export")
        return np.ctypeslib.as_array(C.cast(w, C.POINTER(C.c_uint32)), (n.value,)).copy()

    def fetch(self, stream=None):
        w, n = C.c_void_p(), C.c_uint64()
        return self._words(self.L.pa_overflow_fetch(self._h, stream, C.byref(w), C.byref(n)), w, n)

    def allgather(self, comm, stream=None):
        w, n = C.c_void_p(), C.c_uint64()
        return self._words(self.L.pa_overflow_allgather(self._h, comm, stream, C.byref(w), C.byref(n)), w, n)

    def reset(self):
        ok(self.L.pa_overflow_reset(self._h, None), "reset")

    def dump(self):
        cap, pool_cap = C.c_uint64(), C.c_uint64()
        ok(self.L.ovp_dump(self._h, C.byref(cap), C.byref(pool_cap), None, None, None), "dump")
        keys, meta, ctl = np.zeros(cap.value, np.uint64), np.zeros((cap.value, om.META_WORDS), np.uint32), np.zeros(4, np.uint64)
        ok(self.L.ovp_dump(self._h, None, None, keys.ctypes.data, meta.ctypes.data, ctl.ctypes.data), "dump")
        return dict(cap=cap.value, pool_cap=pool_cap.value, keys=keys, meta=meta, pool_top=int(ctl[0]), status=int(ctl[1]), entries=int(ctl[3]))

    def poke_count(self, slot, count):
        ok(self.L.ovp_poke_count(self._h, slot, count), "poke")

    def or_status(self, value):
        ok(self.L.ovp_or_status(self._h, value, None), "status")

    def must_be(self, want):
        """fetch == the model's serialisation of `want`, word for word"""
        got = self.fetch()
        if not np.array_equal(got, om.serialise(want)):
            have = om.parse(got)
            diff = {k: (have.get(k), want.get(k)) for k in set(have) | set(want) if have.get(k) != want.get(k)}
            raise AssertionError("%d records differ (got, want): %r" % (len(diff), sorted(diff.items())[:4]))

    def must_be_full(self, how="fetch", comm=None):
        with pytest.raises(pa.PaError) as e:
            self.fetch() if how == "fetch" else self.allgather(comm)
        assert e.value.code == ARENA_FULL, e.value
        return e.value

    def __del__(self):
        if self._h:
            self.L.pa_overflow_destroy(self._h)
            self._h = C.c_void_p()


def slots_of_keys(d):
    """{key: [slots]} of a dump"""
    out = {}
    for s in np.flatnonzero(d["keys"]):
        out.setdefault(int(d["keys"][s]), []).append(int(s))
    return out


def check_entries(d, want):
    """the dump holds exactly one published entry per list of `want`, with its length and its count, and a pool that holds each list once"""
    where = slots_of_keys(d)
    by_key = {}
    for ids in want:
        by_key.setdefault(om.key_of(ids), []).append(ids)
    assert sorted(where) == sorted(by_key) and d["entries"] == len(want) == sum(len(v) for v in where.values())
    assert d["pool_top"] == sum(len(ids) for ids in want) and d["status"] == 0
    for key, slots in where.items():
        assert len(slots) == len(by_key[key])
        got = sorted((int(d["meta"][s][1]), int(d["meta"][s][2]) | int(d["meta"][s][3]) << 32) for s in slots)
        assert got == sorted((len(ids), want[ids]) for ids in by_key[key]), (key, got)
        assert all(d["meta"][s][4] == 1 and d["meta"][s][0] + d["meta"][s][1] <= d["pool_top"] for s in slots)


# ---- the designed lists (all of them go through test_model_hash_is_the_device_hash) ----
CHAIN_STARTS = (517, 1023, 1021)                     # a chain in the middle of 1024 slots; two that wrap through slot 0
CHAINS = {s: om.lists_for_slot(s, 41) for s in CHAIN_STARTS}
NEAR_SLOT = 1022
NEAR_FIRST, NEAR_LAST = om.near_lists_for_slot(NEAR_SLOT)
NEAR_LONGER = om.longer_list_for_slot(NEAR_FIRST[0], NEAR_SLOT)
COLLIDE = [om.colliding_lists(), om.colliding_lists(tail=(77, 1000)), om.colliding_lists(prefix=(5, 9)), om.colliding_lists(prefix=(3,), tail=(0xFFFFFFFE,))]
BIG = tuple(range(11, 3 * 5000 + 11, 3))             # 5000 ids
EDGE_LISTS = [(0,), (0xFFFFFFFE,), (0, 0xFFFFFFFE), tuple(range(64)), tuple(range(1, 66)), (0,) + tuple(range(7, 70)) + (0xFFFFFFFE,), BIG]
CONTENDED = om.lists_for_slot(100, 32) + [tuple(range(1000 * j, 1000 * j + 1 + j % 9)) for j in range(1, 33)]   # 32 of one chain, 32 of 1 .. 9 ids


def distinct_lists(n):
    """n lists of 2 .. 6 ids over disjoint id ranges (so that a list cut short is still none of the others)"""
    return [tuple(range(8 * i, 8 * i + 2 + i % 5)) for i in range(n)]


def test_model_hash_is_the_device_hash(L):
    lists = [l for s in CHAIN_STARTS for l in CHAINS[s]] + list(NEAR_FIRST) + list(NEAR_LAST) + [NEAR_LONGER] + [l for p in COLLIDE for l in p]
    lists += EDGE_LISTS + CONTENDED + distinct_lists(2049) + [l[:-1] for l in distinct_lists(1025)] + [(i,) for i in range(1, 8)] + [(9, 9), (2, 1)]
    assert {len(l) for l in lists} >= {1, 2, 64, 65, 5000} and any(0 in l for l in lists) and any(0xFFFFFFFE in l for l in lists)
    arena, entries = pack(lists)
    out = np.zeros(len(lists), np.uint64)
    ok(L.ovp_hash(arena.ctypes.data, len(arena), entries.ctypes.data, len(entries), out.ctypes.data, None), "hash")
    bad = [(l[:4], hex(int(h)), hex(om.list_hash(l))) for l, h in zip(lists, out) if int(h) != om.list_hash(l)]
    assert not bad, "%d of %d lists hash differently on the device; first: %r" % (len(bad), len(lists), bad[0])
    for x, y in COLLIDE:   # what the collision design rests on, said by the device itself
        assert x != y and out[lists.index(x)] == out[lists.index(y)]


@pytest.mark.parametrize("start", CHAIN_STARTS)
def test_probe_chain(L, start):
    lists = CHAINS[start]
    rng = np.random.RandomState(start)
    want = Counter(dict(zip(lists[:40], (int(m) for m in rng.permutation(40) + 1))))
    batch = [l for l, m in want.items() for _ in range(m)]
    t = Table(L, 512, 2 * 41)
    t.insert([batch[i] for i in rng.permutation(len(batch))])
    d = t.dump()
    assert d["cap"] == 1024
    run = [(start + j) % 1024 for j in range(40)]
    assert sorted(np.flatnonzero(d["keys"])) == sorted(run), "the 40 lists of start slot %d do not sit in the 40 slots from it on" % start
    assert {int(k) for k in d["keys"][run]} == {om.key_of(l) for l in lists[:40]}
    check_entries(d, want)
    t.must_be(want)
    # every list again and a 41st of the same start slot, which walks the whole chain
    second = lists[:40] + [lists[40]] * 3
    t.insert([second[i] for i in rng.permutation(len(second))])
    want.update(second)
    d = t.dump()
    assert int(d["keys"][(start + 40) % 1024]) == om.key_of(lists[40]) and len(np.flatnonzero(d["keys"])) == 41
    check_entries(d, want)
    t.must_be(want)


def test_near_equal_lists_of_one_start_slot(L):
    want = Counter()
    for n, ids in enumerate([NEAR_FIRST[0], NEAR_FIRST[1], NEAR_LAST[0], NEAR_LAST[1], NEAR_LONGER]):   # same last id / same first id / a list and its extension
        want[ids] += 3 + 2 * n
    assert len(want) >= 4 and {om.slot_of(l) for l in want} == {NEAR_SLOT}
    batch = [l for l, m in want.items() for _ in range(m)]
    t = Table(L, 512, 64)
    t.insert(batch[::-1])
    d = t.dump()
    assert sorted(np.flatnonzero(d["keys"])) == sorted((NEAR_SLOT + j) % 1024 for j in range(len(want)))   # 1022, 1023, 0, 1 ...
    check_entries(d, want)
    t.must_be(want)


@pytest.mark.parametrize("k", range(len(COLLIDE)))
def test_lists_of_one_key_are_told_apart_by_content(L, k):
    """two lists whose 64-bit hashes are EQUAL: same key, same start slot — only the comparison of the ids keeps them apart"""
    x, y = COLLIDE[k]
    assert om.key_of(x) == om.key_of(y) and x != y
    want = Counter({x: 5, y: 11})
    rng = np.random.RandomState(k)
    batch = [x] * 5 + [y] * 11
    t = Table(L, 512, 64)
    t.insert([batch[i] for i in rng.permutation(16)])
    d = t.dump()
    s = om.slot_of(x)
    assert slots_of_keys(d) == {om.key_of(x): [s, (s + 1) % 1024] if s != 1023 else [0, 1023]}
    check_entries(d, want)
    t.must_be(want)
    t.insert([y, x, y] + [x] * 4096 + [y] * 4096)                      # and with many lanes at both entries
    want.update({x: 4097, y: 4098})
    check_entries(t.dump(), want)
    t.must_be(want)


def test_one_content_at_two_arena_offsets_is_one_record(L):
    x, y = CHAINS[517][0], EDGE_LISTS[4]
    t = Table(L, 512, 128)
    arena, entries = pack([x, y, x, y, y], share=False)
    assert len(set(map(tuple, entries))) == 5 and len(arena) == 2 * 2 + 3 * 65
    t.insert_entries(arena, entries)
    want = Counter({x: 2, y: 3})
    check_entries(t.dump(), want)
    t.must_be(want)


def test_a_launch_of_one_list(L):
    for ids in (CHAINS[1023][0], EDGE_LISTS[3]):                        # 2 ids; 64 ids
        t = Table(L, 1, len(ids))
        t.insert_entries(np.array(ids, np.uint32), np.tile(np.array([0, len(ids)], np.uint32), (LAUNCH, 1)))
        want = Counter({ids: LAUNCH})
        d = t.dump()
        assert len(np.flatnonzero(d["keys"])) == 1 and d["entries"] == 1
        check_entries(d, want)
        t.must_be(want)


@pytest.mark.parametrize("first", ["mixed", "uniform"])
def test_64_lists_by_4096_in_two_orders(L, first):
    """mixed: the 64 lanes of a wave hold 64 different lists; uniform: 64 copies of one list (64 lanes create the same new class at once)"""
    assert len(set(CONTENDED)) == 64
    arena, one = pack(CONTENDED)
    i = np.arange(LAUNCH)
    order = {"mixed": i % 64, "uniform": (i // 64) % 64}
    t = Table(L, 64, len(arena))
    want = Counter()
    for n, how in enumerate([first] + ["mixed", "uniform"]):             # into the empty table, then both orders into the filled one
        t.insert_entries(arena, one[order[how]])
        want.update({l: 4096 for l in CONTENDED})
        d = t.dump()
        assert d["entries"] == 64 and d["pool_top"] == len(arena), (n, how, d["entries"], d["pool_top"])
        check_entries(d, want)
        t.must_be(want)


@pytest.mark.parametrize("max_classes", [1, 512, 513, 1024])
def test_exact_capacity(L, max_classes):
    lists = distinct_lists(max_classes)
    max_ids = sum(len(l) for l in lists)
    rng = np.random.RandomState(max_classes)
    twice = [lists[i % max_classes] for i in rng.permutation(2 * max_classes)]
    want = Counter(twice)
    t = Table(L, max_classes, max_ids)                                   # exactly what was asked for: fits
    t.insert(twice)
    d = t.dump()
    cap = d["cap"]
    assert cap == om.table_cap(max_classes) and d["pool_cap"] == max_ids == d["pool_top"]
    check_entries(d, want)
    t.must_be(want)

    t = Table(L, max_classes, max_ids - 1)                               # one id short: reported, by fetch and again by the next fetch
    t.insert(twice)
    assert t.dump()["status"] == om.STATUS_POOL_FULL
    t.must_be_full()
    t.must_be_full()
    t.reset()                                                            # ... and after a reset the same table takes what fits, exactly
    smaller = [l if l != lists[-1] else l[:-1] for l in twice]
    t.insert(smaller)
    d = t.dump()
    assert d["pool_top"] == max_ids - 1 == d["pool_cap"]
    check_entries(d, Counter(smaller))
    t.must_be(Counter(smaller))

    roomy = 6 * (cap + 1)
    t = Table(L, max_classes, roomy)                                     # more distinct lists than the table has slots: reported
    t.insert(distinct_lists(cap + 1))
    d = t.dump()
    assert d["status"] == om.STATUS_TABLE_FULL and d["entries"] == cap and not (d["keys"] == 0).any()
    t.must_be_full()
    for n in sorted({(max_classes + cap) // 2, cap - 1, cap}):           # between max_classes and cap the header promises nothing:
        t.reset()                                                        # an exact table or the error, never a wrong table
        some = distinct_lists(n) + distinct_lists(n)[::3]
        t.insert(some)
        try:
            got = t.fetch()
        except pa.PaError as e:
            assert e.code == ARENA_FULL, e
        else:
            assert np.array_equal(got, om.serialise(Counter(some))), n


def test_count_beyond_32_bits(L):
    x, y = CHAINS[517][3], CHAINS[517][4]                                # neighbours in one chain: y's count must not move
    t = Table(L, 512, 16)
    t.insert([x, y])
    where = slots_of_keys(t.dump())
    t.poke_count(where[om.key_of(x)][0], (1 << 32) - 1)
    t.must_be(Counter({x: (1 << 32) - 1, y: 1}))
    t.insert([x, x, x])
    got = t.fetch()
    first, second = sorted([x, y])
    assert first == x and list(got[2:5]) == [2, 2, 1], got[:8]           # {len, count low, count high}: 2^32 - 1 + 3
    t.must_be(Counter({x: (1 << 32) + 2, y: 1}))
    t.poke_count(where[om.key_of(x)][0], (1 << 33) - 1000)               # the carry under contention: a launch of one list across it
    t.insert_entries(np.array(x, np.uint32), np.tile(np.array([0, 2], np.uint32), (LAUNCH, 1)))
    t.must_be(Counter({x: (1 << 33) - 1000 + LAUNCH, y: 1}))


def test_export(L):
    t = Table(L, 16, 6000)
    assert list(t.fetch()) == [0, 2] and list(t.fetch()) == [0, 2]       # an empty table, twice
    assert list(t.allgather(None)) == [0, 2]
    small, big = EDGE_LISTS[1], BIG
    first = [small] * 3 + [big] * 2 + [EDGE_LISTS[2]]
    t.insert(first)
    a, b = t.fetch(), t.fetch()
    assert np.array_equal(a, b) and np.array_equal(a, om.serialise(Counter(first)))   # 1 id and 5000 ids in one table; a fetch changes nothing
    assert np.array_equal(t.allgather(None), a)
    second = [big, EDGE_LISTS[0], small, EDGE_LISTS[5]]
    t.insert(second)
    t.must_be(Counter(first) + Counter(second))                          # fetch, insert, fetch: the sum
    check_entries(t.dump(), Counter(first) + Counter(second))


def test_the_list_is_read_up_to_its_bound(L):
    """the counter of a launch may run past the list (the map kernel counts what it could not list): min(*n_ptr, novel_cap) entries are filed"""
    inside = CHAINS[1021][:30] + distinct_lists(70)
    beyond = [(i,) for i in range(1, 8)]                                 # valid lists, in the arena, found nowhere else
    arena, entries = pack(inside + beyond)
    t = Table(L, 512, len(arena))
    t.insert_entries(arena, entries, ctr=len(inside) + 7, novel_cap=len(inside))
    want = Counter(inside)
    check_entries(t.dump(), want)
    t.must_be(want)
    t.insert_entries(arena, entries, ctr=0, novel_cap=len(inside))       # nothing listed: nothing filed
    t.must_be(want)
    t.insert_entries(arena, entries, ctr=10, novel_cap=len(inside))      # a counter below the bound
    want.update(inside[:10])
    t.must_be(want)
    t.insert_entries(arena, entries, ctr=1 << 40, novel_cap=1)           # a counter far beyond it
    want.update(inside[:1])
    check_entries(t.dump(), want)
    t.must_be(want)


def one_rank_comm(L):
    uid = (C.c_uint8 * 128)()
    ok(L.pa_comm_unique_id(uid), "unique id")
    comm = C.c_void_p()
    ok(L.pa_comm_create(0, 1, 0, uid, C.byref(comm)), "communicator")
    return comm


def test_status_bits_and_the_gather(L):
    comm = one_rank_comm(L)
    try:
        lists = CHAINS[517][:5]
        t = Table(L, 512, 10)
        t.insert(lists)
        assert np.array_equal(t.allgather(comm), om.serialise(Counter(lists)))   # a healthy table: the gather of one rank is the fetch
        t.or_status(om.STATUS_LIST_FULL)                                 # as resolve.hip reports a novel list that was too short
        assert t.dump()["status"] == om.STATUS_LIST_FULL
        for how, c in (("fetch", None), ("gather", None), ("gather", comm), ("fetch", None)):
            t.must_be_full(how, c)
        t.reset()
        assert t.dump()["status"] == 0 and list(t.fetch()) == [0, 2]
        t.insert(lists)
        t.must_be(Counter(lists))

        t = Table(L, 512, 9)                                             # a pool one id short: one error code from all three exports
        t.insert(lists)
        assert t.dump()["status"] == om.STATUS_POOL_FULL
        codes = [t.must_be_full(how, c).code for how, c in (("fetch", None), ("gather", None), ("gather", comm))]
        assert codes == [ARENA_FULL] * 3
    finally:
        L.pa_comm_destroy(comm)


def test_two_streams_into_one_table(L):
    chain = CHAINS[1023]
    batches = [chain[:30] * 200 + CONTENDED * 100, chain[10:41] * 300 + CONTENDED[20:] * 50 + [BIG]]   # overlapping: 20 chain lists and 44 others in both
    t = Table(L, 512, 2 * 41 + sum(len(l) for l in CONTENDED) + len(BIG))
    streams, rcs = [C.c_void_p(), C.c_void_p()], [[], []]
    for s in streams:
        ok(L.ovp_stream_new(C.byref(s)), "stream")
    packed = [pack(b) for b in batches]
    rounds = 6

    def work(k):
        for _ in range(rounds):
            rcs[k].append(t.insert_entries(*packed[k], stream=streams[k], checked=False))

    threads = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    for k in range(2):
        assert len(rcs[k]) == rounds
        for rc in rcs[k]:
            ok(rc, "insert on stream %d" % k)
    for s in streams:
        ok(L.ovp_stream_free(s), "stream")
    want = Counter()
    for b in batches:
        for l, m in Counter(b).items():
            want[l] += rounds * m
    check_entries(t.dump(), want)
    t.must_be(want)
