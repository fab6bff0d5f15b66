"""tests/overflow_model.py checked on the CPU: the designers hit the slots they are asked for (chains, wraps through slot 0, lists that share
their whole key), the serialiser agrees with the package's own in both directions, the sizing rule at its steps. Whether the MODEL's hash is
the device's is the first test of tests/test_gpu_overflow_edges.py; here it is pinned on values worked out by hand from its definition."""
from collections import Counter

import numpy as np
import pytest

import helpers
import overflow_model as om

pa = helpers.pa


def test_hash_by_its_definition():
    assert om.fmix64(0) == 0 and om.fmix64(1) == 0xB456BCFC34C2CB2C            # murmur3's finaliser: its published value for 1
    assert om.list_hash(()) == om.SEED
    h = om.SEED ^ 2
    for i in (7, 0xFFFFFFFE):
        h = (om.fmix64(h ^ i) + om.GOLDEN) % (1 << 64)
    assert om.list_hash((7, 0xFFFFFFFE)) == h
    assert om.list_hash((7, 8)) != om.list_hash((8, 7)) and om.list_hash((7,)) != om.list_hash((7, 0))
    a, b, hs = om.pair_lists()                                                    # the numpy form is the scalar form
    for i in (0, 1, 598, 599, len(a) // 2, len(a) - 1):
        assert int(hs[i]) == om.list_hash((int(a[i]), int(b[i])))
        assert int(om.pair_slots(1024)[i]) == om.slot_of((int(a[i]), int(b[i])), 1024)
    assert om.key_of((3, 4)) >> 63 == 1 and om.key_of((3, 4)) & ~(1 << 63) == om.list_hash((3, 4)) & ~(1 << 63)
    assert om.slot_of((3, 4), 2048) & 1023 == om.slot_of((3, 4), 1024)          # a larger table takes more bits of the same product


def test_every_start_slot_is_reachable_with_two_small_ids():
    census = np.bincount(om.pair_slots(1024), minlength=1024)
    assert len(census) == 1024 and census.min() >= 141, census.min()
    census = np.bincount(om.pair_slots(2048), minlength=2048)
    assert census.min() >= 41, census.min()                                       # a chain of 41 in a table of 2048 slots as well


@pytest.mark.parametrize("slot", [517, 1023, 1021, 0])
def test_chain_designer(slot):
    lists = om.lists_for_slot(slot, 41)
    assert len(set(lists)) == 41 and all(a < b < om.PAIR_IDS for a, b in lists)
    assert {om.slot_of(l) for l in lists} == {slot}
    assert len({om.key_of(l) for l in lists}) == 41
    got = om.chain_slots(lists)
    assert got == [(slot + j) % 1024 for j in range(41)]                          # the j-th walks j slots; from 1023 and 1021 through slot 0
    if slot in (1023, 1021):
        assert 0 in got and 1023 in got
    rng = np.random.RandomState(slot)                                             # any insertion order fills the same 41 slots
    assert sorted(om.chain_slots([lists[i] for i in rng.permutation(41)])) == sorted(got)


def test_near_equal_designers():
    for slot in (5, 1023):
        first, last = om.near_lists_for_slot(slot)
        assert first and last
        (a, b), (a2, b2) = first
        assert a == a2 and b != b2 and om.slot_of((a, b)) == om.slot_of((a2, b2)) == slot
        (a, b), (a2, b2) = last
        assert a != a2 and b == b2 and om.slot_of((a, b)) == om.slot_of((a2, b2)) == slot
        longer = om.longer_list_for_slot(first[0], slot)
        assert longer[:2] == first[0] and len(longer) == 3 and om.slot_of(longer) == slot


@pytest.mark.parametrize("prefix,tail", [((), ()), ((), (77, 1000)), ((5, 9), ()), ((3,), (0xFFFFFFFE,))])
def test_colliding_lists_share_their_whole_key(prefix, tail):
    x, y = om.colliding_lists(prefix, tail)
    p = len(prefix)
    assert x != y and len(x) == len(y) == p + 2 + len(tail) and x[:p] == y[:p] == prefix and x[p + 2:] == y[p + 2:] == tail
    assert x[p] != y[p] and x[p + 1] != y[p + 1]                                  # two positions differ: one never suffices
    assert om.list_hash(x) == om.list_hash(y)
    assert all(0 <= i < 1 << 32 for i in x + y)
    for cap in (1024, 2048, 1 << 20):
        assert om.slot_of(x, cap) == om.slot_of(y, cap)


def test_serialiser_round_trip_against_the_package():
    rng = np.random.RandomState(3)
    table = Counter()
    for n in (1, 2, 3, 64, 65, 700):
        table[tuple(int(i) for i in np.sort(rng.choice(1 << 20, n, replace=False)))] = int(rng.randint(1, 1 << 30))
    table[(0,)] = 1
    table[(0, 0xFFFFFFFE)] = (1 << 32) + 2                                        # a count beyond 32 bits: low word 2, high word 1
    table[(0xFFFFFFFE,)] = (1 << 64) - 1
    w = om.serialise(table)
    assert w.dtype == np.uint32 and w[0] == len(table) and w[1] == len(w)
    assert np.array_equal(w, pa.serialise_overflow(dict(table)))
    assert om.parse(w) == table and pa.parse_overflow(w) == dict(table)
    assert om.parse(pa.serialise_overflow(dict(table))) == table
    at = 2 + 3 + 1                                                                # records are lexicographic: (0,) then (0, 2^32 - 2)
    assert list(w[2:at]) == [1, 1, 0, 0] and list(w[at:at + 5]) == [2, 2, 1, 0, 0xFFFFFFFE]
    assert list(om.serialise(Counter())) == [0, 2] and om.parse(np.array([0, 2], np.uint32)) == Counter()
    assert list(pa.serialise_overflow({})) == [0, 2]
    for bad in ([1, 2], [0, 3], [1, 6, 2, 1, 0, 5], [2, 10, 1, 1, 0, 5, 1, 1, 0, 5]):   # short, wrong word count, a record cut off, one list twice
        with pytest.raises(AssertionError):
            om.parse(np.array(bad, np.uint32))


@pytest.mark.parametrize("max_classes,cap", [(1, 1024), (512, 1024), (513, 2048), (1024, 2048), (1025, 4096)])
def test_sizing_rule(max_classes, cap):
    assert om.table_cap(max_classes) == cap
    assert cap >= 2 * max_classes and cap & (cap - 1) == 0 and (cap == 1024 or cap < 4 * max_classes)
