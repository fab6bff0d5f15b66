"""CPU tier of the designed class sets (tests/class_cases.py): oracle == emulator == the Python set intersection on every read, and
every read takes the path its row names — window AND, masked pending classes, list mode and the tier isect_pick chooses, with the
pending count, the class count and the base length of the row. A case that stops reaching its branch fails here, without a GPU;
tests/test_gpu_class_tiers.py sends the same cases through the product."""
import collections

import numpy as np
import pytest

import class_cases
import helpers

pa = helpers.pa

_cache = {}


def built_case(name, k, tail=0):
    """(host index, case tuple), built once per session and left unchanged"""
    key = (name, k, tail)
    if key not in _cache:
        c = class_cases.case(name, k, tail)
        _cache[key] = (helpers.index_from_node_set(c[0], c[1], c[2], seed=k), c)
    return _cache[key]


def kinds(host, res, colour, expected):
    """per read: "ref" (record by reference), else by the Python sets: "class" (an index class), "novel", "empty"; None when unmapped"""
    a = host.arrays()
    off = a["ec_offset"].astype(np.int64)
    known = {tuple(a["ec_ids"][off[c]:off[c + 1]].tolist()) for c in range(a["num_classes"])}
    out = []
    for i, e in enumerate(expected):
        if not res["mismatches"][i] >> 31:
            out.append(None)
        elif res["class_off"][i] & pa.PA_CLASS_REF:
            out.append("ref")
        else:
            out.append("empty" if not e else "class" if tuple(e) in known else "novel")
    return out


def check_case(name, k, tail=0):
    host, (nodes, k, num_tx, reads, expected, target, bitmap_min) = built_case(name, k, tail)
    tiles, lens, wpr = helpers.pack_reads_tiles(reads)
    o_res, o_coff, o_ids, _ = helpers.Oracle(host).map_tiles(tiles, lens, wpr, 2, 4)
    emu = helpers.Emu(host)
    r = emu.map_tiles(tiles, lens, wpr, 2, want_path=True)
    helpers.assert_same_as_oracle(r["results"], r["coff"], r["ids"], o_res, o_coff, o_ids, "emu %s K=%d" % (name, k))
    for i, e in enumerate(expected):   # the Python sets: every read maps over its whole length without a mismatch
        assert o_res["mapped"][i] == 1 and o_res["coverage"][i] == len(reads[i]) and o_res["mismatches"][i] == 0, (name, i)
        assert o_ids[int(o_coff[i]):int(o_coff[i + 1])].tolist() == e, (name, i, target[i])
    return host, emu, r, target, expected, bitmap_min


@pytest.mark.parametrize("k", [24, 40])
@pytest.mark.parametrize("name", class_cases.CASES)
def test_paths_and_classes(built, name, k):
    host, emu, r, target, expected, bitmap_min = check_case(name, k)
    assert emu.info()["bitmap_min"] == bitmap_min
    kind = kinds(host, r["results"], r["colour"], expected)
    for i, t in enumerate(target):
        got = r["path"][i]
        assert {f: got[f] for f in ("path", "tier", "ncol", "npend", "base_len")} == {f: t[f] for f in ("path", "tier", "ncol", "npend", "base_len")}, (name, i, t, got)
        if t["kind"] is not None:
            assert kind[i] == t["kind"], (name, i, t, kind[i])
            if t["path"] != "lists" and t["kind"] in ("class", "novel"):   # window mode: the emulator asks the window table, which has to say the same
                assert (int(r["colour"][i]) != 0xFFFFFFFF) == (t["kind"] == "class"), (name, i)


def test_the_table_reaches_every_branch(built):
    """the rows the issue lists, counted: a table that lost one of them fails here"""
    seen = collections.Counter()
    for name in class_cases.CASES:
        c = class_cases.case(name, 24)
        for t in c[5]:
            seen[(name.rstrip("0123456789"), t["path"], t["tier"], t["ncol"] or t["npend"], t["base_len"], t["kind"])] += 1
    have = lambda fam, path, **kw: any(k[0] == fam and k[1] == path and all(dict(tier=k[2], n=k[3], base_len=k[4], kind=k[5])[f] == v for f, v in kw.items()) for k in seen)
    for kind in ("ref", "class", "novel", "empty"):
        assert have("seams", "window", kind=kind)
        assert have("lists", "lists", tier=0, kind=kind) and have("lists", "lists", tier=1, kind=kind) and have("lists", "lists", tier=2, kind=kind)
    for fam in ("pending", "nobitmap"):
        for n in (1, 2, 5, 40, 63, 64, 65, 130):
            assert have(fam, "masked", n=n)
        for kind in ("ref", "novel", "empty"):
            assert have(fam, "masked", kind=kind)
    for n in (1, 2, 3):
        assert have("lists", "lists", tier=0, n=n)
    for n in (2, 3, 4, 5, 40, 63, 64, 65, 130):
        assert have("lists", "lists", tier=1, n=n)
    for n in (2, 3, 5, 66, 130):
        assert have("lists", "lists", tier=2, n=n)
    for base_len in (7, 8):
        assert have("lists", "lists", tier=1, base_len=base_len)
    for base_len in (9, 64, 65, 130):
        assert have("lists", "lists", tier=2, base_len=base_len)
    assert have("vectors", "window") and have("vectors", "masked") and have("vectors", "lists")


@pytest.mark.parametrize("name,k", [("seams", 24), ("pending32783", 24), ("lists", 40)])
def test_long_tail_reads(built, name, k):
    """the same chains with a same-class tail node of 500 k-mers (the wide lane packing: reads of more than 512 bases)"""
    check_case(name, k, tail=500)


def test_generator_is_deterministic_and_window_rule():
    assert class_cases.case("lists", 24)[3] == class_cases.case("lists", 24)[3]
    assert class_cases.has_windows([5, 36]) and class_cases.has_windows([5, 37, 68]) and not class_cases.has_windows([5, 37, 69])
    assert class_cases.has_windows([5, 36, 37]) and not class_cases.has_windows([5, 40, 80]) and not class_cases.has_windows([])
