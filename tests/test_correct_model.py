"""CPU tier: the model of the BUS barcode correction (tests/correct_model.py) on the hand cases with their answers written out, its barcode
decision against the cell counter's model on random barcodes, and the constants tests/correct_cases.py restates against the source lines of
csrc/bus_correct.hip and csrc/bus_correct_host.cpp."""
import re

import numpy as np
import pytest

import cells_model
import correct_cases as cc
import correct_model as cm
import helpers

CSRC = helpers.ROOT / "rust-pseudoaligner_amd" / "csrc"


@pytest.mark.parametrize("name", sorted(cc.HAND))
def test_hand_cases_with_written_answers(name):
    rec, wl, bc_len, umi_len, want, kinds = cc.HAND[name]
    assert rec == sorted(rec) and len({r[:3] for r in rec}) == len(rec)            # a valid input
    out, st, decided = cm.correct(rec, wl, bc_len, umi_len)
    assert out == want
    assert {b: k for b, (k, _) in decided.items()} == kinds
    assert st["records_in"] == len(rec) and st["reads_in"] == sum(r[3] for r in rec) and st["barcodes_in"] == len(kinds)
    for kind in ("exact", "corrected", "none", "ambiguous"):
        assert st["barcodes_" + kind] == sum(k == kind for k in kinds.values())
    assert st["records_out"] == len(want) and st["barcodes_out"] == len({r[0] for r in want})
    assert st["reads_dropped"] == sum(r[3] for r in rec if kinds[r[0]] in ("none", "ambiguous"))
    assert cm.correct(rec, wl[::-1], bc_len, umi_len)[:2] == (out, st)              # the whitelist is a set


def test_clamp_and_stats_of_the_merge_case():
    rec, wl, bc_len, umi_len, want, _ = cc.HAND["merges"]
    _, st, _ = cm.correct(rec, wl, bc_len, umi_len)
    assert (st["records_exact"], st["records_corrected"], st["records_dropped"], st["records_out"]) == (2, 11, 0, 7)
    assert sum(r[3] for r in want) < st["reads_in"] - st["reads_dropped"]           # the clamp lost reads, and only the clamp
    assert [r[3] for r in want if r[1] in (2, 3)] == [0xFFFFFFFF, 0xFFFFFFFF]


def test_long_wrap_and_sized_cases_are_what_they_claim():
    for bc_len, umi_len in ((31, 1), (16, 12)):
        rec, wl, _, _ = cc.long_barcode_case(bc_len, umi_len)
        _, st, decided = cm.correct(rec, wl, bc_len, umi_len)
        assert (st["barcodes_exact"], st["barcodes_corrected"], st["barcodes_none"]) == (1, 3, 1)
        targets = {t for k, t in decided.values() if k == "corrected"}
        assert targets == set(wl[:3]) and max(wl).bit_length() <= 2 * bc_len
    first, last = cc.sub(0, 31, 0, 1), cc.sub(0, 31, 30, 2)
    assert first == 1 << 60 and last == 2                                           # shifts 60 and 0
    for sizes in ((60, 3, 0), (200, 40, 17)):
        rec, wl, bc_len, umi_len = cc.sized_case(1, *sizes)
        _, st, _ = cm.correct(rec, wl, bc_len, umi_len)
        assert st["barcodes_in"] == sum(sizes) and st["barcodes_exact"] == sizes[0] and st["barcodes_corrected"] >= sizes[1]
        assert rec == sorted(rec) and len({r[:3] for r in rec}) == len(rec)


def test_wrap_whitelist_displaces_a_key_past_the_last_slot():
    """from the restated hash: two keys are at home in the last slot, so the one that is inserted second goes on to slot 0 — which is another
    key's home, so one of the three ends in slot 1"""
    wl, cap = cc.wrap_whitelist()
    assert cap == cc.capacity(len(wl)) == 16 and len(set(wl)) == len(wl) == 5
    homes = [cc.home(w, cap) for w in wl]
    assert homes.count(cap - 1) == 2 and homes.count(0) == 1 and 1 not in homes
    for order in (wl, wl[::-1]):                                                    # linear probing in either insertion order
        table = [None] * cap
        for w in order:
            j = cc.home(w, cap)
            while table[j] is not None:
                j = (j + 1) & (cap - 1)
            table[j] = w
        assert table[cap - 1] in wl[:2] and table[0] is not None and table[1] is not None
        assert any(cc.home(table[j], cap) == cap - 1 for j in (0, 1))               # a key at home in the last slot sits beyond the wrap
    rec, wl2, bc_len, umi_len = cc.wrap_case()
    _, st, _ = cm.correct(rec, wl2, bc_len, umi_len)
    assert st["barcodes_exact"] == 5 and st["barcodes_corrected"] >= 5 and st["barcodes_none"] + st["barcodes_ambiguous"] >= 1   # (the keys are small: some neighbours are shared)


def test_barcode_decision_equals_the_cell_counters_rule():
    """20 000 random N-free barcodes: exact / corrected with the same target / dropped, as tests/cells_model.py decides for the same whitelist"""
    rng = np.random.default_rng(5)
    bc_len = 8
    wl = sorted({int(x) for x in rng.integers(0, 4 ** bc_len, 6000)})
    wl_set = {w: True for w in wl}
    wl_line = {cm.unpack(w, bc_len): i for i, w in enumerate(wl)}
    seen = {"exact": 0, "corrected": 0, "none": 0, "ambiguous": 0}
    for b in rng.integers(0, 4 ** bc_len, 20000):
        kind, target = cm.decide(int(b), wl_set, bc_len)
        cell, how = cells_model.correct_barcode(cm.unpack(int(b), bc_len), wl_line)
        seen[kind] += 1
        if kind in ("exact", "corrected"):
            assert how == kind and wl[cell] == target
        else:
            assert cell is None and how == "invalid"
    assert min(seen.values()) > 200, seen


def test_restated_constants_are_the_sources():
    hip = (CSRC / "bus_correct.hip").read_text()
    host = (CSRC / "bus_correct_host.cpp").read_text()
    body = (CSRC / "lane_steps_body.hpp").read_text()
    const = lambda name: int(re.search(r"constexpr uint32_t %s = (\d+);" % name, hip).group(1))
    assert const("CORRECT_GROUP") == cc.GROUP and const("CORRECT_BLOCK") == cc.BLOCK and const("CORRECT_MAX_ROUNDS") == cc.MAX_ROUNDS
    assert cc.GROUP * cc.MAX_ROUNDS >= 3 * 31 and 64 % cc.GROUP == 0
    assert "constexpr ull WL_EMPTY = ~0ull;" in hip
    # probing starts at pa_mix64(barcode) & (cap - 1), in the build and in both lookups
    assert hip.count("pa_mix64(k) & mask") == 1 and hip.count("pa_mix64(key) & mask") == 1 and hip.count("pa_mix64(cand[r]) & mask") == 1
    m = re.search(r"PA_HD uint64_t pa_mix64\(uint64_t x\) \{.*?\n\}", body, re.S).group(0)
    assert "0xff51afd7ed558ccd" in m and "0xc4ceb9fe1a85ec53" in m and m.count("x >> 33") == 3
    assert cc.mix64(0) == 0 and cc.mix64(1) == 0xb456bcfc34c2cb2c                   # murmur3 fmix64 of 1
    # the capacity rule
    rule = re.search(r"uint64_t table_capacity\(uint64_t n_whitelist\) \{(.*?)\n\}", host, re.S).group(1)
    assert "uint64_t cap = 2;" in rule and "while (cap < 2 * n_whitelist) cap <<= 1;" in rule
    assert [cc.capacity(n) for n in (1, 2, 3, 4, 5, 1024, 1025, 6_800_000)] == [2, 4, 8, 8, 16, 2048, 4096, 1 << 24]
    # the header's stat count and the model's names
    header = (helpers.ROOT / "include" / "pseudoaligner_amd.h").read_text()
    assert "#define PA_BUS_CORRECT_STATS 13" in header and len(cm.STAT_NAMES) == 13
