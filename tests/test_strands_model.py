"""The unstranded model (tests/strands_model.py) against the header's rule and the oracle, without a GPU: the rows of the rule on hand-written
candidates, the stats, that an unstranded library is only half mapped by a stranded orientation, and that the end-to-end case of
tests/test_gpu_strands.py reaches every fate of the rule on the model's side."""
import numpy as np

import helpers
import pairs_model as pm
import strands_cases
import strands_model as sm


def test_merge_rule_rows():
    R = lambda s, r: sm.merge_rule(s, r)[0]
    assert sm.merge_rule(None, None) == (None, "neither")
    assert sm.merge_rule(([1, 5], 40, 1), None) == (([1, 5], 40, 1), "sense_only")
    assert sm.merge_rule(None, ([], 33, 0)) == (([], 33, 0), "antisense_only")
    # both mapped: class non-empty first, then coverage, then fewer mismatches
    assert R(([], 150, 0), ([7], 32, 2)) == ([7], 32, 2)                 # empty against non-empty at HIGHER coverage: the non-empty one
    assert R(([7], 32, 2), ([], 150, 0)) == ([7], 32, 2)
    assert R(([1, 2], 150, 2), ([3], 32, 0)) == ([1, 2], 150, 2)         # a weaker hit on the other strand does not dilute
    assert R(([3], 32, 0), ([1, 2], 150, 2)) == ([1, 2], 150, 2)
    assert R(([1, 2], 100, 2), ([3], 100, 1)) == ([3], 100, 1)           # the mismatch tie-break
    assert R(([1, 2], 100, 0), ([3], 100, 1)) == ([1, 2], 100, 0)
    assert R(([], 90, 1), ([], 100, 3)) == ([], 100, 3)                  # two empties: still by coverage
    # ties
    assert sm.merge_rule(([1, 5, 9], 100, 1), ([0, 5, 11], 100, 1)) == (([0, 1, 5, 9, 11], 100, 1), "tie")
    assert R(([1, 5], 100, 1), ([1, 5], 100, 1)) == ([1, 5], 100, 1)
    assert R(([1, 5], 100, 1), ([5], 100, 1)) == ([1, 5], 100, 1)
    assert sm.merge_rule(([], 64, 0), ([], 64, 0)) == (([], 64, 0), "tie")   # mapped, even when the union is empty
    s = [None, ([1, 5], 40, 1), None, ([1, 5, 9], 40, 1), ([], 32, 0), ([4], 50, 0)]
    r = [None, None, ([7], 33, 2), ([5, 10], 40, 1), ([], 32, 0), ([2], 60, 0)]
    res, coff, ids, st, fates = sm.merge(s, r)
    assert coff.tolist() == [0, 0, 2, 3, 7, 7, 8] and ids.tolist() == [1, 5, 7, 1, 5, 9, 10, 2]
    assert (res["mismatches"] >> 31).tolist() == [0, 1, 1, 1, 1, 1] and res["coverage"].tolist() == [0, 40, 33, 40, 32, 60]
    assert st == dict(items=6, both_mapped=3, sense_only=1, antisense_only=1, neither=1, ties=2, by_reference=0, in_arena=0)
    assert fates == ["neither", "sense_only", "antisense_only", "tie", "tie", "antisense_wins"]
    sm.check_stats(dict(st, in_arena=4), res)


def test_a_union_can_be_an_index_class(small_index):
    """two lists whose union is an index class: the table counts the tie in that class's slot, not as novel"""
    host = small_index(20)
    a = host.arrays()
    off = a["ec_offset"].astype(np.int64)
    c = int(np.argmax(off[1:] - off[:-1]))
    ids = a["ec_ids"][off[c]:off[c + 1]].tolist()
    assert len(ids) >= 3
    res, coff, cids, st, fates = sm.merge([(ids[::2], 80, 1)], [(ids[1:], 80, 1)])
    assert fates == ["tie"] and cids.tolist() == ids
    table, novel = sm.table_and_novel(res, coff, cids, host)
    assert table[c] == 1 and table.sum() == 1 and novel == {}


def test_unstranded_pairs_are_half_mapped_by_a_stranded_orientation(small_index):
    host = small_index(20)
    r1, r2 = strands_cases.pairs_of(host, 600, 21)
    fr = pm.model_pairs(host, r1, r2, "fr")
    rf = pm.model_pairs(host, r1, r2, "rf")
    res, coff, ids, st, fates, cs, cr = sm.model_pairs_unstranded(host, r1, r2)
    mapped = lambda r: int((r["mismatches"] >> 31).sum())
    assert 250 <= mapped(fr[0]) <= 350 and 250 <= mapped(rf[0]) <= 350 and mapped(res) == 600 - st["neither"] >= 560
    t_fr, t_un = pm.table_and_novel(fr[0], fr[1], fr[2], host)[0], sm.table_and_novel(res, coff, ids, host)[0]
    assert not np.array_equal(t_fr, t_un)
    # S is the "fr" result and R the "rf" one
    assert sm.candidates_from_results(fr[0], fr[1], fr[2]) == cs and sm.candidates_from_results(rf[0], rf[1], rf[2]) == cr
    # a stranded library shows in the stats: nothing swapped -> nearly everything is S only
    a, b, _ = pm.simulate_pairs(pm.transcripts_text(host), 300, 21, sub_rate=0.01)
    st2 = sm.model_pairs_unstranded(host, a, b)[3]
    assert st2["sense_only"] > 10 * max(1, st2["antisense_only"])


def test_the_antisense_case_reaches_every_fate(small_index):
    host = strands_cases.host_of("anti20", small_index)
    r1, r2 = strands_cases.pairs_of(host, 600, 21)
    res, coff, ids, st, fates, cs, cr = sm.model_pairs_unstranded(host, r1, r2)
    got = sm.fate_counts(fates, cs, cr, res, coff)
    for f in ("sense_only", "antisense_only", "neither", "sense_wins", "antisense_wins", "tie_union_larger", "tie_equal_lists"):
        assert got.get(f, 0) >= 5, (f, got)
    both = [(s, r, f) for s, r, f in zip(cs, cr, fates) if s is not None and r is not None]
    one_empty = [(s, r, f) for s, r, f in both if bool(s[0]) != bool(r[0])]
    assert len(one_empty) >= 5 and all(f != "tie" for _, _, f in one_empty)
    for s, r, f in one_empty:                                  # the non-empty candidate wins whatever the coverage
        assert f == ("sense_wins" if s[0] else "antisense_wins")
    assert sum(1 for s, r, f in one_empty if sm.key_of(s)[1:] == sm.key_of(r)[1:]) >= 1    # ... also where coverage and mismatches tie exactly
    assert sum(1 for s, r, f in both if not s[0] and not r[0]) >= 5
    sm.check_stats(dict(st, in_arena=int(((res["mismatches"] >> 31) & (res["class_len"] > 0)).sum())), res)
    table, novel = sm.table_and_novel(res, coff, ids, host)
    nc = host.arrays()["num_classes"]
    assert table[nc] > 0 and table[nc + 1] > 0 and table[nc + 2] == st["neither"] and sum(novel.values()) == table[nc]


def test_single_reads_reach_the_fates(small_index):
    host = strands_cases.host_of("anti20", small_index)
    r1, _ = strands_cases.pairs_of(host, 600, 21)
    res, coff, ids, st, fates = sm.model_reads(host, r1, "both")
    for f in ("sense_only", "antisense_only", "neither", "tie"):
        assert fates.count(f) >= 1, (f, {k: fates.count(k) for k in set(fates)})
    fwd, rev = sm.model_reads(host, r1, "fwd"), sm.model_reads(host, r1, "rev")
    assert set(fwd[4]) <= {"sense_only", "neither"} and set(rev[4]) <= {"antisense_only", "neither"}
    o_res, o_coff, o_ids, _ = helpers.Oracle(host).map_reads(r1, 2, 4)
    helpers.assert_same_as_oracle(fwd[0], fwd[1], fwd[2], o_res, o_coff, o_ids, "strand fwd")
