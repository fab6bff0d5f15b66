"""CPU tier: the model of the cell calling (tests/knee_model.py) against the answers written out in tests/knee_cases.py and against a brute-force
count, and the constants both restate against the source lines they come from."""
import re

import numpy as np
import pytest

import helpers
import knee_cases as kc
import knee_model as km

CSRC = helpers.ROOT / "rust-pseudoaligner_amd" / "csrc"


@pytest.mark.parametrize("name", sorted(kc.HAND))
def test_hand_cases(name):
    umis, given, want = kc.HAND[name]
    rec = kc.from_umis(umis)
    rows, called, st = km.knee(rec, **given)
    assert st["threshold"] == want["t"] and st["values_above_lower"] == want["L"] and st["barcodes_called"] == want["called"] == len(called)
    assert [r[3] for r in rows] == umis and st["barcodes"] == len(umis) and st["molecules"] == sum(umis) == st["records"] == st["reads"]
    assert called == [r[0] for r in rows if r[3] >= want["t"]] == sorted(called)
    if want["knee"] is not None:
        v, R = km.curve(km.table(rec))
        assert v[km.knee_index(v, R, want["L"])] == want["knee"] and kc.clear_knee(v, R, given["lower"])


def test_the_shoulder_scores_as_written():
    v, R = km.curve(km.table(kc.from_umis(kc.SHOULDER)))
    assert v == [100, 99, 98, 97, 96, 3, 2, 1] and R == [1, 2, 3, 4, 5, 15, 25, 45]
    s = sorted(km.scores(v, R, 8), reverse=True)
    assert (round(s[0], 4), round(s[1], 4)) == kc.SHOULDER_SCORES and km.scores(v, R, 8)[4] == s[0]


def test_expected_rank_is_lowered_to_the_last_row():
    p = km.params(mode="expected", expected_cells=3000)
    v, R = list(range(120, 0, -10)), list(range(1, 13))
    assert km.threshold(p, v, R) == (1, 0) and km.threshold(km.params(mode="expected", expected_cells=99), v, R) == (12, 0)
    assert km.threshold(p, [], []) == (1, 0) and km.threshold(km.params(lower=7), [], []) == (7, 0) and km.threshold(km.params(mode="min", min_umis=4), [], []) == (4, 0)


def test_curve_without_a_shoulder_takes_the_last_point():
    v, R = [1000, 10, 1], [1, 1000, 100000]       # a hollow curve: the middle point lies below the chord
    assert km.scores(v, R, 3)[1] < 0 and km.knee_index(v, R, 3) == 2 and kc.clear_knee(v, R, 1)
    assert km.threshold(km.params(lower=1, divisor=1), v, R) == (1, 3)


def test_stats_identities_and_table_against_brute_force():
    rng = np.random.default_rng(5)
    keys = sorted({(int(b), int(u), int(e)) for b, u, e in zip(rng.integers(0, 300, 20000), rng.integers(0, 40, 20000), rng.integers(0, 6, 20000))})
    rec = [(b, u, e, int(c)) for (b, u, e), c in zip(keys, rng.integers(1, 9, len(keys)))]
    rows, called, st = km.knee(rec, mode="min", min_umis=33)
    mols, reads, nrec = {}, {}, {}
    for b, u, e, c in rec:
        mols.setdefault(b, set()).add(u)
        reads[b] = reads.get(b, 0) + c
        nrec[b] = nrec.get(b, 0) + 1
    assert [(r[0], r[1], r[2], r[3]) for r in rows] == [(b, reads[b], nrec[b], len(mols[b])) for b in sorted(mols)]
    assert st["records"] == len(rec) and st["reads"] == sum(reads.values()) and st["molecules"] == sum(len(s) for s in mols.values()) and st["barcodes"] == len(mols)
    assert st["distinct_values"] == len({len(s) for s in mols.values()}) and st["threshold"] == 33
    assert called == [b for b in sorted(mols) if len(mols[b]) >= 33] and 0 < len(called) < len(mols)
    assert st["molecules_called"] == sum(len(mols[b]) for b in called) and st["reads_called"] == sum(reads[b] for b in called)
    assert sorted(r[4] for r in rows) == list(range(len(rows)))
    out, ks = km.keep(rec, called + [100000])
    assert out == [r for r in rec if r[0] in set(called)] and ks["listed_absent"] == 1 and ks["barcodes_kept"] == len(called) and ks["records_in"] == len(rec)
    assert ks["reads_out"] == st["reads_called"] and ks["records_out"] == len(out)


def test_rank_ties_are_ordered_by_barcode():
    rows, _, _ = km.knee(kc.from_umis([2, 5, 2, 5, 1, 2]), mode="min")
    assert [r[4] for r in rows] == [2, 0, 3, 1, 5, 4]


def test_list_check_and_tsv_text():
    assert km.check_list([], 4) is None and km.check_list([0, 5, 255], 4) is None
    assert km.check_list([0, 5, 256], 4) == 2 and km.check_list([3, 3], 4) == 1 and km.check_list([4, 9, 8, 7], 4) == 2
    rows, _, _ = km.knee([(0, 1, 0, 2), (0, 1, 1, 3), (27, 0, 0, 1)], mode="min")
    assert km.ranks_tsv(rows, 3) == "barcode\trecords\tumis\treads\trank\tcalled\nAAA\t2\t1\t5\t0\t1\nCGT\t1\t1\t1\t1\t1\n"


def test_constants_are_the_sources():
    hip = (CSRC / "bus_knee.hip").read_text()
    const = lambda name: int(re.search(r"constexpr uint32_t %s = (\d+);" % name, hip).group(1))
    assert (const("KNEE_BLOCK"), const("KNEE_ITEMS"), const("KNEE_MAX_GRID")) == (kc.BLOCK, kc.ITEMS, kc.MAX_GRID)
    assert "constexpr uint32_t KNEE_TILE = KNEE_BLOCK * KNEE_ITEMS;" in hip and kc.TILE == kc.BLOCK * kc.ITEMS
    host = (CSRC / "bus_knee_host.cpp").read_text()
    d = km.DEFAULTS
    for line in ("p->mode = PA_KNEE_CURVE;", "p->lower = %d;" % d["lower"], "p->divisor = %d;" % d["divisor"], "p->expected_cells = %d;" % d["expected_cells"],
                 "p->min_umis = %d;" % d["min_umis"]):
        assert line in host, line
    hpp = (CSRC / "bus_knee_host.hpp").read_text()
    assert "EXPECTED_PERCENTILE = 100;" in hpp and "EXPECTED_DIVISOR = 10;" in hpp
    header = (helpers.ROOT / "include" / "pseudoaligner_amd.h").read_text()
    for name, value in (("PA_KNEE_CURVE", km.CURVE), ("PA_KNEE_EXPECTED", km.EXPECTED), ("PA_KNEE_MIN", km.MIN), ("PA_KNEE_STATS", len(km.STAT_NAMES)),
                        ("PA_BUS_KEEP_STATS", len(km.KEEP_STAT_NAMES))):
        assert "#define %s %d\n" % (name, value) in header
    assert '"%s"' % km.TSV_HEADER.replace("\t", "\\t").replace("\n", "\\n") in host
    assert kc.ROW_DTYPE.itemsize == 32 and kc.ROW_DTYPE.names == ("barcode", "reads", "records", "umis", "rank", "called")
