"""CPU tier: the host half of the cell calling on BUS records (csrc/bus_knee_host.cpp: the checks of the params, of the records and of a barcode
list with their messages, the three threshold rules, the barcode_ranks.tsv writer) driven by a stand-alone host program under AddressSanitizer +
UndefinedBehaviorSanitizer (tests/knee/): it must be silent and agree with tests/knee_model.py and tests/knee_cases.py."""
import importlib.util
import subprocess

import pytest

import helpers
import knee_cases as kc
import knee_model as km

PA_ERR_INVALID_ARG, PA_ERR_UNSUPPORTED = -1, -8                       # include/pseudoaligner_amd.h
VALID_RECORDS = [(1, 0, 0, 1), (1, 0, 1, 1), (1, 1, 0, 1), (2, 0, 0, 1), (7, 3, 2, 1)]


def _exe():
    spec = importlib.util.spec_from_file_location("pa_knee_build", str(helpers.ROOT / "tests" / "knee" / "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.build_check()


def _run(tmp_path, p=None, curve=((), ()), barcodes=(), records=(), rows=(), bc_len=4, umi_len=4):
    """-> {first word: line}, the bytes of the TSV"""
    p = km.params(**(p or {}))
    v, R = curve
    tokens = [bc_len, umi_len, p["mode"], p["lower"], p["divisor"], p["expected_cells"], p["min_umis"], len(v)]
    tokens += [x for pair in zip(v, R) for x in pair] + [len(barcodes)] + list(barcodes) + [len(records)] + [x for r in records for x in r]
    tokens += [len(rows)] + [x for r in rows for x in r]
    (tmp_path / "case.txt").write_text(" ".join(map(str, tokens)) + "\n")
    run = subprocess.run([str(_exe()), str(tmp_path / "case.txt"), str(tmp_path / "ranks.tsv")], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and run.stderr == "", (run.returncode, run.stdout[-3000:], run.stderr[-3000:])   # the sanitizers stay silent
    lines = run.stdout.splitlines()
    assert lines[-1] == "OK" and not any(l.startswith("MISS") for l in lines), run.stdout[-3000:]
    return {l.split()[0]: l for l in lines}, (tmp_path / "ranks.tsv").read_bytes()


def _threshold(got):
    return tuple(int(x) for x in got["threshold"].split()[1:])


@pytest.mark.parametrize("name", sorted(kc.HAND))
def test_thresholds_of_the_hand_cases(name, tmp_path):
    umis, given, want = kc.HAND[name]
    rec = kc.from_umis(umis)
    v, R = km.curve(km.table(rec))
    rows, _, st = km.knee(rec, **given)
    got, tsv = _run(tmp_path, given, (v, R), records=rec, rows=rows, bc_len=8, umi_len=6)
    assert got["params"].split()[:2] == ["params", "0"] and got["records"].split()[:2] == ["records", "0"]
    assert _threshold(got) == (want["t"], want["L"]) == (st["threshold"], st["values_above_lower"])
    assert tsv.decode() == km.ranks_tsv(rows, 8) and got["tsv"].split()[:2] == ["tsv", "0"]
    d = km.DEFAULTS
    assert got["defaults"] == "defaults 0 %d %d %d %d %d 1" % (d["mode"], d["lower"], d["divisor"], d["expected_cells"], d["min_umis"])


@pytest.mark.parametrize("L", [0, 1, 2, 3])
def test_curve_with_few_points(L, tmp_path):
    v, R = [900, 800, 20][:L] + [3, 1], [5, 6, 30][:L] + [40 + L, 90]
    assert kc.clear_knee(v, R, 10)
    for divisor in (1, 10):
        p = dict(lower=10, divisor=divisor)
        got, _ = _run(tmp_path, p, (v, R))
        assert _threshold(got) == km.threshold(km.params(**p), v, R) and _threshold(got)[1] == L
    if L == 3:
        assert km.knee_index(v, R, 3) == 1 and _threshold(got) == (80, 3)          # the shoulder is the middle point
    got, _ = _run(tmp_path, dict(lower=10), ((), ()))                              # no barcode at all
    assert _threshold(got) == (10, 0)
    got, _ = _run(tmp_path, dict(mode="expected"), ((), ()))
    assert _threshold(got) == (1, 0)


def test_refused_params(tmp_path):
    for field in ("lower", "divisor", "min_umis", "expected_cells"):
        for mode in ("curve", "expected", "min"):
            got, _ = _run(tmp_path, {field: 0, "mode": mode})
            assert got["params"].startswith("params %d " % PA_ERR_INVALID_ARG) and field in got["params"] and "threshold" not in got
    got, _ = _run(tmp_path, dict(mode=3))
    assert got["params"].startswith("params %d " % PA_ERR_INVALID_ARG) and "mode 3" in got["params"]


def test_refusals_name_the_entry_and_the_record(tmp_path):
    rec = VALID_RECORDS
    barcodes = [1, 5, 9, 77, 200, 255]
    got, _ = _run(tmp_path, records=rec, barcodes=barcodes)
    assert got["records"].split()[:2] == ["records", "0"] and got["list"].split()[:2] == ["list", "0"]
    got, _ = _run(tmp_path)                                                                # nothing at all is valid
    assert got["records"].split()[:2] == ["records", "0"] and got["list"].split()[:2] == ["list", "0"] and got["tsv"].split()[:2] == ["tsv", "0"]
    for at in (0, 3, 5):
        bad = list(barcodes)
        bad[at] = 256                                                                      # 4^bc_len
        got, _ = _run(tmp_path, barcodes=bad)
        assert got["list"].startswith("list %d barcode list entry %d:" % (PA_ERR_INVALID_ARG, km.check_list(bad, 4))) and km.check_list(bad, 4) == at
        if at:
            for value in (barcodes[at - 1], 0):                                            # a duplicate; a descent
                bad = list(barcodes)
                bad[at] = value
                got, _ = _run(tmp_path, barcodes=bad)
                assert got["list"].startswith("list %d barcode list entry %d:" % (PA_ERR_INVALID_ARG, at)) and km.check_list(bad, 4) == at
    for at in (0, 2, 4):
        for field, value in ((0, 256), (1, 256)):                                          # a barcode / a UMI of 4^len
            bad = [list(r) for r in rec]
            bad[at][field] = value
            got, _ = _run(tmp_path, records=bad)
            assert got["records"].startswith("records %d record %d:" % (PA_ERR_INVALID_ARG, at)), got["records"]
        if at:
            bad = list(rec)
            bad[at] = bad[at - 1]                                                          # equal: not STRICTLY ascending
            got, _ = _run(tmp_path, records=bad)
            assert got["records"].startswith("records %d record %d: not above record %d" % (PA_ERR_INVALID_ARG, at, at - 1))
    for bc_len, umi_len in ((0, 4), (4, 0), (17, 16), (32, 1)):
        got, _ = _run(tmp_path, bc_len=bc_len, umi_len=umi_len)
        assert got["records"].startswith("records %d" % PA_ERR_UNSUPPORTED)


def test_tsv_of_the_longest_barcode_and_the_largest_values(tmp_path):
    rows = [(0, 2 ** 64 - 1, 2 ** 32 - 1, 2 ** 32 - 1, 1, 0), (4 ** 31 - 1, 1, 1, 1, 0, 1)]
    got, tsv = _run(tmp_path, rows=rows, bc_len=31, umi_len=1)
    assert got["tsv"].split()[:2] == ["tsv", "0"] and tsv.decode() == km.ranks_tsv(rows, 31)
    assert tsv.decode().splitlines()[1] == "A" * 31 + "\t4294967295\t4294967295\t18446744073709551615\t1\t0"
