"""CPU tier: the host half of the BUS barcode correction (csrc/bus_correct_host.cpp: packing a whitelist, the checks of the whitelist and of the
records with their messages, the capacity rule) driven by a stand-alone host program under AddressSanitizer + UndefinedBehaviorSanitizer
(tests/correct/): it must be silent and agree with tests/correct_model.py and tests/correct_cases.py."""
import importlib.util
import subprocess

import numpy as np
import pytest

import correct_cases as cc
import correct_model as cm
import helpers

PA_ERR_INVALID_ARG, PA_ERR_UNSUPPORTED = -1, -8                       # include/pseudoaligner_amd.h


def _exe():
    spec = importlib.util.spec_from_file_location("pa_correct_build", str(helpers.ROOT / "tests" / "correct" / "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.build_check()


def _run(tmp_path, bc_len, umi_len, strings, values, records):
    case = "%d %d\n%d\n%s\n%d\n%s\n%d\n%s" % (bc_len, umi_len, len(strings), "\n".join(strings), len(values), " ".join(map(str, values)), len(records),
                                          "".join("%d %d %d %d\n" % tuple(r) for r in records))
    (tmp_path / "case.txt").write_text(case)
    run = subprocess.run([str(_exe()), str(tmp_path / "case.txt")], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and run.stderr == "", (run.returncode, run.stdout[-3000:], run.stderr[-3000:])   # the sanitizers stay silent
    lines = run.stdout.splitlines()
    assert lines[-1] == "OK" and not any(l.startswith("MISS") for l in lines), run.stdout[-3000:]
    return {l.split()[0]: l for l in lines if not l.startswith("capacity")}, [tuple(map(int, l.split()[1:])) for l in lines if l.startswith("capacity")]


@pytest.mark.parametrize("name", ["merges", "exact_wins_midway_far", "one_base_ambiguous", "no_records"])
def test_valid_cases_pass_and_pack_as_the_model(name, tmp_path):
    rec, wl, bc_len, umi_len, _, _ = cc.HAND[name]
    got, caps = _run(tmp_path, bc_len, umi_len, [cm.unpack(w, bc_len) for w in wl], wl, rec)
    assert got["lengths"] == "lengths 0" and got["whitelist"].split()[:2] == ["whitelist", "0"] and got["records"].split()[:2] == ["records", "0"]
    assert [int(x) for x in got["pack"].split()[2:]] == wl and got["pack"].split()[1] == "0"
    assert caps == [(n, cc.capacity(n)) for n in (1, 2, 3, 1024, 1025, 6_800_000, 2 ** 31 - 1)] and caps[-1][1] == 2 ** 32


def test_longest_barcode_and_every_base(tmp_path):
    rng = np.random.default_rng(3)
    strings = ["".join(cm.BASES[x] for x in rng.integers(0, 4, 31)) for _ in range(9)] + ["T" * 31, "A" * 31]
    values = [cm.pack(s) for s in strings]
    rec = sorted((v, 3, -5 + i, 0xFFFFFFFF) for i, v in enumerate(values))              # a negative ec and the largest count are no offence
    got, _ = _run(tmp_path, 31, 1, strings, values, rec)
    assert [int(x) for x in got["pack"].split()[2:]] == values and max(values) == 4 ** 31 - 1
    assert got["whitelist"].split()[1] == "0" and got["records"].split()[1] == "0" and got["lengths"] == "lengths 0"


def test_refusals_name_the_entry_and_the_record(tmp_path):
    wl = [5, 9, 200, 77, 31, 64]
    rec = [(1, 0, 0, 1), (1, 0, 1, 1), (1, 1, 0, 1), (2, 0, 0, 1), (7, 3, 2, 1)]
    for at in (0, 3, 5):                                                                   # a value of 4^bc_len; a non-ACGT byte
        bad = list(wl)
        bad[at] = 256
        strings = [cm.unpack(w, 4) for w in wl]
        strings[at] = strings[at][:2] + "N" + strings[at][3:]
        got, _ = _run(tmp_path, 4, 4, strings, bad, rec)
        assert got["whitelist"].startswith("whitelist %d whitelist entry %d:" % (PA_ERR_INVALID_ARG, at)) and cm.check_whitelist(bad, 4) == at
        assert got["pack"].startswith("pack %d whitelist entry %d: byte 3" % (PA_ERR_INVALID_ARG, at))
    for small, large in ((0, 5), (2, 3), (4, 5), (0, 1)):                                  # duplicates: the smaller index is named
        bad = list(wl)
        bad[large] = bad[small]
        got, _ = _run(tmp_path, 4, 4, [], bad, rec)
        assert got["whitelist"].startswith("whitelist %d whitelist entry %d: entry %d " % (PA_ERR_INVALID_ARG, small, large)) and cm.check_whitelist(bad, 4) == small
    got, _ = _run(tmp_path, 4, 4, [], [5, 9, 5, 9, 5], rec)                               # several: the smallest named index
    assert got["whitelist"].startswith("whitelist %d whitelist entry 0: entry 2 " % PA_ERR_INVALID_ARG) and cm.check_whitelist([5, 9, 5, 9, 5], 4) == 0
    got, _ = _run(tmp_path, 4, 4, [], [], rec)
    assert got["whitelist"].startswith("whitelist %d" % PA_ERR_INVALID_ARG)                # an empty whitelist
    for at in (0, 2, 4):
        for field, value in ((0, 256), (1, 256)):                                          # a barcode / a UMI of 4^len
            bad = [list(r) for r in rec]
            bad[at][field] = value
            got, _ = _run(tmp_path, 4, 4, [], wl, bad)
            assert got["records"].startswith("records %d record %d:" % (PA_ERR_INVALID_ARG, at)), got["records"]
        if at:
            bad = list(rec)
            bad[at] = bad[at - 1]                                                          # equal: not STRICTLY ascending
            got, _ = _run(tmp_path, 4, 4, [], wl, bad)
            assert got["records"].startswith("records %d record %d:" % (PA_ERR_INVALID_ARG, at))
            bad = [list(r) for r in rec]
            bad[at][0] = 0                                                                 # below the record before
            got, _ = _run(tmp_path, 4, 4, [], wl, bad)
            assert got["records"].startswith("records %d record %d:" % (PA_ERR_INVALID_ARG, at))
    for bc_len, umi_len in ((0, 4), (4, 0), (17, 16), (32, 1)):
        got, _ = _run(tmp_path, bc_len, umi_len, [], wl, [])
        assert got["lengths"] == "lengths %d" % PA_ERR_UNSUPPORTED
