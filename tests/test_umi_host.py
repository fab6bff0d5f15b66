"""CPU tier: the host half of the UMI correction (csrc/bus_umi_host.cpp: the checks of the arguments with their messages and their order, the stat
names; with the gene-set builder of csrc/genes_host.cpp it reuses) driven by a stand-alone host program under AddressSanitizer +
UndefinedBehaviorSanitizer (tests/umi/): it must be silent and agree with tests/umi_model.py and tests/umi_cases.py."""
import importlib.util
import subprocess

import pytest

import helpers
import umi_cases as uc
import umi_model as um

PA_ERR_INVALID_ARG, PA_ERR_UNSUPPORTED = -1, -8                       # include/pseudoaligner_amd.h


def _exe():
    spec = importlib.util.spec_from_file_location("pa_umi_build", str(helpers.ROOT / "tests" / "umi" / "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.build_check()


def _run(tmp_path, case, mode=0, records=None, tx_gene=None, lens=None, off=None, ids=None):
    rec, o, i, tg, num_genes, bc_len, umi_len = case
    records = [tuple(int(x) for x in (r["barcode"], r["umi"], r["ec"], r["count"])) for r in rec] if records is None else records
    o, i, tg = (o.tolist() if off is None else off), (i.tolist() if ids is None else ids), (tg.tolist() if tx_gene is None else tx_gene)
    bc_len, umi_len = lens or (bc_len, umi_len)
    text = "%d %d %d %d %d\n%s\n%d\n%s\n%d\n%s\n%d\n%s" % (bc_len, umi_len, mode, len(tg), num_genes, " ".join(map(str, tg)), len(o) - 1, " ".join(map(str, o)), len(i),
                                                         " ".join(map(str, i)), len(records), "".join("%d %d %d %d\n" % tuple(r) for r in records))
    (tmp_path / "case.txt").write_text(text)
    run = subprocess.run([str(_exe()), str(tmp_path / "case.txt")], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and run.stderr == "", (run.returncode, run.stdout[-3000:], run.stderr[-3000:])   # the sanitizers stay silent
    lines = run.stdout.splitlines()
    assert lines[-1] == "OK" and not any(l.startswith("MISS") for l in lines), run.stdout[-3000:]
    return {l.split()[0]: l for l in lines}


@pytest.mark.parametrize("name", ["clamped_sum", "inert_in_between", "nothing_moves"])
def test_valid_cases_pass_and_the_gene_sets_are_the_models(name, tmp_path):
    case = uc.hand(name)[0]
    for mode in (0, 1):
        got = _run(tmp_path, case, mode)
        assert got["mode"] == "mode 0" and got["records"].split()[:2] == ["records", "0"] and got["call"].split()[:2] == ["call", "0"]
        G = um.gene_sets(case[1], case[2], case[3])
        assert got["sets"] == "sets " + " ".join(" ".join(map(str, sorted(g))) + " ;" if g else ";" for g in G)
        assert tuple(got["names"].split()[1:]) == um.STAT_NAMES
    empty = _run(tmp_path, case, records=[])
    assert empty["call"].split()[:2] == ["call", "0"]                                      # n = 0 is legal


def test_widest_values_are_no_offence(tmp_path):
    case = uc.widths_cases()["umi_len_31"]
    got = _run(tmp_path, case)
    assert got["call"].split()[:2] == ["call", "0"] and int(case[0]["umi"].max()) == 4 ** 31 - 1
    big = uc.hand("n_beyond_32_bits")[0]
    assert _run(tmp_path, big)["call"].split()[:2] == ["call", "0"]                        # the largest count


def test_refusals_name_the_record_and_come_in_the_gene_counters_order(tmp_path):
    case = uc.hand("nothing_moves")[0]
    rec = [tuple(int(x) for x in (r["barcode"], r["umi"], r["ec"], r["count"])) for r in case[0]]
    n, n_ecs = len(rec), len(case[1]) - 1
    bad_call = lambda got, needle: got["call"].startswith("call %d " % PA_ERR_INVALID_ARG) and needle in got["call"]
    for at in (0, n // 2, n - 1):
        for field, value, word in ((0, 256, "barcode"), (1, 256, "UMI"), (2, n_ecs, "ec %d" % n_ecs), (2, -1, "ec -1")):
            bad = [list(r) for r in rec]
            bad[at][field] = value
            got = _run(tmp_path, case, records=bad)
            assert got["records"].startswith("records %d record %d:" % (PA_ERR_INVALID_ARG, at)) and word in got["records"], got["records"]
            assert bad_call(got, "record %d:" % at)
        if at:
            bad = list(rec)
            bad[at] = bad[at - 1]                                                          # equal: not STRICTLY ascending
            assert bad_call(_run(tmp_path, case, records=bad), "record %d:" % at)
            bad = [list(r) for r in rec]
            bad[at][0] = 0                                                                 # below the record before
            assert bad_call(_run(tmp_path, case, records=bad), "record %d:" % at)
    assert _run(tmp_path, case, mode=2)["mode"] == "mode %d" % PA_ERR_INVALID_ARG
    tg = case[3].tolist()
    tg[3] = case[4]
    assert bad_call(_run(tmp_path, case, tx_gene=tg), "tx_gene[3]")
    ids = case[2].tolist()
    ids[-1] = len(tg)
    assert bad_call(_run(tmp_path, case, ids=ids), "is no transcript")
    for lens in ((0, 4), (4, 0), (17, 16), (32, 1)):
        assert bad_call(_run(tmp_path, case, lens=lens), "barcode length")
    # the order: mode, lengths, tables, records
    bad = [list(r) for r in rec]
    bad[0][2] = n_ecs
    assert bad_call(_run(tmp_path, case, records=bad, tx_gene=tg), "tx_gene[3]")
    assert bad_call(_run(tmp_path, case, records=bad, tx_gene=tg, lens=(0, 4)), "barcode length")
    assert bad_call(_run(tmp_path, case, records=bad, tx_gene=tg, lens=(0, 4), mode=5), "mode 5")
