"""CPU tier: the host half of the BUS writer (csrc/bus_host.cpp: ec numbering, output.bus, matrix.ec, transcripts.txt) driven by a stand-alone
host program under AddressSanitizer + UndefinedBehaviorSanitizer (tests/bus/) on the model's cases: it must be silent and agree with
tests/bus_model.py in every ec and in every byte of the three files."""
import importlib.util
import subprocess

import numpy as np
import pytest

import bus_model as bm
import helpers

T = 8
CLASSES = [(3,), (1, 5), (), (2, 3, 4), (0, 6), (6,), (T,)]   # (the last: an id that is no transcript — no ec)


def _exe():
    spec = importlib.util.spec_from_file_location("pa_bus_build", str(helpers.ROOT / "tests" / "bus" / "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.build_check()


def _random_case(seed):
    rng = np.random.default_rng(seed)
    num_tx = 40
    classes = [tuple(sorted(rng.choice(num_tx, int(rng.integers(0, 6)), replace=False).tolist())) for _ in range(60)]
    classes = list(dict.fromkeys(classes))   # (an index has no two classes of one content)
    lists = [tuple(sorted(rng.choice(num_tx, int(rng.integers(2, 7)), replace=False).tolist())) for _ in range(300)]
    lists += [c for c in classes if len(c) >= 2][:10] + lists[:50]   # lists that equal an index class; repeats
    order = rng.permutation(len(lists))
    return num_tx, classes, [lists[i] for i in order]


CASES = {
    "hand": (T, CLASSES, [(1, 5), (2, 3), (1, 5, 7), (1, 7), (2, 3), (0, 6), (1, 5, 7)]),
    "no_lists": (T, CLASSES, []),
    "no_classes": (3, [], [(0, 2), (0, 1), (0, 1, 2)]),
    "random": _random_case(5),
}


@pytest.mark.parametrize("name", list(CASES))
def test_host_half_equals_model(name, tmp_path):
    num_tx, classes, lists = CASES[name]
    ec_of, table, novel = bm.number_ecs(num_tx, classes, lists)
    if name == "hand":
        assert novel == [(1, 5, 7), (1, 7), (2, 3)] and ec_of[(1, 5)] == T and ec_of[(0, 6)] == T + 2
    if name == "random":
        assert len(novel) > 100 and any(l in map(tuple, classes) for l in lists)
    rng = np.random.default_rng(1)
    records = sorted({(int(rng.integers(0, 1 << 62)) * 4 + 3, int(rng.integers(0, 1 << 24)), int(rng.integers(0, len(table)))) for _ in range(50)})
    records = [(b, u, ec, int(rng.integers(1, 1 << 32))) for b, u, ec in records] + [((1 << 64) - 1, (1 << 24) - 1, len(table) - 1, (1 << 32) - 1)]
    names = ["tx%d|gene" % t for t in range(num_tx)]
    out = tmp_path / "out"
    out.mkdir()
    fmt = lambda lst: "".join("%d %s\n" % (len(l), " ".join(map(str, l))) for l in lst)
    case = "%d\n20 12\n%d\n%s%d\n%s%d\n%s%d\n%s\n%s\n" % (num_tx, len(classes), fmt(classes), len(lists), fmt(lists), len(records),
                                                          "".join("%d %d %d %d\n" % r for r in records), len(names), "\n".join(names), out)
    (tmp_path / "case.txt").write_text(case)
    run = subprocess.run([str(_exe()), str(tmp_path / "case.txt")], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and run.stderr == "", (run.returncode, run.stdout[-3000:], run.stderr[-3000:])   # the sanitizers stay silent
    lines = run.stdout.splitlines()
    assert lines[-1] == "OK" and not any(l.startswith("MISS") for l in lines), run.stdout[-3000:]
    got = {l.split()[0]: [int(x) for x in l.split()[1:]] for l in lines[:-1]}
    multi = [c for c in classes if len(c) >= 2]
    want_class_ec = [c[0] if len(c) == 1 and c[0] < num_tx else num_tx + multi.index(c) if len(c) >= 2 else -1 for c in classes]
    assert got["class_ec"] == want_class_ec
    assert got["list_ec"] == [ec_of[l] for l in lists]
    assert got["table"] == [num_tx, len(multi), len(novel), sum(len(x) for x in table)]
    assert (out / "output.bus").read_bytes() == bm.bus_bytes(records, 20, 12)
    assert (out / "matrix.ec").read_text() == bm.matrix_ec_text(table)
    assert (out / "transcripts.txt").read_text() == bm.transcripts_text(names)
    assert bm.read_bus((out / "output.bus").read_bytes()) == (20, 12, b"", records) and bm.read_matrix_ec((out / "matrix.ec").read_text()) == table
