"""CPU tier: the host half of the gene counter (csrc/genes_host.cpp: the ec -> gene-set table, the argument checks, barcode decoding, the
three file writers) driven by a stand-alone host program under AddressSanitizer + UndefinedBehaviorSanitizer (tests/genes/): it must be
silent and agree with tests/genes_model.py in every gene set and in every byte of the three files."""
import importlib.util
import subprocess

import numpy as np
import pytest

import genes_cases as gc
import genes_model as gm
import helpers

PA_ERR_INVALID_ARG, PA_ERR_IO = -1, -2                       # include/pseudoaligner_amd.h


def _exe():
    spec = importlib.util.spec_from_file_location("pa_genes_build", str(helpers.ROOT / "tests" / "genes" / "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.build_check()


def _run(tmp_path, T, num_genes, bc_len, umi_len, tx_gene, ecs, records, barcodes, entries, names):
    out = tmp_path / "out"
    out.mkdir(exist_ok=True)
    fmt = lambda lst: "".join("%d %s\n" % (len(l), " ".join(map(str, l))) for l in lst)
    case = "%d %d %d %d\n%s\n%d\n%s%d\n%s%d\n%s\n%d\n%s%s\n%s\n%s\n" % (
        T, num_genes, bc_len, umi_len, " ".join(map(str, tx_gene)), len(ecs), fmt(ecs), len(records), "".join("%d %d %d %d\n" % tuple(r) for r in records),
        len(barcodes), " ".join(map(str, barcodes)), len(entries), "".join("%d %d %s\n" % (c, g, float(v).hex()) for c, g, v in entries), "\n".join(names), out,
        tmp_path / "no_such_dir")
    (tmp_path / "case.txt").write_text(case)
    run = subprocess.run([str(_exe()), str(tmp_path / "case.txt")], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and run.stderr == "", (run.returncode, run.stdout[-3000:], run.stderr[-3000:])   # the sanitizers stay silent
    lines = run.stdout.splitlines()
    assert lines[-1] == "OK" and not any(l.startswith("MISS") for l in lines), run.stdout[-3000:]
    return lines, out


def _ecs(off, ids):
    return [[int(t) for t in ids[int(off[e]):int(off[e + 1])]] for e in range(len(off) - 1)]


def test_gene_set_table_edges_and_files(tmp_path):
    """an ec without ids, all transcripts of one gene, ids of several genes out of gene order; the three files byte for byte; an unwritable out_dir"""
    tx_gene = [2, 2, 0, 1, 2, 0]
    ecs = [[], [0, 1, 4], [0, 2, 3], [5], [2, 5], [1, 3, 5]]
    records = [(0, 0, 1, 1), (0, 1, 2, 7), (5, 0, 0, 1), (4 ** 5 - 1, 3, 5, 2)]
    barcodes = [0, 5, 4 ** 5 - 1]
    entries = [(0, 0, 1.5), (0, 2, 1 / 3), (1, 1, 1e-7), (2, 0, 12345678.0), (2, 2, 2.5e-3)]
    names = ["gC", "gC", "gA", "gB", "gC", "gA"]                       # numbered by first appearance: gC = 0 ... but tx_gene above is the caller's own numbering
    lines, out = _run(tmp_path, 6, 3, 5, 3, tx_gene, ecs, records, barcodes, entries, names)
    assert "tables 0" in lines and "records 0 " in lines and "lengths 0" in lines and "features 0" in lines and "write 0" in lines
    assert "unwritable %d" % PA_ERR_IO in lines
    sets = {int(l.split()[1]): [int(x) for x in l.split()[2:]] for l in lines if l.startswith("set ")}
    want = gm.gene_sets(np.cumsum([0] + [len(e) for e in ecs]), np.array([t for e in ecs for t in e], np.int64), tx_gene)
    assert sets == {e: list(s) for e, s in enumerate(want)} and sets[0] == [] and sets[1] == [2] and sets[2] == [0, 1, 2] and sets[4] == [0]
    hashes = {int(l.split()[1]): int(l.split()[2]) for l in lines if l.startswith("hash ")}
    assert hashes[3] == hashes[4] and hashes[1] != hashes[3] and len(set(hashes.values())) == 4   # equal sets hash alike, whatever their transcripts
    cell, gene, value = zip(*entries)
    assert (out / "matrix.mtx").read_text() == gm.matrix_text(3, 3, cell, gene, value)
    assert (out / "barcodes.tsv").read_text() == gm.barcodes_text(barcodes, 5) == "AAAAA\nAAACC\nTTTTT\n"
    assert (out / "features.tsv").read_text() == gm.features_text(["gC", "gA", "gB"])


def test_one_gene_and_no_records(tmp_path):
    lines, out = _run(tmp_path, 2, 1, 16, 12, [0, 0], [[0], [1], [0, 1]], [], [], [], ["g", "g"])
    assert "records 0 " in lines and [l for l in lines if l.startswith("set ")] == ["set 0 0", "set 1 0", "set 2 0"]
    assert (out / "matrix.mtx").read_text() == "%%MatrixMarket matrix coordinate real general\n1 0 0\n" and (out / "barcodes.tsv").read_text() == ""


@pytest.mark.parametrize("name", ["molecules", "umi1"])
def test_designed_case_through_the_host_half(name, tmp_path):
    rec, off, ids, tx_gene, num_genes, bc_len, umi_len = gc.case(name)
    m = gc.model(name)
    full, _, _, _ = m.run()
    cell, gene, value = m.matrix(full)
    names = ["g%d" % g for g in tx_gene]
    lines, out = _run(tmp_path, len(tx_gene), num_genes, bc_len, umi_len, tx_gene.tolist(), _ecs(off, ids), [(r["barcode"], r["umi"], r["ec"], r["count"]) for r in rec],
                      m.barcodes.tolist(), list(zip(cell.tolist(), gene.tolist(), value.tolist())), names)
    assert "records 0 " in lines
    sets = [[int(x) for x in l.split()[2:]] for l in lines if l.startswith("set ")]
    assert sets == [list(s) for s in m.G]
    assert (out / "matrix.mtx").read_text() == gm.matrix_text(num_genes, len(m.cells), cell, gene, value)
    assert (out / "barcodes.tsv").read_text() == gm.barcodes_text(m.barcodes, bc_len)
    assert (out / "features.tsv").read_text() == gm.features_text(["g%d" % g for g in range(num_genes)])


def test_refusals(tmp_path):
    ecs = [[0], [1], [0, 1]]
    lines, _ = _run(tmp_path, 2, 2, 4, 4, [0, 2], ecs, [], [], [], ["a", "b"])
    assert lines[0] == "tables %d" % PA_ERR_INVALID_ARG
    lines, _ = _run(tmp_path, 2, 2, 4, 4, [0, 1], [[1, 0]], [], [], [], ["a", "b"])
    assert lines[0] == "tables %d" % PA_ERR_INVALID_ARG
    lines, _ = _run(tmp_path, 2, 2, 17, 16, [0, 1], ecs, [(1, 1, 0, 1), (1, 1, 2, 1), (1, 1, 1, 1)], [], [], ["a", "b"])
    assert any(l.startswith("records %d record 2" % PA_ERR_INVALID_ARG) for l in lines) and "lengths %d" % PA_ERR_INVALID_ARG in lines
    lines, _ = _run(tmp_path, 2, 2, 4, 4, [0, 1], ecs, [(1, 1, 0, 1), (1, 2, 3, 1)], [], [], ["a", "a"])
    assert any(l.startswith("records %d record 1" % PA_ERR_INVALID_ARG) for l in lines) and "features %d" % PA_ERR_INVALID_ARG in lines
