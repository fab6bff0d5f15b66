"""The gene counter on the GPU (pa_genes, pa_count_cells_em) against the model of tests/genes_model.py on the designed cases of
tests/genes_cases.py: the molecule stage exactly (stats [0..11], the (cell, gene) list, the start point bit for bit), one step against the
EM map within the bound of tests/test_gpu_quant.py, 200 steps against the long-double model within its criterion, the stop rule and the
freeze per cell, and the chain from two FASTQ files against the model fed with the oracle's mapping."""
import json
import os

import numpy as np
import pytest

import bus_model as bm
import genes_cases as gc
import genes_model as gm
import helpers

pa = helpers.pa
pytestmark = pytest.mark.gpu

EPS = 2.0 ** -53
STEP_POINTS = (0, 1, 2, 10, 49)
BC, UMI = 16, 12
_cache = {}


def _gencode():
    if "gencode" not in _cache:
        host = pa.build_index(str(helpers.FASTA), 24, 8)
        _cache["gencode"] = (host, pa.Pseudoaligner(host))
    return _cache["gencode"]


def counter(name, **params):
    return pa.GeneCounter.from_arrays(_gencode()[1], *gc.case(name), **params), gc.model(name, **params)


def assert_structure(g, m):
    """stats [0..11], the cells, the (cell, gene) list and the start point, exactly"""
    st = g.stats()
    assert {k: st[k] for k in gm.STAT_NAMES} == m.stats
    bc, cell, gene, alpha = g.values()
    assert g.layout() == (len(m.cells), len(m.gene))
    assert np.array_equal(bc, m.barcodes) and np.array_equal(cell, m.cell) and np.array_equal(gene, m.gene)
    assert np.array_equal(alpha, m.start())
    return st


def step_tolerance(st):
    return 4 * (st["longest_multi_row"] + st["largest_degree"] + 4) * EPS


def assert_steps(name, g, m, points=STEP_POINTS):
    tol = step_tolerance(g.stats())
    done = 0
    for i in points:
        g.step(i - done)
        before = g.values()[3]
        want = m.step(before)                                      # one model step from the GPU's own alpha_i
        g.step(1)
        done = i + 1
        got = g.values()[3]
        ok = want > 1e-290
        worst = float(np.max(np.abs(got[ok] - want[ok]) / want[ok])) if ok.any() else 0.0
        print("%s step %d: worst relative deviation %.3g (bound %.3g, ratio %.3g)" % (name, i, worst, tol, worst / tol))
        assert np.all(np.abs(got[ok] - want[ok]) <= tol * want[ok]), (name, i, worst, tol)
        assert np.all(got[~ok] < 1e-289)
    multi = np.array([bool(c.multi) for c in m.cells])
    assert np.array_equal(g.cell_iters(), np.where(multi, done, 0))


MOLECULE_CASES = ("molecules", "umi1", "run_ends", "empty", "one_record", "all_dropped")


@pytest.mark.parametrize("name", MOLECULE_CASES)
def test_molecule_stage_is_exact(name):
    g, m = counter(name)
    gc.check(name, m)
    assert_structure(g, m)
    it, notconv = g.run()
    full, iters, conv, _ = m.run()
    assert np.array_equal(g.cell_iters(), iters) and it == int(iters.max(initial=0)) and notconv == int((~conv).sum())
    cell, gene, value = g.matrix()
    assert np.array_equal(cell, m.matrix(full)[0]) and np.array_equal(gene, m.matrix(full)[1]) and g.stats()["matrix_entries"] == len(value)


@pytest.mark.parametrize("name", MOLECULE_CASES + ("rows", "stop", "truncation"))
def test_unique_mode_is_the_counter(name):
    g, m = counter(name, mode="unique")
    st = g.stats()
    assert {k: st[k] for k in gm.STAT_NAMES} == m.stats
    assert g.run() == (0, 0) and not g.cell_iters().any()
    cell, gene, value = g.matrix()
    assert np.array_equal(value, np.round(value))
    assert {(int(c), int(k)): int(v) for c, k, v in zip(cell, gene, value)} == dict(m.unique_counter())


@pytest.mark.parametrize("name", ("molecules", "umi1", "run_ends", "all_multi", "stop", "truncation", "one_cell"))
def test_one_step_is_the_em_map(name):
    g, m = counter(name)
    assert_structure(g, m)
    assert_steps(name, g, m)


@pytest.mark.parametrize("name", gc.EM_CASES)
def test_200_steps_against_the_long_double_model(name):
    """GPU deviation <= 16 x D_ref, D_ref = the float64 model's deviation from the long-double model (floored at 2^-50), over the entries
    with alpha >= 1e-2: the criterion and margin of tests/test_gpu_quant.py"""
    g, m = counter(name)
    g.step(200)
    got = g.values()[3]
    a64, a80 = m.iterate(200), m.iterate(200, np.longdouble)
    sel = np.asarray(a80, np.float64) >= 1e-2
    assert sel.any()
    ref = a80[sel]
    d_ref = max(float(np.max(np.abs(a64[sel].astype(np.longdouble) - ref) / ref)), 2.0 ** -50)
    d_gpu = float(np.max(np.abs(got[sel].astype(np.longdouble) - ref) / ref))
    print("%s: D_ref %.3g, GPU %.3g, ratio %.3g" % (name, d_ref, d_gpu, d_gpu / d_ref))
    out = os.environ.get("PA_GENES_PARITY_JSON")
    if out:
        rec = json.load(open(out)) if os.path.exists(out) else {}
        rec[name] = dict(d_ref=d_ref, d_gpu=d_gpu, ratio=d_gpu / d_ref, cells=len(m.cells), entries=int(sel.sum()), **{k: m.stats[k] for k in gm.STAT_NAMES[7:]})
        json.dump(rec, open(out, "w"), indent=1, sort_keys=True)
    assert d_gpu <= 16 * d_ref, (name, d_gpu, d_ref)


def test_stop_rule_and_freeze():
    """two cells that stop at different checked iterations: the iteration counts are the model's (whose decisions are clear of the
    thresholds: tests/test_genes_model.py), the cell that stopped first is frozen at that iterate, a second run() reports the same"""
    g, m = counter("stop")
    full, iters, conv, _ = m.run()
    assert iters.tolist() == [50, 210] and conv.all()
    assert g.run() == (210, 0)
    assert g.cell_iters().tolist() == [50, 210]
    final = g.values()[3]
    assert g.run() == (210, 0) and np.array_equal(g.values()[3], final) and g.cell_iters().tolist() == [50, 210]
    with pytest.raises(pa.PaError):
        g.step(1)
    # the frozen iterates, replayed by exact steps on a second object: cell 0 as after 50 steps, cell 1 as after 210
    h, _ = counter("stop")
    h.step(50)
    a50 = h.values()[3]
    h.step(160)
    a210 = h.values()[3]
    lim = g.params.alpha_limit
    cut = lambda a: np.where(a < lim, 0.0, a)
    assert np.array_equal(final[m.base[0]:m.base[1]], cut(a50)[m.base[0]:m.base[1]])
    assert np.array_equal(final[m.base[1]:m.base[2]], cut(a210)[m.base[1]:m.base[2]])
    assert not np.array_equal(a50[m.base[0]:m.base[1]], a210[m.base[0]:m.base[1]])      # (freezing mattered)
    # the model's values by the 200-step criterion at the run's own iteration counts
    a80 = m.iterate_per_cell(iters, np.longdouble)
    a64 = m.iterate_per_cell(iters)
    sel = np.asarray(a80, np.float64) >= 1e-2
    d_ref = max(float(np.max(np.abs(a64[sel].astype(np.longdouble) - a80[sel]) / a80[sel])), 2.0 ** -50)
    assert float(np.max(np.abs(final[sel].astype(np.longdouble) - a80[sel]) / a80[sel])) <= 16 * d_ref
    st = g.stats()
    assert st["most_iterations"] == 210 and st["cells_not_converged"] == 0 and st["matrix_entries"] == int((final != 0).sum()) and st["cells_in_hbm"] == 0


def test_max_iters_ends_an_unconverged_run():
    g, m = counter("stop", max_iters=120)
    assert g.run() == (120, 1) and g.cell_iters().tolist() == [50, 120] and g.stats()["cells_not_converged"] == 1
    g, m = counter("stop", max_iters=37, min_iters=5, check_every=7)
    full, iters, conv, _ = m.run()
    it, notconv = g.run()
    assert g.cell_iters().tolist() == iters.tolist() and notconv == int((~conv).sum()) and it == 37


def test_truncation_is_exactly_at_alpha_limit():
    """alpha_limit 2: u = 2 stays (not below the limit), u = 1 goes, and so does the starved gene"""
    g, m = counter("truncation", alpha_limit=2.0)
    g.run()
    cell, gene, value = g.matrix()
    assert gene.tolist() == [0, 2] and value[1] == 2.0 and 31.9 < value[0] < 32.0001
    _, _, vg, alpha = g.values()
    assert vg.tolist() == [0, 1, 2, 3] and alpha[1] == 0.0 and alpha[3] == 0.0 and g.stats()["matrix_entries"] == 2
    full, _, _, _ = m.run()
    assert np.array_equal(full != 0, alpha != 0)


def _e2e():
    if "e2e" not in _cache:
        host, al = _gencode()
        ix = host.arrays()
        _, seqs = helpers.read_fasta()
        case = bm.make_case(12, seqs, BC, UMI)
        mapping = bm.mapping_from_oracle(helpers.Oracle(host), case["r2"])
        records, table, st, _ = bm.model(case["r1"], mapping, int(ix["num_transcripts"]), bm.index_classes(ix), BC, UMI)
        _cache["e2e"] = (case, records, table, st)
    return _cache["e2e"]


def _fastq(ids, seqs):
    return "".join("@%s extra\n%s\n+\n%s\n" % (i, s, "I" * len(s)) for i, s in zip(ids, seqs)).encode()


def test_count_cells_em_from_fastq(tmp_path):
    host, al = _gencode()
    case, records, table, bus_st = _e2e()
    tx_gene, gene_names = host.genes()
    rec = np.array([(b, u, e, c, 0, 0) for b, u, e, c in records], gm.BUS_RECORD_DTYPE)
    off = np.cumsum([0] + [len(t) for t in table]).astype(np.uint64)
    ids = np.array([t for lst in table for t in lst], np.uint32)
    m = gm.Model(rec, off, ids, tx_gene, len(gene_names), BC, UMI)
    assert m.stats["multi_gene_molecules"] > 0 and m.stats["cells_with_multi_rows"] > 0 and m.stats["cells"] > 20     # not vacuous
    n = len(case["r1"])
    names = ["read%d" % i for i in range(n)]
    (tmp_path / "r1.fq").write_bytes(_fastq([i + "/1" for i in names], case["r1"]))
    (tmp_path / "r2.fq").write_bytes(_fastq([i + "/2" for i in names], case["r2"]))
    out, out_bus = tmp_path / "out", tmp_path / "bus"
    out.mkdir()
    out_bus.mkdir()
    st = al.count_cells_em(host, tmp_path / "r1.fq", tmp_path / "r2.fq", out, BC, UMI, num_threads=4)
    assert {k: st[k] for k in gm.STAT_NAMES} == m.stats and st["multi_gene_molecules"] > 0 and st["cells_with_multi_rows"] > 0
    assert not list(out.glob("*.bus")) and sorted(p.name for p in out.iterdir()) == ["barcodes.tsv", "features.tsv", "matrix.mtx"]
    assert (out / "barcodes.tsv").read_text() == gm.barcodes_text(m.barcodes, BC)
    assert (out / "features.tsv").read_text() == gm.features_text(gene_names)
    # the same records through the objects: from the writer in HBM and from its arrays on the host, byte for byte
    import test_gpu_bus as tb
    writer = tb.gpu_bus(al, host, case["r1"], case["r2"], BC, UMI, cuts=(n // 3,))
    g1 = pa.GeneCounter.from_bus(writer, tx_gene, len(gene_names))
    g2 = pa.GeneCounter.from_arrays(al, writer.records(), *writer.ecs(), tx_gene, len(gene_names), BC, UMI)
    assert np.array_equal(writer.records(), rec)
    for g in (g1, g2):
        assert_structure(g, m)
    for a, b in zip(g1.values(), g2.values()):
        assert a.tobytes() == b.tobytes()
    run1, run2 = g1.run(), g2.run()
    assert run1 == run2 == (st["most_iterations"], st["cells_not_converged"])
    for a, b in zip(g1.values() + g1.matrix(), g2.values() + g2.matrix()):
        assert a.tobytes() == b.tobytes()
    # structure exact, values by the 200-step criterion at the run's own iteration counts
    iters = g1.cell_iters()
    full, m_iters, _, margin = m.run()
    assert np.array_equal(iters, m_iters) or margin < 1e-9, (iters, m_iters, margin)
    a80, a64 = m.iterate_per_cell(iters, np.longdouble), m.iterate_per_cell(iters)
    lim = g1.params.alpha_limit
    want = np.where(a64 < lim, 0.0, a64)
    cell, gene, value = g1.matrix()
    assert np.array_equal(cell, m.cell[want != 0]) and np.array_equal(gene, m.gene[want != 0]) and st["matrix_entries"] == len(value)
    got = g1.values()[3]
    sel = np.asarray(a80, np.float64) >= 1e-2
    d_ref = max(float(np.max(np.abs(a64[sel].astype(np.longdouble) - a80[sel]) / a80[sel])), 2.0 ** -50)
    assert float(np.max(np.abs(got[sel].astype(np.longdouble) - a80[sel]) / a80[sel])) <= 16 * d_ref
    # the files parse and hold the matrix
    lines = (out / "matrix.mtx").read_text().splitlines()
    assert lines[0] == "%%MatrixMarket matrix coordinate real general" and lines[1] == "%d %d %d" % (len(gene_names), len(m.cells), len(value))
    parsed = [l.split() for l in lines[2:]]
    assert [int(p[1]) - 1 for p in parsed] == cell.tolist() and [int(p[0]) - 1 for p in parsed] == gene.tolist()
    assert [float(p[2]) for p in parsed] == value.tolist()                              # shortest digits that read back as the same double
    # pa_write_bus on the same input still writes the bytes the BUS model expects
    assert al.write_bus(host, tmp_path / "r1.fq", tmp_path / "r2.fq", out_bus, BC, UMI, num_threads=4) == bus_st
    assert (out_bus / "output.bus").read_bytes() == bm.bus_bytes(records, BC, UMI) and (out_bus / "matrix.ec").read_text() == bm.matrix_ec_text(table)


def test_invalid_records_are_named():
    """each invalid-record kind at the first, a middle and the last record: PA_ERR_INVALID_ARG naming the record, before any device work; the
    valid input is taken afterwards"""
    al = _gencode()[1]
    inp = list(gc.case("run_ends"))
    n = len(inp[0])

    def refused(rec, at):
        with pytest.raises(pa.PaError) as e:
            pa.GeneCounter.from_arrays(al, rec, *inp[1:])
        assert e.value.code == pa._ffi.PA_ERR_INVALID_ARG and "record %d" % at in str(e.value), str(e.value)

    for at in (0, 256, n - 1):
        for ec in (len(inp[1]) - 1, -1):                           # == n_ecs, negative
            rec = inp[0].copy()
            rec["ec"][at] = ec
            refused(rec, at)
        if at:
            rec = inp[0].copy()
            rec[at] = rec[at - 1]                                  # not STRICTLY ascending
            refused(rec, at)
            rec = inp[0].copy()
            rec["barcode"][at] = 0                                 # descending
            refused(rec, at)
    bad = inp[3].copy()
    bad[1] = inp[4]
    with pytest.raises(pa.PaError) as e:
        pa.GeneCounter.from_arrays(al, inp[0], inp[1], inp[2], bad, *inp[4:])
    assert e.value.code == pa._ffi.PA_ERR_INVALID_ARG and "tx_gene[1]" in str(e.value)
    g = pa.GeneCounter.from_arrays(al, *inp)
    assert g.stats()["records"] == n and g.layout()[0] == 1
    with pytest.raises(pa.PaError):
        g.matrix()                                                 # the matrix exists after run()
    with pytest.raises(pa.PaError) as e:
        g.write(_gencode()[0], "/nonexistent")
    assert e.value.code == pa._ffi.PA_ERR_INVALID_ARG               # ... and so do the files
