"""Properties of the gene counter's model (tests/genes_model.py) on the designed cases (tests/genes_cases.py): no GPU, no library."""
from collections import Counter

import numpy as np
import pytest

import genes_cases as gc
import genes_model as gm


def test_thresholds_are_the_sources():
    """genes_cases.py restates the thresholds of genes_state.hpp: a change there fails here until the cases follow"""
    src = gc.thresholds_in_source()
    assert src["GN_LANE_RECORDS"] == gc.GN_LANE_RECORDS and src["GN_WAVE_CELLS"] == gc.GN_WAVE_CELLS
    assert src["GN_WAVE_MAX"] == gc.GN_WAVE_MAX and src["GN_LDS_CAP"] == gc.GN_LDS_CAP
    assert 2 * 8 * gc.GN_LDS_CAP <= 160 * 1024                 # two blocks' working arrays share a CU's LDS


@pytest.mark.parametrize("name", sorted(gc.CASES))
def test_case_reaches_its_shape(name):
    m = gc.model(name)
    gc.check(name, m)
    rec = gc.case(name)[0]
    key = list(zip(rec["barcode"].tolist(), rec["umi"].tolist(), rec["ec"].tolist()))
    assert key == sorted(set(key))                              # strictly ascending, as the header asks


@pytest.mark.parametrize("name", gc.EM_CASES)
def test_mass_is_kept(name):
    """sum of alpha over a cell == its kept molecules after every step, to within summation rounding"""
    m = gc.model(name)
    a = m.start()
    for _ in range(12):
        for k, c in enumerate(m.cells):
            got = float(np.sum(a[m.base[k]:m.base[k + 1]].astype(np.longdouble)))
            assert abs(got - c.molecules) <= 4 * (len(c.genes) + c.longest + c.degree + 4) * 2.0 ** -53 * c.molecules * 12, (name, k, got, c.molecules)
        a = m.step(a)


def test_cell_without_multi_rows_is_exact_and_iteration_free():
    inp = gm.directed([(1, [[[0]], [[0]], [[2], [2, 3]]]), (2, [[[0, 1]], [[1]]])], 4)
    m = gm.Model(*inp)
    full, iters, conv, _ = m.run()
    assert iters[0] == 0 and conv[0] and iters[1] >= 50
    assert full[m.base[0]:m.base[1]].tolist() == [2.0, 1.0] and m.gene[m.base[0]:m.base[1]].tolist() == [0, 2]
    assert np.array_equal(m.step(m.start())[m.base[0]:m.base[1]], m.start()[m.base[0]:m.base[1]])


@pytest.mark.parametrize("name", sorted(gc.CASES))
def test_unique_mode_is_the_counter(name):
    m = gc.model(name, mode="unique")
    full, iters, _, _ = m.run()
    assert not iters.any() and np.array_equal(full, np.round(full))
    want = m.unique_counter()
    cell, gene, value = m.matrix(full)
    assert {(int(c), int(g)): int(v) for c, g, v in zip(cell, gene, value)} == dict(want)
    inp = gc.case(name)
    G = gm.gene_sets(inp[1], inp[2], inp[3])
    plain = Counter((b, s[0]) for b, s in gm.molecules(inp[0], G) if len(s) == 1)
    assert sum(want.values()) == sum(plain.values()) == m.stats["unique_gene_molecules"]


def test_a_cell_alone_and_among_others():
    names = ("molecules", "wave_edge", "stop", "ragged")
    batch, where = gc.batch_of(names)
    mb = gm.Model(*batch)
    full_b, iters_b, _, _ = mb.run()
    bc = mb.barcodes.tolist()
    for name in names:
        m = gc.model(name)
        full, iters, _, _ = m.run()
        for n2, b0, b in where:
            if n2 != name or b0 not in m.barcodes.tolist():
                continue
            j, k = bc.index(b), m.barcodes.tolist().index(b0)
            assert iters_b[j] == iters[k]
            assert np.array_equal(full_b[mb.base[j]:mb.base[j + 1]], full[m.base[k]:m.base[k + 1]]), (name, k)
            assert np.array_equal(mb.gene[mb.base[j]:mb.base[j + 1]], m.gene[m.base[k]:m.base[k + 1]])


@pytest.mark.parametrize("name", gc.EM_CASES)
def test_float64_model_meets_the_200_step_criterion(name):
    """the criterion the GPU is held to is one the float64 model itself meets, and every case has entries to select"""
    m = gc.model(name)
    a64, a80 = m.iterate(200), m.iterate(200, np.longdouble)
    sel = np.asarray(a80, np.float64) >= 1e-2
    assert sel.any()
    d_ref = max(float(np.max(np.abs(a64[sel].astype(np.longdouble) - a80[sel]) / a80[sel])), 2.0 ** -50)
    assert d_ref <= 16 * 2.0 ** -50 or d_ref < 1e-9, (name, d_ref)


def test_stop_case_decisions_are_clear_of_the_threshold():
    """the two cells of `stop` end at different checked iterations, and no decision of the model lies within the one-step bound of its
    threshold: the GPU must report the same iteration counts"""
    m = gc.model("stop")
    _, iters, conv, margin = m.run()
    assert conv.all() and iters[0] == m.par["min_iters"] and iters[1] > iters[0] and iters[1] % m.par["check_every"] == 0
    bound = 4 * (m.stats["longest_multi_row"] + m.stats["largest_degree"] + 4) * 2.0 ** -53
    assert margin > 1e3 * bound, (margin, bound)


def test_file_text():
    assert gm.decode_barcode(0b00011011, 4) == "ACGT" and gm.decode_barcode(0, 2) == "AA"
    assert [gm.f64_text(v) for v in (1.0, 0.5, 1e-7, 1e22, 2.5e-3, 1 / 3)] == ["1", "0.5", "0.0000001", "10000000000000000000000", "0.0025", "0.3333333333333333"]
    t = gm.matrix_text(5, 2, [0, 1], [3, 0], [1.5, 2.0])
    assert t == "%%MatrixMarket matrix coordinate real general\n5 2 2\n4 1 1.5\n1 2 2\n"
