"""The gene counter's kernels at their edges (csrc/genes.hip, thresholds in csrc/genes_state.hpp): rows and degrees around the wave and
block widths, cells at both bin thresholds and around the LDS cap (the HBM variant), a ragged last block of the wave bin, more cells
than the grid's first wave of blocks, and the independence of a cell from its neighbours: alone and inside a shuffled batch of all
designed cells, byte for byte."""
import numpy as np
import pytest

import genes_cases as gc
import genes_model as gm
import helpers
from test_gpu_genes import _gencode, assert_steps, assert_structure, counter

pa = helpers.pa
pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", ("rows", "degrees", "wave_edge", "cap_edge", "ragged"))
def test_shapes_at_every_threshold(name):
    """structure exact and the EM map step by step, on the shapes that change the path: a row / a degree of 2, 3, 63, 64, 65, 256, 257; a
    cell of |E| + rows at GN_WAVE_MAX and GN_LDS_CAP with both neighbours, and at twice the cap"""
    g, m = counter(name, max_iters=300)
    gc.check(name, m)
    st = assert_structure(g, m)
    if name == "rows":
        assert st["longest_multi_row"] == 257
    if name == "degrees":
        assert st["largest_degree"] == 257
    assert_steps(name, g, m, points=(0, 1, 10))
    h, _ = counter(name, max_iters=300)
    it, notconv = h.run()
    full, iters, conv, margin = m.run()
    assert np.array_equal(h.cell_iters(), iters) or margin < 1e-9
    assert notconv == int((~conv).sum()) and it == int(iters.max())
    want_hbm = sum(c.size > gc.GN_LDS_CAP for c in m.cells)
    assert h.stats()["cells_in_hbm"] == want_hbm and (want_hbm == 2) == (name == "cap_edge")


def test_more_cells_than_the_first_wave_of_blocks():
    """9001 cells of the wave bin: more blocks than 256 CUs hold at once (8 blocks of 256 threads each), a ragged last block. The cells repeat
    30 patterns: the first 30 against the model, every other cell byte for byte against the first of its pattern"""
    n = 9001
    inp = gc.many_cells_case(n)
    g = pa.GeneCounter.from_arrays(_gencode()[1], *inp)
    head = gm.Model(*gc.many_cells_case(30))
    st = g.stats()
    assert st["cells"] == n and st["cells_with_multi_rows"] == n and n > 256 * 8 * gc.GN_WAVE_CELLS and n % gc.GN_WAVE_CELLS == 1
    for when in ("start", "steps", "run"):
        if when == "steps":
            g.step(7)
        if when == "run":
            g.run()
        bc, cell, gene, alpha = g.values()
        base = np.searchsorted(cell, np.arange(n + 1))
        want = {"start": head.start, "steps": lambda: head.iterate(7), "run": lambda: head.run()[0]}[when]()
        got30 = alpha[:base[30]]
        assert np.array_equal(gene[:base[30]], head.gene) and np.all(np.abs(got30 - want) <= 1e-12 * np.maximum(want, got30))
        for j in range(30, n):
            k = j % 30
            assert alpha[base[j]:base[j + 1]].tobytes() == alpha[base[k]:base[k + 1]].tobytes(), (when, j)
    assert (g.cell_iters() == g.cell_iters()[0]).all() or len(set(g.cell_iters().tolist())) <= 30


def test_independence_and_repeats():
    """every designed cell alone (in its own case) and inside a batch of all cases shuffled by barcode: byte-identical values after 50 steps
    and after run; two objects give the same bytes"""
    names = gc.EM_CASES
    batch, where = gc.batch_of(names)
    al = _gencode()[1]
    par = dict(max_iters=400)

    def collect(inp, steps):
        g = pa.GeneCounter.from_arrays(al, *inp, **par)
        if steps:
            g.step(steps)
        else:
            g.run()
        bc, cell, gene, alpha = g.values()
        base = np.searchsorted(cell, np.arange(len(bc) + 1))
        iters = g.cell_iters()
        return {int(b): (gene[base[k]:base[k + 1]].tobytes(), alpha[base[k]:base[k + 1]].tobytes(), int(iters[k])) for k, b in enumerate(bc)}, g

    for steps in (50, 0):
        in_batch, gb = collect(batch, steps)
        again, gb2 = collect(batch, steps)
        assert in_batch == again                                     # two objects, the same bytes
        for a, b in zip(gb.values(), gb2.values()):
            assert a.tobytes() == b.tobytes()
        seen = 0
        for name in names:
            alone, _ = collect(gc.case(name), steps)
            for n2, b0, b in where:
                if n2 == name and b0 in alone:
                    assert in_batch[b] == alone[b0], (name, b0, steps)
                    seen += 1
        assert seen == len(in_batch) > 30
    assert gb.stats()["cells_in_hbm"] == 2 and gb.stats()["largest_cell"] == 2 * gc.GN_LDS_CAP
