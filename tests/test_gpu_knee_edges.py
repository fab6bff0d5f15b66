"""The cell calling on BUS records (pa_bus_knee_records, pa_bus_knee, pa_bus_keep_records, pa_bus_keep; csrc/bus_knee.hip) on designed records
against the pure-Python model of tests/knee_model.py: every row field for field, the called list and all ten stats, at the smallest shapes at
which the kernels can go wrong: the seams of a wave, of the block's waves, of a tile and of the grid stride, long barcodes, the widths of the
sort. All integers (the threshold's floats are decided by a clear margin: knee_cases.clear_knee): equality, no tolerance."""
import ctypes as C

import numpy as np
import pytest

import bus_model as bm
import helpers
import knee_cases as kc
import knee_model as km

pa = helpers.pa
pytestmark = pytest.mark.gpu

T = kc.TILE
BC, UMI = 12, 10
_cache = {}


def _setup():
    if "ix" not in _cache:
        host = pa.build_index(str(helpers.FASTA), 24, 8)
        _cache["ix"] = (host, pa.Pseudoaligner(host), host.arrays())
        assert bm.RECORD_DTYPE == pa.BUS_RECORD_DTYPE and kc.ROW_DTYPE == pa.BARCODE_ROW_DTYPE and km.STAT_NAMES == pa.KNEE_STAT_NAMES
    return _cache["ix"]


def _gpu(arr, bc_len=BC, umi_len=UMI, **params):
    return pa.bus_knee(arr, bc_len, umi_len, _setup()[1], **params)


def _check(rec, bc_len=BC, umi_len=UMI, **params):
    """the GPU result equals the model's; -> (rows, called, stats) of the model"""
    if params.get("mode", "curve") in ("curve", km.CURVE):
        kc.assert_clear(rec, params.get("lower", km.DEFAULTS["lower"]))
    want = km.knee(rec, **params)
    rows, called, st = _gpu(kc.to_array(rec), bc_len, umi_len, **params)
    assert st == want[2]
    assert kc.rows_from_array(rows) == want[0]
    assert called.tolist() == want[1]
    return want


MIN1 = dict(mode="min", min_umis=1)


def test_no_record_and_one_record():
    for params, t in ((dict(), 10), (dict(mode="expected"), 1), (dict(mode="min", min_umis=4), 4)):
        rows, called, st = _check([], **params)
        assert rows == [] and called == [] and st["threshold"] == t and st["barcodes"] == 0
    rows, called, st = _check([(9, 3, -2, 7)], **MIN1)
    assert rows == [(9, 7, 1, 1, 0, 1)] and called == [9] and st["reads_called"] == 7


def test_one_barcode_owns_every_record_and_every_record_its_own_barcode():
    rng = np.random.default_rng(1)
    n = 700
    rows, _, st = _check(kc.from_heads(n, [], np.flatnonzero(rng.integers(0, 3, n) == 0).tolist()), **MIN1)
    assert len(rows) == 1 and rows[0][2] == n and 1 < rows[0][3] < n
    rows, called, st = _check(kc.from_heads(n, range(n), []), mode="min", min_umis=2)
    assert len(rows) == n and called == [] and st["distinct_values"] == 1
    rows, _, st = _check(kc.from_heads(900, range(0, 900, 9), []), **MIN1)         # every barcode one molecule of nine records (equal UMI, ec counts up)
    assert len(rows) == 100 and all(r[2] == 9 and r[3] == 1 for r in rows) and st["molecules"] == 100


@pytest.mark.parametrize("seam", [64, 256, T])
def test_runs_that_start_end_and_straddle_at_a_seam(seam):
    """a barcode head / a molecule head at record seam - 1, seam, seam + 1, or none near it, in every combination"""
    n = seam + 70
    spots = (None, seam - 1, seam, seam + 1)
    for b in spots:
        for m in spots:
            heads = [3] + ([b] if b is not None else []) + [n - 2]
            mols = [1, 5] + ([m] if m is not None else []) + [n - 1]
            rows, _, st = _check(kc.from_heads(n, heads, mols), **MIN1)
            assert len(rows) == len(set(heads) | {0}) and st["records"] == n
    # every record around the seam a barcode of its own, then a molecule of its own
    _check(kc.from_heads(n, range(seam - 3, seam + 3), []), **MIN1)
    _check(kc.from_heads(n, [], range(seam - 3, seam + 3)), **MIN1)


def test_one_barcode_over_three_whole_tiles_with_molecule_heads_on_both_seams():
    n = 5 * T
    rec = kc.from_heads(n, [T, 4 * T], [2 * T, 3 * T, T + 5, 4 * T - 1])
    rows, _, _ = _check(rec, **MIN1)
    assert [(r[2], r[3]) for r in rows] == [(T, 1), (3 * T, 5), (T, 1)]


def test_reads_sum_past_32_bits_across_a_tile_seam():
    big = 2 ** 32 - 1
    rec = kc.from_heads(T + 40, [T - 3, T + 3], [T - 1, T + 1], count=lambda i: big if T - 3 <= i < T + 3 else 2)
    rows, _, st = _check(rec, **MIN1)
    assert rows[1][1] == 6 * big > 2 ** 32 and rows[1][2:4] == (6, 3) and st["reads"] == 6 * big + 2 * (T + 34)


@pytest.mark.parametrize("bc_len", [1, 16, 31])
def test_shortest_and_longest_barcodes_and_umis(bc_len):
    top = 4 ** bc_len - 1
    for umi_len in (1, 32 - bc_len):
        u = 4 ** umi_len - 1
        rec = [(0, 0, 0, 1), (0, u, 0, 2), (0, u, 5, 1), (top, 0, -1, 4), (top, 0, 0, 1), (top, u, 2 ** 31 - 1, 3)]
        rows, called, _ = _check(rec, bc_len, umi_len, **MIN1)
        assert rows == [(0, 4, 3, 2, 0, 1), (top, 8, 3, 2, 1, 1)] and called == [0, top]


def test_rank_with_every_value_equal_and_with_ties_across_the_sort_blocks():
    rows, _, st = _check(kc.from_umis([3] * 300), **MIN1)
    assert st["distinct_values"] == 1 and [r[4] for r in rows] == list(range(300))
    rows, _, st = _check(kc.from_umis([1 + i % 2 for i in range(2600)]), **MIN1)                    # two-way ties; one bit is not enough, two are
    assert st["distinct_values"] == 2 and rows[1][4] == 0 and rows[0][4] == 1300
    rows, _, st = _check(kc.from_umis([1] * 2600), **MIN1)                                           # umis that need one bit
    assert [r[4] for r in rows] == list(range(2600))
    rows, _, st = _check(kc.from_umis([1 + (i * 7) % 5 for i in range(3000)]), **MIN1)              # many-way ties
    assert st["distinct_values"] == 5


def test_umis_that_need_twenty_bits():
    m = 2 ** 19 + 5
    arr = np.zeros(m + 4, pa.BUS_RECORD_DTYPE)
    arr["barcode"][:2], arr["barcode"][2:m + 2], arr["barcode"][m + 2:] = 3, 8, 9
    arr["umi"][:2], arr["umi"][2:m + 2], arr["umi"][m + 2:] = (0, 1), np.arange(m), (4, 4)
    arr["ec"][-1] = 1
    arr["count"] = 1
    rows, called, st = _gpu(arr, 4, 12, **MIN1)
    assert kc.rows_from_array(rows) == [(3, 2, 2, 2, 1, 1), (8, m, m, m, 0, 1), (9, 2, 2, 1, 2, 1)] and st["molecules"] == m + 3 and st["distinct_values"] == 3


def test_first_tile_of_the_second_grid_stride():
    arr, tab = kc.strided_case()
    assert len(arr) > kc.MAX_GRID * T and arr["barcode"][kc.MAX_GRID * T] != arr["barcode"][kc.MAX_GRID * T - 1]
    want_rows, want_called, want_st = km.knee_of_table(tab, len(arr), mode="min", min_umis=700)
    rows, called, st = _gpu(arr, mode="min", min_umis=700)
    assert st == want_st and called.tolist() == want_called and 0 < len(want_called) < len(want_rows)
    assert kc.rows_from_array(rows) == want_rows


def _library():
    if "library" not in _cache:
        _cache["library"] = kc.cells_and_ambient(3, 12, 80, cell_umis=(60, 120), ambient_umis=(1, 4))
    return _cache["library"]


def test_each_mode_and_its_edges():
    rec, bc_len, umi_len = _library()
    top = max(r[3] for r in km.knee(rec)[0])
    rows, called, st = _check(rec, bc_len, umi_len)                                                   # the defaults: the curve's knee
    assert st["barcodes_called"] == 12 and st["values_above_lower"] >= 3
    _, called, st = _check(rec, bc_len, umi_len, lower=top + 1)                                       # above every value: nothing is called, an empty list is legal
    assert called == [] and st["threshold"] == top + 1 and st["values_above_lower"] == 0
    _check(rec, bc_len, umi_len, lower=1, divisor=1)
    _, called, st = _check(rec, bc_len, umi_len, mode="expected", expected_cells=100 * 92 + 50)       # rank 92 is beyond the 92 rows: the last row's
    assert st["threshold"] == 1 and len(called) == 92
    _, called, st = _check(rec, bc_len, umi_len, mode="expected", expected_cells=1100)                # rank 11: the weakest of the twelve cells
    assert len(called) == 12 and st["threshold"] >= 6
    _, called, st = _check(rec, bc_len, umi_len, mode="min", min_umis=top + 1)
    assert called == [] and st["molecules_called"] == 0
    _, called, st = _check(rec, bc_len, umi_len, mode="min", min_umis=top)
    assert len(called) >= 1


def test_caps_and_null_outputs():
    rec, bc_len, umi_len = _library()
    want_rows, want_called, want_st = km.knee(rec)
    arr, al, lib = kc.to_array(rec), _setup()[1], pa.lib()
    nr, nc, st = C.c_uint64(), C.c_uint64(), np.zeros(10, np.uint64)
    rows, called = np.zeros(len(want_rows), pa.BARCODE_ROW_DTYPE), np.zeros(len(want_called), np.uint64)
    call = lambda r, rcap, c, ccap, s=st: lib.pa_bus_knee_records(al._h, arr.ctypes.data, len(arr), bc_len, umi_len, None, r, rcap, C.byref(nr), c, ccap, C.byref(nc),
                                                                 s.ctypes.data if s is not None else None)
    assert call(None, 0, None, 0) == 0 and (nr.value, nc.value) == (len(want_rows), len(want_called)) and st.tolist() == list(want_st.values())
    assert call(rows.ctypes.data, len(rows) - 1, called.ctypes.data, len(called)) == pa._ffi.PA_ERR_BUFFER_TOO_SMALL and (nr.value, nc.value) == (len(rows), len(called))
    assert call(rows.ctypes.data, len(rows), called.ctypes.data, len(called) - 1) == pa._ffi.PA_ERR_BUFFER_TOO_SMALL and (nr.value, nc.value) == (len(rows), len(called))
    assert call(rows.ctypes.data, len(rows), None, 0, None) == 0 and kc.rows_from_array(rows) == want_rows                  # only the rows, no stats
    assert call(None, 0, called.ctypes.data, len(called)) == 0 and called.tolist() == want_called                           # only the called list


def test_two_runs_and_a_shuffled_construction_give_the_same_bytes():
    rec, bc_len, umi_len = _library()
    a = _gpu(kc.to_array(rec), bc_len, umi_len)
    b = _gpu(kc.to_array(rec), bc_len, umi_len)
    rng = np.random.default_rng(0)
    shuffled = [rec[i] for i in rng.permutation(len(rec))]
    c = _gpu(kc.to_array(sorted(shuffled)), bc_len, umi_len)
    for x in (b, c):
        assert a[0].tobytes() == x[0].tobytes() and a[1].tobytes() == x[1].tobytes() and a[2] == x[2]
    assert set(pa.bus_knee_phase_ms()) == set(pa._ffi.KNEE_PHASE_NAMES)


# ---- pa_bus_keep_records ----
def _keep(rec, barcodes, bc_len=BC, umi_len=UMI):
    want, want_st = km.keep(rec, barcodes)
    out, st = pa.bus_keep(kc.to_array(rec), np.array(barcodes, np.uint64), bc_len, umi_len, _setup()[1])
    assert st == want_st and kc.from_array(out) == want
    assert all(a < b for a, b in zip(want, want[1:]))                                  # strictly ascending as they lie
    return want, st


def test_keep_lists():
    rec, bc_len, umi_len = _library()
    present = sorted({r[0] for r in rec})
    out, st = _keep(rec, [], bc_len, umi_len)
    assert out == [] and st["listed_absent"] == 0 and st["barcodes_in"] == len(present)
    out, st = _keep(rec, present, bc_len, umi_len)
    assert out == rec and st["barcodes_kept"] == len(present)
    absent = sorted(set(range(0, 4 ** bc_len, 4 ** bc_len // 37)) - set(present))
    out, st = _keep(rec, sorted(present[::3] + absent), bc_len, umi_len)               # listed barcodes that occur nowhere
    assert st["listed_absent"] == len(absent) and st["barcodes_kept"] == len(present[::3])
    out, st = _keep(rec, [present[0], present[-1]], bc_len, umi_len)                   # the first and the last barcode only
    assert out[0] == rec[0] and out[-1] == rec[-1] and st["barcodes_kept"] == 2
    out, st = _keep(rec, absent, bc_len, umi_len)
    assert out == [] and st["listed_absent"] == len(absent)
    assert _keep([], [1, 2], bc_len, umi_len)[1]["listed_absent"] == 2


@pytest.mark.parametrize("seam", [64, 256, T])
def test_keep_survivors_across_a_seam(seam):
    n = seam + 70
    rec = kc.from_heads(n, [seam - 40, seam - 1, seam, seam + 1, seam + 30], range(0, n, 3))
    barcodes = sorted({r[0] for r in rec})
    assert len(barcodes) == 6
    for listed in (barcodes[::2], barcodes[1::2], barcodes[2:4], barcodes[:1], barcodes[-1:]):
        _keep(rec, listed)
    rec = kc.from_heads(n, range(n), [])                                               # every record its own barcode, every other one kept
    _keep(rec, sorted({r[0] for r in rec})[::2])


def test_keep_refuses_an_unsorted_or_duplicate_list():
    rec, bc_len, umi_len = _library()
    present = sorted({r[0] for r in rec})
    for bad, at in ((present[:5] + [present[3]], 5), ([present[1], present[0]], 1), (present[:3] + [present[2]] + present[3:], 3), ([4 ** bc_len], 0)):
        with pytest.raises(pa.PaError) as e:
            pa.bus_keep(kc.to_array(rec), np.array(bad, np.uint64), bc_len, umi_len, _setup()[1])
        assert e.value.code == pa._ffi.PA_ERR_INVALID_ARG and "entry %d:" % at in str(e.value) and km.check_list(bad, bc_len) == at


# ---- on a writer ----
def _writer(rec, bc_len, umi_len):
    import test_gpu_correct_edges as tce
    return tce._writer(rec, bc_len, umi_len)


def _writer_case():
    """40 barcodes of 1 .. 6 molecules over the two one-id classes"""
    rng = np.random.default_rng(8)
    rec = []
    for b in sorted(int(x) for x in rng.choice(4 ** 8, 40, replace=False)):
        for u in sorted(int(x) for x in rng.choice(4 ** 6, int(rng.integers(1, 7)), replace=False)):
            for ec in ((0,), (1,), (0, 1))[int(rng.integers(0, 3))]:
                rec.append((b, u, ec, int(rng.integers(1, 4))))
    return rec, 8, 6


def test_writer_knee_leaves_the_records_and_keep_works_in_place():
    rec, bc_len, umi_len = _writer_case()
    writer, held = _writer(rec, bc_len, umi_len)
    want_rows, want_called, want_st = km.knee(held, mode="min", min_umis=3)
    rows, called, st = writer.knee(mode="min", min_umis=3)
    assert st == want_st and kc.rows_from_array(rows) == want_rows and called.tolist() == want_called and 0 < len(want_called) < len(want_rows)
    assert bm.records_from_array(writer.records()) == held                              # the writer is unchanged
    a, _, a_st = pa.bus_knee(kc.to_array(held), bc_len, umi_len, _setup()[1], mode="min", min_umis=3)
    assert a.tobytes() == rows.tobytes() and a_st == st
    want_out, want_keep = km.keep(held, want_called)
    ks = writer.keep(called)
    assert ks == want_keep and bm.records_from_array(writer.records()) == want_out
    assert writer.finish()[0] == len(want_out) == writer.stats()["records"]
    again = writer.keep(called)                                                         # a second keep with the same list changes nothing
    assert again["records_in"] == again["records_out"] == len(want_out) and again["listed_absent"] == 0 and again["barcodes_kept"] == again["barcodes_in"]
    assert bm.records_from_array(writer.records()) == want_out
    none = writer.keep([])
    assert none["records_out"] == 0 and writer.finish()[0] == 0 and len(writer.records()) == 0
    assert writer.keep([5])["listed_absent"] == 1 and writer.knee()[2]["barcodes"] == 0


def test_failing_call_leaves_the_writer_as_it_was():
    rec, bc_len, umi_len = _writer_case()
    writer, held = _writer(rec, bc_len, umi_len)
    present = sorted({r[0] for r in held})
    with pytest.raises(pa.PaError) as e:
        writer.keep(present[:4] + [present[2]])
    assert e.value.code == pa._ffi.PA_ERR_INVALID_ARG and "entry 4:" in str(e.value)
    with pytest.raises(pa.PaError) as e:
        writer.knee(lower=0)
    assert e.value.code == pa._ffi.PA_ERR_INVALID_ARG
    assert bm.records_from_array(writer.records()) == held and writer.stats()["records"] == len(held)
    fresh = pa.BusWriter(_setup()[1], _setup()[0], bc_len, umi_len)
    n = C.c_uint64()
    for call in (lambda: pa.lib().pa_bus_keep(fresh._h, None, 0, None), lambda: pa.lib().pa_bus_knee(fresh._h, None, None, 0, C.byref(n), None, 0, C.byref(n), None)):
        with pytest.raises(pa.PaError) as e:
            pa.check(call())                                                            # before pa_bus_finish
        assert e.value.code == pa._ffi.PA_ERR_INVALID_ARG
