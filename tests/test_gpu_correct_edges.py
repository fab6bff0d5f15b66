"""The BUS barcode correction (pa_bus_correct_records, pa_bus_correct; csrc/bus_correct.hip) on hand-written records against the pure-Python
model of tests/correct_model.py: the records byte for byte and all thirteen stats, at the edges the kernels have branches and arithmetic
for. All integers: equality, no tolerance."""
import numpy as np
import pytest

import bus_model as bm
import correct_cases as cc
import correct_model as cm
import helpers

pa = helpers.pa
pytestmark = pytest.mark.gpu

_cache = {}


def _setup():
    if "ix" not in _cache:
        host = pa.build_index(str(helpers.FASTA), 24, 8)
        _cache["ix"] = (host, pa.Pseudoaligner(host), host.arrays())
        assert bm.RECORD_DTYPE == pa.BUS_RECORD_DTYPE and cm.STAT_NAMES == pa.CORRECT_STAT_NAMES
    return _cache["ix"]


def _gpu(rec, wl, bc_len, umi_len):
    out, st = pa.bus_correct(cc.to_array(rec), np.array(wl, np.uint64), bc_len, umi_len, _setup()[1])
    return out, st


def _check(rec, wl, bc_len, umi_len):
    """the GPU result equals the model's; -> (records out, stats, the model's decisions)"""
    want, want_st, decided = cm.correct(rec, wl, bc_len, umi_len)
    out, st = _gpu(rec, wl, bc_len, umi_len)
    assert st == want_st
    assert cc.from_array(out) == want
    return want, want_st, decided


@pytest.mark.parametrize("name", sorted(cc.HAND))
def test_hand_cases(name):
    rec, wl, bc_len, umi_len, want, _ = cc.HAND[name]
    got, _, _ = _check(rec, wl, bc_len, umi_len)
    assert got == want


@pytest.mark.parametrize("bc_len,umi_len", [(31, 1), (16, 12), (16, 16)])
def test_long_barcodes_first_and_last_base(bc_len, umi_len):
    rec, wl, _, _ = cc.long_barcode_case(bc_len, umi_len)
    _, st, _ = _check(rec, wl, bc_len, umi_len)
    assert (st["barcodes_exact"], st["barcodes_corrected"], st["barcodes_none"]) == (1, 3, 1)


def test_out_null_counts_only_and_small_cap():
    import ctypes as C
    rec, wl, bc_len, umi_len, want, _ = cc.HAND["merges"]
    arr, w = cc.to_array(rec), np.array(wl, np.uint64)
    n, st = C.c_uint64(), np.zeros(13, np.uint64)
    al = _setup()[1]
    assert pa.lib().pa_bus_correct_records(al._h, arr.ctypes.data, len(arr), bc_len, umi_len, w.ctypes.data, len(w), None, 0, C.byref(n), st.ctypes.data) == 0
    assert n.value == len(want) and int(st[11]) == len(want)
    out = np.zeros(len(want), pa.BUS_RECORD_DTYPE)
    rc = pa.lib().pa_bus_correct_records(al._h, arr.ctypes.data, len(arr), bc_len, umi_len, w.ctypes.data, len(w), out.ctypes.data, len(want) - 1, C.byref(n), None)
    assert rc == pa._ffi.PA_ERR_BUFFER_TOO_SMALL and n.value == len(want)


@pytest.mark.parametrize("n_whitelist", [1, 2, 64, 65, 1024, 1025])
def test_whitelist_sizes_across_a_capacity_step(n_whitelist):
    """n_whitelist = 2^k fills the table to a half, 2^k + 1 doubles it"""
    assert cc.capacity(64) * 2 == cc.capacity(65) and cc.capacity(1024) * 2 == cc.capacity(1025)
    rec, wl, bc_len, umi_len = cc.sized_case(n_whitelist, min(n_whitelist, 40), 25, 10, n_whitelist=n_whitelist)
    assert len(wl) == n_whitelist
    _check(rec, wl, bc_len, umi_len)


def test_wrap_whitelist():
    rec, wl, bc_len, umi_len = cc.wrap_case()
    _, st, decided = _check(rec, wl, bc_len, umi_len)
    assert st["barcodes_exact"] == len(wl) and {t for k, t in decided.values() if k == "corrected"} >= set(wl[:2])   # both keys of the last slot are found as targets


@pytest.mark.parametrize("distinct", [63, 64, 65, 255, 256, 257])
def test_distinct_barcode_counts_round_a_wave_and_a_block(distinct):
    rec, wl, bc_len, umi_len = cc.sized_case(distinct, distinct - 20, 12, 8)
    _, st, _ = _check(rec, wl, bc_len, umi_len)
    assert st["barcodes_in"] == distinct


@pytest.mark.parametrize("missed", [cc.GROUPS_PER_WAVE - 1, cc.GROUPS_PER_WAVE, cc.GROUPS_PER_WAVE + 1, cc.GROUPS_PER_BLOCK - 1, cc.GROUPS_PER_BLOCK, cc.GROUPS_PER_BLOCK + 1])
def test_miss_list_sizes_round_a_wave_and_a_block_of_groups(missed):
    rec, wl, bc_len, umi_len = cc.sized_case(100 + missed, 30, missed - 1, 1)
    _, st, _ = _check(rec, wl, bc_len, umi_len)
    assert st["barcodes_in"] - st["barcodes_exact"] == missed


def test_sort_free_path_against_one_corrected_barcode_added():
    """nothing corrected: the kept records are written as they lie; with one corrected barcode added the sort and the collapse run"""
    rec, wl, bc_len, umi_len = cc.sized_case(9, 50, 0, 30)
    rec = [r for r in rec if cm.decide(r[0], set(wl), bc_len)[0] != "corrected"]
    want, st, _ = _check(rec, wl, bc_len, umi_len)
    assert st["barcodes_corrected"] == 0 and st["records_dropped"] > 0 and want == [r for r in rec if r[0] in set(wl)]
    target = want[0][0]
    moved = cc.sub(target, bc_len, 4, 2)
    assert cm.decide(moved, set(wl), bc_len) == ("corrected", target)
    more = sorted(rec + [(moved, want[0][1], want[0][2], 7), (moved, 31, 1, 2)])
    want2, st2, _ = _check(more, wl, bc_len, umi_len)
    assert st2["barcodes_corrected"] == 1 and len(want2) == len(want) + 1 and want2[0][3] == want[0][3] + 7


def test_two_runs_and_a_shuffled_whitelist_give_the_same_bytes():
    rec, wl, bc_len, umi_len = cc.sized_case(21, 150, 120, 40)
    a, st_a = _gpu(rec, wl, bc_len, umi_len)
    b, st_b = _gpu(rec, wl, bc_len, umi_len)
    rng = np.random.default_rng(0)
    c, st_c = _gpu(rec, [wl[i] for i in rng.permutation(len(wl))], bc_len, umi_len)
    assert a.tobytes() == b.tobytes() == c.tobytes() and st_a == st_b == st_c
    assert cc.from_array(a) == cm.correct(rec, wl, bc_len, umi_len)[0]


def _writer(rec, bc_len, umi_len):
    """a finished BusWriter that holds `rec` (ec = 0 / 1 -> the transcripts of the index's first two one-id classes)"""
    import torch
    host, al, ix = _setup()
    single = bm.singleton_classes(ix)[:2]
    reads = [(cm.unpack(b, bc_len) + cm.unpack(u, umi_len), single[ec][0], n) for b, u, ec, n in rec]
    r1, results, arena, _ = bm.directed(reads, ix, 1)
    writer = pa.BusWriter(al, host, bc_len, umi_len)
    text, off = pa.concat_reads(r1)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).cuda()
    d = [up(results), up(arena), up(np.concatenate([text, np.zeros(8, np.uint8)])), up(off)]
    torch.cuda.synchronize()
    writer.add_device(d[0].data_ptr(), d[1].data_ptr(), len(arena), d[2].data_ptr(), d[3].data_ptr(), len(r1))
    writer.finish()
    held = sorted((b, u, single[ec][1], n) for b, u, ec, n in rec)
    assert bm.records_from_array(writer.records()) == held
    return writer, held


def test_writer_correct_equals_the_array_call_and_a_second_one_is_the_identity(tmp_path):
    rec, wl, bc_len, umi_len = cc.sized_case(33, 60, 50, 20)
    writer, held = _writer(rec, bc_len, umi_len)
    want, want_st = pa.bus_correct(cc.to_array(held), np.array(wl, np.uint64), bc_len, umi_len, _setup()[1])
    assert cc.from_array(want) == cm.correct(held, wl, bc_len, umi_len)[0] and want_st["barcodes_corrected"] >= 50
    st = writer.correct(np.array(wl, np.uint64))
    assert st == want_st
    got = writer.records()
    assert got.tobytes() == want.tobytes()
    assert writer.finish()[0] == len(want) == writer.stats()["records"]
    writer.write(tmp_path)
    assert bm.read_bus((tmp_path / "output.bus").read_bytes())[3] == cc.from_array(want)
    again = writer.correct([cm.unpack(w, bc_len) for w in wl])                  # the whitelist as strings
    assert again["barcodes_exact"] == again["barcodes_in"] == st["barcodes_out"] and again["records_out"] == again["records_in"] == len(want)
    assert writer.records().tobytes() == want.tobytes()


def test_failing_call_leaves_the_writer_as_it_was():
    rec, wl, bc_len, umi_len = cc.sized_case(34, 20, 10, 5)
    writer, held = _writer(rec, bc_len, umi_len)
    with pytest.raises(pa.PaError) as e:
        writer.correct(np.array(wl + [wl[3]], np.uint64))
    assert e.value.code == pa._ffi.PA_ERR_INVALID_ARG and "entry 3:" in str(e.value)
    assert bm.records_from_array(writer.records()) == held and writer.stats()["records"] == len(held)
    fresh = pa.BusWriter(_setup()[1], _setup()[0], bc_len, umi_len)
    with pytest.raises(pa.PaError) as e:
        pa.check(pa.lib().pa_bus_correct(fresh._h, np.array(wl, np.uint64).ctypes.data, len(wl), None))   # before pa_bus_finish
    assert e.value.code == pa._ffi.PA_ERR_INVALID_ARG
