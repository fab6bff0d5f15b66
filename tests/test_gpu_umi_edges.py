"""The UMI correction (pa_bus_umi_correct_records; csrc/bus_umi.hip) on hand-written records against the pure-Python model of tests/umi_model.py:
the records byte for byte and all fifteen stats, at every rule of the header and at the edges the kernels have branches and arithmetic for (the
three bins of the search, the two word widths, 64-bit sums, the directional threshold). All integers: equality, no tolerance."""
import ctypes as C

import numpy as np
import pytest

import helpers
import umi_cases as uc
import umi_model as um

pa = helpers.pa
pytestmark = pytest.mark.gpu

_cache = {}


def _aligner():
    if "al" not in _cache:
        host = pa.build_index(str(helpers.FASTA), 24, 8)
        _cache["al"] = (host, pa.Pseudoaligner(host))
        assert um.BUS_RECORD_DTYPE == pa.BUS_RECORD_DTYPE and um.STAT_NAMES == pa.UMI_STAT_NAMES and uc.thresholds_in_source() == dict(
            UM_BLOCK=256, UM_LANE_MAX=uc.UM_LANE_MAX, UM_LDS_CAP=uc.UM_LDS_CAP)
    return _cache["al"][1]


def _gpu(case, mode):
    rec, off, ids, tx_gene, num_genes, bc_len, umi_len = case
    return pa.bus_umi_correct(rec, off, ids, tx_gene, num_genes, bc_len, umi_len, _aligner(), mode=mode)


def _check(key, case, mode):
    """the GPU's records and stats equal the model's -> (records, stats)"""
    want, want_st = uc.model(key, case, mode)
    out, st = _gpu(case, mode)
    print(key, mode, st)
    assert st == want_st
    assert out.tobytes() == want.tobytes()
    assert st["molecules_moved"] <= st["molecules_with_neighbour"] <= st["molecules_with_hamming1"] <= st["molecules_in"] - st["molecules_inert"]
    assert st["records_out"] <= st["records_in"] and st["molecules_out"] <= st["molecules_in"]
    return out, st


@pytest.mark.parametrize("mode", ["greatest", "directional"])
@pytest.mark.parametrize("name", sorted(uc.HAND))
def test_hand_cases(name, mode):
    case, want, want_st = uc.hand(name)
    out, st = _check(name, case, mode)
    if mode == "greatest":
        assert out.tobytes() == want.tobytes() and all(st[k] == v for k, v in want_st.items()), (st, want_st)
    if name == "nothing_moves":
        assert out.tobytes() == case[0].tobytes() and pa.bus_umi_correct_phase_ms()["rewrite_ms"] >= 0.0


def test_chain_is_one_step_and_a_second_call_moves_again():
    case, want, _ = uc.hand("chain_not_transitive")
    out, st = _check("chain_not_transitive", case, "greatest")
    assert st["molecules_moved_onto_moved"] == 1 and out["umi"].tolist() == [um.pack("AAAC"), um.pack("AACC")]
    again = (out,) + tuple(case[1:])
    out2, st2 = _check("chain_again", again, "greatest")
    assert st2["molecules_moved"] == 1 and out2["umi"].tolist() == [um.pack("AACC")] and out2["count"].tolist() == [8]


def test_sums_are_64_bit_and_the_output_count_is_clamped():
    case, want, _ = uc.hand("n_beyond_32_bits")
    out, st = _check("n_beyond_32_bits", case, "greatest")
    assert set(out["umi"].tolist()) == {um.pack("AAAA")} and st["reads_moved"] == uc.BIG       # in 32 bits the two would tie and AAAA would move instead
    out, st = _check("clamped_sum", uc.hand("clamped_sum")[0], "greatest")
    assert out["count"].max() == uc.BIG and st["reads_in"] == uc.BIG + 16


@pytest.mark.parametrize("mode", ["greatest", "directional"])
def test_directional_threshold_edges(mode):
    case, left = uc.directional_case()
    out, _ = _check("directional_edges", case, mode)
    assert [set(out["umi"][out["barcode"] == b].tolist()) for b in range(6)] == left[mode]


@pytest.mark.parametrize("mode", ["greatest", "directional"])
@pytest.mark.parametrize("name", ["umi_len_1", "umi_len_16", "umi_len_17", "umi_len_31"])
def test_widths_and_first_and_last_base(name, mode):
    case = uc.cached("widths", uc.widths_cases)[name]
    out, st = _check(name, case, mode)
    if name == "umi_len_1":
        assert st["molecules_with_hamming1"] == 4 and (mode != "greatest" or out["umi"].tolist() == [1, 2])
    elif mode == "greatest":
        umi_len, t = case[6], 4 ** case[6] - 1
        assert case[0]["barcode"].max() == 4 ** case[5] - 1 and case[0]["umi"].max() == t
        top = out[out["barcode"] == out["barcode"].max()]
        assert int(top["count"][top["umi"] == t][0]) == 7 + 1 + 2 and um.pack("C" + "T" * (umi_len - 2) + "C") in top["umi"].tolist()   # first and last base joined, two bases not


@pytest.mark.parametrize("umi_len", [16, 17])
def test_bin_edges_for_both_word_widths(umi_len):
    """one barcode of exactly UM_LANE_MAX, UM_LANE_MAX + 1, UM_LDS_CAP and UM_LDS_CAP + 1 molecules, each with neighbours at its first and last molecule"""
    case = uc.cached(("bins", umi_len), lambda: uc.bins_case(umi_len))
    out, st = _check(("bins", umi_len), case, "greatest")
    assert st["barcodes_hbm"] == 1 and st["largest_barcode"] == uc.UM_LDS_CAP + 1 and st["barcodes"] == 4
    _check(("bins", umi_len), case, "directional")


@pytest.mark.parametrize("umi_len", [16, 17])
def test_every_designed_barcode_alone_and_in_a_shuffled_batch(umi_len):
    """a barcode's output records depend on its own input records alone: the bin barcodes and the hand cases' barcodes, renumbered by a shuffle"""
    case = uc.cached(("bins", umi_len), lambda: uc.bins_case(umi_len))
    batch, _ = _check(("bins", umi_len), case, "greatest")
    rec = case[0]
    order = np.random.RandomState(3).permutation(np.unique(rec["barcode"]))
    renamed = rec.copy()
    for new, old in enumerate(order):                                          # the same barcodes under other numbers, so with other neighbours
        renamed["barcode"][rec["barcode"] == old] = 7 * new + 1
    shuffled = renamed[np.argsort(renamed["barcode"], kind="stable")]
    out_s, _ = _gpu((shuffled,) + tuple(case[1:]), "greatest")
    for new, old in enumerate(order):
        alone, st = _gpu(uc.one_barcode(case, old), "greatest")
        size = len(np.unique(rec["umi"][rec["barcode"] == old]))
        assert st["barcodes"] == 1 and st["largest_barcode"] == size and st["barcodes_hbm"] == (size > uc.UM_LDS_CAP) and st["molecules_with_neighbour"] >= 4
        assert alone.tobytes() == batch[batch["barcode"] == old].tobytes()
        again = out_s[out_s["barcode"] == 7 * new + 1].copy()
        again["barcode"] = old
        assert again.tobytes() == alone.tobytes()


def test_every_hand_barcode_alone_and_in_a_shuffled_batch():
    batch, where = uc.cached("hand_batch", uc.hand_batch)
    out, _ = _check("hand_batch", batch, "greatest")
    for name, old, new in where:
        case = uc.hand(name)[0]
        alone, _ = _gpu(uc.one_barcode(case, old), "greatest")
        got = out[out["barcode"] == new].copy()
        got["barcode"] = old
        assert uc.rows_of(batch, got) == uc.rows_of(case, alone), name


@pytest.mark.parametrize("mode", ["greatest", "directional"])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_cases(seed, mode):
    case = uc.cached(("random", seed), lambda: uc.random_case(seed))
    out, st = _check(("random", seed), case, mode)
    assert st["molecules_moved"] > 50 and st["molecules_inert"] > 0 and st["molecules_with_hamming1"] > st["molecules_with_neighbour"] > st["molecules_moved"]
    again, st2 = _gpu(case, mode)
    assert again.tobytes() == out.tobytes() and st2 == st                      # two runs, the same bytes


def test_empty_out_null_small_cap_and_refusals_on_the_device():
    al = _aligner()
    case, want, _ = uc.hand("clamped_sum")
    rec, off, ids, tx_gene, num_genes, bc_len, umi_len = case
    out, st = pa.bus_umi_correct(rec[:0], off, ids, tx_gene, num_genes, bc_len, umi_len, al)
    assert len(out) == 0 and not any(st.values())
    n, stats = C.c_uint64(), np.zeros(15, np.uint64)
    call = lambda out_ptr, cap, mode=0: pa.lib().pa_bus_umi_correct_records(al._h, rec.ctypes.data, len(rec), off.ctypes.data, ids.ctypes.data, len(off) - 1, len(tx_gene),
                                                                           tx_gene.ctypes.data, num_genes, bc_len, umi_len, mode, out_ptr, cap, C.byref(n), stats.ctypes.data)
    assert call(None, 0) == 0 and n.value == len(want) and stats[11] == len(want)
    buf = np.zeros(len(want), pa.BUS_RECORD_DTYPE)
    assert call(buf.ctypes.data, len(want) - 1) == pa._ffi.PA_ERR_BUFFER_TOO_SMALL and n.value == len(want)
    assert call(buf.ctypes.data, len(want)) == 0 and buf.tobytes() == want.tobytes()
    assert call(buf.ctypes.data, len(want), mode=2) == pa._ffi.PA_ERR_INVALID_ARG and n.value == 0
    with pytest.raises(pa.PaError) as e:
        pa.bus_umi_correct(rec, off, ids, tx_gene, num_genes, bc_len, umi_len, None)
    assert e.value.code == pa._ffi.PA_ERR_INVALID_ARG                          # a valid call without an index handle
