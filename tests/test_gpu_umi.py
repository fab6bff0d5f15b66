"""The UMI correction end to end (pa_bus_umi_correct, pa_write_bus_umi, pa_count_cells_em_umi) on gencode_small: the cells and ambient barcodes of
tests/test_gpu_knee.py with some percent of the pairs given a copy whose UMI carries one substitution. A finished writer corrected in place against
tests/umi_model.py on the BUS model's records; what pa_bus_records, pa_bus_knee and the gene counter see afterwards; the two file-level calls
against the model fed with the oracle's mapping, alone and behind a whitelist plus cell calling (which pins the order of the steps). All integers
and bits: equality."""
import numpy as np
import pytest

import bus_model as bm
import correct_model as cm
import helpers
import knee_cases as kc
import knee_model as km
import umi_cases as uc
import umi_model as um

pa = helpers.pa
pytestmark = pytest.mark.gpu

BC, UMI = 16, 12
_cache = {}


def _gencode():
    if "gencode" not in _cache:
        host = pa.build_index(str(helpers.FASTA), 24, 8)
        ix = host.arrays()
        _, seqs = helpers.read_fasta()
        _cache["gencode"] = (host, pa.Pseudoaligner(host), helpers.Oracle(host), int(ix["num_transcripts"]), bm.index_classes(ix), seqs)
    return _cache["gencode"]


def _arrays(records, table):
    rec = np.array([(b, u, e, c, 0, 0) for b, u, e, c in records], pa.BUS_RECORD_DTYPE)
    off = np.cumsum([0] + [len(t) for t in table]).astype(np.uint64)
    ids = np.array([t for lst in table for t in lst], np.uint32)
    return rec, off, ids


def _umi(records, table, tx_gene, mode):
    rec, off, ids = _arrays(records, table)
    out, st = um.correct(rec, off, ids, tx_gene, UMI, mode, lds_cap=uc.UM_LDS_CAP)
    return bm.records_from_array(out), st


def _case():
    """the pairs, the BUS model's records of them and the models' answers: computed once and left unchanged"""
    if "case" not in _cache:
        host, al, oracle, T, classes, seqs = _gencode()
        case = uc.with_umi_errors(kc.make_pairs_case(17, seqs, BC, UMI), BC, UMI, 0.06, seed=5)
        mapping = bm.mapping_from_oracle(oracle, case["r2"])
        held, table, bus_st, _ = bm.model(case["r1"], mapping, T, classes, BC, UMI)
        tx_gene = host.genes()[0]
        plain = {mode: _umi(held, table, tx_gene, mode) for mode in ("greatest", "directional")}
        # not vacuous: error copies are merged in both modes, some molecules are kept apart by their genes, and the modes differ in what they see
        for mode in plain:
            st = plain[mode][1]
            assert st["molecules_moved"] > 100 and st["molecules_with_hamming1"] >= st["molecules_with_neighbour"] >= st["molecules_moved"] and st["records_out"] < st["records_in"]
        # whitelist + cell calling: corrected against the list, ranked, filtered; the UMI correction last
        packed = [cm.pack(w) for w in case["whitelist"]]
        fixed, correct_st, _ = cm.correct(held, packed, BC, UMI)
        rows, called, knee_st = km.knee(fixed)
        kept, _ = km.keep(fixed, called)
        out, umi_st = _umi(kept, table, tx_gene, "greatest")
        assert called == [cm.pack(c) for c in case["cells"]] and umi_st["molecules_moved"] > 100 and umi_st["barcodes"] == 30
        # ... and not first: the knee's table counts the molecules before UMI correction
        rows_after, _, _ = km.knee(cm.correct(plain["greatest"][0], packed, BC, UMI)[0])
        assert rows_after != rows
        _cache["case"] = (case, held, table, bus_st, plain, dict(rows=rows, correct=correct_st, knee=knee_st, out=out, umi=umi_st))
    return _cache["case"]


def _writer():
    import test_gpu_bus as tb
    host, al, *_ = _gencode()
    case = _case()[0]
    n = len(case["r1"])
    return tb.gpu_bus(al, host, case["r1"], case["r2"], BC, UMI, cuts=(n // 3,))


@pytest.mark.parametrize("mode", ["greatest", "directional"])
def test_writer_in_place_equals_the_model(mode):
    host, al, *_ = _gencode()
    case, held, table, bus_st, plain, _ = _case()
    want, want_st = plain[mode]
    tx_gene, gene_names = host.genes()
    writer = _writer()
    assert bm.records_from_array(writer.records()) == held
    before = writer.records().tobytes()
    bad = tx_gene.copy()
    bad[len(bad) // 2] = len(gene_names)
    with pytest.raises(pa.PaError) as e:
        writer.umi_correct(bad, mode, num_genes=len(gene_names))
    assert e.value.code == pa._ffi.PA_ERR_INVALID_ARG and "tx_gene[%d]" % (len(bad) // 2) in str(e.value)
    assert writer.records().tobytes() == before                                         # a failing call leaves the writer as it was
    with pytest.raises(pa.PaError) as e:
        writer.umi_correct(mode=7)
    assert e.value.code == pa._ffi.PA_ERR_INVALID_ARG and writer.records().tobytes() == before
    st = writer.umi_correct(mode=mode) if mode == "greatest" else writer.umi_correct(tx_gene, mode, num_genes=len(gene_names))
    assert st == want_st
    assert bm.records_from_array(writer.records()) == want
    assert bm.table_from_csr(*writer.ecs()) == table                                    # the ec table is untouched
    assert writer.finish() == (len(want), len(table)) and writer.stats()["records"] == len(want)
    rows, called, knee_st = writer.knee()                                               # the knee and the gene counter see the new records
    want_rows, want_called, want_knee = km.knee(want)
    assert kc.rows_from_array(rows) == want_rows and called.tolist() == want_called and knee_st == want_knee and knee_st["molecules"] == want_st["molecules_out"]
    g1 = pa.GeneCounter.from_bus(writer, tx_gene, len(gene_names))
    g2 = pa.GeneCounter.from_arrays(al, *_arrays(want, table), tx_gene, len(gene_names), BC, UMI)
    assert g1.run() == g2.run() and g1.stats() == g2.stats() and g1.stats()["molecules"] == want_st["molecules_out"]
    for a, b in zip(g1.values() + g1.matrix(), g2.values() + g2.matrix()):
        assert a.tobytes() == b.tobytes()
    out, st2 = pa.bus_umi_correct(*_arrays(held, table), tx_gene, len(gene_names), BC, UMI, al, mode=mode)
    assert st2 == want_st and bm.records_from_array(out) == want                         # the array route, the same bytes


def test_before_finish_is_refused():
    host, al, *_ = _gencode()
    tx_gene, gene_names = host.genes()
    writer = pa.BusWriter(al, host, BC, UMI)
    st = np.zeros(15, np.uint64)
    assert pa.lib().pa_bus_umi_correct(writer._h, tx_gene.ctypes.data, len(gene_names), 0, st.ctypes.data) == pa._ffi.PA_ERR_INVALID_ARG
    assert "pa_bus_finish" in pa.lib().pa_last_error().decode()
    assert pa.lib().pa_bus_umi_correct(None, tx_gene.ctypes.data, len(gene_names), 0, st.ctypes.data) == pa._ffi.PA_ERR_INVALID_ARG


def _fastq(ids, seqs):
    return "".join("@%s extra\n%s\n+\n%s\n" % (i, s, "I" * len(s)) for i, s in zip(ids, seqs)).encode()


def _files(tmp_path):
    case = _case()[0]
    names = ["read%d" % i for i in range(len(case["r1"]))]
    p1, p2, wl = tmp_path / "r1.fq", tmp_path / "r2.fq", tmp_path / "whitelist.txt"
    p1.write_bytes(_fastq([i + "/1" for i in names], case["r1"]))
    p2.write_bytes(_fastq([i + "/2" for i in names], case["r2"]))
    wl.write_text("".join(w + "\n" for w in case["whitelist"]))
    return p1, p2, wl


@pytest.mark.parametrize("mode", ["greatest", "directional"])
def test_from_fastq_equals_the_model_fed_with_the_oracles_mapping(mode, tmp_path):
    host, al, *_ = _gencode()
    case, held, table, bus_st, plain, _ = _case()
    want, want_st = plain[mode]
    tx_gene, gene_names = host.genes()
    p1, p2, _ = _files(tmp_path)
    out_bus, out_em, ref = tmp_path / "bus", tmp_path / "em", tmp_path / "ref"
    for d in (out_bus, out_em, ref):
        d.mkdir()
    st = al.write_bus(host, p1, p2, out_bus, BC, UMI, num_threads=4, umi_correct=mode)
    assert st.pop("umi") == want_st and st == dict(bus_st, records=len(want)) and "correct" not in st and "knee" not in st
    assert (out_bus / "output.bus").read_bytes() == bm.bus_bytes(want, BC, UMI)
    assert (out_bus / "matrix.ec").read_text() == bm.matrix_ec_text(table) and not (out_bus / "barcode_ranks.tsv").exists()
    g = pa.GeneCounter.from_arrays(al, *_arrays(want, table), tx_gene, len(gene_names), BC, UMI)
    g.run()
    g.write(host, ref)
    st = al.count_cells_em(host, p1, p2, out_em, BC, UMI, num_threads=4, umi_correct=mode)
    assert st.pop("umi") == want_st and st == g.stats()
    for name in ("matrix.mtx", "barcodes.tsv", "features.tsv"):
        assert (out_em / name).read_bytes() == (ref / name).read_bytes(), name
    with pytest.raises(ValueError):
        al.write_bus(host, p1, p2, out_bus, BC, UMI, umi_correct="transitive")


def test_from_fastq_behind_a_whitelist_and_cell_calling(tmp_path):
    """correct(whitelist) -> knee -> keep(called) -> UMI correction: barcode_ranks.tsv shows the molecules before the UMI correction"""
    host, al, *_ = _gencode()
    case, held, table, bus_st, _, want = _case()
    tx_gene, gene_names = host.genes()
    p1, p2, wl = _files(tmp_path)
    out_bus, out_em, ref = tmp_path / "bus", tmp_path / "em", tmp_path / "ref"
    for d in (out_bus, out_em, ref):
        d.mkdir()
    st = al.write_bus(host, p1, p2, out_bus, BC, UMI, num_threads=4, whitelist=wl, call_cells=True, umi_correct="greatest")
    assert st.pop("umi") == want["umi"] and st.pop("correct") == want["correct"] and st.pop("knee") == want["knee"] and st == dict(bus_st, records=len(want["out"]))
    assert (out_bus / "output.bus").read_bytes() == bm.bus_bytes(want["out"], BC, UMI)
    assert (out_bus / "barcode_ranks.tsv").read_text() == km.ranks_tsv(want["rows"], BC)
    g = pa.GeneCounter.from_arrays(al, *_arrays(want["out"], table), tx_gene, len(gene_names), BC, UMI)
    g.run()
    g.write(host, ref)
    st = al.count_cells_em(host, p1, p2, out_em, BC, UMI, num_threads=4, whitelist=wl, call_cells=dict(mode="curve"), umi_correct="greatest")
    assert st.pop("umi") == want["umi"] and st.pop("correct") == want["correct"] and st.pop("knee") == want["knee"] and st == g.stats()
    for name in ("matrix.mtx", "barcodes.tsv", "features.tsv"):
        assert (out_em / name).read_bytes() == (ref / name).read_bytes(), name
    assert (out_em / "barcode_ranks.tsv").read_text() == km.ranks_tsv(want["rows"], BC)
    with pytest.raises(pa.PaError) as e:                                                 # an unknown mode is refused before a read is mapped
        pa.check(pa.lib().pa_write_bus_umi(al._h, host._h, str(p1).encode(), str(p2).encode(), None, BC, UMI, 0, None, 9, str(out_bus).encode(), 1, None, None, None, None))
    assert e.value.code == pa._ffi.PA_ERR_INVALID_ARG and "mode 9" in str(e.value)
