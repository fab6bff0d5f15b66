"""Cell calling end to end (pa_bus_knee, pa_bus_keep, pa_write_bus_called, pa_count_cells_em_called) on gencode_small: 30 simulated cells with many
molecules, 300 ambient barcodes with one to three, 1 % barcode substitutions. Both orders — no whitelist: knee -> correct(called); whitelist:
correct -> knee -> keep(called) — on a writer against tests/knee_model.py and tests/correct_model.py on the BUS model's records; the gene
counter on them against the gene counter on the model's records, bit for bit; the two file-level calls against the files of the array route
and the model's barcode_ranks.tsv, from plain and from BGZF input. All integers and bits: equality."""
import numpy as np
import pytest

import bgzf_cases
import bus_model as bm
import correct_model as cm
import helpers
import knee_cases as kc
import knee_model as km

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


def _case():
    """the pairs, the BUS model's records of them and the models' answers for both orders: computed once and left unchanged"""
    if "case" not in _cache:
        host, al, oracle, T, classes, seqs = _gencode()
        case = kc.make_pairs_case(17, seqs, BC, UMI)
        mapping = bm.mapping_from_oracle(oracle, case["r2"])
        held, table, bus_st, _ = bm.model(case["r1"], mapping, T, classes, BC, UMI)
        cells = [cm.pack(c) for c in case["cells"]]
        # no whitelist: the knee over everything, then the called barcodes as the whitelist of the correction
        kc.assert_clear(held, km.DEFAULTS["lower"])
        rows, called, knee_st = km.knee(held)
        out, correct_st, _ = cm.correct(held, called, BC, UMI)
        plain = dict(rows=rows, called=called, knee=knee_st, out=out, correct=correct_st)
        # not vacuous: exactly the cells are called, erroneous barcodes are rescued into them, the ambient ones are dropped
        assert called == cells and correct_st["barcodes_corrected"] > 20 and correct_st["barcodes_none"] > 250 and knee_st["barcodes"] > 350
        # whitelist: corrected against the list of possible barcodes (the ambient ones are on it), then ranked, then filtered
        packed = [cm.pack(w) for w in case["whitelist"]]
        fixed, correct_st, _ = cm.correct(held, packed, BC, UMI)
        kc.assert_clear(fixed, km.DEFAULTS["lower"])
        rows, called, knee_st = km.knee(fixed)
        out, keep_st = km.keep(fixed, called)
        listed = dict(packed=packed, fixed=fixed, rows=rows, called=called, knee=knee_st, out=out, correct=correct_st, keep=keep_st)
        assert called == cells and correct_st["barcodes_out"] > 300 and keep_st["barcodes_kept"] == 30 and 0 < keep_st["records_out"] < keep_st["records_in"]
        _cache["case"] = (case, held, table, bus_st, plain, listed)
    return _cache["case"]


def _writer():
    import test_gpu_bus as tb
    host, al, *_ = _gencode()
    case = _case()[0]
    n = len(case["r1"])
    return tb.gpu_bus(al, host, case["r1"], case["r2"], BC, UMI, cuts=(n // 3,))


def _arrays(records, table):
    rec = np.array([(b, u, e, c, 0, 0) for b, u, e, c in records], pa.BUS_RECORD_DTYPE)
    off = np.cumsum([0] + [len(t) for t in table]).astype(np.uint64)
    ids = np.array([t for lst in table for t in lst], np.uint32)
    return rec, off, ids


def _same_genes(writer, records, table):
    """the gene counter on the writer's records equals the gene counter on `records`, bit for bit"""
    host, al, *_ = _gencode()
    tx_gene, gene_names = host.genes()
    g1 = pa.GeneCounter.from_bus(writer, tx_gene, len(gene_names))
    g2 = pa.GeneCounter.from_arrays(al, *_arrays(records, table), tx_gene, len(gene_names), BC, UMI)
    assert g1.run() == g2.run()
    for a, b in zip(g1.values() + g1.matrix(), g2.values() + g2.matrix()):
        assert a.tobytes() == b.tobytes()
    assert g1.stats() == g2.stats() and g1.stats()["records"] == len(records)
    return g1


def test_knee_then_correct_on_a_writer_equals_the_models():
    case, held, table, bus_st, plain, _ = _case()
    writer = _writer()
    assert bm.records_from_array(writer.records()) == held and writer.stats() == bus_st
    rows, called, st = writer.knee()
    assert st == plain["knee"] and kc.rows_from_array(rows) == plain["rows"] and called.tolist() == plain["called"]
    assert writer.correct(called) == plain["correct"]
    assert bm.records_from_array(writer.records()) == plain["out"]
    assert bm.table_from_csr(*writer.ecs()) == table                                    # the ec table is untouched
    g = _same_genes(writer, plain["out"], table)
    assert g.layout()[0] == 30


def test_correct_then_knee_then_keep_on_a_writer_equals_the_models():
    case, held, table, bus_st, _, listed = _case()
    writer = _writer()
    assert writer.correct(np.array(listed["packed"], np.uint64)) == listed["correct"]
    rows, called, st = writer.knee()
    assert st == listed["knee"] and kc.rows_from_array(rows) == listed["rows"] and called.tolist() == listed["called"]
    assert bm.records_from_array(writer.records()) == listed["fixed"]
    assert writer.keep(called) == listed["keep"]
    assert bm.records_from_array(writer.records()) == listed["out"] and writer.finish() == (len(listed["out"]), len(table))
    assert bm.table_from_csr(*writer.ecs()) == table
    g = _same_genes(writer, listed["out"], table)
    assert g.layout()[0] == 30


def _fastq(ids, seqs):
    return "".join("@%s extra\n%s\n+\n%s\n" % (i, s, "I" * len(s)) for i, s in zip(ids, seqs)).encode()


def _files(tmp_path, form):
    case = _case()[0]
    names = ["read%d" % i for i in range(len(case["r1"]))]
    r1, r2 = _fastq([i + "/1" for i in names], case["r1"]), _fastq([i + "/2" for i in names], case["r2"])
    if form == "bgzf":
        r1, r2 = bgzf_cases.bgzf(r1, level=1), bgzf_cases.bgzf(r2, level=1)
    suffix = ".gz" if form == "bgzf" else ""
    p1, p2, wl = tmp_path / ("r1.fq" + suffix), tmp_path / ("r2.fq" + suffix), tmp_path / "whitelist.txt"
    p1.write_bytes(r1)
    p2.write_bytes(r2)
    wl.write_text("".join(w + "\n" for w in case["whitelist"]))
    return p1, p2, wl


@pytest.mark.parametrize("form", ["plain", "bgzf"])
@pytest.mark.parametrize("with_whitelist", [False, True])
def test_file_level_calls_give_the_files_of_the_array_route(form, with_whitelist, tmp_path):
    host, al, *_ = _gencode()
    case, held, table, bus_st, plain, listed = _case()
    want = listed if with_whitelist else plain
    tx_gene, gene_names = host.genes()
    p1, p2, wl = _files(tmp_path, form)
    out_bus, out_em, ref = tmp_path / "bus", tmp_path / "em", tmp_path / "ref"
    for d in (out_bus, out_em, ref):
        d.mkdir()
    kwargs = dict(whitelist=wl) if with_whitelist else {}
    st = al.write_bus(host, p1, p2, out_bus, BC, UMI, num_threads=4, call_cells=True, **kwargs)
    assert st.pop("correct") == want["correct"] and st.pop("knee") == want["knee"] and st == dict(bus_st, records=len(want["out"]))
    assert (out_bus / "output.bus").read_bytes() == bm.bus_bytes(want["out"], BC, UMI)
    assert (out_bus / "matrix.ec").read_text() == bm.matrix_ec_text(table) and (out_bus / "transcripts.txt").read_text() == bm.transcripts_text(host.tx_names())
    assert (out_bus / "barcode_ranks.tsv").read_text() == km.ranks_tsv(want["rows"], BC)
    g = pa.GeneCounter.from_arrays(al, *_arrays(want["out"], table), tx_gene, len(gene_names), BC, UMI)
    g.run()
    g.write(host, ref)
    st = al.count_cells_em(host, p1, p2, out_em, BC, UMI, num_threads=4, call_cells=dict(mode="curve"), **kwargs)
    assert st.pop("correct") == want["correct"] and st.pop("knee") == want["knee"] and st == g.stats()
    for name in ("matrix.mtx", "barcodes.tsv", "features.tsv"):
        assert (out_em / name).read_bytes() == (ref / name).read_bytes(), name
    assert (out_em / "barcode_ranks.tsv").read_text() == km.ranks_tsv(want["rows"], BC)
    assert sorted(p.name for p in out_em.iterdir()) == ["barcode_ranks.tsv", "barcodes.tsv", "features.tsv", "matrix.mtx"]
    assert (out_em / "barcodes.tsv").read_text().splitlines() == case["cells"]          # the filtered matrix: the thirty cells


def test_no_barcode_reaches_the_threshold_writes_nothing(tmp_path):
    host, al, *_ = _gencode()
    p1, p2, wl = _files(tmp_path, "plain")
    for call, kwargs in ((al.write_bus, {}), (al.write_bus, dict(whitelist=wl)), (al.count_cells_em, {}), (al.count_cells_em, dict(whitelist=wl))):
        out = tmp_path / ("out%d" % len(list(tmp_path.iterdir())))
        out.mkdir()
        with pytest.raises(pa.PaError) as e:
            call(host, p1, p2, out, BC, UMI, num_threads=4, call_cells=dict(mode="min", min_umis=100000), **kwargs)
        assert e.value.code == pa._ffi.PA_ERR_FORMAT and "no barcode reaches the threshold of 100000 molecules" in str(e.value)
        assert list(out.iterdir()) == []
    with pytest.raises(pa.PaError) as e:                                                 # bad params are refused before a read is mapped
        al.write_bus(host, p1, p2, tmp_path, BC, UMI, call_cells=dict(divisor=0))
    assert e.value.code == pa._ffi.PA_ERR_INVALID_ARG and "divisor" in str(e.value)


def test_without_call_cells_the_calls_are_the_ones_they_were(tmp_path):
    """write_bus / count_cells_em with call_cells left out give the bytes and stats of the entry points they called before (looked up through
    the library itself), with and without a whitelist file, and write no barcode_ranks.tsv"""
    host, al, *_ = _gencode()
    p1, p2, wl = _files(tmp_path, "plain")
    enc =lambda p: str(p).encode()
    for tag, kwargs in (("a", {}), ("b", dict(whitelist=wl))):
        new_bus, old_bus, new_em, old_em = (tmp_path / (tag + d) for d in ("new_bus", "old_bus", "new_em", "old_em"))
        for d in (new_bus, old_bus, new_em, old_em):
            d.mkdir()
        st = al.write_bus(host, p1, p2, new_bus, BC, UMI, num_threads=4, **kwargs)
        bst, cst, gst = np.zeros(pa._ffi.PA_BUS_STATS, np.uint64), np.zeros(pa._ffi.PA_BUS_CORRECT_STATS, np.uint64), np.zeros(pa._ffi.PA_GENES_STATS, np.uint64)
        if kwargs:
            pa.check(pa.lib().pa_write_bus_corrected(al._h, host._h, enc(p1), enc(p2), enc(wl), BC, UMI, enc(old_bus), 4, bst.ctypes.data, cst.ctypes.data))
            assert list(st.pop("correct").values()) == cst.tolist()
        else:
            pa.check(pa.lib().pa_write_bus(al._h, host._h, enc(p1), enc(p2), BC, UMI, enc(old_bus), 4, bst.ctypes.data))
        assert list(st.values()) == bst.tolist() and "knee" not in st
        st = al.count_cells_em(host, p1, p2, new_em, BC, UMI, num_threads=4, **kwargs)
        if kwargs:
            pa.check(pa.lib().pa_count_cells_em_corrected(al._h, host._h, enc(p1), enc(p2), enc(wl), BC, UMI, None, enc(old_em), 4, gst.ctypes.data, cst.ctypes.data))
            assert list(st.pop("correct").values()) == cst.tolist()
        else:
            pa.check(pa.lib().pa_count_cells_em(al._h, host._h, enc(p1), enc(p2), BC, UMI, None, enc(old_em), 4, gst.ctypes.data))
        assert list(st.values()) == gst.tolist() and "knee" not in st
        for new, old in ((new_bus, old_bus), (new_em, old_em)):
            assert sorted(p.name for p in new.iterdir()) == sorted(p.name for p in old.iterdir()) and "barcode_ranks.tsv" not in [p.name for p in new.iterdir()]
            for p in new.iterdir():
                assert p.read_bytes() == (old / p.name).read_bytes(), p.name
