"""The BUS barcode correction end to end (pa_bus_correct, pa_write_bus_corrected, pa_count_cells_em_corrected) on gencode_small: 20 000 pairs whose
barcodes carry substitutions, a whitelist of the true cells among 2 000 others. The writer's records after correct() equal the model of
tests/correct_model.py on the BUS model's records; the gene counter on them equals the gene counter on the model's corrected records bit for
bit; the two file-level calls give the files of the array route, from plain and from BGZF input. All integers and bits: equality."""
import numpy as np
import pytest

import bgzf_cases
import bus_model as bm
import correct_cases as cc
import correct_model as cm
import helpers

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
    """the pairs, the BUS model's records of them, and the correction model's answer: computed once and left unchanged"""
    if "case" not in _cache:
        host, al, oracle, T, classes, seqs = _gencode()
        case = cc.make_pairs_case(41, seqs, BC, UMI)
        mapping = bm.mapping_from_oracle(oracle, case["r2"])
        held, table, bus_st, _ = bm.model(case["r1"], mapping, T, classes, BC, UMI)
        packed = [cm.pack(w) for w in case["whitelist"]]
        want, st, decided = cm.correct(held, packed, BC, UMI)
        # not vacuous: every rule is met, corrected records join their cells' own, and without correction there are strictly more cells
        assert st["barcodes_corrected"] > 200 and st["barcodes_none"] > 20 and st["barcodes_exact"] >= 140 and st["records_out"] < st["records_exact"] + st["records_corrected"]
        assert st["barcodes_out"] < st["barcodes_in"] and st["barcodes_out"] <= 150 and len(case["whitelist"]) > 2000
        _cache["case"] = (case, held, table, bus_st, packed, want, st)
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


def test_writer_correct_equals_the_model():
    case, held, table, bus_st, packed, want, want_st = _case()
    writer = _writer()
    assert bm.records_from_array(writer.records()) == held and writer.stats() == bus_st
    st = writer.correct(case["whitelist"])
    assert st == want_st
    assert bm.records_from_array(writer.records()) == want
    assert bm.table_from_csr(*writer.ecs()) == table                                    # the ec table is untouched
    assert writer.finish() == (len(want), len(table)) and writer.stats()["records"] == len(want)
    out, st2 = pa.bus_correct(_arrays(held, table)[0], np.array(packed, np.uint64), BC, UMI, _gencode()[1])
    assert st2 == want_st and out.tobytes() == writer.records().tobytes()


def test_gene_counter_after_correct_equals_the_array_route():
    host, al, *_ = _gencode()
    case, held, table, _, packed, want, _ = _case()
    tx_gene, gene_names = host.genes()
    writer = _writer()
    plain = pa.GeneCounter.from_bus(writer, tx_gene, len(gene_names))
    writer.correct(case["whitelist"])
    g1 = pa.GeneCounter.from_bus(writer, tx_gene, len(gene_names))
    g2 = pa.GeneCounter.from_arrays(al, *_arrays(want, table), tx_gene, len(gene_names), BC, UMI)
    assert g1.run() == g2.run()
    for a, b in zip(g1.values() + g1.matrix(), g2.values() + g2.matrix()):
        assert a.tobytes() == b.tobytes()
    assert g1.stats() == g2.stats() and g1.stats()["records"] == len(want)
    assert plain.layout()[0] > g1.layout()[0] > 100                                     # without correction: strictly more cells


def _fastq(ids, seqs):
    return "".join("@%s extra\n%s\n+\n%s\n" % (i, s, "I" * len(s)) for i, s in zip(ids, seqs)).encode()


@pytest.mark.parametrize("form", ["plain", "bgzf"])
def test_file_level_calls_give_the_files_of_the_array_route(form, tmp_path):
    host, al, *_ = _gencode()
    case, held, table, bus_st, packed, want, want_st = _case()
    tx_gene, gene_names = host.genes()
    names = ["read%d" % i for i in range(len(case["r1"]))]
    r1, r2 = _fastq([i + "/1" for i in names], case["r1"]), _fastq([i + "/2" for i in names], case["r2"])
    if form == "bgzf":
        r1, r2 = bgzf_cases.bgzf(r1, level=1), bgzf_cases.bgzf(r2, level=1)
    suffix = ".gz" if form == "bgzf" else ""
    p1, p2, wl = tmp_path / ("r1.fq" + suffix), tmp_path / ("r2.fq" + suffix), tmp_path / "whitelist.txt"
    p1.write_bytes(r1)
    p2.write_bytes(r2)
    wl.write_text("".join(w + "\n" for w in case["whitelist"]))
    out_bus, out_em, ref = tmp_path / "bus", tmp_path / "em", tmp_path / "ref"
    for d in (out_bus, out_em, ref):
        d.mkdir()
    st = al.write_bus(host, p1, p2, out_bus, BC, UMI, num_threads=4, whitelist=wl)
    assert st.pop("correct") == want_st and st == dict(bus_st, records=len(want))
    assert (out_bus / "output.bus").read_bytes() == bm.bus_bytes(want, BC, UMI)
    assert (out_bus / "matrix.ec").read_text() == bm.matrix_ec_text(table) and (out_bus / "transcripts.txt").read_text() == bm.transcripts_text(host.tx_names())
    g = pa.GeneCounter.from_arrays(al, *_arrays(want, table), tx_gene, len(gene_names), BC, UMI)
    g.run()
    g.write(host, ref)
    st = al.count_cells_em(host, p1, p2, out_em, BC, UMI, num_threads=4, whitelist=wl)
    assert st.pop("correct") == want_st and st == g.stats()
    for name in ("matrix.mtx", "barcodes.tsv", "features.tsv"):
        assert (out_em / name).read_bytes() == (ref / name).read_bytes(), name
    assert sorted(p.name for p in out_em.iterdir()) == ["barcodes.tsv", "features.tsv", "matrix.mtx"]
    # not vacuous: the same input without correction has strictly more cells
    plain = tmp_path / "plain"
    plain.mkdir()
    al.count_cells_em(host, p1, p2, plain, BC, UMI, num_threads=4)
    assert len((plain / "barcodes.tsv").read_text().splitlines()) > len((out_em / "barcodes.tsv").read_text().splitlines()) > 100


def test_file_level_calls_stop_at_sixteen_bases(tmp_path):
    host, al, *_ = _gencode()
    (tmp_path / "r.fq").write_bytes(_fastq(["a"], ["ACGT" * 10]))
    (tmp_path / "whitelist.txt").write_text("A" * 16 + "\n")
    for call in (lambda: al.write_bus(host, tmp_path / "r.fq", tmp_path / "r.fq", tmp_path, 17, 12, whitelist=tmp_path / "whitelist.txt"),
                 lambda: al.count_cells_em(host, tmp_path / "r.fq", tmp_path / "r.fq", tmp_path, 17, 12, whitelist=tmp_path / "whitelist.txt")):
        with pytest.raises(pa.PaError) as e:
            call()
        assert e.value.code == pa._ffi.PA_ERR_UNSUPPORTED and "16 bases" in str(e.value)
    st = al.write_bus(host, tmp_path / "r.fq", tmp_path / "r.fq", tmp_path, 17, 12)      # without a whitelist 17 bases are taken as before
    assert st["reads"] == 1
