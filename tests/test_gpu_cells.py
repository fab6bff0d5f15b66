"""Single-cell UMI counting on the GPU (pa_cell_counter, pa_count_cells) against the pure-Python model of tests/cells_model.py, with every
R2 mapped by the independent oracle on the model's side: matrix and all ten stats exactly, across barcode / UMI geometries, batch seams,
a (cell, gene) segment beyond one wave, the three output files byte for byte, and the error cases."""
import ctypes as C
import gzip

import numpy as np
import pytest

import cells_model as cm
import helpers

pa = helpers.pa
pytestmark = pytest.mark.gpu

_cache = {}


def _gencode():
    if "gencode" not in _cache:
        host = pa.build_index(str(helpers.FASTA), 24, 8)
        tx_gene, names = host.genes()
        _, seqs = helpers.read_fasta()
        _cache["gencode"] = (host, pa.Pseudoaligner(host), helpers.Oracle(host), np.asarray(tx_gene, np.uint32), names, seqs)
    return _cache["gencode"]


def _synthetic():
    """a synthesized transcriptome whose transcript -> gene map the test chooses (many multi-gene classes)"""
    if "synth" not in _cache:
        tx = pa.Txome.synthesize(120, 400, 11)
        host = pa.HostIndex.from_txome(tx, 24, 8)
        packed, tx_start = host.transcripts()
        seqs = ["".join("ACGT"[b] for b in helpers.unpack_bases(packed, int(tx_start[t + 1]))[int(tx_start[t]):])
                for t in range(len(tx_start) - 1)]
        tx_gene = ((np.arange(len(seqs)) // 4) % 60).astype(np.uint32)   # four neighbours to a gene: isoforms split across genes
        _cache["synth"] = (host, pa.Pseudoaligner(host), helpers.Oracle(host), tx_gene, int(tx_gene.max()) + 1, seqs)
    return _cache["synth"]


def gpu_count(al, host, tx_gene, num_genes, case, bc_len, umi_len, cuts=()):
    """the counter fed device-resident batches [0, cuts..., n): R2s mapped on the GPU, R1s uploaded as they are"""
    import torch
    dev = torch.device("cuda")
    counter = pa.CellCounter(al, host, tx_gene, num_genes, case["whitelist"], bc_len, umi_len)
    bounds = [0] + list(cuts) + [len(case["r1"])]
    for a, b in zip(bounds[:-1], bounds[1:]):
        m = b - a
        tiles, lens, wpr = pa.encode_reads_host(case["r2"][a:b])
        d_tiles = torch.from_numpy(tiles.view(np.int64)).to(dev)
        d_lens = torch.from_numpy(lens.view(np.int32)).to(dev)
        d_res = torch.empty(m * 4, dtype=torch.int32, device=dev)
        cap = al.arena_hint(m)
        for _ in range(3):
            d_arena = torch.empty(cap, dtype=torch.int32, device=dev)
            torch.cuda.synchronize()
            al.map_batch_device(d_tiles.data_ptr(), d_lens.data_ptr(), m, wpr, d_res.data_ptr(), d_arena.data_ptr(), cap)
            try:
                al.map_finish()
                break
            except pa.PaError as e:
                assert e.code == pa._ffi.PA_ERR_ARENA_FULL
                cap *= 4
        ascii, off = pa.concat_reads(case["r1"][a:b])
        d_r1 = torch.from_numpy(np.concatenate([ascii, np.zeros(8, np.uint8)])).to(dev)
        d_off = torch.from_numpy(off.view(np.int64)).to(dev)
        torch.cuda.synchronize()
        counter.add_device(d_res.data_ptr(), d_arena.data_ptr(), d_r1.data_ptr(), d_off.data_ptr(), m)
    cell, gene, umis = counter.matrix()
    matrix = list(zip(cell.tolist(), gene.tolist(), umis.tolist()))
    stats = counter.stats()
    with pytest.raises(pa.PaError) as e:   # finished: no more batches
        counter.add_device(d_res.data_ptr(), d_arena.data_ptr(), d_r1.data_ptr(), d_off.data_ptr(), 1)
    assert e.value.code == pa._ffi.PA_ERR_INVALID_ARG
    return matrix, stats


def check_stats(st):
    assert st["reads"] == st["barcode_invalid"] + st["umi_invalid"] + st["not_confidently_mapped"] + st["reads_counted"]
    assert st["barcode_exact"] + st["barcode_corrected"] == st["umi_invalid"] + st["not_confidently_mapped"] + st["reads_counted"]


@pytest.mark.parametrize("bc_len,umi_len", [(16, 12), (16, 10), (14, 12)])
def test_counter_equals_model(bc_len, umi_len):
    host, al, oracle, tx_gene, names, seqs = _gencode()
    case = cm.make_case(100 + bc_len + umi_len, seqs, tx_gene, bc_len, umi_len)
    want_m, want_s = cm.model_from_oracle(oracle, case, tx_gene, bc_len, umi_len)
    got_m, got_s = gpu_count(al, host, tx_gene, len(names), case, bc_len, umi_len)
    check_stats(want_s)
    for key in ("barcode_corrected", "barcode_invalid", "umi_invalid", "not_confidently_mapped", "umis_corrected", "molecules_lost_to_conflicts"):
        assert want_s[key] > 0, (key, want_s)   # every rule is exercised
    assert got_s == want_s
    assert got_m == want_m


def test_batches_and_a_large_segment():
    host, al, oracle, tx_gene, num_genes, seqs = _synthetic()
    case = cm.make_case(7, seqs, tx_gene, 16, 12, big_segment=160)
    want_m, want_s = cm.model_from_oracle(oracle, case, tx_gene, 16, 12)
    assert cm.largest_group > 64   # the large-segment path runs
    n = len(case["r1"])
    one = gpu_count(al, host, tx_gene, num_genes, case, 16, 12)
    three = gpu_count(al, host, tx_gene, num_genes, case, 16, 12, cuts=(n // 7, n // 2))
    rng = np.random.default_rng(1)
    seven = gpu_count(al, host, tx_gene, num_genes, case, 16, 12, cuts=sorted(rng.choice(np.arange(1, n), 6, replace=False).tolist()))
    assert one == (want_m, want_s)
    assert three == one and seven == one


def _fastq(ids, seqs, crlf=False):
    nl = "\r\n" if crlf else "\n"
    return "".join("@%s extra%s%s%s+%s%s%s" % (i, nl, s, nl, nl, "I" * len(s), nl) for i, s in zip(ids, seqs)).encode()


@pytest.mark.parametrize("form", ["plain", "crlf", "gzip"])
def test_count_cells_files(form, tmp_path):
    host, al, oracle, tx_gene, names, seqs = _gencode()
    case = cm.make_case(55, seqs, tx_gene, 16, 12, n_cells=120)
    want_m, want_s = cm.model_from_oracle(oracle, case, tx_gene, 16, 12)
    ids = ["read%d" % i for i in range(len(case["r1"]))]
    r1 = _fastq([i + "/1" for i in ids], case["r1"], crlf=form == "crlf")
    r2 = _fastq([i + "/2" for i in ids], case["r2"], crlf=form == "crlf")
    wl = ("\r\n" if form == "crlf" else "\n").join(case["whitelist"]).encode() + b"\n"
    suffix = ""
    if form == "gzip":
        r1, r2, wl, suffix = gzip.compress(r1), gzip.compress(r2), gzip.compress(wl), ".gz"
    for name, data in (("r1.fq", r1), ("r2.fq", r2), ("wl.txt", wl)):
        (tmp_path / (name + suffix)).write_bytes(data)
    out = tmp_path / "out"
    out.mkdir()
    st = al.count_cells(host, tmp_path / ("r1.fq" + suffix), tmp_path / ("r2.fq" + suffix), tmp_path / ("wl.txt" + suffix), out, 16, 12, num_threads=4)
    assert st == want_s
    mtx, bcs, feats = cm.render(want_m, case["whitelist"], names)
    assert (out / "matrix.mtx").read_text() == mtx
    assert (out / "barcodes.tsv").read_text() == bcs
    assert (out / "features.tsv").read_text() == feats


def test_count_cells_batch_seams(tmp_path, monkeypatch):
    """the file-level driver in small batches (the next batch read while the one before is on the GPU): same files"""
    host, al, oracle, tx_gene, names, seqs = _gencode()
    case = cm.make_case(56, seqs, tx_gene, 16, 12, n_cells=80)
    want_m, want_s = cm.model_from_oracle(oracle, case, tx_gene, 16, 12)
    ids = ["r%d" % i for i in range(len(case["r1"]))]
    (tmp_path / "r1.fq").write_bytes(_fastq(ids, case["r1"]))
    (tmp_path / "r2.fq").write_bytes(_fastq(ids, case["r2"]))
    (tmp_path / "wl.txt").write_text("\n".join(case["whitelist"]) + "\n")
    monkeypatch.setenv("PA_INGEST_BATCH", "333")
    st = al.count_cells(host, tmp_path / "r1.fq", tmp_path / "r2.fq", tmp_path / "wl.txt", tmp_path, 16, 12, num_threads=3)
    assert st == want_s
    assert (tmp_path / "matrix.mtx").read_text() == cm.render(want_m, case["whitelist"], names)[0]


def test_error_cases(tmp_path):
    host, al, oracle, tx_gene, names, seqs = _gencode()
    r1 = ["ACGTACGTACGTACGT" + "AAAACCCCGGGG"] * 3
    r2 = [seqs[0][:90]] * 3
    wl = tmp_path / "wl.txt"
    wl.write_text("ACGTACGTACGTACGT\nTTTTTTTTTTTTTTTT\n")
    (tmp_path / "r1.fq").write_bytes(_fastq(["a", "b", "c"], r1))

    def run(r2_ids, r2_seqs, whitelist=wl):
        (tmp_path / "r2.fq").write_bytes(_fastq(r2_ids, r2_seqs))
        with pytest.raises(pa.PaError) as e:
            al.count_cells(host, tmp_path / "r1.fq", tmp_path / "r2.fq", whitelist, tmp_path, 16, 12)
        return e.value

    e = run(["a", "b"], r2[:2])
    assert e.code == pa._ffi.PA_ERR_FORMAT and "record 2" in str(e)
    e = run(["a", "x", "c"], r2)
    assert e.code == pa._ffi.PA_ERR_FORMAT and "record 1" in str(e)
    bad = tmp_path / "bad.txt"
    bad.write_text("ACGTACGTACGTACGT\nTTTTTTTTTTTTTTTT\nACGTACGTACGTACGT\n")
    e = run(["a", "b", "c"], r2, bad)
    assert e.code == pa._ffi.PA_ERR_FORMAT and "line 3" in str(e)
    bad.write_text("ACGTACGTACGTACGT\nTTTTTTTTTTTTTTT\n")
    e = run(["a", "b", "c"], r2, bad)
    assert e.code == pa._ffi.PA_ERR_FORMAT and "line 2" in str(e)
    # the key budget: 2 cell bits + 31 gene bits + 32 UMI bits > 64; at exactly 64 the counter exists
    wl4 = ["AAAA", "CCCC", "GGGG", "TTTT"]
    with pytest.raises(pa.PaError) as e:
        pa.CellCounter(al, host, tx_gene, 1 << 31, wl4, 4, 16)
    assert e.value.code == pa._ffi.PA_ERR_UNSUPPORTED
    pa.CellCounter(al, host, tx_gene, 1 << 30, wl4, 4, 16)
    bad_gene = tx_gene.copy()
    bad_gene[0] = len(names)
    with pytest.raises(pa.PaError) as e:
        pa.CellCounter(al, host, bad_gene, len(names), wl4, 4, 12)
    assert e.value.code == pa._ffi.PA_ERR_INVALID_ARG
    # the ids match after /1 and /2 are cut, and the file-level call works on these three reads
    (tmp_path / "r2.fq").write_bytes(_fastq(["a/2", "b/2", "c"], r2))
    st = al.count_cells(host, tmp_path / "r1.fq", tmp_path / "r2.fq", wl, tmp_path, 16, 12)
    assert st["reads"] == 3 and st["barcode_exact"] == 3
