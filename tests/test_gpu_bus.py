"""BUS output on the GPU (pa_bus, pa_write_bus) against the pure-Python model of tests/bus_model.py, with every R2 mapped by the independent
oracle on the model's side: records, the ec table and all eight stats exactly; 1, 3 and 7 uneven batches identical; the records of
pa_pairs_combine_device taken as they are; the three output files byte for byte for plain, CRLF and gzip input; the error cases."""
import gzip

import numpy as np
import pytest

import bus_model as bm
import helpers
import pairs_model as pm

pa = helpers.pa
pytestmark = pytest.mark.gpu

BC, UMI = 16, 12
_cache = {}


def _gencode():
    if "gencode" not in _cache:
        host = pa.build_index(str(helpers.FASTA), 24, 8)
        ix = host.arrays()
        names, seqs = helpers.read_fasta()
        _cache["gencode"] = (host, pa.Pseudoaligner(host), helpers.Oracle(host), int(ix["num_transcripts"]), bm.index_classes(ix), seqs)
    return _cache["gencode"]


def _case():
    """about 20 k pairs and the model's expectation, computed once and left unchanged"""
    if "case" not in _cache:
        host, al, oracle, T, classes, seqs = _gencode()
        case = bm.make_case(12, seqs, BC, UMI)
        mapping = bm.mapping_from_oracle(oracle, case["r2"])
        records, table, st, fates = bm.model(case["r1"], mapping, T, classes, BC, UMI)
        # every rule but bad_class (which no mapping produces) is exercised; records collapse reads; novel lists and lists equal to a class occur
        for key in ("r1_short", "barcode_n", "umi_n", "unmapped", "recorded"):
            assert st[key] > 0, (key, st)
        assert st["bad_class"] == 0 and 0 < st["records"] < st["recorded"] and len(table) > T + sum(len(c) >= 2 for c in classes)
        _cache["case"] = (case, mapping, (records, table, st))
    return _cache["case"]


def gpu_bus(al, host, r1, r2, bc_len, umi_len, cuts=()):
    """the writer fed device-resident batches [0, cuts..., n): R2s mapped on the GPU, R1s uploaded as they are -> the writer, finished"""
    import torch
    dev = torch.device("cuda")
    writer = pa.BusWriter(al, host, bc_len, umi_len)
    bounds = [0] + list(cuts) + [len(r1)]
    for a, b in zip(bounds[:-1], bounds[1:]):
        m = b - a
        tiles, lens, wpr = pa.encode_reads_host(r2[a:b])
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
        ascii, off = pa.concat_reads(r1[a:b])
        d_r1 = torch.from_numpy(np.concatenate([ascii, np.zeros(8, np.uint8)])).to(dev)
        d_off = torch.from_numpy(off.view(np.int64)).to(dev)
        torch.cuda.synchronize()
        writer.add_device(d_res.data_ptr(), d_arena.data_ptr(), cap, d_r1.data_ptr(), d_off.data_ptr(), m)
    return writer


def result(writer):
    return bm.records_from_array(writer.records()), bm.table_from_csr(*writer.ecs()), writer.stats()


def test_writer_equals_model_in_any_batches():
    host, al, oracle, T, classes, seqs = _gencode()
    case, mapping, want = _case()
    n = len(case["r1"])
    one = result(gpu_bus(al, host, case["r1"], case["r2"], BC, UMI))
    assert one[2] == want[2]
    assert one[1] == want[1]
    assert one[0] == want[0]
    three = result(gpu_bus(al, host, case["r1"], case["r2"], BC, UMI, cuts=(n // 7, n // 2)))
    rng = np.random.default_rng(1)
    seven = result(gpu_bus(al, host, case["r1"], case["r2"], BC, UMI, cuts=sorted(rng.choice(np.arange(1, n), 6, replace=False).tolist())))
    assert three == one and seven == one


def test_pair_records_are_taken_unchanged():
    """mates mapped as they are ("ff"), combined by pa_pairs_combine_device: the pair records and the pair arena go to the writer"""
    import torch
    host, al, oracle, T, classes, seqs = _gencode()
    n = 600
    m1, m2, _ = pm.simulate_pairs(seqs, n, 5, sub_rate=0.01, orient="ff", junk_every=9)
    res, coff, ids, st, _, _ = pm.model_pairs(host, m1, m2, "ff")
    mapping = [(bool(int(res["mismatches"][i]) >> 31), [int(t) for t in ids[int(coff[i]):int(coff[i + 1])]]) for i in range(n)]
    rng = np.random.default_rng(2)
    cells = ["".join(bm.BASES[x] for x in rng.integers(0, 4, 8)) for _ in range(6)]
    r1 = [cells[int(rng.integers(6))] + "ACGTA" + bm.BASES[int(rng.integers(4))] for _ in range(n)]
    want = bm.model(r1, mapping, T, classes, 8, 6)[:3]
    assert st["both_mapped"] > 0 and st["mate1_only"] > 0 and len(want[1]) > T + sum(len(c) >= 2 for c in classes) and want[2]["records"] < want[2]["recorded"]
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()
    mates = []
    for reads in (m1, m2):
        tiles, lens, wpr = pa.encode_reads_host(reads)
        d_tiles, d_lens = up(tiles), up(np.concatenate([lens, np.zeros(64, lens.dtype)]))
        cap = al.arena_hint(n)
        d_res = torch.zeros(4 * n, dtype=torch.int32, device="cuda")
        d_arena = torch.zeros(cap, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        al.map_batch_device(d_tiles.data_ptr(), d_lens.data_ptr(), n, wpr, d_res.data_ptr(), d_arena.data_ptr(), cap)
        al.map_finish()
        mates.append((d_res, d_arena, d_tiles, d_lens))
    cap = 16 * n
    d_pres = torch.zeros(4 * n, dtype=torch.int32, device="cuda")
    d_parena = torch.zeros(cap, dtype=torch.int32, device="cuda")
    sb = al.pairs_scratch_bytes(n)
    d_scr = torch.empty(sb + 256, dtype=torch.uint8, device="cuda")
    scr = (d_scr.data_ptr() + 255) & ~255
    torch.cuda.synchronize()
    al.pairs_combine_device(mates[0][0].data_ptr(), mates[0][1].data_ptr(), mates[1][0].data_ptr(), mates[1][1].data_ptr(), n, d_pres.data_ptr(), d_parena.data_ptr(),
                            cap, scr, sb)
    pair_stats, used, _ = al.pairs_finish(scr)
    assert pair_stats["in_arena"] > 0 and pair_stats["by_reference"] > 0   # both representations reach the writer
    text, off = pa.concat_reads(r1)
    d_r1, d_off = up(np.concatenate([text, np.zeros(8, np.uint8)])), up(off)
    torch.cuda.synchronize()
    writer = pa.BusWriter(al, host, 8, 6)
    writer.add_device(d_pres.data_ptr(), d_parena.data_ptr(), used, d_r1.data_ptr(), d_off.data_ptr(), n)
    assert result(writer) == want


def _fastq(ids, seqs, crlf=False):
    nl = "\r\n" if crlf else "\n"
    return "".join("@%s extra%s%s%s+%s%s%s" % (i, nl, s, nl, nl, "I" * len(s), nl) for i, s in zip(ids, seqs)).encode()


def _files_equal_model(out, want, names, bc_len, umi_len):
    data = (out / "output.bus").read_bytes()
    assert data == bm.bus_bytes(want[0], bc_len, umi_len)
    assert (out / "matrix.ec").read_text() == bm.matrix_ec_text(want[1])
    assert (out / "transcripts.txt").read_text() == bm.transcripts_text(names)
    # ... and read back by the model's reader
    assert bm.read_bus(data) == (bc_len, umi_len, b"", want[0]) and bm.read_matrix_ec((out / "matrix.ec").read_text()) == want[1]


@pytest.mark.parametrize("form", ["plain", "crlf", "gzip"])
def test_write_bus_files(form, tmp_path, monkeypatch):
    host, al, oracle, T, classes, seqs = _gencode()
    case, mapping, want = _case()
    names = host.tx_names()
    ids = ["read%d" % i for i in range(len(case["r1"]))]
    r1 = _fastq([i + "/1" for i in ids], case["r1"], crlf=form == "crlf")
    r2 = _fastq([i + "/2" for i in ids], case["r2"], crlf=form == "crlf")
    suffix = ""
    if form == "gzip":
        r1, r2, suffix = gzip.compress(r1, 1), gzip.compress(r2, 1), ".gz"
    (tmp_path / ("r1.fq" + suffix)).write_bytes(r1)
    (tmp_path / ("r2.fq" + suffix)).write_bytes(r2)
    out = tmp_path / "out"
    out.mkdir()
    if form == "crlf":
        monkeypatch.setenv("PA_INGEST_BATCH", "3331")   # (the file-level driver in small batches: the same files)
    st = al.write_bus(host, tmp_path / ("r1.fq" + suffix), tmp_path / ("r2.fq" + suffix), out, BC, UMI, num_threads=4)
    assert st == want[2]
    _files_equal_model(out, want, names, BC, UMI)


def test_writer_writes_the_same_files(tmp_path):
    host, al, oracle, T, classes, seqs = _gencode()
    case, mapping, _ = _case()
    r1, r2, mp = case["r1"][:1500], case["r2"][:1500], mapping[:1500]
    want = bm.model(r1, mp, T, classes, BC, UMI)[:3]
    writer = gpu_bus(al, host, r1, r2, BC, UMI, cuts=(700,))
    writer.write(tmp_path)
    _files_equal_model(tmp_path, want, host.tx_names(), BC, UMI)


def test_error_cases(tmp_path):
    host, al, oracle, T, classes, seqs = _gencode()
    r1 = ["ACGTACGTACGTACGT" + "AAAACCCCGGGG"] * 3
    r2 = [seqs[0][:90]] * 3
    (tmp_path / "r1.fq").write_bytes(_fastq(["a", "b", "c"], r1))

    def run(r2_ids, r2_seqs, out=tmp_path, bc_len=16, umi_len=12):
        (tmp_path / "r2.fq").write_bytes(_fastq(r2_ids, r2_seqs))
        with pytest.raises(pa.PaError) as e:
            al.write_bus(host, tmp_path / "r1.fq", tmp_path / "r2.fq", out, bc_len, umi_len)
        return e.value

    e = run(["a", "b", "c"], r2, out=tmp_path / "missing")
    assert e.code == -2 and "no directory" in str(e)                # PA_ERR_IO
    e = run(["a", "b"], r2[:2])
    assert e.code == pa._ffi.PA_ERR_FORMAT and "record 2" in str(e)   # unequal record counts
    e = run(["a", "x", "c"], r2)
    assert e.code == pa._ffi.PA_ERR_FORMAT and "record 1" in str(e)
    e = run(["a", "b", "c"], r2, bc_len=17, umi_len=16)
    assert e.code == pa._ffi.PA_ERR_UNSUPPORTED
    with pytest.raises(pa.PaError) as e:
        pa.BusWriter(al, host, 16, 12).write(tmp_path / "missing")
    assert e.value.code == -2
    # the ids match after /1 and /2 are cut, and the file-level call works on these three reads
    (tmp_path / "r2.fq").write_bytes(_fastq(["a/2", "b/2", "c"], r2))
    st = al.write_bus(host, tmp_path / "r1.fq", tmp_path / "r2.fq", tmp_path, 16, 12)
    assert st["reads"] == 3 and st["recorded"] == 3 and st["records"] == 1
    assert bm.read_bus((tmp_path / "output.bus").read_bytes())[3][0][3] == 3
