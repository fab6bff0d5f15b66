"""Paired-end reads end to end on the GPU: 2 000 simulated pairs per case (tests/pairs_cases.py: gencode_small at K = 20 and 31, a 400-transcript
synthetic index at K = 24; fragments of 100-400 bases, mates of 75, 1 % substitutions; "fr", "rf", "ff") through the device API (encode, reverse
complement, two map launches, combine) and through map_pairs, bit-exact against the model (tests/pairs_model.py: the oracle per mate + the pair
rule): class content, coverage, mismatches, mapped bit, the class-count table and the overflow records; the compact records of the pair
results; and the abundances of the pair table."""
import gzip

import numpy as np
import pytest

import helpers
import pairs_cases
import pairs_model as pm

pa = helpers.pa
pytestmark = pytest.mark.gpu

_al, _want = {}, {}


def _aligner(name):
    key = pairs_cases.CASES[name][0]
    if key not in _al:
        _al[key] = pa.Pseudoaligner(pairs_cases.host_of(key))
    return _al[key]


def _model(name):
    """the model's (results, coff, ids, stats, table, novel) of a case, computed once"""
    if name not in _want:
        host, r1, r2, orient = pairs_cases.case(name)
        res, coff, ids, st, m1, m2 = pm.model_pairs(host, r1, r2, orient)
        assert pm.fates(res, coff, ids, m1, m2, host) == pm.ALL_FATES
        _want[name] = (res, coff, ids, st) + pm.table_and_novel(res, coff, ids, host)
    return _want[name]


def _up(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def _device_pairs(name, with_counts):
    """the device API, step by step -> (results, arena, stats, counts or None, device handles kept alive)"""
    import torch
    host, r1, r2, orient = pairs_cases.case(name)
    al = _aligner(name)
    n = len(r1)
    mates = []
    for reads, rc in zip((r1, r2), pm.ORIENT[orient]):
        text, off = pa.concat_reads(reads)
        wpr = 3
        d_text, d_off = _up(np.concatenate([text, np.zeros(8, np.uint8)])), _up(off)
        words = ((n + 63) // 64) * wpr * 64
        d_tiles = torch.zeros(words, dtype=torch.int64, device="cuda")
        d_rc = torch.zeros(words, dtype=torch.int64, device="cuda")
        d_lens = torch.zeros(n + 64, dtype=torch.int32, device="cuda")
        cap = al.arena_hint(n)
        d_res = torch.zeros(4 * n, dtype=torch.int32, device="cuda")
        d_arena = torch.zeros(cap, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        al.encode_reads_device(d_text.data_ptr(), d_off.data_ptr(), n, wpr, d_tiles.data_ptr(), d_lens.data_ptr())
        if rc:
            al.revcomp_tiles_device(d_tiles.data_ptr(), d_lens.data_ptr(), n, wpr, d_rc.data_ptr())
        al.map_batch_device((d_rc if rc else d_tiles).data_ptr(), d_lens.data_ptr(), n, wpr, d_res.data_ptr(), d_arena.data_ptr(), cap)
        al.map_finish()
        mates.append((d_res, d_arena, d_tiles, d_rc, d_lens))
    cap = 16 * n
    d_pres = torch.zeros(4 * n, dtype=torch.int32, device="cuda")
    d_parena = torch.zeros(cap, dtype=torch.int32, device="cuda")
    sb = al.pairs_scratch_bytes(n)
    d_scr = torch.empty(sb + 256, dtype=torch.uint8, device="cuda")
    scr = (d_scr.data_ptr() + 255) & ~255
    counts = torch.zeros(al.counts_len(), dtype=torch.int64, device="cuda") if with_counts else None
    torch.cuda.synchronize()
    al.pairs_combine_device(mates[0][0].data_ptr(), mates[0][1].data_ptr(), mates[1][0].data_ptr(), mates[1][1].data_ptr(), n, d_pres.data_ptr(), d_parena.data_ptr(),
                            cap, scr, sb, d_counts=counts.data_ptr() if with_counts else 0)
    stats, used, need = al.pairs_finish(scr)
    res = d_pres.cpu().numpy().view(pa.RESULT_DTYPE).reshape(-1).copy()
    arena = d_parena.cpu().numpy().view(np.uint32)[:used].copy()
    return res, arena, stats, counts, (d_pres, d_parena, cap, used)


def _assert_equal(res, coff, ids, want, what):
    w_res, w_coff, w_ids = want[0], want[1], want[2]
    for f in ("coverage", "mismatches", "class_len"):
        assert np.array_equal(res[f], w_res[f]), (what, f, np.flatnonzero(res[f] != w_res[f])[:5])
    assert np.array_equal(coff, w_coff) and np.array_equal(ids, w_ids), what


@pytest.mark.parametrize("name", list(pairs_cases.CASES))
def test_device_api_counts_and_overflow(name):
    host = pairs_cases.case(name)[0]
    al = _aligner(name)
    want = _model(name)
    ovf = pa.Overflow(0, 1 << 12, 1 << 18)
    al.set_overflow(ovf)
    try:
        res, arena, stats, counts, _ = _device_pairs(name, True)
        novel = pa.parse_overflow(ovf.fetch())
    finally:
        al.set_overflow(None)
    coff, ids = pa.gather_classes(res, arena, host)
    _assert_equal(res, coff, ids, want, name)
    for k in ("pairs", "both_mapped", "mate1_only", "mate2_only", "neither", "both_mapped_empty"):
        assert stats[k] == want[3][k], (k, stats, want[3])
    pm.check_stats(stats, res)
    table = counts.cpu().numpy()
    nc = host.arrays()["num_classes"]
    assert np.array_equal(table, want[4]) and novel == want[5] and sum(novel.values()) == int(table[nc]) and table.sum() == len(res)


@pytest.mark.parametrize("name", list(pairs_cases.CASES))
def test_map_pairs(name):
    host, r1, r2, orient = pairs_cases.case(name)
    res, coff, ids = _aligner(name).map_pairs(r1, r2, orient)
    _assert_equal(res, coff, ids, _model(name), name)
    assert np.array_equal(res["class_off"], coff[:-1].astype(np.uint32))


@pytest.mark.parametrize("name", ["gencode_k20_fr", "synth400_k24_ff"])
def test_compact_records_of_pairs(name):
    import torch
    host = pairs_cases.case(name)[0]
    al = _aligner(name)
    res, arena, stats, _, (d_pres, d_parena, cap, used) = _device_pairs(name, False)
    n = len(res)
    sb = pa.lib().pa_compact_scratch_bytes(n)
    d_compact = torch.zeros(n, dtype=torch.int64, device="cuda")
    d_packed = torch.zeros(used + n + 16, dtype=torch.int32, device="cuda")
    d_pw = torch.zeros(1, dtype=torch.int64, device="cuda")
    d_scr = torch.empty(sb, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    pa.check(pa.lib().pa_results_compact_device(al._h, d_pres.data_ptr(), d_parena.data_ptr(), cap, n, d_compact.data_ptr(), d_packed.data_ptr(), used + n + 16,
                                                d_pw.data_ptr(), d_scr.data_ptr(), sb, None))
    torch.cuda.synchronize()
    pw = int(d_pw.item())
    c_res, c_coff, c_ids = pa.unpack_compact(d_compact.cpu().numpy().view(np.uint64), d_packed.cpu().numpy().view(np.uint32)[:pw], host)
    _assert_equal(c_res, c_coff, c_ids, _model(name), name)


def test_quantifier_on_the_pair_table():
    name = "gencode_k20_fr"
    host = pairs_cases.case(name)[0]
    al = _aligner(name)
    want = _model(name)
    ovf = pa.Overflow(0, 1 << 12, 1 << 18)
    al.set_overflow(ovf)
    try:
        res, arena, stats, counts, _ = _device_pairs(name, True)
        q = al.quantify(counts.data_ptr(), ovf, mean_read_len=250.0)
    finally:
        al.set_overflow(None)
    q2 = pa.Quantifier(al, host, mean_read_len=250.0)
    q2.set_counts(want[4].astype(np.uint64), pa.serialise_overflow(want[5]))
    q2.run()
    for x, y in zip(q.fetch(), q2.fetch()):
        assert x.tobytes() == y.tobytes()
    assert q.fetch()[0].sum() > 0


def test_bad_arguments_are_rejected_before_any_device_call():
    al = _aligner("gencode_k20_fr")
    with pytest.raises(ValueError):
        al.map_pairs(["ACGT"], ["ACGT"], "fx")
    with pytest.raises(ValueError):
        al.map_pairs(["ACGT"], [], "fr")
    d, o = pa.concat_reads(["ACGT"])
    out = np.zeros(1, pa.RESULT_DTYPE)
    L = pa.lib()
    E = pa._ffi.PA_ERR_INVALID_ARG
    assert L.pa_map_pairs(al._h, d.ctypes.data, o.ctypes.data, d.ctypes.data, o.ctypes.data, 1, 3, 2, out.ctypes.data, None, None) == E
    assert L.pa_map_pairs(al._h, d.ctypes.data, o.ctypes.data, d.ctypes.data, o.ctypes.data, 1, -1, 2, out.ctypes.data, None, None) == E
    assert L.pa_map_pairs(al._h, d.ctypes.data, None, d.ctypes.data, o.ctypes.data, 1, 0, 2, out.ctypes.data, None, None) == E
    assert L.pa_map_pairs(al._h, None, o.ctypes.data, d.ctypes.data, o.ctypes.data, 1, 0, 2, out.ctypes.data, None, None) == E
    assert L.pa_map_pairs(al._h, d.ctypes.data, o.ctypes.data, d.ctypes.data, o.ctypes.data, 1, 0, 2, None, None, None) == E
    assert L.pa_map_pairs(None, d.ctypes.data, o.ctypes.data, d.ctypes.data, o.ctypes.data, 1, 0, 2, out.ctypes.data, None, None) == E
    res, coff, ids = al.map_pairs([], [], "fr")
    assert len(res) == 0 and coff.tolist() == [0] and len(ids) == 0


# ---- count_pairs: the same pairs from FASTQ files ----
def _write_pairs(tmp_path, r1, r2, form, tag=("/1", "/2")):
    """the pairs as two FASTQ files: "plain", "gzip" or "crlf" """
    eol = "\r\n" if form == "crlf" else "\n"
    paths = []
    for k, reads in enumerate((r1, r2)):
        text = "".join("@pair%d%s extra words%s%s%s+%s%s%s" % (i, tag[k], eol, s, eol, eol, "I" * len(s), eol) for i, s in enumerate(reads)).encode()
        p = tmp_path / ("R%d.fq%s" % (k + 1, ".gz" if form == "gzip" else ""))
        p.write_bytes(gzip.compress(text) if form == "gzip" else text)
        paths.append(str(p))
    return paths


@pytest.mark.parametrize("name,form", [("gencode_k20_fr", "plain"), ("gencode_k31_rf", "gzip"), ("synth400_k24_ff", "crlf")])
def test_count_pairs_from_fastq_equals_the_device_path(name, form, tmp_path, monkeypatch):
    host, r1, r2, orient = pairs_cases.case(name)
    al = _aligner(name)
    want = _model(name)
    p1, p2 = _write_pairs(tmp_path, r1, r2, form)
    monkeypatch.setenv("PA_INGEST_BATCH", "700")            # 2 000 pairs: batches of 700, 700 and 600
    ovf = pa.Overflow(0, 1 << 12, 1 << 18)
    al.set_overflow(ovf)
    try:
        counts, stats = al.count_pairs(p1, p2, orient)
        novel = pa.parse_overflow(ovf.fetch())
        ovf.reset()
        _, _, d_stats, d_counts, _ = _device_pairs(name, True)
        d_novel = pa.parse_overflow(ovf.fetch())
    finally:
        al.set_overflow(None)
    assert np.array_equal(counts.astype(np.int64), want[4]) and novel == want[5]
    assert np.array_equal(counts.astype(np.int64), d_counts.cpu().numpy()) and novel == d_novel and stats == d_stats
    nc = host.arrays()["num_classes"]
    assert sum(novel.values()) == int(counts[nc]) and int(counts.sum()) == len(r1) == stats["pairs"]
    st = pa.process_reads_stage_seconds()
    assert st and int(list(st.values())[7] if isinstance(st, dict) else st[7]) == len(r1)
    # without an overflow table and in one batch: the same table
    monkeypatch.delenv("PA_INGEST_BATCH")
    counts2, stats2 = al.count_pairs(p1, p2, orient)
    assert np.array_equal(counts2, counts) and stats2 == stats


def test_count_pairs_rejects_pairs_that_do_not_match(tmp_path, monkeypatch):
    host, r1, r2, orient = pairs_cases.case("gencode_k20_fr")
    al = _aligner("gencode_k20_fr")
    monkeypatch.setenv("PA_INGEST_BATCH", "64")
    r1, r2 = r1[:200], r2[:200]
    # ids: record 137 of R2 names another pair
    p1, p2 = _write_pairs(tmp_path, r1, r2, "plain")
    text = open(p2).read().replace("@pair137/2", "@pair731/2")
    open(p2, "w").write(text)
    with pytest.raises(pa.PaError) as e:
        al.count_pairs(p1, p2, "fr")
    assert e.value.code == pa._ffi.PA_ERR_FORMAT and "record 137" in str(e.value)
    # counts: R2 ends after 150 records
    p1, p2 = _write_pairs(tmp_path, r1, r2[:150], "plain")
    with pytest.raises(pa.PaError) as e:
        al.count_pairs(p1, p2, "fr")
    assert e.value.code == pa._ffi.PA_ERR_FORMAT and "record 150" in str(e.value)
    # orientation and null arguments: refused before any device call
    with pytest.raises(ValueError):
        al.count_pairs(p1, p2, "xx")
    out = np.zeros(al.counts_len(), np.uint64)
    L, E = pa.lib(), pa._ffi.PA_ERR_INVALID_ARG
    assert L.pa_count_pairs(al._h, p1.encode(), p2.encode(), 5, 2, 1, out.ctypes.data, None, None) == E
    assert L.pa_count_pairs(al._h, None, p2.encode(), 0, 2, 1, out.ctypes.data, None, None) == E
    assert L.pa_count_pairs(al._h, p1.encode(), p2.encode(), 0, 2, 1, None, None, None) == E
    assert L.pa_count_pairs(None, p1.encode(), p2.encode(), 0, 2, 1, out.ctypes.data, None, None) == E


def test_file_drivers_leave_nothing_behind_on_the_index(tmp_path, monkeypatch):
    """pa_count_pairs, pa_count_cells, pa_count_pairs and pa_map_batch on ONE index in one process: each file driver creates its streams and gives
    their launch contexts back to the index when it returns, so the second table equals the first word for word and the host-buffer call that
    follows sees the index as a fresh one does"""
    name = "gencode_k20_fr"
    host, r1, r2, orient = pairs_cases.case(name)
    al = _aligner(name)
    p1, p2 = _write_pairs(tmp_path, r1, r2, "plain")
    monkeypatch.setenv("PA_INGEST_BATCH", "700")            # three batches: both batch buffers and a last partial batch
    counts, stats = al.count_pairs(p1, p2, orient)
    assert np.array_equal(counts.astype(np.int64), _model(name)[4]) and stats["pairs"] == len(r1)
    # the same files as a single-cell run: the first 28 bases of mate 1 stand in for barcode + UMI, mate 2 is mapped
    wl = sorted({s[:16] for s in r1 if len(s) >= 28 and set(s[:16]) <= set("ACGT")})[:64]
    (tmp_path / "wl.txt").write_text("\n".join(wl) + "\n")
    out = tmp_path / "cells"
    out.mkdir()
    cst = al.count_cells(host, p1, p2, tmp_path / "wl.txt", out, 16, 12, num_threads=4)
    assert cst["reads"] == len(r1) and (out / "matrix.mtx").read_text().startswith("%%MatrixMarket")
    counts2, stats2 = al.count_pairs(p1, p2, orient)
    assert counts2.tobytes() == counts.tobytes() and stats2 == stats
    res, coff, cids = al.map_batch(r1)
    o_res, o_coff, o_ids, _ = helpers.Oracle(host).map_reads(r1, 2, 4)
    helpers.assert_same_as_oracle(res, coff, cids, o_res, o_coff, o_ids, "map_batch after the file drivers")
