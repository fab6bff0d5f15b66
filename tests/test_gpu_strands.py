"""Unstranded libraries end to end on the GPU: 2 000 simulated pairs per case with the mates of every odd pair swapped (tests/strands_cases.py:
gencode_small plus antisense transcripts at K = 20, plain gencode_small at K = 31, a 400-transcript synthetic index at K = 24) through
map_pairs(orient="un"), map_batch(strand=...), the device API (four map launches, two combines, the merge) and count_pairs(orient="un") from
plain, gzip and BGZF files, bit-exact against the model (tests/strands_model.py: the oracle per mate and strand, the pair rule, the merge
rule): class content, coverage, mismatches, mapped bit, the class-count table, the overflow records and the stats."""
import gzip

import numpy as np
import pytest

import bgzf_cases as bc
import helpers
import strands_cases
import strands_model as sm

pa = helpers.pa
pytestmark = pytest.mark.gpu

_al, _want = {}, {}


def _aligner(name):
    key = strands_cases.CASES[name][0]
    if key not in _al:
        _al[key] = pa.Pseudoaligner(strands_cases.host_of(key))
    return _al[key]


def _model(name):
    """the model's (results, coff, ids, stats, fates, table, novel) of a case, computed once"""
    if name not in _want:
        host, r1, r2 = strands_cases.case(name)
        res, coff, ids, st, fates, cs, cr = sm.model_pairs_unstranded(host, r1, r2)
        _want[name] = (res, coff, ids, st, fates) + sm.table_and_novel(res, coff, ids, host)
    return _want[name]


def _assert_equal(res, coff, ids, want, what):
    w_res, w_coff, w_ids = want[0], want[1], want[2]
    for f in ("coverage", "mismatches", "class_len"):
        assert np.array_equal(res[f], w_res[f]), (what, f, np.flatnonzero(res[f] != w_res[f])[:5])
    assert np.array_equal(coff, w_coff) and np.array_equal(ids, w_ids), what


def _up(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def _scratch(nbytes):
    import torch
    t = torch.empty(nbytes + 256, dtype=torch.uint8, device="cuda")
    return t, (t.data_ptr() + 255) & ~255


def _device_unstranded(name, counts):
    """the device API, step by step: both mates as given and reverse-complemented, S = combine(mate 1, rc mate 2), R = combine(rc mate 1, mate 2),
    both uncounted, one counted merge -> (results, arena, stats)"""
    import torch
    host, r1, r2 = strands_cases.case(name)
    al = _aligner(name)
    n, wpr = len(r1), 3
    maps = {}
    keep = []
    for m, reads in enumerate((r1, r2)):
        text, off = pa.concat_reads(reads)
        d_text, d_off = _up(np.concatenate([text, np.zeros(8, np.uint8)])), _up(off)
        words = ((n + 63) // 64) * wpr * 64
        d_tiles = torch.zeros(words, dtype=torch.int64, device="cuda")
        d_rc = torch.zeros(words, dtype=torch.int64, device="cuda")
        d_lens = torch.zeros(n + 64, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        al.encode_reads_device(d_text.data_ptr(), d_off.data_ptr(), n, wpr, d_tiles.data_ptr(), d_lens.data_ptr())
        al.revcomp_tiles_device(d_tiles.data_ptr(), d_lens.data_ptr(), n, wpr, d_rc.data_ptr())
        for rc, tiles in ((False, d_tiles), (True, d_rc)):
            cap = al.arena_hint(n)
            d_res = torch.zeros(4 * n, dtype=torch.int32, device="cuda")
            d_arena = torch.zeros(cap, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            al.map_batch_device(tiles.data_ptr(), d_lens.data_ptr(), n, wpr, d_res.data_ptr(), d_arena.data_ptr(), cap)
            al.map_finish()
            maps[(m, rc)] = (d_res, d_arena)
        keep.append((d_text, d_off, d_tiles, d_rc, d_lens))
    cands = []
    for x, y in ((maps[(0, False)], maps[(1, True)]), (maps[(0, True)], maps[(1, False)])):
        cap = 16 * n
        d_cres = torch.zeros(4 * n, dtype=torch.int32, device="cuda")
        d_carena = torch.zeros(cap, dtype=torch.int32, device="cuda")
        sb = al.pairs_scratch_bytes(n)
        t, scr = _scratch(sb)
        torch.cuda.synchronize()
        al.pairs_combine_device(x[0].data_ptr(), x[1].data_ptr(), y[0].data_ptr(), y[1].data_ptr(), n, d_cres.data_ptr(), d_carena.data_ptr(), cap, scr, sb)
        al.pairs_finish(scr)
        cands.append((d_cres, d_carena))
    cap = 32 * n
    d_res = torch.zeros(4 * n, dtype=torch.int32, device="cuda")
    d_arena = torch.zeros(cap, dtype=torch.int32, device="cuda")
    sb = al.strands_scratch_bytes(n)
    t, scr = _scratch(sb)
    torch.cuda.synchronize()
    al.strands_merge_device(cands[0][0].data_ptr(), cands[0][1].data_ptr(), cands[1][0].data_ptr(), cands[1][1].data_ptr(), n, d_res.data_ptr(), d_arena.data_ptr(), cap,
                            scr, sb, d_counts=counts.data_ptr() if counts is not None else 0)
    stats, used, need = al.strands_finish(scr)
    return d_res.cpu().numpy().view(pa.RESULT_DTYPE).reshape(-1).copy(), d_arena.cpu().numpy().view(np.uint32)[:used].copy(), stats


@pytest.mark.parametrize("name", list(strands_cases.CASES))
def test_map_pairs_unstranded(name):
    host, r1, r2 = strands_cases.case(name)
    want = _model(name)
    res, coff, ids = _aligner(name).map_pairs(r1, r2, "un")
    _assert_equal(res, coff, ids, want, name)
    assert np.array_equal(res["class_off"], coff[:-1].astype(np.uint32))
    fates = want[4]
    assert fates.count("sense_only") > 100 and fates.count("antisense_only") > 100 and fates.count("neither") > 0
    if name == "anti_gencode_k20":
        assert min(fates.count(f) for f in ("sense_wins", "antisense_wins", "tie")) > 100
    # non-vacuity: the stranded orientation gives another answer on these pairs
    fr = _aligner(name).map_pairs(r1, r2, "fr")
    lost = int((res["mismatches"] >> 31).sum()) - int((fr[0]["mismatches"] >> 31).sum())
    assert lost > (100 if name == "anti_gencode_k20" else 500)   # (the antisense transcripts catch part of the other strand)


def test_map_batch_strand():
    name = "anti_gencode_k20"
    host, r1, _ = strands_cases.case(name)
    al = _aligner(name)
    plain = al.map_batch(r1)
    for strand in ("fwd", "rev", "both"):
        want = sm.model_reads(host, r1, strand)
        got = al.map_batch(r1, strand=strand)
        _assert_equal(got[0], got[1], got[2], want, strand)
        if strand == "both":
            for f in ("sense_only", "antisense_only", "neither", "sense_wins", "antisense_wins", "tie"):
                assert want[4].count(f) >= 1, f
    # PA_STRAND_FWD through the new entry point is what pa_map_batch returns
    import ctypes as C
    d, o = pa.concat_reads(r1)
    n = len(r1)
    res, coff, ids = np.zeros(n, pa.RESULT_DTYPE), np.zeros(n + 1, np.uint64), C.c_void_p()
    pa.check(pa.lib().pa_map_batch_strand(al._h, d.ctypes.data, o.ctypes.data, n, pa._ffi.PA_STRAND_FWD, 2, res.ctypes.data, coff.ctypes.data, C.byref(ids)))
    cids = np.ctypeslib.as_array(C.cast(ids, C.POINTER(C.c_uint32)), (int(coff[-1]),)).copy()
    for f in ("coverage", "mismatches", "class_len", "class_off"):
        assert np.array_equal(res[f], plain[0][f]), f
    assert np.array_equal(coff, plain[1]) and np.array_equal(cids, plain[2])
    with pytest.raises(ValueError):
        al.map_batch(r1[:2], strand="un")
    res, coff, ids = al.map_batch([], strand="both")
    assert len(res) == 0 and coff.tolist() == [0] and len(ids) == 0
    res, coff, ids = al.map_pairs([], [], "un")
    assert len(res) == 0 and coff.tolist() == [0] and len(ids) == 0


def _write_pairs(tmp_path, r1, r2, form):
    """the pairs as two FASTQ files: "plain", "gzip" or "bgzf" """
    paths = []
    for k, reads in enumerate((r1, r2)):
        text = "".join("@pair%d/%d extra words\n%s\n+\n%s\n" % (i, k + 1, s, "I" * len(s)) for i, s in enumerate(reads)).encode()
        p = tmp_path / ("R%d.fq%s" % (k + 1, "" if form == "plain" else ".gz"))
        p.write_bytes(text if form == "plain" else gzip.compress(text, 1) if form == "gzip" else bc.bgzf(text, 4000))
        paths.append(str(p))
    return paths


@pytest.mark.parametrize("name,form", [("anti_gencode_k20", "plain"), ("gencode_k31", "gzip"), ("synth400_k24", "bgzf")])
def test_count_pairs_unstranded_from_fastq(name, form, tmp_path, monkeypatch):
    import torch
    host, r1, r2 = strands_cases.case(name)
    al = _aligner(name)
    want = _model(name)
    table, novel = want[5], want[6]
    p1, p2 = _write_pairs(tmp_path, r1, r2, form)
    monkeypatch.setenv("PA_INGEST_BATCH", "700")            # 2 000 pairs: batches of 700, 700 and 600
    ovf = pa.Overflow(0, 1 << 12, 1 << 18)
    al.set_overflow(ovf)
    try:
        counts, stats = al.count_pairs(p1, p2, "un")
        got_novel = pa.parse_overflow(ovf.fetch())
        ovf.reset()
        d_counts = torch.zeros(al.counts_len(), dtype=torch.int64, device="cuda")
        d_res, d_arena, d_stats = _device_unstranded(name, d_counts)
        d_novel = pa.parse_overflow(ovf.fetch())
    finally:
        al.set_overflow(None)
    assert np.array_equal(counts.astype(np.int64), table) and got_novel == novel
    assert np.array_equal(counts.astype(np.int64), d_counts.cpu().numpy()) and got_novel == d_novel and stats == d_stats
    coff, ids = pa.gather_classes(d_res, d_arena, host)
    _assert_equal(d_res, coff, ids, want, name)
    for k in ("items", "both_mapped", "sense_only", "antisense_only", "neither", "ties"):
        assert stats[k] == want[3][k], (k, stats, want[3])
    sm.check_stats(d_stats, d_res)
    nc = host.arrays()["num_classes"]
    assert sum(novel.values()) == int(counts[nc]) and int(counts.sum()) == len(r1) == stats["items"] and counts[nc] > 0
    assert int(list(pa.process_reads_stage_seconds().values())[7]) == len(r1)
    took_device = pa.pairs_input_stats()["device_path"]
    assert took_device == (form == "bgzf")                   # the conditions of the other pair drivers
    # without an overflow table and in one batch: the same table
    monkeypatch.delenv("PA_INGEST_BATCH")
    counts1, stats1 = al.count_pairs(p1, p2, "un")
    assert np.array_equal(counts1, counts) and stats1 == stats
    # ... and through the other path: the host scan for BGZF, the device path on request for plain text (ordinary gzip has the host's alone)
    if form == "bgzf":
        monkeypatch.setenv("PA_PAIRS_HOST_SCAN", "1")
    else:
        monkeypatch.setenv("PA_PAIRS_DEVICE_PLAIN", "1")
    monkeypatch.setenv("PA_INGEST_BATCH", "700")
    counts2, stats2 = al.count_pairs(p1, p2, "un")
    assert pa.pairs_input_stats()["device_path"] == (form == "plain")
    assert np.array_equal(counts2, counts) and stats2 == stats


def test_unstranded_driver_leaves_nothing_behind(tmp_path, monkeypatch):
    """count_pairs "fr", "un", "fr" on one index: the unstranded call creates its four streams and gives their launch contexts back, so the third
    table equals the first word for word"""
    name = "anti_gencode_k20"
    host, r1, r2 = strands_cases.case(name)
    al = _aligner(name)
    p1, p2 = _write_pairs(tmp_path, r1, r2, "plain")
    monkeypatch.setenv("PA_INGEST_BATCH", "700")
    first, st1 = al.count_pairs(p1, p2, "fr")
    un, st_un = al.count_pairs(p1, p2, "un")
    third, st3 = al.count_pairs(p1, p2, "fr")
    assert first.tobytes() == third.tobytes() and st1 == st3 and st1["pairs"] == len(r1)
    assert np.array_equal(un.astype(np.int64), _model(name)[5]) and not np.array_equal(un, first)


def test_stranded_entry_points_are_unchanged():
    al = _aligner("anti_gencode_k20")
    d, o = pa.concat_reads(["ACGT"])
    out = np.zeros(1, pa.RESULT_DTYPE)
    L, E = pa.lib(), pa._ffi.PA_ERR_INVALID_ARG
    assert L.pa_map_pairs(al._h, d.ctypes.data, o.ctypes.data, d.ctypes.data, o.ctypes.data, 1, 3, 2, out.ctypes.data, None, None) == E
    counts = np.zeros(al.counts_len(), np.uint64)
    assert L.pa_count_pairs(al._h, b"a", b"b", 5, 2, 1, counts.ctypes.data, None, None) == E
    for bad in ("fx", "xx"):
        with pytest.raises(ValueError):
            al.map_pairs(["ACGT"], ["ACGT"], bad)
        with pytest.raises(ValueError):
            al.count_pairs("a", "b", bad)
