#!/usr/bin/env python
"""Timing of the paired-end stage (csrc/pair_stage.hpp with the rule of csrc/pairs.hip) on device-resident pairs, and of pa_count_pairs from files in the page cache.

  python tools/bench_pairs.py [--pairs 10000000] [--index config3|17k] [--orient fr|un] [--out profiles/r10_pairs_bench.json]

Pairs of 2 x 100 bases: fragments of 300 bases from Txome.simulate_host (1 % substitutions), cut in numpy — mate 1 = the first 100 bases,
mate 2 = the reverse complement of the last 100 ("fr"). Reported, each the median of 5 runs timed with HIP events on the launch stream:
the reverse complement of mate 2, the two map launches, combine without the table, combine with the table and an overflow table attached;
the stats vector; the ratio combine / map and the bytes the combine stage must move (32 bytes of records in and 16 out per pair plus the ids
of the non-trivial pairs, counted on the host from the mates' records); and count_pairs pairs/s with its stage seconds. None is a gate.

--orient un: the same pairs as an UNSTRANDED library (the mates of every odd pair swapped) through the unstranded stage (the same skeleton with the rule of csrc/strands.hip): the four
map launches, the two uncounted combines, the merge without the table and with the table and an overflow table attached, the merge against the
two combines and against the four maps it follows, the merge's stats vector, and count_pairs pairs/s for "un" beside "fr" on the same files
(default --out profiles/r13_strands_bench.json)."""
import argparse
import importlib
import json
import os
import statistics
import sys
import tempfile
import time
from pathlib import Path

import numpy as np
import torch  # noqa: F401  (before the product library touches HIP: one runtime for both)

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
import pairs_input  # noqa: E402
pa = importlib.import_module("rust-pseudoaligner_amd")
L = pa.lib()
FRAG, MATE = 300, 100


def revcomp_rows(codes):
    return (3 - codes[:, ::-1]).astype(np.uint8)


def fragments(tx, n, seed):
    """n fragments of FRAG bases as codes [n, FRAG]"""
    wpr = L.pa_words_per_read(FRAG)
    out = np.zeros((n, FRAG), np.uint8)
    step = 1 << 20
    shifts = (2 * np.arange(32, dtype=np.uint64))[None, None, :]
    for lo in range(0, n, step):
        m = min(step, n - lo)
        tiles, lens = tx.simulate_host(FRAG, seed, m, sub_rate_ppm=10000, first_read=lo, words_per_read=wpr)
        t3 = tiles.reshape(-1, wpr, 64)
        rid = np.arange(m)
        words = t3[rid >> 6, :, rid & 63]                                   # [m, wpr]
        out[lo:lo + m] = ((words[:, :, None] >> shifts) & np.uint64(3)).reshape(m, -1)[:, :FRAG]
    return out


def to_tiles(codes):
    """codes [n, len] -> the tile layout (tiles, lens, wpr)"""
    n, ln = codes.shape
    wpr = (ln + 31) // 32
    padded = np.zeros((n, wpr * 32), np.uint64)
    padded[:, :ln] = codes
    words = (padded.reshape(n, wpr, 32) << (2 * np.arange(32, dtype=np.uint64))[None, None, :]).sum(axis=2, dtype=np.uint64)
    tiles = np.zeros(((n + 63) // 64, wpr, 64), np.uint64)
    rid = np.arange(n)
    tiles[rid >> 6, :, rid & 63] = words
    return tiles.reshape(-1), np.full(n, ln, np.uint32), wpr


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def timed(fn, reps=5):
    ms = []
    for _ in range(reps):
        e0, e1 = pa.vp(), pa.vp()
        pa.check(L.pa_event_create(e0)); pa.check(L.pa_event_create(e1))
        pa.check(L.pa_event_record(e0, None))
        fn()
        pa.check(L.pa_event_record(e1, None))
        t = pa._ffi.C.c_float()
        pa.check(L.pa_event_elapsed_ms(e0, e1, t))
        ms.append(t.value)
        L.pa_event_destroy(e0); L.pa_event_destroy(e1)
    return statistics.median(ms), ms


def count_pairs_leg(a, al, m1, m2, orients):
    """count_pairs from files in the page cache, once per orientation on the same two files -> {orient: report}"""
    fn = min(a.file_pairs, len(m1))
    lut = np.frombuffer(b"ACGT", np.uint8)
    rep = {}
    with tempfile.TemporaryDirectory(dir=os.environ.get("TMPDIR")) as d:
        paths = []
        for k, mate in enumerate((m1, m2)):
            p = os.path.join(d, "R%d.fq%s" % (k + 1, pairs_input.suffix(a)))
            with pairs_input.Writer(p, a.input) as f:
                for lo in range(0, fn, 1 << 18):
                    rows = lut[mate[lo:min(fn, lo + (1 << 18))]]
                    f.write(b"".join(b"@p%d/%d\n%s\n+\n%s\n" % (lo + i, k + 1, r.tobytes(), b"I" * MATE) for i, r in enumerate(rows)))
            paths.append(p)
        for orient in orients:
            al.count_pairs(paths[0], paths[1], orient, num_threads=a.threads)          # warm: page cache, buffers
            secs, (_, st) = pairs_input.timed_calls(lambda: al.count_pairs(paths[0], paths[1], orient, num_threads=a.threads), a.calls)
            dt = secs[-1]
            rep[orient] = {"pairs": fn, "pairs_per_s": fn / dt, "stage_seconds": pa.process_reads_stage_seconds(), "stats": st, **pairs_input.report(pa, a, fn, secs)}
    return rep


def unstranded(a, al, tx, m1, m2):
    """--orient un: the device-resident legs of the unstranded stage, then count_pairs "un" beside "fr" on the same files"""
    n = a.pairs
    m1, m2 = m1.copy(), m2.copy()
    odd = np.arange(1, n, 2)
    m1[odd], m2[odd] = m2[odd].copy(), m1[odd].copy()
    out = {"pairs": n, "index": a.index, "transcripts": tx.num_transcripts, "mate_len": MATE, "fragment": FRAG, "orient": "un"}
    cap = al.arena_hint(n)
    mate = []
    for m in (m1, m2):
        t, l, wpr = to_tiles(m)
        d_t, d_l = up(t), up(l)
        d_rc = torch.zeros(len(t), dtype=torch.int64, device="cuda")
        res = [torch.zeros(4 * n, dtype=torch.int32, device="cuda") for _ in range(2)]
        arena = [torch.zeros(cap, dtype=torch.int32, device="cuda") for _ in range(2)]
        torch.cuda.synchronize()
        al.revcomp_tiles_device(d_t.data_ptr(), d_l.data_ptr(), n, wpr, d_rc.data_ptr())
        mate.append((d_t, d_rc, d_l, res, arena, wpr))

    def four_maps():
        for d_t, d_rc, d_l, res, arena, wpr in mate:
            for k, tiles in enumerate((d_t, d_rc)):
                al.map_batch_device(tiles.data_ptr(), d_l.data_ptr(), n, wpr, res[k].data_ptr(), arena[k].data_ptr(), cap)
                al.map_finish()
    out["four_maps_ms"], _ = timed(four_maps)

    pcap = 8 * n + 4096
    cand = [(torch.zeros(4 * n, dtype=torch.int32, device="cuda"), torch.zeros(pcap, dtype=torch.int32, device="cuda")) for _ in range(2)]
    d_ir = torch.zeros(4 * n, dtype=torch.int32, device="cuda")
    d_ia = torch.zeros(2 * pcap, dtype=torch.int32, device="cuda")
    sb = max(al.pairs_scratch_bytes(n), al.strands_scratch_bytes(n))
    d_scr = torch.empty(sb + 256, dtype=torch.uint8, device="cuda")
    scr = (d_scr.data_ptr() + 255) & ~255
    counts = torch.zeros(al.counts_len(), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    last = {}

    def two_combines():   # S = (mate 1, rc mate 2), R = (rc mate 1, mate 2), both uncounted
        for c, (x, y) in enumerate(((0, 1), (1, 0))):
            al.pairs_combine_device(mate[0][3][x].data_ptr(), mate[0][4][x].data_ptr(), mate[1][3][y].data_ptr(), mate[1][4][y].data_ptr(), n, cand[c][0].data_ptr(),
                                    cand[c][1].data_ptr(), pcap, scr, sb)
            al.pairs_finish(scr)
    out["two_combines_ms"], _ = timed(two_combines)

    def merge(d_counts):
        al.strands_merge_device(cand[0][0].data_ptr(), cand[0][1].data_ptr(), cand[1][0].data_ptr(), cand[1][1].data_ptr(), n, d_ir.data_ptr(), d_ia.data_ptr(), 2 * pcap,
                                scr, sb, d_counts=d_counts)
        last["stats"], last["used"], _ = al.strands_finish(scr)
    out["merge_ms"], _ = timed(lambda: merge(0))
    ovf = pa.Overflow(0, 1 << 22, 1 << 26)
    al.set_overflow(ovf)
    out["merge_table_overflow_ms"], _ = timed(lambda: merge(counts.data_ptr()))
    al.set_overflow(None)
    out["stats"] = last["stats"]
    out["merge_arena_ids"] = int(last["used"])
    out["merge_over_two_combines"] = out["merge_ms"] / out["two_combines_ms"]
    out["merge_over_four_maps"] = out["merge_ms"] / out["four_maps_ms"]
    out["count_pairs"] = count_pairs_leg(a, al, m1, m2, ["fr", "un"])
    out["count_pairs_un_over_fr"] = out["count_pairs"]["un"]["pairs_per_s"] / out["count_pairs"]["fr"]["pairs_per_s"]
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=10_000_000)
    ap.add_argument("--index", choices=["config3", "17k"], default="config3")
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--file-pairs", type=int, default=2_000_000, help="pairs written to FASTQ for the count_pairs leg")
    ap.add_argument("--orient", choices=["fr", "un"], default="fr", help="un: the pairs as an unstranded library, through the unstranded stage")
    ap.add_argument("--out", default=None)
    pairs_input.add_args(ap)   # the count_pairs leg on BGZF files / on the host path / timed several times
    a = ap.parse_args()
    a.out = a.out or str(ROOT / "profiles" / ("r10_pairs_bench.json" if a.orient == "fr" else "r13_strands_bench.json"))
    pairs_input.apply(a)
    n = a.pairs
    tx = pa.Txome.synthesize(20000, 200000, 7) if a.index == "config3" else pa.Txome.synthesize(5000, 17000, 7)
    host = pa.HostIndex.from_txome(tx, 24, a.threads)
    al = pa.Pseudoaligner(host)
    frag = fragments(tx, n, 11)
    m1, m2 = frag[:, :MATE], revcomp_rows(frag[:, -MATE:])
    if a.orient == "un":
        return unstranded(a, al, tx, m1, m2)
    t1, l1, wpr = to_tiles(m1)
    t2, l2, _ = to_tiles(m2)
    d_t1, d_t2, d_l1, d_l2 = up(t1), up(t2), up(l1), up(l2)
    d_rc = torch.zeros(len(t2), dtype=torch.int64, device="cuda")
    cap = al.arena_hint(n)
    d_r1 = torch.zeros(4 * n, dtype=torch.int32, device="cuda"); d_r2 = torch.zeros(4 * n, dtype=torch.int32, device="cuda")
    d_a1 = torch.zeros(cap, dtype=torch.int32, device="cuda"); d_a2 = torch.zeros(cap, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    out = {"pairs": n, "index": a.index, "transcripts": tx.num_transcripts, "mate_len": MATE, "fragment": FRAG}

    out["revcomp_ms"], _ = timed(lambda: al.revcomp_tiles_device(d_t2.data_ptr(), d_l2.data_ptr(), n, wpr, d_rc.data_ptr()))

    def two_maps():
        al.map_batch_device(d_t1.data_ptr(), d_l1.data_ptr(), n, wpr, d_r1.data_ptr(), d_a1.data_ptr(), cap)
        al.map_finish()
        al.map_batch_device(d_rc.data_ptr(), d_l2.data_ptr(), n, wpr, d_r2.data_ptr(), d_a2.data_ptr(), cap)
        al.map_finish()
    out["two_maps_ms"], _ = timed(two_maps)

    pcap = 8 * n + 4096
    d_pr = torch.zeros(4 * n, dtype=torch.int32, device="cuda")
    d_pa = torch.zeros(pcap, dtype=torch.int32, device="cuda")
    sb = al.pairs_scratch_bytes(n)
    d_scr = torch.empty(sb + 256, dtype=torch.uint8, device="cuda")
    scr = (d_scr.data_ptr() + 255) & ~255
    counts = torch.zeros(al.counts_len(), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    last = {}

    def combine(d_counts):
        al.pairs_combine_device(d_r1.data_ptr(), d_a1.data_ptr(), d_r2.data_ptr(), d_a2.data_ptr(), n, d_pr.data_ptr(), d_pa.data_ptr(), pcap, scr, sb, d_counts=d_counts)
        last["stats"], last["used"], _ = al.pairs_finish(scr)
    out["combine_ms"], _ = timed(lambda: combine(0))
    ovf = pa.Overflow(0, 1 << 22, 1 << 26)
    al.set_overflow(ovf)
    out["combine_table_overflow_ms"], _ = timed(lambda: combine(counts.data_ptr()))
    al.set_overflow(None)
    out["stats"] = last["stats"]
    # bytes the combine stage must move: the records, and the ids of the pairs that are not settled where they are classified
    r1 = d_r1.cpu().numpy().view(pa.RESULT_DTYPE); r2 = d_r2.cpu().numpy().view(pa.RESULT_DTYPE)
    mp1, mp2 = (r1["mismatches"] >> 31).astype(bool), (r2["mismatches"] >> 31).astype(bool)
    ref1, ref2 = (r1["class_off"] >> 31).astype(bool), (r2["class_off"] >> 31).astype(bool)
    both = mp1 & mp2 & (r1["class_len"] > 0) & (r2["class_len"] > 0) & ~(ref1 & ref2 & (r1["class_off"] == r2["class_off"]))
    alone = (mp1 ^ mp2) & np.where(mp1, ~ref1 & (r1["class_len"] > 0), ~ref2 & (r2["class_len"] > 0))
    ids_in = int((r1["class_len"][both].astype(np.int64) + r2["class_len"][both]).sum() + np.where(mp1, r1["class_len"], r2["class_len"])[alone].astype(np.int64).sum())
    out["combine_bytes"] = 48 * n + 4 * (ids_in + int(last["used"]))
    out["combine_over_two_maps"] = out["combine_ms"] / out["two_maps_ms"]
    out["combine_GBps_of_must_move"] = out["combine_bytes"] / out["combine_ms"] / 1e6

    out["count_pairs"] = count_pairs_leg(a, al, m1, m2, ["fr"])["fr"]
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
