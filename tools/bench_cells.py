"""Single-cell UMI counting, measured (DESIGN.md "Single-cell UMI counts"): prints one JSON line with
  add_device_ms_per_10M   pa_cell_counter_add_device per 10 M device-resident pairs (R2s mapped beforehand, R1s in HBM)
  finish_ms               pa_cell_counter_finish of that run (UMI correction, gene conflicts, count)
  file_pairs_per_s        pa_count_cells on generated plain R1 / R2 FASTQ of the same size (files in the page cache)
  file_stages_s           that call's stage split (pa_process_reads_stage_seconds)
  --input plain|bgzf, --host-scan, --calls N   the file-level leg on BGZF files / on the host path / timed N times (tools/pairs_input.py);
  --files-only skips the device-resident leg
Usage: python tools/bench_cells.py [--pairs N] [--threads T] [--dir DIR] [--input plain|bgzf] [--host-scan] [--calls N] [--files-only]"""
import argparse
import json
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))

import pairs_input

BASES = np.frombuffer(b"ACGT", np.uint8)


def fastq_chunk(first, seqs):
    """fixed-length records '@p<9 digits>\\n<seq>\\n+\\n<qual>\\n' for rows of seqs (n, L) uint8"""
    n, L = seqs.shape
    rec = np.empty((n, 11 + L + 3 + L + 1), np.uint8)
    rec[:, 0] = ord("@")
    rec[:, 1] = ord("p")
    ids = np.arange(first, first + n, dtype=np.int64)
    for k in range(9):
        rec[:, 10 - k] = 48 + (ids // 10 ** k) % 10
    rec[:, 11] = ord("\n")
    rec[:, 12:12 + L] = seqs
    rec[:, 12 + L:15 + L] = np.frombuffer(b"\n+\n", np.uint8)
    rec[:, 15 + L:15 + 2 * L] = ord("I")
    rec[:, -1] = ord("\n")
    return rec.tobytes()


def make_pairs(rng, txome_bytes, starts, lens, whitelist, n, read_len, umi_len):
    """(R1 rows (n, bc + umi), R2 rows (n, read_len)): R2 cut from transcripts, R1 = a whitelisted barcode (3 % with one substitution)
    + a random UMI"""
    ok = np.nonzero(lens >= read_len)[0]
    w = (lens[ok] - read_len + 1).astype(np.float64)
    t = ok[np.searchsorted(np.cumsum(w) / w.sum(), rng.random(n))]
    pos = starts[t] + (rng.random(n) * (lens[t] - read_len + 1)).astype(np.int64)
    r2 = txome_bytes[pos[:, None] + np.arange(read_len)[None, :]]
    bc = whitelist[rng.integers(0, len(whitelist), n)].copy()
    hit = np.nonzero(rng.random(n) < 0.03)[0]
    bc[hit, rng.integers(0, bc.shape[1], len(hit))] = BASES[rng.integers(0, 4, len(hit))]
    r1 = np.concatenate([bc, BASES[rng.integers(0, 4, (n, umi_len))]], axis=1)
    return r1, r2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=10_000_000)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--cells", type=int, default=10_000)
    ap.add_argument("--whitelist", type=int, default=100_000)
    ap.add_argument("--dir", default=None)
    ap.add_argument("--files-only", action="store_true")
    pairs_input.add_args(ap)
    a = ap.parse_args()
    pairs_input.apply(a)
    import torch
    import importlib
    pa = importlib.import_module("rust-pseudoaligner_amd")
    bc_len, umi_len, read_len = 16, 12, 90
    rng = np.random.default_rng(7)
    t0 = time.perf_counter()
    tmp = tempfile.TemporaryDirectory(dir=a.dir)
    d = Path(tmp.name)
    # a synthesized transcriptome written as GENCODE-style FASTA (four transcripts to a gene: the gene names reach features.tsv)
    tx = pa.Txome.synthesize(5000, 17000, 7)
    packed, tx_start = tx.arrays()
    total = int(tx_start[-1])
    pos = np.arange(total, dtype=np.int64)
    txome_bytes = BASES[((packed[pos >> 5] >> ((pos & 31) * 2).astype(np.uint64)) & np.uint64(3)).astype(np.int64)]
    with open(d / "tx.fa", "w") as f:
        for t in range(len(tx_start) - 1):
            f.write(">T%d|G%d|-|-|-|G%d|%d|protein_coding|\n%s\n" % (t, t // 4, t // 4, int(tx_start[t + 1] - tx_start[t]),
                                                                         txome_bytes[int(tx_start[t]):int(tx_start[t + 1])].tobytes().decode()))
    host = pa.build_index(str(d / "tx.fa"), 31, a.threads)
    al = pa.Pseudoaligner(host)
    tx_gene, names = host.genes()
    starts = tx_start[:-1].astype(np.int64)
    lens = np.diff(tx_start.astype(np.int64))
    whitelist = BASES[rng.integers(0, 4, (a.whitelist, bc_len))]
    whitelist = np.unique(whitelist, axis=0)
    cells = whitelist[rng.choice(len(whitelist), a.cells, replace=False)]
    print("[bench_cells] index + data setup %.1f s" % (time.perf_counter() - t0), file=sys.stderr)

    # ---- device-resident leg: chunks of 1 M pairs mapped on the GPU, then counted ----
    dev = torch.device("cuda")
    add_s = finish_s = 0.0
    entries, dev_stats = 0, None
    chunk = 1_000_000
    counter = None if a.files_only else pa.CellCounter(al, host, tx_gene, len(names), [bytes(r).decode() for r in whitelist], bc_len, umi_len)
    for first in range(0, 0 if a.files_only else a.pairs, chunk):
        m = min(chunk, a.pairs - first)
        r1, r2 = make_pairs(rng, txome_bytes, starts, lens, cells, m, read_len, umi_len)
        d_r2 = torch.from_numpy(r2.reshape(-1)).to(dev)
        d_r2off = torch.from_numpy(np.arange(0, (m + 1) * read_len, read_len, dtype=np.int64)).to(dev)
        d_r1 = torch.from_numpy(r1.reshape(-1)).to(dev)
        d_r1off = torch.from_numpy(np.arange(0, (m + 1) * (bc_len + umi_len), bc_len + umi_len, dtype=np.int64)).to(dev)
        wpr = pa.lib().pa_words_per_read(read_len)
        d_tiles = torch.empty(pa.lib().pa_tiles_words(m, wpr), dtype=torch.int64, device=dev)
        d_lens = torch.empty(m + 64, dtype=torch.int32, device=dev)
        d_res = torch.empty(m * 4, dtype=torch.int32, device=dev)
        cap = al.arena_hint(m)
        d_arena = torch.empty(cap, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        al.encode_reads_device(d_r2.data_ptr(), d_r2off.data_ptr(), m, wpr, d_tiles.data_ptr(), d_lens.data_ptr())
        al.map_batch_device(d_tiles.data_ptr(), d_lens.data_ptr(), m, wpr, d_res.data_ptr(), d_arena.data_ptr(), cap)
        al.map_finish()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        counter.add_device(d_res.data_ptr(), d_arena.data_ptr(), d_r1.data_ptr(), d_r1off.data_ptr(), m)
        add_s += time.perf_counter() - t1
        del d_r2, d_r1, d_tiles, d_res, d_arena
    if counter is not None:
        t1 = time.perf_counter()
        entries = counter.finish()
        finish_s = time.perf_counter() - t1
        dev_stats = counter.stats()
        del counter
    torch.cuda.empty_cache()

    # ---- file-level leg: the same number of pairs as plain FASTQ ----
    t1 = time.perf_counter()
    p1, p2 = d / ("r1.fq" + pairs_input.suffix(a)), d / ("r2.fq" + pairs_input.suffix(a))
    with pairs_input.Writer(p1, a.input) as f1, pairs_input.Writer(p2, a.input) as f2:
        for first in range(0, a.pairs, chunk):
            m = min(chunk, a.pairs - first)
            r1, r2 = make_pairs(rng, txome_bytes, starts, lens, cells, m, read_len, umi_len)
            f1.write(fastq_chunk(first, r1))
            f2.write(fastq_chunk(first, r2))
    (d / "wl.txt").write_bytes(b"".join(bytes(r) + b"\n" for r in whitelist))
    print("[bench_cells] files written in %.1f s" % (time.perf_counter() - t1), file=sys.stderr)
    out = d / "out"
    out.mkdir()
    al.count_cells(host, p1, p2, d / "wl.txt", out, bc_len, umi_len, num_threads=a.threads)   # warm-up: page cache, buffers
    secs, file_stats = pairs_input.timed_calls(lambda: al.count_cells(host, p1, p2, d / "wl.txt", out, bc_len, umi_len, num_threads=a.threads), a.calls)
    file_s = secs[-1]
    st = (pa._ffi.C.c_double * 8)()
    pa.lib().pa_process_reads_stage_seconds(st)
    stages = dict(zip(("scan", "gather", "map_wait", "launch", "count", "write", "whole", "pairs"), [round(x, 4) for x in st]))
    print(json.dumps({"pairs": a.pairs, "threads": a.threads, "cells": a.cells, "whitelist": len(whitelist), "read_len": read_len,
                      "add_device_ms_per_10M": round(add_s * 1e3 * 1e7 / a.pairs, 2), "finish_ms": round(finish_s * 1e3, 2),
                      "matrix_entries": entries, "device_stats": dev_stats,
                      "file_seconds": round(file_s, 3), "file_pairs_per_s": round(a.pairs / file_s), "file_stages_s": stages,
                      "count_share_of_file_call": round(stages["count"] / stages["whole"], 4) if stages["whole"] else None,
                      "file_stats": file_stats, **pairs_input.report(pa, a, a.pairs, secs)}))
    tmp.cleanup()


if __name__ == "__main__":
    main()
