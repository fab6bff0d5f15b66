"""BUS output, measured next to the cell counter: prints one JSON line with
  bus_add_ms_per_10M / bus_finish_ms      pa_bus_add_device per 10 M device-resident pairs (R2s mapped beforehand, R1s in HBM) and pa_bus_finish
  cells_add_ms_per_10M / cells_finish_ms  pa_cell_counter_add_device and pa_cell_counter_finish on the same records in the same process
each as the median of `--rounds` rounds with its min and max; within a round the two take turns chunk by chunk (who goes first alternates),
so that both see the same clocks. Then
  file_pairs_per_s, file_stages_s         pa_write_bus on the plain R1 / R2 FASTQ tools/bench_cells.py makes (files in the page cache)
  --input plain|bgzf, --host-scan, --calls N   the file-level leg on BGZF files / on the host path / timed N times (tools/pairs_input.py);
  --files-only skips the device-resident leg
Usage: python tools/bench_bus.py [--pairs N] [--rounds R] [--threads T] [--dir DIR] [--no-files] [--input plain|bgzf] [--host-scan] [--calls N] [--files-only]"""
import argparse
import json
import statistics
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))

import pairs_input
from bench_cells import BASES, fastq_chunk, make_pairs   # the same pairs and the same files


def spread(xs):
    return {"median": round(statistics.median(xs), 2), "min": round(min(xs), 2), "max": round(max(xs), 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=10_000_000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--cells", type=int, default=10_000)
    ap.add_argument("--whitelist", type=int, default=100_000)
    ap.add_argument("--dir", default=None)
    ap.add_argument("--no-files", action="store_true")
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
    wl_text = [bytes(r).decode() for r in whitelist]
    print("[bench_bus] index + data setup %.1f s" % (time.perf_counter() - t0), file=sys.stderr)

    # ---- device-resident leg: chunks of 1 M pairs mapped once and kept in HBM ----
    dev = torch.device("cuda")
    chunk = 1_000_000
    chunks = []
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
        used, _ = al.map_finish()
        torch.cuda.synchronize()
        chunks.append((d_res, d_arena, used, d_r1, d_r1off, m))
        del d_r2, d_r2off, d_tiles, d_lens
    print("[bench_bus] %d chunks mapped %.1f s" % (len(chunks), time.perf_counter() - t0), file=sys.stderr)

    def timed(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = fn()
        return (time.perf_counter() - t) * 1e3, out

    times = {"bus_add": [], "bus_finish": [], "cells_add": [], "cells_finish": []}
    bus_stats = cells_stats = None
    n_records = n_ecs = entries = 0
    for rnd in range(0 if a.files_only else a.rounds + 1):   # (round 0 warms the allocators and the code objects up and is left out)
        bus = pa.BusWriter(al, host, bc_len, umi_len)
        counter = pa.CellCounter(al, host, tx_gene, len(names), wl_text, bc_len, umi_len)
        t_bus = t_cells = 0.0
        for j, (d_res, d_arena, used, d_r1, d_r1off, m) in enumerate(chunks):
            add_bus = lambda: bus.add_device(d_res.data_ptr(), d_arena.data_ptr(), used, d_r1.data_ptr(), d_r1off.data_ptr(), m)
            add_cells = lambda: counter.add_device(d_res.data_ptr(), d_arena.data_ptr(), d_r1.data_ptr(), d_r1off.data_ptr(), m)
            if (rnd + j) % 2 == 0:
                t_bus += timed(add_bus)[0]
                t_cells += timed(add_cells)[0]
            else:
                t_cells += timed(add_cells)[0]
                t_bus += timed(add_bus)[0]
        if rnd % 2 == 0:
            f_bus, (n_records, n_ecs) = timed(bus.finish)
            f_cells, entries = timed(counter.finish)
        else:
            f_cells, entries = timed(counter.finish)
            f_bus, (n_records, n_ecs) = timed(bus.finish)
        bus_stats, cells_stats = bus.stats(), counter.stats()
        del bus, counter
        if rnd == 0:
            continue
        times["bus_add"].append(t_bus * 1e7 / a.pairs)
        times["bus_finish"].append(f_bus)
        times["cells_add"].append(t_cells * 1e7 / a.pairs)
        times["cells_finish"].append(f_cells)
    del chunks
    torch.cuda.empty_cache()
    result = {"pairs": a.pairs, "rounds": a.rounds, "threads": a.threads, "cells": a.cells, "read_len": read_len}
    if not a.files_only:
        result.update({
              "bus_add_ms_per_10M": spread(times["bus_add"]), "bus_finish_ms": spread(times["bus_finish"]),
              "cells_add_ms_per_10M": spread(times["cells_add"]), "cells_finish_ms": spread(times["cells_finish"]),
              "add_ratio_bus_over_cells": round(statistics.median(times["bus_add"]) / statistics.median(times["cells_add"]), 3),
              "finish_ratio_bus_over_cells": round(statistics.median(times["bus_finish"]) / statistics.median(times["cells_finish"]), 3),
              "bus_records": n_records, "bus_ecs": n_ecs, "matrix_entries": entries, "bus_stats": bus_stats, "cells_stats": cells_stats})

    # ---- file-level leg: the same number of pairs as plain FASTQ ----
    if not a.no_files:
        t1 = time.perf_counter()
        p1, p2 = d / ("r1.fq" + pairs_input.suffix(a)), d / ("r2.fq" + pairs_input.suffix(a))
        with pairs_input.Writer(p1, a.input) as f1, pairs_input.Writer(p2, a.input) as f2:
            for first in range(0, a.pairs, chunk):
                m = min(chunk, a.pairs - first)
                r1, r2 = make_pairs(rng, txome_bytes, starts, lens, cells, m, read_len, umi_len)
                f1.write(fastq_chunk(first, r1))
                f2.write(fastq_chunk(first, r2))
        print("[bench_bus] files written in %.1f s" % (time.perf_counter() - t1), file=sys.stderr)
        out = d / "out"
        out.mkdir()
        al.write_bus(host, p1, p2, out, bc_len, umi_len, num_threads=a.threads)   # warm-up: page cache, buffers
        secs, file_stats = pairs_input.timed_calls(lambda: al.write_bus(host, p1, p2, out, bc_len, umi_len, num_threads=a.threads), a.calls)
        file_s = secs[-1]
        st = (pa._ffi.C.c_double * 8)()
        pa.lib().pa_process_reads_stage_seconds(st)
        stages = dict(zip(("scan", "gather", "map_wait", "launch", "bus", "write", "whole", "pairs"), [round(x, 4) for x in st]))
        result.update({"file_seconds": round(file_s, 3), "file_pairs_per_s": round(a.pairs / file_s), "file_stages_s": stages,
                       "bus_share_of_file_call": round(stages["bus"] / stages["whole"], 4) if stages["whole"] else None,
                       "output_bus_bytes": (out / "output.bus").stat().st_size, "file_stats": file_stats, **pairs_input.report(pa, a, a.pairs, secs)})
    print(json.dumps(result))
    tmp.cleanup()


if __name__ == "__main__":
    main()
