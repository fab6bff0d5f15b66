"""The gene counter, measured: prints one JSON line with
  setup_ms          pa_genes_create on host arrays (upload + molecule stage + per-cell layout), median of --rounds with min and max
  step200_ms        pa_genes_step(200) from the start point (every cell with multi rows, no stop rule), and the same per iteration
  run_ms            pa_genes_run to the stop rule from the start point, with the iteration counts it reports
  matrix_ms         pa_genes_matrix (D2H + the host merge)
on `--cells` x `--molecules` synthetic molecules over `--genes` genes, a share `--multi` of them with two or three genes (gene families
{2k, 2k+1} and {3k, 3k+1, 3k+2}; a cell expresses a Zipf-like subset). With --pairs N also the file-level leg: pa_count_cells_em beside
pa_write_bus on the same plain FASTQ pair (the files of tools/bench_cells.py), seconds and stage seconds of each.
Usage: python tools/bench_genes.py [--cells N] [--molecules M] [--genes G] [--multi 0.15] [--rounds R] [--pairs N] [--threads T] [--dir DIR]"""
import argparse
import importlib
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


def spread(xs):
    return {"median": round(statistics.median(xs), 3), "min": round(min(xs), 3), "max": round(max(xs), 3)}


def synthetic(pa, n_cells, molecules, genes, multi, seed):
    """one record per molecule, (barcode, UMI) ascending by construction; ecs: g, genes + pair, genes + genes // 2 + triple"""
    rng = np.random.default_rng(seed)
    n = n_cells * molecules
    weights = 1.0 / np.arange(1, genes + 1) ** 0.9
    gene = rng.choice(genes, n, p=weights / weights.sum()).astype(np.int64)
    gene = (gene * 7919 + np.repeat(rng.integers(0, genes, n_cells), molecules)) % genes      # every cell its own favourites
    kind = rng.random(n)
    pairs, triples = genes // 2, genes // 3
    ec = gene.copy()
    is_pair = (kind < multi * 0.6) & (gene // 2 < pairs)
    is_triple = (kind >= multi * 0.6) & (kind < multi) & (gene // 3 < triples)
    ec[is_pair] = genes + gene[is_pair] // 2
    ec[is_triple] = genes + pairs + gene[is_triple] // 3
    rec = np.zeros(n, pa.BUS_RECORD_DTYPE)
    rec["barcode"] = np.repeat(np.arange(n_cells, dtype=np.uint64) * 5 + 1, molecules)
    rec["umi"] = np.tile(np.arange(molecules, dtype=np.uint64), n_cells)
    rec["ec"] = ec
    rec["count"] = 1
    lists = [np.arange(genes)[:, None], np.arange(2 * pairs).reshape(pairs, 2), np.arange(3 * triples).reshape(triples, 3)]
    ids = np.concatenate([l.reshape(-1) for l in lists]).astype(np.uint32)
    off = np.cumsum(np.concatenate([[0], np.ones(genes, np.int64), np.full(pairs, 2), np.full(triples, 3)])).astype(np.uint64)
    return rec, off, ids, np.arange(genes, dtype=np.uint32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=10_000)
    ap.add_argument("--molecules", type=int, default=3_000)
    ap.add_argument("--genes", type=int, default=20_000)
    ap.add_argument("--multi", type=float, default=0.15)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--pairs", type=int, default=0)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--dir", default=None)
    a = ap.parse_args()
    pa = importlib.import_module("rust-pseudoaligner_amd")
    t0 = time.perf_counter()
    tmp = tempfile.TemporaryDirectory(dir=a.dir)
    d = Path(tmp.name)
    tx = pa.Txome.synthesize(5000, 17000, 7)
    from bench_cells import BASES, fastq_chunk, make_pairs
    packed, tx_start = tx.arrays()
    pos = np.arange(int(tx_start[-1]), dtype=np.int64)
    txome_bytes = BASES[((packed[pos >> 5] >> ((pos & 31) * 2).astype(np.uint64)) & np.uint64(3)).astype(np.int64)]
    with open(d / "tx.fa", "w") as f:
        for t in range(len(tx_start) - 1):
            f.write(">T%d|G%d|-|-|-|G%d|%d|protein_coding|\n%s\n" % (t, t // 4, t // 4, int(tx_start[t + 1] - tx_start[t]),
                                                                         txome_bytes[int(tx_start[t]):int(tx_start[t + 1])].tobytes().decode()))
    host = pa.build_index(str(d / "tx.fa"), 31, a.threads)
    al = pa.Pseudoaligner(host)
    rec, off, ids, tx_gene = synthetic(pa, a.cells, a.molecules, a.genes, a.multi, 7)
    print("[bench_genes] index + %d records in %.1f s" % (len(rec), time.perf_counter() - t0), file=sys.stderr)

    def timed(fn):
        t = time.perf_counter()
        out = fn()
        return (time.perf_counter() - t) * 1e3, out

    make = lambda: pa.GeneCounter.from_arrays(al, rec, off, ids, tx_gene, a.genes, 16, 12)
    times = {"setup": [], "step200": [], "run": [], "matrix": []}
    stats = report = None
    for rnd in range(a.rounds + 1):   # (round 0 warms the allocators and the code objects up and is left out)
        ms_setup, g = timed(make)
        ms_step, _ = timed(lambda: g.step(200))
        del g
        g = make()
        ms_run, report = timed(g.run)
        ms_matrix, m = timed(g.matrix)
        stats = g.stats()
        del g, m
        if rnd:
            for k, v in zip(("setup", "step200", "run", "matrix"), (ms_setup, ms_step, ms_run, ms_matrix)):
                times[k].append(v)
    result = {"cells": a.cells, "molecules_per_cell": a.molecules, "genes": a.genes, "multi_share": a.multi, "rounds": a.rounds,
              "setup_ms": spread(times["setup"]), "step200_ms": spread(times["step200"]), "ms_per_iteration": round(statistics.median(times["step200"]) / 200, 4),
              "run_ms": spread(times["run"]), "run_most_iterations": report[0], "run_cells_not_converged": report[1], "matrix_ms": spread(times["matrix"]),
              "stats": stats}
    if a.pairs:
        rng = np.random.default_rng(7)
        starts, lens = tx_start[:-1].astype(np.int64), np.diff(tx_start.astype(np.int64))
        cells = np.unique(BASES[rng.integers(0, 4, (a.cells, 16))], axis=0)
        p1, p2 = d / "r1.fq", d / "r2.fq"
        with open(p1, "wb") as f1, open(p2, "wb") as f2:
            for first in range(0, a.pairs, 1_000_000):
                m = min(1_000_000, a.pairs - first)
                r1, r2 = make_pairs(rng, txome_bytes, starts, lens, cells, m, 90, 12)
                f1.write(fastq_chunk(first, r1))
                f2.write(fastq_chunk(first, r2))
        out = d / "out"
        out.mkdir()
        stage = (pa._ffi.C.c_double * 8)()
        names = ("scan", "gather", "map_wait", "launch", "tally", "write", "whole", "pairs")
        legs = {}
        for leg, fn in (("write_bus", lambda: al.write_bus(host, p1, p2, out, 16, 12, num_threads=a.threads)),
                        ("count_cells_em", lambda: al.count_cells_em(host, p1, p2, out, 16, 12, num_threads=a.threads))):
            fn()                                                   # warm-up: page cache, buffers
            secs = []
            for _ in range(3):
                ms, st = timed(fn)
                secs.append(ms / 1e3)
            pa.lib().pa_process_reads_stage_seconds(stage)
            legs[leg] = {"seconds": spread(secs), "stages_s": dict(zip(names, [round(x, 4) for x in stage])), "stats": st}
        result.update({"file_pairs": a.pairs, "file_legs": legs})
    print(json.dumps(result))
    tmp.cleanup()


if __name__ == "__main__":
    main()
