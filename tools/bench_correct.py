"""The BUS barcode correction, measured: prints one JSON line per setting with the GPU milliseconds of the four phases of
pa_bus_correct_records (pa_bus_correct_phase_ms; median of --rounds runs after --warmup, with min and max)
  table_ms                 whitelist upload, sort, insert into the open-addressing table
  classify_exact_ms        distinct barcodes of the records (heads, scan, scatter), one exact probe each, the miss list
  classify_neighbours_ms   a group of lanes per missed barcode, its 3 bc_len substitutions probed
  rewrite_ms               kept records as keys, radix sort over the live bits, collapse, whole records
on synthetic sorted records: `--records` reads of `--cells` true cells (barcodes drawn from a whitelist of `--whitelist` random 16-base
barcodes, 12-base UMIs); a share `--bc-error-rate` of them carries one barcode substitution and a share `--off-list-share` a random
barcode that is (almost surely) not listed. Several rates / shares may be given, comma separated: every pair is one setting. The records
go up from the host in every run (that copy and the host's checks are not in the phases); `wall_ms` is the whole call.
Usage: python tools/bench_correct.py [--records N] [--cells C] [--whitelist W] [--bc-error-rate r,..] [--off-list-share s,..] [--rounds 5] [--warmup 2] [--out FILE]"""
import argparse
import ctypes as C
import importlib
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
BC, UMI = 16, 12


def spread(xs):
    return {"median": round(statistics.median(xs), 3), "min": round(min(xs), 3), "max": round(max(xs), 3)}


def synthetic(pa, whitelist, n_records, n_cells, error_rate, off_share, seed):
    """strictly ascending (barcode, UMI, ec) records: one per distinct (barcode, UMI), ec a function of them"""
    rng = np.random.default_rng(seed)
    cells = whitelist[rng.choice(len(whitelist), n_cells, replace=False)]
    bc = cells[rng.integers(0, n_cells, n_records)]
    kind = rng.random(n_records)
    err = kind < error_rate
    bc[err] ^= rng.integers(1, 4, int(err.sum())).astype(np.uint64) << (2 * rng.integers(0, BC, int(err.sum()))).astype(np.uint64)
    off = (kind >= error_rate) & (kind < error_rate + off_share)
    bc[off] = rng.integers(0, 4 ** BC, int(off.sum()), dtype=np.uint64)
    key = np.unique((bc << np.uint64(2 * UMI)) | rng.integers(0, 4 ** UMI, n_records, dtype=np.uint64))
    rec = np.zeros(len(key), pa.BUS_RECORD_DTYPE)
    rec["barcode"] = key >> np.uint64(2 * UMI)
    rec["umi"] = key & np.uint64(4 ** UMI - 1)
    rec["ec"] = (key % np.uint64(1000)).astype(np.int32)
    rec["count"] = 1
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=50_000_000)
    ap.add_argument("--cells", type=int, default=10_000)
    ap.add_argument("--whitelist", type=int, default=6_800_000)
    ap.add_argument("--bc-error-rate", default="0.01")
    ap.add_argument("--off-list-share", default="0.01")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    pa = importlib.import_module("rust-pseudoaligner_amd")
    tx = pa.Txome.synthesize(50, 150, 7)
    al = pa.Pseudoaligner(pa.HostIndex.from_txome(tx, 31, 4))      # (names the GPU; the index itself is not used)
    rng = np.random.default_rng(1)
    wl = np.unique(rng.integers(0, 4 ** BC, int(a.whitelist * 1.01) + 16, dtype=np.uint64))
    wl = wl[rng.permutation(len(wl))[:a.whitelist]].copy()
    results = []
    for rate in [float(x) for x in a.bc_error_rate.split(",")]:
        for share in [float(x) for x in a.off_list_share.split(",")]:
            t0 = time.perf_counter()
            rec = synthetic(pa, wl, a.records, a.cells, rate, share, 7)
            print("[bench_correct] %d records (rate %g, off-list %g) in %.1f s" % (len(rec), rate, share, time.perf_counter() - t0), file=sys.stderr, flush=True)
            st = np.zeros(pa._ffi.PA_BUS_CORRECT_STATS, np.uint64)
            n_out = C.c_uint64()
            phases = {k: [] for k in pa._ffi.CORRECT_PHASE_NAMES}
            wall = []
            for rnd in range(a.warmup + a.rounds):
                t = time.perf_counter()
                pa.check(pa.lib().pa_bus_correct_records(al._h, rec.ctypes.data, len(rec), BC, UMI, wl.ctypes.data, len(wl), None, 0, C.byref(n_out), st.ctypes.data))
                ms = (time.perf_counter() - t) * 1e3
                if rnd >= a.warmup:
                    wall.append(ms)
                    for k, v in pa.bus_correct_phase_ms().items():
                        phases[k].append(v)
                print("[bench_correct] run %d: %.0f ms" % (rnd, ms), file=sys.stderr, flush=True)
            med = {k: statistics.median(v) for k, v in phases.items()}
            results.append({"records": len(rec), "cells": a.cells, "whitelist": len(wl), "table_slots": 1 << int(np.ceil(np.log2(2 * len(wl)))), "bc_error_rate": rate,
                            "off_list_share": share, "rounds": a.rounds, "warmup": a.warmup, **{k: spread(v) for k, v in phases.items()}, "gpu_ms": round(sum(med.values()), 3),
                            "bound": max(med, key=med.get), "wall_ms": spread(wall), "stats": dict(zip(pa.CORRECT_STAT_NAMES, (int(x) for x in st)))})
            print(json.dumps(results[-1]), flush=True)
            del rec
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(results, indent=1) + "\n")


if __name__ == "__main__":
    main()
