"""Cell calling on BUS records, measured: prints one JSON line with the GPU milliseconds of the three phases of
pa_bus_knee_records (pa_bus_knee_phase_ms; median of --rounds runs after --warmup, with min and max)
  table_ms         the barcode table: tile totals, the scan over them, the head rows, their differences
  rank_curve_ms    the descending sort of the rows' molecule counts, the ranks, the run-length encoded curve
  called_rows_ms   the threshold (host), the rows, the called list
on synthetic sorted records: `--records` records, most of them of `--cells` true cells, the rest an ambient tail of `--ambient` random barcodes
with one to five molecules each (16-base barcodes, 12-base UMIs, one record per molecule). The yardstick of the table phase is a
device-to-device copy of the same record bytes (32 B x n) timed in the same job with device events: `table_over_copy` is the ratio of the two
medians. The records go up from the host in every run (that copy and the host's checks are not in the phases); `wall_ms` is the whole call.
pa_bus_keep_records with the called list is timed as a whole call (`keep_wall_ms`: it has no phase clock, so the upload is in it), next to
`upload_wall_ms`, a plain host-to-device copy of the same bytes.
Usage: python tools/bench_knee.py [--records N] [--cells C] [--ambient A] [--rounds 5] [--warmup 2] [--out FILE]"""
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


def synthetic(pa, n_records, n_cells, n_ambient, seed):
    """strictly ascending (barcode, UMI, ec) records: one per distinct (barcode, UMI), ec a function of them"""
    rng = np.random.default_rng(seed)
    names = np.unique(rng.integers(0, 4 ** BC, int((n_cells + n_ambient) * 1.01) + 16, dtype=np.uint64))
    names = names[rng.permutation(len(names))[:n_cells + n_ambient]]
    tail = np.repeat(names[n_cells:], rng.integers(1, 6, n_ambient))
    bc = np.concatenate([names[rng.integers(0, n_cells, max(n_records - len(tail), n_cells))], tail])
    key = np.unique((bc << np.uint64(2 * UMI)) | rng.integers(0, 4 ** UMI, len(bc), dtype=np.uint64))
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
    ap.add_argument("--ambient", type=int, default=3_000_000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    pa = importlib.import_module("rust-pseudoaligner_amd")
    tx = pa.Txome.synthesize(50, 150, 7)
    al = pa.Pseudoaligner(pa.HostIndex.from_txome(tx, 31, 4))      # (names the GPU; the index itself is not used)
    t0 = time.perf_counter()
    rec = synthetic(pa, a.records, a.cells, a.ambient, 7)
    print("[bench_knee] %d records in %.1f s" % (len(rec), time.perf_counter() - t0), file=sys.stderr, flush=True)
    runs = range(a.warmup + a.rounds)

    # the yardsticks: the same bytes copied device to device (events), and host to device (wall)
    nbytes = len(rec) * rec.itemsize
    src = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    host_bytes = torch.from_numpy(rec.view(np.uint8))
    copy_ms, upload_ms = [], []
    for rnd in runs:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        dst.copy_(src)
        e1.record()
        torch.cuda.synchronize()
        t = time.perf_counter()
        src.copy_(host_bytes)
        torch.cuda.synchronize()
        if rnd >= a.warmup:
            copy_ms.append(e0.elapsed_time(e1))
            upload_ms.append((time.perf_counter() - t) * 1e3)
    del src, dst, host_bytes
    torch.cuda.empty_cache()

    st = np.zeros(pa._ffi.PA_KNEE_STATS, np.uint64)
    n_rows, n_called = C.c_uint64(), C.c_uint64()
    phases = {k: [] for k in pa._ffi.KNEE_PHASE_NAMES}
    wall = []
    for rnd in runs:
        t = time.perf_counter()
        pa.check(pa.lib().pa_bus_knee_records(al._h, rec.ctypes.data, len(rec), BC, UMI, None, None, 0, C.byref(n_rows), None, 0, C.byref(n_called), st.ctypes.data))
        ms = (time.perf_counter() - t) * 1e3
        if rnd >= a.warmup:
            wall.append(ms)
            for k, v in pa.bus_knee_phase_ms().items():
                phases[k].append(v)
        print("[bench_knee] knee run %d: %.0f ms" % (rnd, ms), file=sys.stderr, flush=True)
    rows, called, _ = pa.bus_knee(rec, BC, UMI, al)
    kst = np.zeros(pa._ffi.PA_BUS_KEEP_STATS, np.uint64)
    n_out = C.c_uint64()
    keep_wall = []
    for rnd in runs:
        t = time.perf_counter()
        pa.check(pa.lib().pa_bus_keep_records(al._h, rec.ctypes.data, len(rec), BC, UMI, called.ctypes.data, len(called), None, 0, C.byref(n_out), kst.ctypes.data))
        if rnd >= a.warmup:
            keep_wall.append((time.perf_counter() - t) * 1e3)
    med = {k: statistics.median(v) for k, v in phases.items()}
    result = {"records": len(rec), "cells": a.cells, "ambient": a.ambient, "record_bytes": nbytes, "rounds": a.rounds, "warmup": a.warmup,
              **{k: spread(v) for k, v in phases.items()}, "gpu_ms": round(sum(med.values()), 3), "d2d_copy_ms": spread(copy_ms),
              "table_over_copy": round(med["table_ms"] / statistics.median(copy_ms), 3), "wall_ms": spread(wall), "keep_wall_ms": spread(keep_wall),
              "upload_wall_ms": spread(upload_ms), "stats": dict(zip(pa.KNEE_STAT_NAMES, (int(x) for x in st))),
              "keep_stats": dict(zip(pa.KEEP_STAT_NAMES, (int(x) for x in kst)))}
    print(json.dumps(result), flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps([result], indent=1) + "\n")


if __name__ == "__main__":
    main()
