"""The UMI correction on BUS records, measured: prints one JSON line with the GPU milliseconds of the four phases of
pa_bus_umi_correct_records (pa_bus_umi_correct_phase_ms; median of --rounds runs after --warmup, with min and max)
  molecules_ms   heads over (barcode, UMI), gene sets by intersection, n(m) by a segmented sum, barcode segments and bins
  search_ms      the neighbour search: one launch per bin (lane, block with the UMIs in LDS, HBM)
  rewrite_ms     records of moved molecules under their target's UMI, radix sort over the live bits, collapse, whole records
  stats_ms       the counters that need the finished targets and records
on a synthetic sorted library: about `--records` records of 16-base barcodes and 12-base UMIs, `--cells` cells that share 60 % of the molecules and
`--ambient` tiny barcodes that share the rest, `--umi-error-rate` of the molecules with a copy one UMI substitution away, `--multi-gene` of them
under an ec of two genes. Two yardsticks are timed in the same job: a device-to-device copy of the records' bytes (events) and phase [3] (rewrite +
sort + collapse) of pa_bus_correct_records on the same records against their own barcodes, a few of them taken off the list so that the sort runs.
With --variant-so (a build of _build.build_umi_hbm_variant) a child process repeats the UMI correction under PA_PRODUCT_SO: its search phase is the
HBM variant on the barcodes that the block bin searched in LDS. The records go up from the host in every run (not in the phases).
Usage: python tools/bench_umi.py [--records N] [--cells C] [--ambient A] [--umi-error-rate r] [--multi-gene s] [--mode greatest|directional]
       [--rounds 2] [--warmup 1] [--variant-so FILE] [--out FILE]"""
import argparse
import ctypes as C
import importlib
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
BC, UMI, GENES = 16, 12, 2000


def spread(xs):
    return {"median": round(statistics.median(xs), 3), "min": round(min(xs), 3), "max": round(max(xs), 3)}


def mix(x):
    x = (x ^ (x >> np.uint64(33))) * np.uint64(0xff51afd7ed558ccd)
    return x ^ (x >> np.uint64(29))


def tables():
    """gene g = transcripts 2g, 2g + 1; ec g < GENES = {2g}; ec GENES + j = {2j, 2 ((7j + 3) mod GENES)}: two genes"""
    tx_gene = np.repeat(np.arange(GENES, dtype=np.uint32), 2)
    pairs = [sorted((2 * j, 2 * ((7 * j + 3) % GENES))) for j in range(GENES)]
    off = np.concatenate([np.arange(GENES + 1), GENES + 2 * np.arange(1, GENES + 1)]).astype(np.uint64)
    ids = np.concatenate([2 * np.arange(GENES), np.array(pairs).ravel()]).astype(np.uint32)
    return off, ids, tx_gene


def synthetic(dtype, n_records, n_cells, n_ambient, error_rate, multi_share, seed):
    """strictly ascending (barcode, UMI, ec) records, one per molecule: the ec and the count are functions of (barcode, UMI), an error copy carries its
    original's ec and one read"""
    rng = np.random.default_rng(seed)
    n0 = int(n_records / (1 + error_rate))
    names = np.unique(rng.integers(0, 4 ** BC, n_cells + n_ambient + 1024, dtype=np.uint64))
    names = names[rng.permutation(len(names))]
    n_in_cells = int(0.6 * n0)
    cells, ambient = names[:n_cells], names[n_cells:n_cells + n_ambient]                # (the draw may hold a few barcodes twice: the ambient list is then that much shorter)
    bc = np.concatenate([cells[rng.integers(0, len(cells), n_in_cells)], ambient[rng.integers(0, len(ambient), n0 - n_in_cells)]])
    key = np.unique((bc << np.uint64(2 * UMI)) | rng.integers(0, 4 ** UMI, n0, dtype=np.uint64))
    del bc
    pick = np.flatnonzero(rng.random(len(key)) < error_rate)
    err = np.unique(key[pick] ^ (rng.integers(1, 4, len(pick)).astype(np.uint64) << (2 * rng.integers(0, UMI, len(pick))).astype(np.uint64)))
    err = err[key[np.minimum(np.searchsorted(key, err), len(key) - 1)] != err]         # (a copy that lands on a molecule that exists is that molecule)
    h = mix(key)
    multi = (h % np.uint64(1000)) < np.uint64(int(multi_share * 1000))
    ec = ((h >> np.uint64(20)) % np.uint64(GENES)).astype(np.int32) + np.where(multi, GENES, 0).astype(np.int32)
    count = (1 + (h >> np.uint64(40)) % np.uint64(4)).astype(np.uint32)
    all_key = np.concatenate([key, err])
    all_ec = np.concatenate([ec, np.zeros(len(err), np.int32)])
    all_count = np.concatenate([count, np.ones(len(err), np.uint32)])
    orig = key[pick]
    # an error copy takes the ec of a molecule it is one substitution from: the 36 substitutions of the copy are looked up among the picked originals
    picked_sorted = np.sort(orig)
    picked_ec = ec[np.searchsorted(key, picked_sorted)]
    err_ec = np.full(len(err), -1, np.int32)
    for p in range(UMI):
        for s in (1, 2, 3):
            cand = err ^ (np.uint64(s) << np.uint64(2 * p))
            at = np.minimum(np.searchsorted(picked_sorted, cand), len(picked_sorted) - 1)
            hit = (picked_sorted[at] == cand) & (err_ec < 0)
            err_ec[hit] = picked_ec[at[hit]]
    all_ec[len(key):] = err_ec
    order = np.argsort(all_key, kind="stable")
    rec = np.zeros(len(all_key), dtype)
    rec["barcode"] = all_key[order] >> np.uint64(2 * UMI)
    rec["umi"] = all_key[order] & np.uint64(4 ** UMI - 1)
    rec["ec"] = all_ec[order]
    rec["count"] = all_count[order]
    assert (rec["ec"] >= 0).all()
    return rec


def run_umi(pa, al, rec, tabs, mode, warmup, rounds, tag):
    off, ids, tx_gene = tabs
    st = np.zeros(pa._ffi.PA_BUS_UMI_STATS, np.uint64)
    n_out = C.c_uint64()
    phases = {k: [] for k in pa._ffi.UMI_PHASE_NAMES}
    wall = []
    for rnd in range(warmup + rounds):
        t = time.perf_counter()
        pa.check(pa.lib().pa_bus_umi_correct_records(al._h, rec.ctypes.data, len(rec), off.ctypes.data, ids.ctypes.data, len(off) - 1, len(tx_gene), tx_gene.ctypes.data, GENES,
                                                     BC, UMI, pa._ffi.UMI_MODES[mode], None, 0, C.byref(n_out), st.ctypes.data))
        ms = (time.perf_counter() - t) * 1e3
        if rnd >= warmup:
            wall.append(ms)
            for k, v in pa.bus_umi_correct_phase_ms().items():
                phases[k].append(v)
        print("[bench_umi] %s run %d: %.0f ms" % (tag, rnd, ms), file=sys.stderr, flush=True)
    return {**{k: spread(v) for k, v in phases.items()}, "gpu_ms": round(sum(statistics.median(v) for v in phases.values()), 3), "wall_ms": spread(wall),
            "stats": dict(zip(pa.UMI_STAT_NAMES, (int(x) for x in st)))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=50_000_000)
    ap.add_argument("--cells", type=int, default=10_000)
    ap.add_argument("--ambient", type=int, default=8_000_000)
    ap.add_argument("--umi-error-rate", type=float, default=0.03)
    ap.add_argument("--multi-gene", type=float, default=0.15)
    ap.add_argument("--mode", default="greatest")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--variant-so", default=None)
    ap.add_argument("--records-file", default=None, help=argparse.SUPPRESS)   # the child of --variant-so: the parent's records, only the UMI correction
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch                                                   # (before the product library initialises HIP: both then share one runtime)
    pa = importlib.import_module("rust-pseudoaligner_amd")
    tx = pa.Txome.synthesize(50, 150, 7)
    al = pa.Pseudoaligner(pa.HostIndex.from_txome(tx, 31, 4))      # (names the GPU; the index itself is not used)
    tabs = tables()
    if a.records_file:
        rec = np.load(a.records_file)
        print(json.dumps(run_umi(pa, al, rec, tabs, a.mode, a.warmup, a.rounds, "variant")), flush=True)
        return
    t0 = time.perf_counter()
    rec = synthetic(pa.BUS_RECORD_DTYPE, a.records, a.cells, a.ambient, a.umi_error_rate, a.multi_gene, 7)
    print("[bench_umi] %d records in %.1f s" % (len(rec), time.perf_counter() - t0), file=sys.stderr, flush=True)
    runs = range(a.warmup + a.rounds)

    # yardstick 1: the same bytes copied device to device
    nbytes = len(rec) * rec.itemsize
    src = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    copy_ms = []
    for rnd in runs:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        dst.copy_(src)
        e1.record()
        torch.cuda.synchronize()
        if rnd >= a.warmup:
            copy_ms.append(e0.elapsed_time(e1))
    del src, dst
    torch.cuda.empty_cache()

    res = {"records": len(rec), "cells": a.cells, "ambient": a.ambient, "umi_error_rate": a.umi_error_rate, "multi_gene": a.multi_gene, "mode": a.mode, "rounds": a.rounds,
           "warmup": a.warmup, **run_umi(pa, al, rec, tabs, a.mode, a.warmup, a.rounds, "umi"), "d2d_copy_ms": spread(copy_ms)}

    # yardstick 2: the barcode correction's rewrite + sort + collapse on the same records (their own barcodes as the whitelist, a few taken off it and
    # their neighbour put on, so that a barcode moves and the sort runs)
    wl = np.unique(rec["barcode"])
    off_list = wl[:: max(1, len(wl) // 16)][:16]
    wl = np.unique(np.concatenate([wl[~np.isin(wl, off_list)], off_list ^ np.uint64(1)]))
    cst = np.zeros(pa._ffi.PA_BUS_CORRECT_STATS, np.uint64)
    n_out = C.c_uint64()
    rewrite = []
    for rnd in runs:
        pa.check(pa.lib().pa_bus_correct_records(al._h, rec.ctypes.data, len(rec), BC, UMI, wl.ctypes.data, len(wl), None, 0, C.byref(n_out), cst.ctypes.data))
        if rnd >= a.warmup:
            rewrite.append(pa.bus_correct_phase_ms()["rewrite_ms"])
    res["correct_rewrite_ms"] = spread(rewrite)
    res["correct_barcodes_corrected"] = int(cst[4])
    res["search_over_copy"] = round(res["search_ms"]["median"] / statistics.median(copy_ms), 3)
    res["search_over_correct_rewrite"] = round(res["search_ms"]["median"] / statistics.median(rewrite), 3)

    if a.variant_so:   # the block bin's barcodes through the HBM variant, in a fresh process with that library
        with tempfile.TemporaryDirectory() as tmp:
            np.save(os.path.join(tmp, "records.npy"), rec)
            child = subprocess.run([sys.executable, __file__, "--records-file", os.path.join(tmp, "records.npy"), "--mode", a.mode, "--rounds", str(a.rounds), "--warmup",
                                    str(a.warmup)], env=dict(os.environ, PA_PRODUCT_SO=str(a.variant_so)), capture_output=True, text=True)
        sys.stderr.write(child.stderr)
        if child.returncode != 0:
            raise SystemExit("the variant run failed (%d)" % child.returncode)
        v = json.loads(child.stdout.strip().splitlines()[-1])
        same = {k: v["stats"][k] for k in v["stats"] if k != "barcodes_hbm"} == {k: res["stats"][k] for k in res["stats"] if k != "barcodes_hbm"}
        res["hbm_variant"] = {"search_ms": v["search_ms"], "barcodes_hbm": v["stats"]["barcodes_hbm"], "same_stats_otherwise": same,
                              "search_over_lds": round(v["search_ms"]["median"] / res["search_ms"]["median"], 3)}
    print(json.dumps(res), flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps([res], indent=1) + "\n")


if __name__ == "__main__":
    main()
