#!/usr/bin/env python3
"""Measurements of BGZF input: synthetic 150-base reads built as tools/bench_ingest.py builds them, qualities drawn from four
binned values with run structure (a constant quality line would compress absurdly well), written three ways: plain text, an ordinary
multi-member .gz without BC fields (64 MiB of text per member: the one-zlib-stream path), and BGZF (members of 65 280 bytes of text, zlib
level 6, what bgzip writes).
  ingest   reads/s of pa_process_reads into /dev/null for: plain text, the ordinary .gz, the BGZF file, and the BGZF file with
           PA_INGEST_BGZF=0 (the path before this feature on the same bytes) -- one warm-up each, then --repeats rounds that ALTERNATE the four;
           median and spread; bytes_h2d per read and the host stage seconds of the BGZF runs
  kernel   pa_bgzf_inflate_device alone by device events, compressed bytes already in HBM: one launch per --window-members members back
           to back; text and payload GB/s
One JSON object on stdout and in --out. No target is set for these numbers.

    python tools/bench_inflate.py [--reads 16000000] [--repeats 5] [--threads 16] [--out profiles/r10_inflate_bench.json]
"""
import argparse
import gzip
import json
import os
import statistics
import sys
import time
import zlib
from concurrent.futures import ProcessPoolExecutor
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]

CHUNK = 65280


def _member(text: bytes) -> bytes:
    import bgzf_cases as bc
    return bc.good_member(text, 6)


def _gz_member(text: bytes) -> bytes:
    return gzip.compress(text, 6)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=16_000_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--dir", default="/dev/shm" if os.path.isdir("/dev/shm") else "/tmp")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--window-members", type=int, default=1024)
    ap.add_argument("--workers", type=int, default=16, help="host processes that compress the input")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r10_inflate_bench.json"))
    args = ap.parse_args()
    import numpy as np
    import torch
    import helpers
    pa = helpers.pa
    if pa.lib().pa_device_count() < 1:
        raise SystemExit("bench_inflate needs a GPU: there is no CPU fallback")
    n, L, wpr = args.reads, 150, 5
    t0 = time.time()
    tx = pa.Txome.synthesize(58000, 203000, 7)
    rng = np.random.default_rng(5)
    lut, qlut = np.frombuffer(b"ACGT", np.uint8), np.frombuffer(b"#-:F", np.uint8)
    parts = []
    for first in range(0, n, 1 << 20):
        m = min(1 << 20, n - first)
        tiles, _ = tx.simulate_host(L, 2, m, 0, first, wpr)
        words = tiles.reshape(-1, wpr, 64).transpose(0, 2, 1).reshape(-1, wpr)[:m]
        shifts = (2 * np.arange(32, dtype=np.uint64))[None, None, :]
        bases = ((words[:, :, None] >> shifts) & np.uint64(3)).astype(np.uint8).reshape(m, wpr * 32)[:, :L]
        starts = rng.random((m, L)) < 0.08            # a new quality run begins here
        starts[:, 0] = True
        at = np.maximum.accumulate(np.where(starts, np.arange(L)[None, :], 0), axis=1)
        qual = qlut[rng.integers(0, 4, (m, L), dtype=np.uint8)[np.arange(m)[:, None], at]]
        rec = np.empty((m, 16 + 2 * L), np.uint8)
        ids = np.char.zfill(np.arange(first, first + m).astype("U9"), 9)
        rec[:, 0] = ord("@"); rec[:, 1] = ord("r")
        rec[:, 2:11] = np.frombuffer("".join(ids).encode(), np.uint8).reshape(m, 9)
        rec[:, 11] = 10
        rec[:, 12:12 + L] = lut[bases]
        rec[:, 12 + L:12 + L + 3] = np.frombuffer(b"\n+\n", np.uint8)
        rec[:, 15 + L:15 + 2 * L] = qual
        rec[:, 15 + 2 * L] = 10
        parts.append(rec.tobytes())
    text = b"".join(parts)
    del parts
    print("[inflate] %d reads, %.2f GB of text in %.1f s" % (n, len(text) / 1e9, time.time() - t0), file=sys.stderr)
    t0 = time.time()
    with ProcessPoolExecutor(args.workers) as ex:
        comp = b"".join(ex.map(_member, (text[i:i + CHUNK] for i in range(0, len(text), CHUNK)), chunksize=64))
    print("[inflate] BGZF: %.2f GB, ratio %.2f, in %.1f s" % (len(comp) / 1e9, len(text) / len(comp), time.time() - t0), file=sys.stderr)
    members, text_bytes = pa.bgzf_scan(comp)
    assert text_bytes == len(text)
    payload = int(members["in_len"].sum())

    # ---- ingest: pa_process_reads on the three forms ----
    big = 64 << 20
    with ProcessPoolExecutor(args.workers) as ex:
        plain_gz = b"".join(ex.map(_gz_member, (text[i:i + big] for i in range(0, len(text), big))))
    d = Path(args.dir)
    files = {"plain": d / "pa_inflate_bench.fq", "gz": d / "pa_inflate_bench.plain.fq.gz", "bgzf": d / "pa_inflate_bench.bgzf.fq.gz"}
    files["plain"].write_bytes(text); files["gz"].write_bytes(plain_gz); files["bgzf"].write_bytes(comp)
    hi = pa.HostIndex.from_txome_device(tx, 24, 0)
    al = pa.Pseudoaligner(hi)
    legs = [("plain", "plain", None), ("gz", "gz", None), ("bgzf", "bgzf", None), ("bgzf_switch_off", "bgzf", "0")]
    times = {k: [] for k, _, _ in legs}
    stats = {}

    def ingest(name, which, switch):
        if switch is None:
            os.environ.pop("PA_INGEST_BGZF", None)
        else:
            os.environ["PA_INGEST_BGZF"] = switch
        t = time.perf_counter()
        got, _ = pa.process_reads(str(files[which]), al, "/dev/null", args.threads)
        dt = time.perf_counter() - t
        assert got == n, (name, got)
        stats[name] = dict(pa.process_reads_input_stats(), stages=pa.process_reads_stage_seconds())
        return dt
    for name, which, switch in legs:
        ingest(name, which, switch)                       # warm-up (page cache, pinned buffers, code objects)
    for r in range(args.repeats):
        for name, which, switch in legs:                  # alternating
            times[name].append(ingest(name, which, switch))
    os.environ.pop("PA_INGEST_BGZF", None)
    assert stats["bgzf"]["text_kind"] == 2 and stats["bgzf_switch_off"]["text_kind"] == 1 and stats["gz"]["text_kind"] == 1 and stats["plain"]["text_kind"] == 0
    for f in files.values():
        f.unlink()
    del al, plain_gz

    def rate(xs):
        med = statistics.median(xs)
        return {"reads_per_s_median": n / med, "reads_per_s_spread": [n / max(xs), n / min(xs)], "seconds": xs}
    ingest_res = {k: rate(v) for k, v in times.items()}
    ingest_res["bgzf"]["bytes_h2d_per_read"] = stats["bgzf"]["bytes_h2d"] / n
    ingest_res["plain"]["bytes_h2d_per_read"] = stats["plain"]["bytes_h2d"] / n
    ingest_res["bgzf"]["input_stats"] = {k: v for k, v in stats["bgzf"].items() if k != "stages"}
    ingest_res["bgzf"]["stage_seconds_last_run"] = stats["bgzf"]["stages"]
    ingest_res["bgzf_switch_off"]["stage_seconds_last_run"] = stats["bgzf_switch_off"]["stages"]
    lo_new, hi_old = ingest_res["bgzf"]["reads_per_s_spread"][0], ingest_res["bgzf_switch_off"]["reads_per_s_spread"][1]
    ingest_res["bgzf_beats_switch_off_by_more_than_both_spreads"] = bool(lo_new > hi_old)
    print("[inflate] ingest: " + ", ".join("%s %.1f M reads/s" % (k, v["reads_per_s_median"] / 1e6) for k, v in ingest_res.items() if isinstance(v, dict)), file=sys.stderr)

    dev = torch.device("cuda", 0)
    d_comp = torch.frombuffer(bytearray(comp), dtype=torch.uint8).to(dev)
    d_members = torch.from_numpy(members.view(np.uint8).copy()).to(dev)
    d_text = torch.zeros(len(text), dtype=torch.uint8, device=dev)
    d_status = torch.zeros(len(members), dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    W = args.window_members

    def gpu_run():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for first in range(0, len(members), W):
            k = min(W, len(members) - first)
            off = int(members["out_off"][first])
            cap = int(members["out_off"][first + k - 1] + members["out_len"][first + k - 1]) - off
            pa.bgzf_inflate_device(0, d_comp.data_ptr(), d_comp.numel(), d_members.data_ptr() + first * members.itemsize, k, d_text.data_ptr() + off, cap,
                                   d_status.data_ptr() + 4 * first, stream)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / 1e3

    for _ in range(args.warmup):
        gpu_run()
    assert int(d_status.count_nonzero()) == 0
    assert bytes(d_text.cpu().numpy().data) == text, "the kernel's text differs from the input"
    gpu = [gpu_run() for _ in range(max(args.repeats, 5))]
    assert int(d_status.count_nonzero()) == 0

    def summary(xs, nbytes):
        med = statistics.median(xs)
        return {"median_s": med, "min_s": min(xs), "max_s": max(xs), "runs": len(xs), "text_GBps_median": nbytes / med / 1e9,
                "text_GBps_spread": [nbytes / max(xs) / 1e9, nbytes / min(xs) / 1e9]}
    res = {"reads": n, "read_len": L, "text_bytes": len(text), "bgzf_bytes": len(comp), "payload_bytes": payload, "members": int(len(members)),
           "compression_ratio": len(text) / len(comp), "compressed_bytes_per_read": len(comp) / n, "window_members": W,
           "threads": args.threads, "ingest": ingest_res,
           "kernel": dict(summary(gpu, len(text)), payload_GBps_median=payload / statistics.median(gpu) / 1e9),
           "device": torch.cuda.get_device_name(0)}
    line = json.dumps(res)
    print(line)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
