#!/usr/bin/env python3
"""First measurements of the abundance EM (pa_quant_*) on bench.py's config 3: the index, the class-count table and
overflow of ONE step of --batch reads (default 100 M), then setup time (pa_quant_set_counts), time per iteration (median over
repeats of pa_quant_step(q, 200): the call ends in a synchronise of its stream, so a host clock around it measures the device work
plus 400 launches), iterations to convergence, and the numpy model's time per iteration on the same input as context. One JSON
object on stdout and in --out. No target is set for these numbers.

--boot R adds the bootstrap leg (pa_quant_bootstrap_*) on the same table and writes it to --boot-out: the draw per replicate on that
table and on a skewed one (one class raised to a tenth of the reads), the time of one batched iteration at 8, 32 and 64 replicates,
R replicates end to end in batches of 64, and as the baseline the same R resampled tables one at a time through pa_quant_set_counts
+ pa_quant_run in the same session.

    python tools/bench_quant.py [--workload config3] [--batch N] [--repeats 5] [--out profiles/r08_quant_bench.json]
                                [--boot 64 --boot-out profiles/r09_quant_boot_bench.json]
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="config3")
    ap.add_argument("--batch", type=int, default=0)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--model-iters", type=int, default=3)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r08_quant_bench.json"))
    ap.add_argument("--boot", type=int, default=0, help="replicates of the bootstrap leg (0: no such leg)")
    ap.add_argument("--boot-out", default=str(ROOT / "profiles" / "r09_quant_boot_bench.json"))
    ap.add_argument("--boot-seed", type=int, default=42)
    args = ap.parse_args()
    import numpy as np
    import torch
    import bench
    import helpers
    import quant_model as qm
    pa = helpers.pa
    if pa.lib().pa_device_count() < 1:
        raise SystemExit("bench_quant needs a GPU: there is no CPU fallback")
    wl = bench.WORKLOADS[args.workload]
    B = args.batch or wl["batch"]
    dev = torch.device("cuda", 0)
    tx = pa.Txome.synthesize_repeats(wl["genes"], wl["transcripts"], wl["txome_seed"]) if wl.get("repeats") else pa.Txome.synthesize(wl["genes"], wl["transcripts"], wl["txome_seed"])
    host = pa.HostIndex.from_txome_device(tx, wl["k"], 0)
    a = pa.Pseudoaligner(host, 0)
    wpr = pa.lib().pa_words_per_read(wl["read_len"])
    d_tiles = torch.empty(pa.lib().pa_tiles_words(B, wpr), dtype=torch.int64, device=dev)
    d_lens = torch.empty(B, dtype=torch.int32, device=dev)
    d_res = torch.empty(B * 4, dtype=torch.int32, device=dev)
    cap = a.arena_hint(B)
    d_arena = torch.empty(cap, dtype=torch.int32, device=dev)
    d_counts = torch.zeros(a.counts_len(), dtype=torch.int64, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    tx.simulate_device(wl["read_len"], wl["read_seed"], B, d_tiles.data_ptr(), d_lens.data_ptr(), wl["ppm"], 0, wpr, 0, stream)
    ovf = pa.Overflow(0, 1 << 20, 1 << 24)
    a.set_overflow(ovf)
    a.map_count_batch_device(d_tiles.data_ptr(), d_lens.data_ptr(), B, wpr, d_res.data_ptr(), d_arena.data_ptr(), cap, d_counts.data_ptr(), 2, stream)
    a.map_finish(stream)
    counts = d_counts.cpu().numpy().astype(np.uint64)
    words = ovf.fetch()
    a.set_overflow(None)
    del d_tiles, d_lens, d_res, d_arena
    q = pa.Quantifier(a, host, mean_read_len=float(wl["read_len"]))
    q.set_counts(counts, words)                                   # (warm: code objects, rocPRIM's choices)
    setup = []
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        q.set_counts(counts, words)
        setup.append(time.perf_counter() - t0)
    st = q.stats()
    q.step(200)
    per_iter = []
    for _ in range(max(args.repeats, 1)):
        t0 = time.perf_counter()
        q.step(200)
        per_iter.append((time.perf_counter() - t0) / 200)
    q.set_counts(counts, words)
    t0 = time.perf_counter()
    iters, converged = q.run()
    t_run = time.perf_counter() - t0
    est, tpm, _ = q.fetch()
    arr = host.arrays()
    p = qm.Problem.from_table(arr, np.diff(host.transcripts()[1].astype(np.int64)), counts, words, mean_read_len=float(wl["read_len"]))
    al = p.start()
    t0 = time.perf_counter()
    for _ in range(args.model_iters):
        al = p.step(al)
    t_model = (time.perf_counter() - t0) / args.model_iters
    # bytes one iteration touches: per id 4 (the index) + 8 (the gathered f64) in each pass; per row offset, count, quotient; per
    # transcript with a row its slot, offsets, w, eff, alpha read and written, w written
    touched = st["ids"] * 24 + st["rows"] * 20 + st["transcripts_with_a_row"] * 52
    it_s = statistics.median(per_iter)
    out = dict(workload=args.workload, reads=int(B), transcripts=p.T, classes=int(arr["num_classes"]), stats=st,
               setup_ms=dict(median=1e3 * statistics.median(setup), min=1e3 * min(setup), max=1e3 * max(setup)),
               iteration_us=dict(median=1e6 * it_s, min=1e6 * min(per_iter), max=1e6 * max(per_iter), samples=len(per_iter), iterations_per_sample=200),
               bytes_touched_per_iteration=int(touched), implied_GB_per_s=touched / it_s / 1e9,
               run=dict(iterations=iters, converged=converged, ms=1e3 * t_run),
               numpy_model_ms_per_iteration=1e3 * t_model, est_counts_sum=float(est.sum()), tpm_sum=float(tpm.sum()))
    text = json.dumps(out, indent=1, sort_keys=True)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(text + "\n")
    print(json.dumps(out, sort_keys=True))
    if args.boot > 0:
        boot = bootstrap_leg(args, q, counts, words, st, it_s)
        Path(args.boot_out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.boot_out).write_text(json.dumps(boot, indent=1, sort_keys=True) + "\n")
        print(json.dumps(boot, sort_keys=True))


def bootstrap_leg(args, q, counts, words, st, single_iteration_s):
    import numpy as np
    import boot_model as bm
    R, seed, reps = args.boot, args.boot_seed, max(args.repeats, 1)

    def clock(fn):
        t0 = time.perf_counter()
        fn()
        return time.perf_counter() - t0

    def note(what):
        print("bootstrap leg: " + what, file=sys.stderr, flush=True)

    def draw_ms_per_replicate(n=64):
        q.bootstrap_draw(seed, 0, n)                              # (warm: code objects, the candidate-order tables of this table)
        t = [clock(lambda: q.bootstrap_draw(seed, 0, n)) for _ in range(reps)]
        return dict(median=1e3 * statistics.median(t) / n, min=1e3 * min(t) / n, max=1e3 * max(t) / n, replicates_per_call=n)

    # the skewed table: the largest class raised so that it owns a tenth of the reads
    skew = counts.copy()
    C = len(counts) - 3
    skew[int(np.argmax(counts[:C]))] += np.uint64(st["reads_used"] // 9)
    q.set_counts(skew, words)
    note("draw, skewed table")
    draw_skewed = draw_ms_per_replicate()
    skew_reads = q.stats()["reads_used"]
    q.set_counts(counts, words)
    note("draw")
    draw = draw_ms_per_replicate()
    iteration = {}
    for B in (8, 32, 64):
        note("iteration at %d replicates" % B)
        q.bootstrap_draw(seed, 0, B)
        q.bootstrap_step(20)
        t = [clock(lambda: q.bootstrap_step(50)) / 50 for _ in range(reps)]
        iteration[str(B)] = dict(us_median=1e6 * statistics.median(t), us_min=1e6 * min(t), us_max=1e6 * max(t),
                                 us_per_replicate=1e6 * statistics.median(t) / B, single_run_iteration_us=1e6 * single_iteration_s)

    def batched():
        q.set_counts(counts, words)
        out = []
        for first in range(0, R, 64):
            n = min(64, R - first)
            q.bootstrap_draw(seed, first, n)
            out.append(q.bootstrap_run()[0])
            q.bootstrap_fetch()
        return np.concatenate(out)

    note("%d replicates end to end" % R)
    batched()
    t0 = time.perf_counter()
    iters = batched()
    t_batched = time.perf_counter() - t0
    # the baseline: the same R tables one at a time through the single-run path (fetching the tables is not timed)
    note("the same tables one at a time")
    q.set_counts(counts, words)
    tables = []
    for first in range(0, R, 64):
        n = min(64, R - first)
        q.bootstrap_draw(seed, first, n)
        for k in range(n):
            cc, oc = q.bootstrap_counts(k)
            tables.append((cc, bm.overflow_with_counts(words, oc)))
    t_single, single_iters = 0.0, []
    for cc, w in tables:
        t0 = time.perf_counter()
        q.set_counts(cc, w)
        single_iters.append(q.run()[0])
        q.fetch()
        t_single += time.perf_counter() - t0
    q.set_counts(counts, words)
    # bytes of one batched iteration per replicate: per id a gathered f64 in each pass (the 4-byte ids are shared by the batch), per row
    # its count (4) and quotient (8), per transcript with a row alpha read and written, w read and written
    per_replicate = st["ids"] * 16 + st["rows"] * 12 + st["transcripts_with_a_row"] * 32
    shared = st["ids"] * 8 + st["rows"] * 8 + st["transcripts_with_a_row"] * 20
    for B, rec in iteration.items():
        rec["bytes_touched"] = int(per_replicate * int(B) + shared)
        rec["implied_GB_per_s"] = rec["bytes_touched"] / (rec["us_median"] * 1e-6) / 1e9
    return dict(workload=args.workload, reads=st["reads_used"], stats=st, replicates=R, seed=seed,
                draw_ms_per_replicate=draw, draw_ms_per_replicate_skewed=dict(draw_skewed, reads=skew_reads, share_of_the_largest_row=0.1),
                batched_iteration=iteration,
                end_to_end=dict(batched_ms=1e3 * t_batched, one_at_a_time_ms=1e3 * t_single, speedup=t_single / t_batched,
                                batched_iterations=dict(min=int(iters.min()), max=int(iters.max()), sum=int(iters.sum())),
                                one_at_a_time_iterations=dict(min=min(single_iters), max=max(single_iters), sum=sum(single_iters))))


if __name__ == "__main__":
    main()
