"""Child process of tests/test_dict_model.py and tests/test_gpu_dict_dense.py: loaded with the dictknobs test build of the product (PA_PRODUCT_SO), whose
CPU flattener and GPU filler read PA_DICT_LOAD, so that the 16-byte slots (K <= 32) and the two-word lines (K > 32) are DENSE: keys in named slots, in
later buckets, behind the table's end, and builders that have to retry.

  cpu OUTDIR SEED,SEED,...   the CPU flattener's tables of helpers.random_txome_case(seed) at the shipped load and at 0.5 / 0.9 -> OUTDIR/s<seed>_<load>.npy
  cpu-gencode OUTDIR K       the CPU flattener's tables of gencode_small at the shipped load and at 0.5 -> OUTDIR/gencode_k<K>_<load>.npy
  fuzz SEED LOAD             GPU: one random_txome_case — the GPU filler's table audited and compared with the CPU flattener's, the case's reads mapped
  gencode K LOAD             GPU: gencode_small — the same, and reads that BEGIN with keys of every placement the audit names

The GPU modes print one line "RESULT {json}" with what the audit of the GPU filler's table counted."""
import json
import os
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
for p in (str(ROOT), str(ROOT / "tests"), str(ROOT / "tests" / "pairdict")):
    if p not in sys.path:
        sys.path.insert(0, p)
import helpers  # noqa: E402
import dict_model as dm  # noqa: E402
from gpu_worker import dict_table  # noqa: E402
from probe_refill_worker import aligner, device_check, random_reads, reads_at, tx_text  # noqa: E402

pa = helpers.pa
LOADS = ("shipped", "0.5", "0.9")


def set_load(load):
    """shipped: no named load, and (K <= 24) the pair format refused by its own hook, so that the table has the 16-byte slots at 0.25"""
    os.environ.pop("PA_DICT_LOAD", None)
    os.environ.pop("PA_PAIR_LOG2", None)
    if load == "shipped":
        os.environ["PA_PAIR_LOG2"] = "0"
    else:
        os.environ["PA_DICT_LOAD"] = load


def slots_table(host, device):
    table, pairs, _ = dict_table(host, device)
    assert pairs == 0, "the pair format was not refused"
    return table, table.size // 8


def cpu_tables(outdir, seeds):
    for seed in seeds:
        with tempfile.TemporaryDirectory() as tmp:
            host = helpers.random_txome_case(seed, Path(tmp))[0]
        if host is None:
            continue
        for load in LOADS:
            set_load(load)
            np.save(Path(outdir) / ("s%d_%s.npy" % (seed, load)), slots_table(host, -1)[0])


def cpu_gencode_tables(outdir, k):
    host = pa.build_index(str(helpers.FASTA), k, 8)
    for load in ("shipped", "0.5"):
        set_load(load)
        np.save(Path(outdir) / ("gencode_k%d_%s.npy" % (k, load)), slots_table(host, -1)[0])


def compare_tables(host, k, samples=0):
    """the GPU filler's table against the model, the graph and the CPU flattener's table -> (audit of the GPU table, audit of the CPU table, buckets of both)"""
    cpu, nb_cpu = slots_table(host, -1)
    gpu, nb_gpu = slots_table(host, 0)
    a_cpu, a_gpu = dm.audit(cpu, nb_cpu, k), dm.audit(gpu, nb_gpu, k, samples=samples)
    lo, hi = dm.index_kmers(host.arrays())
    order = np.lexsort((lo, hi))
    lo, hi = lo[order], hi[order]
    for name, a, table, nb in (("CPU", a_cpu, cpu, nb_cpu), ("GPU", a_gpu, gpu, nb_gpu)):
        assert np.array_equal(a["lo"], lo) and np.array_equal(a["hi"], hi), "the %s table's keys are not the graph's k-mers" % name
        # (which buckets are how full does not depend on the order of insertion: dict_model.expected_keys_per_bucket)
        assert np.array_equal(a["keys_per_bucket"], dm.expected_keys_per_bucket(lo, hi, nb, k)), "%s table: keys per bucket" % name
    # a retry more or less (a key beyond 15 buckets depends on who came first) gives another size: the buckets then compare with the model's alone
    if nb_cpu == nb_gpu:
        assert np.array_equal(a_cpu["keys_per_bucket"], a_gpu["keys_per_bucket"]), "keys per bucket differ between the CPU and the GPU table"
    assert np.array_equal(a_cpu["handle"], a_gpu["handle"]) and np.array_equal(a_cpu["off"], a_gpu["off"]), "(handle, off) differ between the CPU and the GPU table"
    return a_gpu, a_cpu, gpu, nb_gpu, nb_cpu


def result(k, load, nk, a_gpu, nb_gpu, nb_cpu, t0, **more):
    first = dm.first_sizing(nk, k, float(load))
    out = dict(dm.summary(a_gpu), k=k, load=load, num_kmers=nk, nbuckets=nb_gpu, nbuckets_cpu=nb_cpu, first_sizing=first, retried=nb_gpu > first,
               shares=[round(x, 4) for x in dm.shares(a_gpu)], seconds=round(time.time() - t0, 2), **more)
    print("RESULT " + json.dumps(out))


def assert_dense(host, k, nk):
    """the table the aligner maps through (a build of its own) is denser than the shipped load"""
    st = aligner(host).stats()
    assert st.num_kmers == nk and st.table_slots % 4 == 0
    assert (st.table_slots // 4) * dm.slots_per_bucket(k) * dm.shipped_load(k) < nk, (st.table_slots, nk)


def fuzz(seed, load):
    import torch  # noqa: F401  (before the product library initialises HIP: tests/conftest.py)
    t0 = time.time()
    set_load(load)
    with tempfile.TemporaryDirectory() as tmp:
        host, k, reads, _, allowed = helpers.random_txome_case(seed, Path(tmp))
    a_gpu, _, _, nb_gpu, nb_cpu = compare_tables(host, k)
    nk = len(a_gpu["lo"])
    assert_dense(host, k, nk)
    device_check(host, reads, allowed, "random_txome_case(%d) K=%d load=%s allowed=%d" % (seed, k, load, allowed))
    result(k, load, nk, a_gpu, nb_gpu, nb_cpu, t0, seed=seed)


def simulated(host, n, ppm, length=100):
    """the reads of Txome.simulate_host as strings (tests/test_gpu_dict_pairs.py maps the same call's tiles)"""
    wpr = pa.lib().pa_words_per_read(length)
    tiles, lens = pa.Txome.from_host_index(host).simulate_host(length, 4, n, ppm, 0, wpr)
    t3 = np.asarray(tiles).reshape(-1, wpr, 64)
    return ["".join("ACGT"[c] for c in helpers.unpack_bases(t3[r >> 6, :, r & 63], int(lens[r]))) for r in range(n)]


def absent_prefixes(table, nb, k, want, rng):
    """random k-mers that are no key, and whose home slot (K > 32: home line) sends the probe on to the next bucket"""
    T = dm.words(table, nb)
    out = []
    for _ in range(40):
        lo = rng.randint(0, 1 << 62, 40000).astype(np.uint64) * np.uint64(4) + rng.randint(0, 4, 40000).astype(np.uint64)
        hi = rng.randint(0, 1 << 62, 40000).astype(np.uint64) * np.uint64(4) + rng.randint(0, 4, 40000).astype(np.uint64)
        lo = lo & np.uint64((1 << (2 * min(k, 32))) - 1)
        hi = hi & np.uint64((1 << (2 * (k - 32))) - 1) if k > 32 else np.zeros(len(lo), np.uint64)
        b, j = dm.bucket_of(lo, hi, nb, k)
        if k <= 32:
            on = ((~T[b, 4 * j + 3] >> np.uint32(24)) & np.uint32(8)) != 0
        else:
            on = (T[b, 4] != dm.EMPTY) & (T[b, 12] != dm.EMPTY)
        on &= ~dm.lookup_many(table, nb, k, lo, hi)[0]
        out += [dm.kmer_string(lo[i], hi[i], k) for i in np.nonzero(on)[0][: want - len(out)]]
        if len(out) >= want:
            break
    return out


def gencode(k, load):
    import torch  # noqa: F401
    t0 = time.time()
    set_load(load)
    host = pa.build_index(str(helpers.FASTA), k, 8)
    a_gpu, a_cpu, gpu, nb_gpu, nb_cpu = compare_tables(host, k, samples=80)
    nk = len(a_gpu["lo"])
    assert_dense(host, k, nk)
    rng = np.random.RandomState(11)
    text = tx_text()
    groups = {"simulated 0 %": simulated(host, 2048, 0), "simulated 1 %": simulated(host, 2048, 10000)}
    # reads that begin with keys of every placement: named slot 0 / 1 / 2 (16-byte slots), 1, 2 and 3 or more buckets on, wrapped ones. Which of the
    # keys of one home slot got it is a race between two builds, so the key that HOLDS the home slot of each named-slot key goes beside it
    S = a_gpu["samples"]
    far = [s for name, keys in S.items() if name.endswith("buckets on") and int(name.split()[0]) >= 3 for s in keys]
    wanted = {"1 buckets on": S.get("1 buckets on", []), "2 buckets on": S.get("2 buckets on", []), "3 or more buckets on": far[:: max(1, len(far) // 80)][:80]}
    if k <= 32:
        wanted.update({"named slot %d" % i: S.get("named slot %d" % i, []) for i in range(3)})
    for name, keys in wanted.items():
        assert keys, "the table has no key %s" % name
    if S["wrapped"]:
        wanted["wrapped"] = S["wrapped"]
    off_home_starts = []
    for name, keys in wanted.items():
        starts = [text.find(s) for s in keys]
        assert min(starts) >= 0, "a key of the table is no k-mer of the transcripts"
        off_home_starts += starts
        groups["begin " + name] = [r for length in (150, 100, k) for r in reads_at(starts, length)]
    if k <= 32:
        T = dm.words(gpu, nb_gpu)
        rivals = []
        for i in range(3):
            lo = np.array([dm.kmer_of_string(s) for s in wanted["named slot %d" % i]], np.uint64)
            b, j = dm.pa_bucket_home(lo, nb_gpu)
            holder = T[b, 4 * j].astype(np.uint64) | (T[b, 4 * j + 1].astype(np.uint64) << np.uint64(32))
            rivals += [text.find(dm.kmer_string(h, 0, k)) for h in holder.tolist()]
        assert min(rivals) >= 0
        groups["begin home-slot holders"] = reads_at(rivals, 150)
    prefixes = absent_prefixes(gpu, nb_gpu, k, 240, rng)
    groups["absent first k-mer, probe goes on"] = [p + r for p, r in zip(prefixes, random_reads(len(prefixes), 150 - k, 21))]
    assert len(groups["absent first k-mer, probe goes on"]) >= 200
    groups["random places"] = random_reads(200, 150, 5)
    longs = []   # (mapped in a batch of their own: a batch's longest read decides between the LDS and the HBM-tile instantiation)
    for s in rng.permutation(off_home_starts).tolist():
        longs += reads_at([s], int(rng.randint(600, 2001)))
        if len(longs) == 64:
            break
    assert len(longs) == 64, "%d long reads" % len(longs)
    short = [(g, r) for g, rs in groups.items() for r in rs]
    for g, rs in groups.items():
        assert rs, "no reads: " + g
    assert len(short) <= 6500, len(short)
    order = rng.permutation(len(short))
    batch = [short[i][1] for i in order]
    names = np.array([short[i][0] for i in order])
    beside = [short[i][1] for i in order[:400] if short[i][0].startswith("begin")]
    long_batch = longs + beside
    long_batch = [long_batch[i] for i in rng.permutation(len(long_batch))]
    for allowed in (0, 2):
        o_res = device_check(host, batch, allowed, "gencode_small K=%d load=%s allowed=%d" % (k, load, allowed))
        for g in groups:
            assert o_res["mapped"][names == g].any(), "the oracle maps no read of: " + g
        o_res = device_check(host, long_batch, allowed, "gencode_small K=%d load=%s allowed=%d, reads of 600-2000 bases" % (k, load, allowed))
        assert o_res["mapped"][np.array([len(r) >= 600 for r in long_batch])].any()
    result(k, load, nk, a_gpu, nb_gpu, nb_cpu, t0, reads=len(batch), long_reads=len(long_batch), groups={g: len(rs) for g, rs in groups.items()},
           cpu_shares=[round(x, 4) for x in dm.shares(a_cpu)])


if __name__ == "__main__":
    mode = sys.argv[1]
    if mode == "cpu":
        cpu_tables(sys.argv[2], [int(s) for s in sys.argv[3].split(",")])
    elif mode == "cpu-gencode":
        cpu_gencode_tables(sys.argv[2], int(sys.argv[3]))
    elif mode == "fuzz":
        fuzz(int(sys.argv[2]), sys.argv[3])
    else:
        gencode(int(sys.argv[2]), sys.argv[3])
