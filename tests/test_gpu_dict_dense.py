"""GPU tier: the dictionary's probe and the GPU filler on DENSE tables of the 16-byte slots (K <= 32) and of the two-word lines (K > 32). At the loads
the library ships (0.25 and 1/3) nine keys in ten lie where the first load looks; the overflow flag, chains of several buckets, the wrap at the table's
end and the builders' retry practically never run on the GPU. The dictknobs test build (its flattener and its filler read PA_DICT_LOAD) makes them common.
One child process per (case, load): tests/dict_dense_worker.py. There the GPU filler's table is audited by tests/dict_model.py and compared with the CPU
flattener's, and reads go through the mapping kernel — records, arena and count table against the oracle, exact.

The fuzz cases are seeds of helpers.random_txome_case, chosen on the CPU with the model (tests/test_dict_model.py asserts the same conditions on the CPU
flattener's tables): every K of the family at both loads; wrapped keys under both formats (seeds 15, 4 and 22: how many keys move on from a bucket depends on
the hashes alone); builders that retry whoever comes first (seed 41: one retry at 0.5 and three at 0.9 in every order of insertion tried; every 0.9 case
retries at least once) and cases whose number of retries depends on the order (seeds 19 and 22 at 0.9: one or two), where the GPU table may have another
size than the CPU's."""
import importlib
import json
import os
import re
import subprocess
import sys

import pytest

import helpers

WORKER = helpers.ROOT / "tests" / "dict_dense_worker.py"
FUZZ_CASES = [(seed, load) for seed in (10, 15, 46, 11, 4, 41, 22) for load in ("0.5", "0.9")] + [(19, "0.9")]   # K = 8, 16, 21, 32, 33, 47, 64; 16
GENCODE_CASES = [(31, "0.5"), (31, "0.9"), (24, "0.5"), (48, "0.5")]   # (K = 24 with a named load: the 16-byte slots below K = 25, the refused-pair path)
_results = {}


def run_child(mode, what, load, timeout):
    """one fresh process under the dictknobs build -> what its RESULT line says. A child that ends by a signal, by abort or at its time limit may have
    left the GPU faulted: nothing more is started on it"""
    key = (mode, what, load)
    if key not in _results:
        sys.path.insert(0, str(helpers.ROOT))
        so = importlib.import_module("rust-pseudoaligner_amd._build").build_dictknobs_variant()
        env = {k: v for k, v in os.environ.items() if k not in ("PA_DICT_LOAD", "PA_PAIR_LOG2", "PA_PAIR_MAX_BLOCKS", "PA_PAIR_LOAD")}
        env["PA_PRODUCT_SO"] = str(so)
        try:
            proc = subprocess.run([sys.executable, str(WORKER), mode, str(what), load], capture_output=True, text=True, env=env, timeout=timeout)
        except subprocess.TimeoutExpired:
            pytest.exit("dense dictionary: the child %s %s %s did not end within %d s" % (mode, what, load, timeout), returncode=3)
        out = proc.stdout + proc.stderr
        if proc.returncode < 0 or proc.returncode in (124, 134, 137, 139) or re.search(r"illegal memory access|hip ?error|pseudoaligner_amd error -5|HSA_STATUS_ERROR|Memory access fault", out, re.I):
            pytest.exit("dense dictionary: the child %s %s %s ended with %d\n%s" % (mode, what, load, proc.returncode, out[-3000:]), returncode=3)
        assert proc.returncode == 0, out[-6000:]
        lines = [l for l in proc.stdout.splitlines() if l.startswith("RESULT ")]
        assert lines, out[-3000:]
        _results[key] = json.loads(lines[-1][len("RESULT "):])
        print(lines[-1])
    return _results[key]


def assert_coverage(results):
    """what the audits counted, summed over the cases, for each of the two formats: the rare paths are there"""
    for name, rs in (("16-byte slots", [r for r in results if r["k"] <= 32]), ("two-word lines", [r for r in results if r["k"] > 32])):
        on = {}
        for r in rs:
            for d, n in r["on"].items():
                on[int(d)] = on.get(int(d), 0) + n
        assert sum(n for d, n in on.items() if d >= 2) > 0, name + ": no key 2 or more buckets from its home"
        assert sum(n for d, n in on.items() if d >= 4) > 0, name + ": no key 4 or more buckets from its home"
        assert sum(r["wrapped"] for r in rs) >= 1, name + ": no wrapped key"
        assert any(r["retried"] for r in rs), name + ": no builder retried"
        if name == "16-byte slots":
            for i in range(3):
                assert sum(r["named"][i] for r in rs) > 0, "no key in named slot %d" % i


@pytest.mark.gpu
@pytest.mark.parametrize("seed,load", FUZZ_CASES)
def test_fuzz_case_on_a_dense_table(built, seed, load):
    r = run_child("fuzz", seed, load, 180)
    assert r["keys"] == r["num_kmers"] and r["nbuckets"] * (4 if r["k"] <= 32 else 2) * (0.25 if r["k"] <= 32 else 1 / 3) < r["num_kmers"]


@pytest.mark.gpu
def test_the_fuzz_cases_reach_the_rare_placements_on_the_gpu(built):
    assert_coverage([run_child("fuzz", seed, load, 180) for seed, load in FUZZ_CASES])


@pytest.mark.gpu
@pytest.mark.parametrize("k,load", GENCODE_CASES)
def test_gencode_small_on_a_dense_table(built, k, load):
    """reads that BEGIN with keys in named slots, 1, 2 and 3 or more buckets on and behind the table's end take the probe of the refill step into every
    state it can continue from; reads whose absent first k-mer finds the overflow flag walk the chain before the two-position scan starts; reads of 600
    to 2 000 bases run the instantiation whose first probes go through the SEEK queue. (Informational: the shares of keys in their home slot, in a
    named slot and in a later bucket, next to the 78 % home that csrc/device_layout.hpp quotes for load 0.5.)"""
    r = run_child("gencode", k, load, 420)
    assert r["keys"] == r["num_kmers"] and all(n > 0 for n in r["groups"].values())
    assert sum(n for d, n in r["on"].items() if int(d) >= 3) > 0 and (k > 32 or min(r["named"]) > 0)
    print("gencode_small K=%d load %s: home %.1f %%, named slot %.1f %%, later bucket %.1f %% of %d keys" % ((k, load) + tuple(100 * x for x in r["shares"]) + (r["keys"],)))
