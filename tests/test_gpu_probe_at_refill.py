"""A read's first dictionary probe in the step that refills its pool slot (map_pool_kernel.inc, PA_PROBE_AT_REFILL) on the GPU: the batches and
reads at the edges of that path through pa_map_batch_device and pa_map_count_batch_device against the oracle, bit exact, and the count table
against helpers.counts_reference (tests/probe_refill_worker.py: device_check). gencode_small at K = 24 (pair dictionary) and K = 31 (16-byte
slots); K = 64 (the two-word dictionary, whose kernel text is unchanged) once as the control."""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers
import probe_refill_worker as w
from test_class_cases import built_case

pa = helpers.pa
pytestmark = pytest.mark.gpu

SIZES = [1, 63, 64, 65, 127, 128, 129, 1000, 8193]
_pools = {}


def pool(small_index, k, allowed):
    """8193 reads of 150 bases and the oracle's answer to them, once per (k, allowed): a batch of n reads is the first n of them"""
    if (k, allowed) not in _pools:
        host = small_index(k)
        reads = w.random_reads(max(SIZES), 150, 7)
        _pools[k, allowed] = (host, reads, helpers.Oracle(host).map_reads(reads, allowed, 8)[:3])
    return _pools[k, allowed]


def first_n(oracle, n):
    o_res, o_coff, o_ids = oracle
    return o_res[:n], o_coff[:n + 1], o_ids[: int(o_coff[n])]


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("allowed", [0, 2])
@pytest.mark.parametrize("k", [24, 31])
def test_batch_sizes(small_index, k, allowed, n):
    """one lane, one short of a wave, a wave, one more; the pool's 128 slots and one either side; a last chunk that is no multiple of anything; more
    than one chunk per wave. The first iterations of a wave are refill steps that probe; its last output steps refill fewer reads than they free"""
    host, reads, oracle = pool(small_index, k, allowed)
    w.device_check(host, reads[:n], allowed, "K=%d allowed=%d n=%d" % (k, allowed, n), first_n(oracle, n))


def test_two_word_dictionary_is_the_control(small_index):
    host = small_index(64)
    w.device_check(host, w.random_reads(1000, 150, 7), 2, "K=64 control")


@pytest.mark.parametrize("allowed", [0, 2])
@pytest.mark.parametrize("k", [24, 31])
def test_mixed_lengths(small_index, k, allowed):
    """reads shorter than K (ST_NONE: refilled, never probed) beside reads of K, K + 1, 100, 150 and 192 bases in one wave"""
    reads = []
    for i, length in enumerate((k - 1, k, k + 1, 100, 150, 192, 5)):
        reads += w.random_reads(250, length, 20 + i)
    order = np.random.RandomState(1).permutation(len(reads))
    o_res = w.device_check(small_index(k), [reads[i] for i in order], allowed, "mixed lengths K=%d allowed=%d" % (k, allowed))
    lens = np.array([len(reads[i]) for i in order])
    assert not o_res["mapped"][lens < k].any() and o_res["mapped"][lens >= 100].any()


@pytest.mark.parametrize("allowed", [0, 2])
@pytest.mark.parametrize("k", [24, 31])
def test_first_kmer_absent(small_index, k, allowed):
    """a random prefix, then transcript sequence: the probe made at refill misses, and the scan goes on from the SEEK queue (3 bases further
    on, two positions per step from then on); a prefix of 1 .. K + 6 bases moves the first k-mer that is in the index over the scan's stride"""
    rng = np.random.RandomState(9)
    reads = []
    for plen in list(range(1, 8)) + [k - 1, k, k + 6]:
        for r in w.random_reads(100, 150 - plen, 40 + plen):
            reads.append("".join("ACGT"[x] for x in rng.randint(0, 4, plen)) + r)
    reads += w.random_reads(200, 150, 39)
    order = rng.permutation(len(reads))
    o_res = w.device_check(small_index(k), [reads[i] for i in order], allowed, "first k-mer absent K=%d allowed=%d" % (k, allowed))
    assert o_res["mapped"].any()


def node_edge_reads(host, k, count):
    """reads that begin with the first and with the last k-mer of a node (nodes of more than one k-mer), of 150, 60 and K bases"""
    a = host.arrays()
    text = w.tx_text()
    multi = np.nonzero(a["node_len"] > k)[0]
    starts = []
    for n in multi[:: max(1, len(multi) // count)][:count].tolist():
        s, ln = int(a["node_start"][n]), int(a["node_len"][n])
        pos = np.arange(s, s + ln)
        seq = "".join("ACGT"[int(c)] for c in (a["node_seq"][pos >> 5] >> ((pos & 31) * 2).astype(np.uint64)) & np.uint64(3))
        first, last = text.find(seq[:k]), text.find(seq[-k:])
        assert first >= 0 and last >= 0, "node %d is not in the transcripts" % n
        starts += [first, last]
    return [r for length in (150, 60, k) for r in w.reads_at(starts, length)]


@pytest.mark.parametrize("allowed", [0, 2])
@pytest.mark.parametrize("k", [24, 31])
def test_first_kmer_at_a_node_edge(small_index, k, allowed):
    """position 0 is below L / 5, so no left extension is seeded whatever the entry says (F_FIRST_SEEK), also when the k-mer is the first of its
    node (the entry's node-start flag) or the last (the forward step leaves the node with its first base)"""
    host = small_index(k)
    reads = node_edge_reads(host, k, 150)
    assert len(reads) >= 500
    o_res = w.device_check(host, reads, allowed, "node edges K=%d allowed=%d" % (k, allowed))
    assert o_res["mapped"].any()


@pytest.mark.parametrize("allowed", [0, 2])
def test_list_mode_restarts(built, allowed):
    """the designed class sets whose reads meet only classes without windows (tests/class_cases.py, "lists": tests/test_class_cases.py asserts the
    path): restart_lists sends them back to ST_SEEK, and that probe goes through the queue, not through the refill step"""
    host, c = built_case("lists", 24)[:2]
    rng = np.random.RandomState(2)
    reads = list(c[3]) * 2 + ["".join("ACGT"[x] for x in rng.randint(0, 4, 150)) for _ in range(40)]
    w.device_check(host, [reads[i] for i in rng.permutation(len(reads))], allowed, "list-mode restarts allowed=%d" % allowed)


def test_first_kmers_off_their_home_pair(built, k=24):
    """the forced-smallest pair dictionary (the pairknobs test build reads PA_PAIR_LOG2; a child process: tests/probe_refill_worker.py)"""
    sys.path.insert(0, str(helpers.ROOT))
    so = importlib.import_module("rust-pseudoaligner_amd._build").build_pairknobs_variant()
    env = dict(os.environ, PA_PRODUCT_SO=str(so), PA_PAIR_LOG2="21")
    proc = subprocess.run([sys.executable, str(helpers.ROOT / "tests" / "probe_refill_worker.py"), str(k)], capture_output=True, text=True, env=env)
    assert proc.returncode == 0, proc.stdout + proc.stderr
    assert "off_home_reads=" in proc.stdout
