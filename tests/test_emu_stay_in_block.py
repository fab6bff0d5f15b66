"""The forward step's stay-in-block rule (lane_steps.hpp, fwd_next_block) on the CPU: the product's lane state machine, executed by
tests/emu, against the oracle — bit exact — on reads that put node ends, read ends and the step that goes on in its chain on and
around every seam of a chain block (tests/stay_cases.py); and the rule's effect counted by tools/chain_stats.cpp --kernel."""
import re
import subprocess

import numpy as np
import pytest

import helpers
import stay_cases

pa = helpers.pa


def check(host, reads, allowed, nodes=False):
    tiles, lens, wpr = pa.encode_reads_host(reads)
    o_res, o_coff, o_ids, _ = helpers.Oracle(host).map_tiles(tiles, lens, wpr, allowed, 4)
    r = helpers.Emu(host).map_tiles(tiles, lens, wpr, allowed, 8, want_nodes=nodes)
    helpers.assert_same_as_oracle(r["results"], r["coff"], r["ids"], o_res, o_coff, o_ids, "emu")
    return r, o_res


def check_both_packings(host, reads, allowed, monkeypatch):
    """reads of up to 512 bases in the narrow lane packing, longer ones in the wide one (as the kernel picks) — and all of them in the wide one"""
    short = [r for r in reads if len(r) <= 512]
    long_ = [r for r in reads if len(r) > 512]
    _, o_res = check(host, short, allowed)
    if long_:
        check(host, long_, allowed)
    monkeypatch.setenv("PA_EMU_WIDE", "1")
    check(host, short, allowed)
    return o_res


@pytest.mark.parametrize("allowed", [0, 2])
@pytest.mark.parametrize("k", [20, 24, 31, 64])
def test_hand_built_node_ends_on_block_seams(built, tmp_path, monkeypatch, k, allowed):
    host, triples, forks = stay_cases.hand_built_txome(k, tmp_path)
    reads = stay_cases.sweep_reads(k, triples, forks)
    assert {len(r) for r in reads} >= set(stay_cases.READ_LENS)
    o_res = check_both_packings(host, reads, allowed, monkeypatch)
    assert o_res["mapped"].all()                       # every read starts with an error-free k-mer of its transcript
    # the error-free reads of the triples (the first ones generated per offset) are covered whole: they walked A, B and C
    assert (o_res["coverage"] == np.array([len(r) for r in reads if len(r) <= 512], np.uint32)).sum() > len(reads) // 3


@pytest.mark.parametrize("k", [24, 64])
def test_hand_built_node_traces(built, tmp_path, k):
    """the traced (general) step: 64 h + x, which names a node in the trace, is the same whether the lane stayed or re-based"""
    host, triples, forks = stay_cases.hand_built_txome(k, tmp_path)
    reads = stay_cases.sweep_reads(k, triples[3:6], forks[:2], offsets=range(0, 131, 7))
    r, _ = check(host, [x for x in reads if len(x) <= 512], 2, nodes=True)
    o = helpers.Oracle(host)
    short = [x for x in reads if len(x) <= 512]
    for i in range(0, len(short), max(1, len(short) // 300)):
        rc, _, _, _, nodes = o.map_read(short[i], 2)
        assert r["nodes"][i][: r["nodes_len"][i]].tolist() == (nodes if rc else []), i


@pytest.mark.parametrize("seed", range(3))
def test_long_chains(built, tmp_path, monkeypatch, seed):
    host, reads, allowed = helpers.long_chain_case(seed, tmp_path)
    k = int(host.arrays()["k"])
    check_both_packings(host, reads + stay_cases.case_reads(reads, k, 2000), allowed, monkeypatch)
    check_both_packings(host, stay_cases.case_reads(reads, k, 1000, seed=4), 0, monkeypatch)


@pytest.mark.parametrize("seed", range(4))
def test_branch_points(built, tmp_path, monkeypatch, seed):
    host, reads, allowed = helpers.branch_case(seed, tmp_path)
    assert host is not None
    k =int(host.arrays()["k"])
    check_both_packings(host, reads + stay_cases.case_reads(reads, k, 2000), allowed, monkeypatch)
    check_both_packings(host, stay_cases.case_reads(reads, k, 1000, seed=4), 2, monkeypatch)


@pytest.fixture(scope="module")
def chain_stats(built, tmp_path_factory):
    """tools/chain_stats.cpp linked against the product library (its host half: index build, flattener, read simulator)"""
    exe = tmp_path_factory.mktemp("chain_stats") / "chain_stats"
    pkg = helpers.ROOT / "rust-pseudoaligner_amd"
    subprocess.run(["g++", "-O1", "-std=c++17", "-pthread", str(helpers.ROOT / "tools" / "chain_stats.cpp"), "-L", str(pkg), "-lpseudoaligner_amd",
                    "-Wl,-rpath," + str(pkg), "-o", str(exe)], check=True, capture_output=True, text=True)
    return exe


@pytest.mark.parametrize("k,read_len,ppm", [(24, 150, 0), (24, 192, 0), (24, 192, 20000), (31, 187, 10000), (20, 100, 30000), (64, 192, 5000)])
def test_reads_of_up_to_192_bases_never_look_for_their_slot(chain_stats, k, read_len, ppm):
    """On gencode_small.fa, stepping as the kernel does (two nodes per step): a read of <= 192 bases fits the window of the block its
    first k-mer is in (p + L <= 63 + 192), so no forward step re-bases, none has to look for its node's slot, and the distinct blocks
    fetched are those of the general step (which walks the same bases, as many nodes per step as there are)."""
    out = subprocess.run([str(chain_stats), "--kernel", "--no-cache", str(k), str(read_len), str(ppm), "20000", str(helpers.FASTA)],
                         check=True, capture_output=True, text=True).stdout
    m = re.search(r"kernel_step_counts (.*)", out)
    c = {a: int(b) for a, b in (kv.split("=") for kv in m.group(1).split())}
    assert c["reads"] == 20000 and c["fwd"] > 0
    assert c["unknown"] == 0 and c["rebased"] == 0
    assert c["blocks"] == c["general_blocks"]


def test_longer_reads_still_re_base(chain_stats):
    """(the counters do count: 300-base reads leave their first block, and no re-based step would have fitted the block it left)"""
    out = subprocess.run([str(chain_stats), "--kernel", "--no-cache", "24", "300", "0", "5000", str(helpers.FASTA)], check=True, capture_output=True, text=True).stdout
    c = {a: int(b) for a, b in (kv.split("=") for kv in re.search(r"kernel_step_counts (.*)", out).group(1).split())}
    assert c["rebased"] > 0 and c["unknown"] == c["rebased"] and c["rebased_fits"] == 0
