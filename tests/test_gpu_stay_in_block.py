"""The forward step's stay-in-block rule (lane_steps.hpp, fwd_next_block) on the GPU: the read families of tests/stay_cases.py through
pa_map_batch_device and pa_map_count_batch_device against the oracle, bit exact, and the count table against helpers.counts_reference."""
import numpy as np
import pytest

import helpers
import stay_cases

pa = helpers.pa
pytestmark = pytest.mark.gpu


def _subsample(reads, n, seed=11):
    if len(reads) <= n:
        return reads
    rng = np.random.RandomState(seed)
    return [reads[i] for i in np.sort(rng.choice(len(reads), n, replace=False))]


def device_check(host, reads, allowed, what):
    """map the reads on device-resident tiles (results + arena, then the fused count table) and compare with the oracle"""
    import torch
    a = pa.Pseudoaligner(host)
    tiles, lens, wpr = pa.encode_reads_host(reads)
    n = len(reads)
    dev = torch.device("cuda", 0)
    d_tiles, d_lens = torch.from_numpy(tiles.view(np.int64)).to(dev), torch.from_numpy(np.asarray(lens, np.uint32).view(np.int32)).to(dev)
    cap = a.arena_hint(n)
    d_res = torch.zeros(n * 4, dtype=torch.int32, device=dev)
    d_arena = torch.zeros(cap, dtype=torch.int32, device=dev)
    a.map_batch_device(d_tiles.data_ptr(), d_lens.data_ptr(), n, wpr, d_res.data_ptr(), d_arena.data_ptr(), cap, allowed)
    used, _ = a.map_finish()
    res = d_res.cpu().numpy().view(pa.RESULT_DTYPE)
    coff, cids = pa.gather_classes(res, d_arena[: max(used, 1)].cpu().numpy().view(np.uint32), host)
    o_res, o_coff, o_ids, _ = helpers.Oracle(host).map_tiles(tiles, lens, wpr, allowed, 8)
    helpers.assert_same_as_oracle(res, coff, cids, o_res, o_coff, o_ids, what)
    d_counts = torch.zeros(a.counts_len(), dtype=torch.int64, device=dev)
    d_res.zero_()
    a.map_count_batch_device(d_tiles.data_ptr(), d_lens.data_ptr(), n, wpr, d_res.data_ptr(), d_arena.data_ptr(), cap, d_counts.data_ptr(), allowed)
    used, _ = a.map_finish()
    res2 = d_res.cpu().numpy().view(pa.RESULT_DTYPE)
    coff2, cids2 = pa.gather_classes(res2, d_arena[: max(used, 1)].cpu().numpy().view(np.uint32), host)
    helpers.assert_same_as_oracle(res2, coff2, cids2, o_res, o_coff, o_ids, what + " (map + count)")
    assert np.array_equal(d_counts.cpu().numpy(), helpers.counts_reference(o_res, o_coff, o_ids, host)), what
    return o_res


def both_kernels(host, reads, allowed, what):
    """reads of up to 512 bases (the pooled kernel: reads in LDS, narrow lane state) and a batch with longer ones (reads in HBM, wide lane state)"""
    short = [r for r in reads if len(r) <= 512]
    o_res = device_check(host, _subsample(short, 5000), allowed, what)
    long_ = [r for r in reads if len(r) > 512]
    if long_:
        device_check(host, _subsample(long_, 1500) + _subsample(short, 1500, seed=12), allowed, what + " wide")
    return o_res


@pytest.mark.parametrize("allowed", [0, 2])
@pytest.mark.parametrize("k", [20, 24, 31, 64])
def test_hand_built_node_ends_on_block_seams(tmp_path, k, allowed):
    host, triples, forks = stay_cases.hand_built_txome(k, tmp_path)
    reads = stay_cases.sweep_reads(k, triples, forks)
    o_res = both_kernels(host, reads, allowed, "hand-built k=%d allowed=%d" % (k, allowed))
    assert o_res["mapped"].all()


@pytest.mark.parametrize("seed", range(2))
def test_long_chains(tmp_path, seed):
    host, reads, allowed = helpers.long_chain_case(seed, tmp_path)
    k = int(host.arrays()["k"])
    both_kernels(host, reads + stay_cases.case_reads(reads, k, 3000), allowed, "long chains seed %d" % seed)


@pytest.mark.parametrize("seed", range(3))
def test_branch_points(tmp_path, seed):
    host, reads, allowed = helpers.branch_case(seed, tmp_path)
    assert host is not None
    k = int(host.arrays()["k"])
    both_kernels(host, reads + stay_cases.case_reads(reads, k, 3000), allowed, "branch points seed %d" % seed)
