"""`-m gpu` tier of the designed class sets (tests/class_cases.py): the five finishing states of map_pool_kernel.inc (ST_F_BITS,
ST_F_MASK with window_hits' bitmap read and its binary search into lists without a bitmap, ST_F_LIGHT, ST_F_SCAN, ST_F_COOP), resolve.hip
behind them, the overflow table and compact.hip — every read compared, exactly, with the oracle built on the same arrays AND with the
Python set intersection of its nodes' id sets. tests/test_class_cases.py (CPU tier) asserts that every read of these cases takes the
path its row names; here the same reads, several copies of each and shuffled so that one wave holds reads of every path and of 1 .. 130
classes at once, go through the product."""
import collections

import numpy as np
import pytest

import class_cases
import helpers
from test_class_cases import built_case

pa = helpers.pa
pytestmark = pytest.mark.gpu

_aligners = {}


def aligner(name, k, tail=0):
    key = (name, k, tail)
    if key not in _aligners:
        if pa.lib().pa_device_count() < 1:
            raise RuntimeError("the gpu tier needs a GPU and the HIP library: %s" % pa.lib().pa_last_error().decode())
        _aligners[key] = pa.Pseudoaligner(built_case(name, k, tail)[0], 0)
    return _aligners[key]


def batch(name, k, tail=0, reps=3, unmapped=40, seed=1, total=None):
    """the case's reads `reps` times over and `unmapped` random reads, shuffled (or tiled to `total` reads)
    -> (reads, expected id list per read or None for the random ones)"""
    c = built_case(name, k, tail)[1]
    rng = np.random.RandomState(seed)
    reads, expected = list(c[3]) * reps, list(c[4]) * reps
    for _ in range(unmapped):   # random sequence: none of its k-mers is in the graph
        reads.append("".join("ACGT"[x] for x in rng.randint(0, 4, rng.randint(k, 200))))
        expected.append(None)
    order = rng.permutation(len(reads)) if total is None else rng.randint(0, len(reads), total)
    return [reads[i] for i in order], [expected[i] for i in order]


def assert_python_sets(res, coff, cids, reads, expected, what):
    mapped = (res["mismatches"] >> 31).astype(bool)
    assert np.array_equal(mapped, np.array([e is not None for e in expected])), what
    assert np.array_equal(res["coverage"][mapped], np.array([len(r) for r, e in zip(reads, expected) if e is not None], np.uint32)), what
    assert not (res["mismatches"][mapped] & 0x7FFFFFFF).any(), what
    want_len = np.array([len(e) if e is not None else 0 for e in expected], np.int64)
    assert np.array_equal((coff[1:] - coff[:-1]).astype(np.int64), want_len), what
    assert np.array_equal(cids, np.array([i for e in expected if e for i in e], np.uint32)), what


def check_map_batch(name, k, tail=0, **kw):
    a = aligner(name, k, tail)
    reads, expected = batch(name, k, tail, **kw)
    res, coff, cids = a.map_batch(reads, 2)
    what = "%s K=%d tail=%d" % (name, k, tail)
    assert_python_sets(res, coff, cids, reads, expected, what)
    o_res, o_coff, o_ids, _ = helpers.Oracle(a.host).map_reads(reads, 2, 8)
    helpers.assert_same_as_oracle(res, coff, cids, o_res, o_coff, o_ids, what)


@pytest.mark.parametrize("k", [24, 40])
@pytest.mark.parametrize("name", class_cases.CASES)
def test_map_batch(built, name, k):
    """K = 24 and K = 40 (the K > 32 instantiation is another kernel)"""
    check_map_batch(name, k)


@pytest.mark.parametrize("name,k", [("seams", 24), ("pending32783", 24), ("pending32768", 40), ("nobitmap", 24), ("lists", 40), ("lists", 24)])
def test_wide_packing(built, name, k):
    """the same chains with a same-class tail node of 500 k-mers: reads of more than 512 bases take the wide lane state"""
    check_map_batch(name, k, tail=500, reps=2)


def test_reads_beyond_16383_bases(built):
    check_map_batch("seams", 24, tail=16400, reps=1, unmapped=2)


@pytest.mark.parametrize("name", ["seams", "vectors", "pending32768"])
def test_node_traces(built, name):
    """map_batch_nodes (the trace instantiation): results and visited nodes against the oracle's map_read"""
    a = aligner(name, 24)
    reads, expected = batch(name, 24, reps=1, unmapped=5)
    res, nodes, nlen = a.map_batch_nodes(reads)
    o = helpers.Oracle(a.host)
    for i, r in enumerate(reads):
        rc, ids, cov, mm, onodes = o.map_read(r)
        assert rc == (expected[i] is not None) and (not rc or ids == expected[i]), (name, i)
        assert int(res["mismatches"][i] >> 31) == rc and nodes[i][: nlen[i]].tolist() == (onodes if rc else []), (name, i)
        if rc:
            assert (int(res["coverage"][i]), int(res["mismatches"][i] & 0x7FFFFFFF), int(res["class_len"][i])) == (cov, mm, len(ids)), (name, i)


def device_run(a, reads, ovf=None):
    """map_batch_device with the colour hint, the fused count launch (with the overflow table attached, if any) and the compact records"""
    import torch
    tiles, lens, wpr = pa.encode_reads_host(reads)
    dev = torch.device("cuda", 0)
    n = len(reads)
    d_tiles, d_lens = torch.from_numpy(tiles.view(np.int64)).to(dev), torch.from_numpy(np.asarray(lens, np.uint32).view(np.int32)).to(dev)
    cap = a.arena_hint(n)
    d_res = torch.zeros(n * 4, dtype=torch.int32, device=dev)
    d_arena = torch.zeros(cap, dtype=torch.int32, device=dev)
    d_col = torch.full((n,), -2, dtype=torch.int32, device=dev)
    a.map_batch_device(d_tiles.data_ptr(), d_lens.data_ptr(), n, wpr, d_res.data_ptr(), d_arena.data_ptr(), cap, 2, d_col.data_ptr())
    used, _ = a.map_finish()
    res = d_res.cpu().numpy().view(pa.RESULT_DTYPE).copy()
    coff, cids = pa.gather_classes(res, d_arena[: max(used, 1)].cpu().numpy().view(np.uint32), a.host)
    colour = d_col.cpu().numpy().view(np.uint32).copy()
    d_counts_sep = torch.zeros(a.counts_len(), dtype=torch.int64, device=dev)
    a.counts_accumulate_device(d_res.data_ptr(), d_arena.data_ptr(), d_col.data_ptr(), n, d_counts_sep.data_ptr())
    torch.cuda.synchronize()
    # the fused launch
    d_counts = torch.zeros(a.counts_len(), dtype=torch.int64, device=dev)
    if ovf is not None:
        a.set_overflow(ovf)
    a.map_count_batch_device(d_tiles.data_ptr(), d_lens.data_ptr(), n, wpr, d_res.data_ptr(), d_arena.data_ptr(), cap, d_counts.data_ptr(), 2)
    used2, _ = a.map_finish()
    res2 = d_res.cpu().numpy().view(pa.RESULT_DTYPE).copy()
    coff2, cids2 = pa.gather_classes(res2, d_arena[: max(used2, 1)].cpu().numpy().view(np.uint32), a.host)
    # the compact records of that launch
    scr = pa.lib().pa_compact_scratch_bytes(n)
    d_scr = torch.zeros(scr, dtype=torch.uint8, device=dev)
    d_compact = torch.zeros(n, dtype=torch.int64, device=dev)
    d_packed = torch.zeros(cap + n + 16, dtype=torch.int32, device=dev)
    d_pw = torch.zeros(1, dtype=torch.int64, device=dev)
    pa.check(pa.lib().pa_results_compact_device(a._h, d_res.data_ptr(), d_arena.data_ptr(), cap, n, d_compact.data_ptr(), d_packed.data_ptr(), cap + n + 16,
                                                d_pw.data_ptr(), d_scr.data_ptr(), scr, None))
    torch.cuda.synchronize()
    pw = int(d_pw.item())
    comp = pa.unpack_compact(d_compact.cpu().numpy().view(np.uint64), d_packed[:pw].cpu().numpy().view(np.uint32), a.host)
    if ovf is not None:
        a.set_overflow(None)
    return dict(first=(res, coff, cids), colour=colour, counts_sep=d_counts_sep.cpu().numpy(), fused=(res2, coff2, cids2), counts=d_counts.cpu().numpy(),
                compact=comp)


def check_device(name, k, **kw):
    a = aligner(name, k)
    reads, expected = batch(name, k, **kw)
    what = "%s K=%d" % (name, k)
    ovf = pa.Overflow(0, 1 << 14, 1 << 20)
    r = device_run(a, reads, ovf)
    novel = pa.parse_overflow(ovf.fetch())
    o_res, o_coff, o_ids, _ = helpers.Oracle(a.host).map_reads(reads, 2, 8)
    for key in ("first", "fused", "compact"):
        res, coff, cids = r[key]
        assert_python_sets(res, coff, cids, reads, expected, what + " " + key)
        helpers.assert_same_as_oracle(res, coff, cids, o_res, o_coff, o_ids, what + " " + key)
    # the Python sets say which class every read has: the colour hint, the count table, the overflow table
    arr = a.host.arrays()
    off = arr["ec_offset"].astype(np.int64)
    nc = int(arr["num_classes"])
    known = {tuple(arr["ec_ids"][off[c]:off[c + 1]].tolist()): c for c in range(nc)}
    want_counts = np.zeros(nc + 3, np.int64)
    want_novel = collections.Counter()
    kinds = collections.Counter()
    for i, e in enumerate(expected):
        c = known.get(tuple(e)) if e else None
        if e is None:
            want_counts[nc + 2] += 1
        elif not e:
            want_counts[nc + 1] += 1
        elif c is None:
            want_counts[nc] += 1
            want_novel[tuple(e)] += 1
        else:
            want_counts[c] += 1
        col = int(r["colour"][i])
        assert col == 0xFFFFFFFF or (e is not None and col == known.get(tuple(e))), (what, i, col)   # a hint: right or absent
        kinds["unmapped" if e is None else "empty" if not e else "novel" if c is None else "class"] += 1
    assert np.array_equal(want_counts, helpers.counts_reference(o_res, o_coff, o_ids, a.host))
    assert np.array_equal(r["counts"], want_counts) and np.array_equal(r["counts_sep"], want_counts), what
    assert novel == dict(want_novel), what
    return kinds, want_novel


@pytest.mark.parametrize("name", ["seams", "pending32783", "nobitmap", "lists"])
def test_counts_overflow_and_compact_records(built, name):
    """by-reference, resolved-to-a-class, novel, empty and unmapped reads in one batch: the count table, the overflow table (several
    reads sharing one novel class, and classes met once) and the compact records"""
    kinds, want_novel = check_device(name, 24, reps=3)
    assert all(kinds[x] > 0 for x in ("unmapped", "empty", "novel", "class")), kinds
    assert all(v >= 3 for v in want_novel.values()) and len(want_novel) >= 5
    kinds, want_novel = check_device(name, 24, reps=1, unmapped=3, seed=2)
    assert name == "seams" or min(want_novel.values()) == 1   # (every novel class of the seams is met by two reads of its chain)


@pytest.mark.parametrize("name", ["lists", "pending32768"])
def test_a_batch_beyond_the_direct_count_path(built, name):
    """65 536 + 1 reads tiled from the cases: the key stream of a batch too large for the direct count path (count_sort.hip)"""
    check_device(name, 24, total=65537)
