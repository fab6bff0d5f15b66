"""Shared by tests/test_gpu_probe_at_refill.py, and its child process for the forced-smallest pair dictionary.

A read's first dictionary probe runs in the step that refills its pool slot (map_pool_kernel.inc, PA_PROBE_AT_REFILL). Here: the reads that walk the
edges of that path and the device check they go through — pa_map_batch_device and pa_map_count_batch_device, both bit exact against the oracle,
and the count table against helpers.counts_reference.

As a program (loaded with the pairknobs test build through PA_PRODUCT_SO, PA_PAIR_LOG2 set): the dictionary of gencode_small starts from the
smallest table, the keys that lie behind their home pair are read out of the table itself, and reads that BEGIN with such k-mers are mapped: their
first probe, made at refill, finds another key's pair, and the lane goes on through the SEEK queue."""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
for p in (str(ROOT), str(ROOT / "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import helpers  # noqa: E402

pa = helpers.pa

_text = None
_aligners = {}


def tx_text():
    """the transcripts of gencode_small.fa, joined by N"""
    global _text
    if _text is None:
        _text = "N".join(s.upper() for s in helpers.read_fasta()[1])
    return _text


def reads_at(starts, length):
    """text[s : s + length] for every start whose read lies inside one transcript"""
    text = tx_text()
    out = [text[s:s + length] for s in starts]
    return [r for r in out if len(r) == length and set(r) <= set("ACGT")]


def random_reads(n, length, seed):
    """n reads of `length` bases from random places of the transcripts"""
    rng = np.random.RandomState(seed)
    out = []
    while len(out) < n:
        out += reads_at(rng.randint(0, len(tx_text()) - length, n - len(out)).tolist(), length)
    return out


def aligner(host):
    if id(host) not in _aligners:
        _aligners[id(host)] = (host, pa.Pseudoaligner(host, 0))
    return _aligners[id(host)][1]


def device_check(host, reads, allowed, what, oracle=None):
    """map the reads on device-resident tiles (results + arena, then the fused count table) and compare with the oracle;
    oracle = (res, coff, ids) of these reads when the caller has it already"""
    import torch
    a = aligner(host)
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
    o_res, o_coff, o_ids = oracle if oracle is not None else helpers.Oracle(host).map_tiles(tiles, lens, wpr, allowed, 8)[:3]
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


# ---- the pair dictionary read backwards (device_layout.hpp): entry = tag << 36 | ..., tag = d << (48 - b) | remainder, home pair = pair - d,
# pair_mix(key) = home << (48 - b) | remainder
_M48 = (1 << 48) - 1
_INV1, _INV2 = pow(0x9E3779B1, -1, 1 << 48), pow(0x85EBCA77, -1, 1 << 48)


def pair_unmix(m):
    m = (m * _INV2) & _M48
    m ^= m >> 24
    m = (m * _INV1) & _M48
    return m ^ (m >> 24)


def off_home_kmers(table, b, k, limit):
    """the k-mers (as strings) of up to `limit` entries that lie behind their home pair"""
    rbits = 48 - b
    idx = np.nonzero((table != np.uint64(0xFFFFFFFFFFFFFFFF)) & ((table >> np.uint64(36 + rbits)) != 0))[0]
    out = []
    for i in idx[:: max(1, len(idx) // limit)][:limit].tolist():
        tag = int(table[i]) >> 36
        d, r = tag >> rbits, tag & ((1 << rbits) - 1)
        key = pair_unmix(((((i >> 1) - d) & ((1 << b) - 1)) << rbits) | r)
        out.append("".join("ACGT"[(key >> (2 * j)) & 3] for j in range(k)))
    return out


def main(k):
    import torch  # noqa: F401  (before the product library initialises HIP: tests/conftest.py)
    sys.path.insert(0, str(ROOT / "tests" / "pairdict"))
    import gpu_worker
    host = pa.build_index(str(helpers.FASTA), k, 8)
    table, b, _ = gpu_worker.dict_table(host, -1)   # (the CPU flattener's table: the GPU filler builds the same bytes, tests/test_gpu_dict_pairs.py)
    assert b != 0 and aligner(host).stats().table_slots == 1 << b
    kmers = off_home_kmers(table, b, k, 400)
    text = tx_text()
    starts = [text.find(s) for s in kmers]
    assert min(starts) >= 0, "a key of the table is no k-mer of the transcripts"
    reads = [r for length in (150, 100, k) for r in reads_at(starts, length)]
    assert len(reads) >= 300, len(reads)
    reads += random_reads(200, 150, 5)   # lanes whose first probe hits, beside them
    order = np.random.RandomState(3).permutation(len(reads))
    for allowed in (0, 2):
        o_res = device_check(host, [reads[i] for i in order], allowed, "first k-mers off their home pair, K=%d allowed=%d" % (k, allowed))
        assert o_res["mapped"].any()
    print("pairs=%d off_home_reads=%d" % (b, len(reads) - 200))


if __name__ == "__main__":
    main(int(sys.argv[1]))
