"""Child process of tests/test_gpu_dict_pairs.py: loaded with the pairknobs test build of the product (PA_PRODUCT_SO) and PA_PAIR_LOG2 set, so that the
dictionary of gencode_small starts from the smallest table and keys that lie behind their home pair are common. Checks, in this order: the GPU filler's
table equals the CPU flattener's byte for byte; fifty GPU builds give one table; the table holds keys off their home; reads map like the oracle."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
for p in (str(ROOT), str(ROOT / "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import helpers  # noqa: E402

pa = helpers.pa


def dict_table(host, device, builds=1):
    """(bytes as a u64 array, dict_pairs, later builds that differ) through the library's test surface padbg_dict_table"""
    fn = pa.lib().padbg_dict_table
    fn.restype = C.c_int
    flat = host.flat()
    n, pairs, diff = C.c_uint64(), C.c_uint32(), C.c_uint32()
    args = lambda buf, cap: (C.byref(flat), C.c_int(device), C.c_uint32(1 if buf is None else builds), buf, C.c_uint64(cap), C.byref(n), C.byref(pairs), C.byref(diff))
    assert fn(*args(None, 0)) == 0, pa.lib().pa_last_error()
    out = np.empty(n.value // 8, np.uint64)
    assert fn(*args(C.c_void_p(out.ctypes.data), out.nbytes)) == 0, pa.lib().pa_last_error()
    return out, pairs.value, diff.value


def off_home(table, pairs):
    """entries whose tag holds a displacement (device_layout.hpp: tag = bits 36.., d above the 48 - b remainder bits)"""
    full = table[table != np.uint64(0xFFFFFFFFFFFFFFFF)]
    return int(np.count_nonzero((full >> np.uint64(36 + 48 - pairs)) != 0)), len(full)


def main(k):
    import torch
    host = pa.build_index(str(helpers.FASTA), k, 8)
    cpu, cpu_pairs, _ = dict_table(host, -1)
    gpu, gpu_pairs, differing = dict_table(host, 0, builds=50)
    assert cpu_pairs == gpu_pairs != 0 and cpu.shape == gpu.shape and np.array_equal(cpu, gpu), "GPU filler and CPU flattener disagree"
    assert differing == 0, "%d of 50 GPU builds differ" % differing
    far, keys = off_home(gpu, gpu_pairs)
    assert far > 0, "no key off its home"
    N, L = 4096, 100
    a = pa.Pseudoaligner(host, 0)
    assert a.stats().table_slots == 1 << gpu_pairs
    wpr = pa.lib().pa_words_per_read(L)
    dev = torch.device("cuda", 0)
    for ppm in (0, 10000):
        tiles, lens = pa.Txome.from_host_index(host).simulate_host(L, 4, N, ppm, 0, wpr)
        o_res, o_coff, o_ids, _ = helpers.Oracle(host).map_tiles(tiles, lens, wpr, 2, 4)
        d_tiles = torch.from_numpy(tiles.view(np.int64)).to(dev)
        d_lens = torch.from_numpy(lens.view(np.int32)).to(dev)
        cap = a.arena_hint(N)
        d_res = torch.zeros(N * 4, dtype=torch.int32, device=dev)
        d_arena = torch.zeros(cap, dtype=torch.int32, device=dev)
        d_col = torch.zeros(N, dtype=torch.int32, device=dev)
        a.map_batch_device(d_tiles.data_ptr(), d_lens.data_ptr(), N, wpr, d_res.data_ptr(), d_arena.data_ptr(), cap, 2, d_col.data_ptr())
        used, _ = a.map_finish()
        res = d_res.cpu().numpy().view(pa.RESULT_DTYPE)
        coff, cids = pa.gather_classes(res, d_arena[: max(used, 1)].cpu().numpy().view(np.uint32), host)
        helpers.assert_same_as_oracle(res, coff, cids, o_res, o_coff, o_ids, "gpu, forced table, K=%d ppm=%d" % (k, ppm))
    print("pairs=%d keys=%d off_home=%d" % (gpu_pairs, keys, far))


if __name__ == "__main__":
    main(int(sys.argv[1]))
