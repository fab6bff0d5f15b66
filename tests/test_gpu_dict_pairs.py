"""GPU tier: mapping through the pair dictionary (K <= 24) at the smallest shapes that reach it, against the oracle — records and class ids — and one
K = 25 index through the 16-byte slots beside it. The dictionary is the one the GPU filler builds (index_fill.hip)."""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers

pa = helpers.pa

N, READ_LEN = 4096, 100
_cases = {}


def _case(k, ppm):
    """index, reads and the oracle's answer: computed once per (k, ppm)"""
    if k not in _cases:
        _cases[k] = {"host": pa.build_index(str(helpers.FASTA), k, 8)}
    c = _cases[k]
    if ppm not in c:
        wpr = pa.lib().pa_words_per_read(READ_LEN)
        tiles, lens = pa.Txome.from_host_index(c["host"]).simulate_host(READ_LEN, 4, N, ppm, 0, wpr)
        c[ppm] = (tiles, lens, wpr, helpers.Oracle(c["host"]).map_tiles(tiles, lens, wpr, 2, 4))
    return (c["host"],) + c[ppm]


@pytest.mark.gpu
@pytest.mark.parametrize("k", [24, 21, 25])
@pytest.mark.parametrize("ppm", [0, 10000])
def test_gpu_maps_like_the_oracle(built, k, ppm):
    """error-free reads, and reads with 1 % substitutions: their lanes probe past a miss, two positions per step"""
    import torch
    host, tiles, lens, wpr, (o_res, o_coff, o_ids, ctr) = _case(k, ppm)
    a = pa.Pseudoaligner(host, 0)
    st = a.stats()
    # the format: a power of two of 16-byte pairs for K <= 24; the 16-byte slots at load 0.25 (4 n + 4 of them: no power of two) for K = 25
    assert (st.table_slots & (st.table_slots - 1) == 0) == (k <= 24) and st.table_slots >= 4 * st.num_kmers
    dev = torch.device("cuda", 0)
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
    helpers.assert_same_as_oracle(res, coff, cids, o_res, o_coff, o_ids, "gpu K=%d ppm=%d" % (k, ppm))
    if ppm:
        assert ctr["reseeks"] > 0   # the oracle re-seeked behind errors: the scan past a miss was exercised


@pytest.mark.gpu
def test_gpu_filler_builds_the_cpu_flatteners_table(built):
    """gencode_small at K = 24, the size the library chooses: index_fill.hip and device_flatten.cpp give the same bytes"""
    sys.path.insert(0, str(helpers.ROOT / "tests" / "pairdict"))
    worker = importlib.import_module("gpu_worker")
    host = _case(24, 0)[0]
    cpu, cpu_pairs, _ = worker.dict_table(host, -1)
    gpu, gpu_pairs, differing = worker.dict_table(host, 0, builds=2)
    assert cpu_pairs == gpu_pairs != 0 and differing == 0 and np.array_equal(cpu, gpu)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [24, 21])
def test_forced_small_table_on_the_gpu(built, k):
    """The same reads with the sizing hook forcing the smallest table the builders can stand (PA_PAIR_LOG2=21, read by the pairknobs test build in
    a child process: tests/pairdict/gpu_worker.py). There: GPU table == CPU table byte for byte, fifty GPU builds give one table, the table holds
    keys behind their home pair, and error-free reads and reads with 1 % substitutions map like the oracle. That the reads MEET such keys is
    asserted where a counter exists: tests/test_dict_pairs.py maps the same reads through the same (byte-equal) table on the host emulator and
    asserts that its seek steps exceed the oracle's probes."""
    sys.path.insert(0, str(helpers.ROOT))
    so = importlib.import_module("rust-pseudoaligner_amd._build").build_pairknobs_variant()
    env = dict(os.environ, PA_PRODUCT_SO=str(so), PA_PAIR_LOG2="21")
    proc = subprocess.run([sys.executable, str(helpers.ROOT / "tests" / "pairdict" / "gpu_worker.py"), str(k)], capture_output=True, text=True, env=env)
    assert proc.returncode == 0, proc.stdout + proc.stderr
    assert "off_home=" in proc.stdout
