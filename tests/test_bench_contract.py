"""bench.py's helpers and the shape of the bench line it emits (checked on the committed line of the last GPU run)."""
import importlib.util
import json
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
spec = importlib.util.spec_from_file_location("bench", ROOT / "bench.py")
bench = importlib.util.module_from_spec(spec)
spec.loader.exec_module(bench)


def test_algorithmic_bytes_formula():
    # SURVEY.md §8(d) with p=1, n=2, c=126, E=10, r=3 at L=150, K=24
    ctr = dict(reads=1, probes=1, node_visits=2, bases_compared=126, class_sizes=10, result_sizes=3)
    want = 38 + 4 + 1 * (8 + 6 + 12) + 2 * 21 + 2 * 126 / 8 + 8 * 2 + 4 * 10 + 12 + 4 * 3
    assert abs(bench.algorithmic_bytes_per_read(ctr, 150, 24) - want) < 1e-9


def test_usable_cpus_is_sane():
    import os
    n = bench.usable_cpus()
    assert 1 <= n <= (os.cpu_count() or 1)


import pytest


@pytest.mark.parametrize("name", ["r01_pool_bench.json", "r02_bench_config3.json", "r02_bench_config5.json", "r03_bench_config3.json", "r03_bench_config5.json"])
def test_committed_bench_line_has_the_contract_fields(name):
    line = json.loads((ROOT / "profiles" / name).read_text())
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype",
                "data", "config", "roofline", "cpu_baseline"):
        assert key in line, key
    assert line["vs_baseline"] is None and line["scaling"] == "weak" and line["higher_is_better"] is True and "workload" in line["config"]
    r = line["roofline"]
    assert r["bound"] == "hbm" and r["unit"] == "GB/s" and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-9 and r["peak"] == 8000.0
    assert abs(r["achieved"] - r["algorithmic_bytes_per_read"] * r["reads_per_launch"] / (r["kernel_ms"] * 1e-3) / 1e9) < 1e-6 * r["achieved"]
    assert r["traffic"] is None or r["traffic"] > r["algorithmic_bytes_per_read"] * r["reads_per_launch"]
    c = line["cpu_baseline"]
    assert c["kind"] in ("port", "reference") and c["cores"] >= 1 and c["unit"] == line["unit"] and "sample" in c
    assert abs(line["value"] - line["config"]["reads_per_step_per_gpu"] * line["n_gpus"] / (line["ms_per_step"] * 1e-3)) < 1e-6 * line["value"]
    assert r["kernel_ms"] <= line["ms_per_step"] * 1.001   # the dominant kernel fits inside the step it belongs to
    if name.startswith("r03"):   # round 3: the map kernel is timed by the library, the step holds more kernels; config 5 rides in the default line
        assert r["kernel"] == "pa_map_pool_kernel" and r["kernel_ms"] <= r["step_device_ms"] <= line["ms_per_step"] * 1.001 and "rccl_ranks" in line
        assert c["cpus_visible"] >= c["cores"]
        if "config3" in name:
            c5 = line["config5"]
            assert c5["value"] > 0 and c5["parity_sample"]["bit_exact_vs_oracle"] is True and 0 < c5["roofline"]["frac"] < 1
            assert r["traffic"] is not None and line["e2e_reads_per_s"] > 0
    if name.startswith("r02"):   # round 2: the host-to-host leg (config 3 only) and the index set-up times ride along as extra keys
        assert "index_build_s" in line["config"] and "kernel_ms_steps" in r and len(r["kernel_ms_steps"]) == line["steps"]
        if "config3" in name:
            assert line["e2e_reads_per_s"] > 0 and 0 < line["e2e_pcie_frac"] < 1


def test_dump_outputs_resolves_every_class_and_repeats(small_index, tmp_path, monkeypatch):
    """bench.dump_outputs on hand-made records (CPU tensors in place of the device buffers): a seeded sample of the reads, each read's class
    read back as ids whether it is an index class (by reference) or a range of the arena, and the same files from a second call"""
    from types import SimpleNamespace

    import numpy as np
    import torch
    import helpers
    pa = helpers.pa
    host = small_index(24)
    a = host.arrays()
    off, ids, nc = a["ec_offset"].astype(np.int64), a["ec_ids"], int(a["num_classes"])
    rng = np.random.default_rng(3)
    B = 60
    arena = rng.integers(0, 5000, 700).astype(np.uint32)
    res = np.zeros(B, pa.RESULT_DTYPE)
    want = []
    for i in range(B):
        if i % 3 == 0:                                        # unmapped
            want.append(np.zeros(0, np.uint32))
            continue
        if i % 3 == 1:                                        # an index class, returned by reference
            c = int(rng.integers(0, nc))
            res[i]["class_off"], res[i]["class_len"] = pa.PA_CLASS_REF | c, off[c + 1] - off[c]
            want.append(ids[off[c]:off[c + 1]])
        else:                                                 # an intersection: ids in the arena
            o, n = int(rng.integers(0, 680)), int(rng.integers(1, 20))
            res[i]["class_off"], res[i]["class_len"] = o, n
            want.append(arena[o:o + n])
        res[i]["coverage"], res[i]["mismatches"] = 100 + i, pa.PA_MAPPED_BIT | (i % 3)
    run = SimpleNamespace(B=B, host=host, counts=torch.arange(nc + 3, dtype=torch.int64),
                          results=torch.from_numpy(res.view(np.int32).copy()), arena=torch.from_numpy(arena.view(np.int32).copy()))
    monkeypatch.setattr(bench, "DUMP_SAMPLE_READS", 25)
    env = dict(pa=pa, torch=torch, np=np)
    bench.dump_outputs(env, run, str(tmp_path / "a"))
    bench.dump_outputs(env, run, str(tmp_path / "b"))
    names = ("counts", "sample_read", "coverage", "mismatches", "mapped", "class_offsets", "class_ids")
    got = {n: np.load(tmp_path / "a" / (n + ".npy")) for n in names}
    for n in names:
        assert got[n].dtype == np.float64 and np.array_equal(got[n], np.load(tmp_path / "b" / (n + ".npy"))), n
    assert np.array_equal(got["counts"], np.arange(nc + 3))
    sample = got["sample_read"].astype(np.int64)
    assert len(sample) == 25 and np.all(np.diff(sample) > 0) and 0 <= sample[0] and sample[-1] < B
    coff = got["class_offsets"].astype(np.int64)
    assert len(coff) == 26 and coff[-1] == len(got["class_ids"])
    for j, r in enumerate(sample):
        assert np.array_equal(got["class_ids"][coff[j]:coff[j + 1]], want[r].astype(np.float64)), r
        assert got["coverage"][j] == res[r]["coverage"] and got["mapped"][j] == (r % 3 != 0) and got["mismatches"][j] == r % 3
