"""`-m gpu` tier: bench.py's plain run as it is launched for every change: the result line, --steps honoured, and --dump-outputs
writing the same outputs from two runs with the same arguments."""
import json
import subprocess
import sys

import numpy as np
import pytest

import helpers

pytestmark = pytest.mark.gpu

ARGS = ["--gpus", "1", "--steps", "3", "--warmup", "1", "--workload", "config2", "--batch", "2000000"]


def _bench(*extra):
    out = subprocess.run([sys.executable, str(helpers.ROOT / "bench.py")] + ARGS + list(extra), capture_output=True, text=True, timeout=600,
                         cwd=str(helpers.ROOT))
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    return json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])


def test_plain_run_line_and_outputs_repeat(tmp_path):
    lines = [_bench("--dump-outputs", str(tmp_path / d)) for d in ("a", "b")]
    for line in lines:
        assert line["steps"] == 3 and line["warmup"] == 1 and line["n_gpus"] == 1 and line["higher_is_better"] is True
        assert line["unit"] == "reads/s" and line["dtype"] == "u64" and line["ms_per_step"] > 0
        assert abs(line["value"] - 2_000_000 / (line["ms_per_step"] * 1e-3)) < 1e-6 * line["value"]
        assert "parity_sample" not in line and "roofline" not in line and "cpu_baseline" not in line   # (--full only)
    files = sorted(p.name for p in (tmp_path / "a").iterdir())
    assert files == sorted(p.name for p in (tmp_path / "b").iterdir()) and "counts.npy" in files and "class_ids.npy" in files
    assert sum((tmp_path / "a" / f).stat().st_size for f in files) <= 64 << 20
    for f in files:
        x, y = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert x.dtype == np.float64 and np.array_equal(x, y), f
    counts = np.load(tmp_path / "a" / "counts.npy")
    assert counts.sum() == 3 * 2_000_000                              # the table of the three timed steps
    mapped = np.load(tmp_path / "a" / "mapped.npy")
    assert len(mapped) == 1 << 18 and mapped.mean() > 0.5               # error-free reads of the indexed transcripts
