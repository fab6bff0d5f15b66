"""`-m gpu`: the GPU index builder (csrc/index_build.hip) on the designed transcriptomes of tests/index_cases.py — the grid-stride trip of the jump
kernel and 22 jump rounds, transcript ids at 2^24 - 2 and the refusal at 2^24, runs of empty transcripts, every bit alignment of a node's first k-mer,
packed words that end with the buffer, a k-mer with 102 000 occurrence records — and, under the ibknobs test build in a child process
(tests/index_retry_worker.py), the rerun of the colour stage after colliding set hashes and the failure after four attempts.

Every case is built twice on the device (identical bytes: the racing in-place updates of the jump kernel are not observable) and must equal (a) the CPU
builder's index array for array and (b) the model's expectation (tests/test_index_cases.py pins the CPU builder on it, so a fault the two builders share
still shows). Every comparison is exact. A HIP error, or a child that ends by a signal, by abort or at its time limit, ends the session: nothing more is
started on a GPU that may have faulted, and nothing is retried."""
import json
import os
import re
import subprocess
import sys
import time

import numpy as np
import pytest

import helpers
import index_cases as ic
from test_gpu_index_build import KEYS, assert_same_index
from test_index_cases import assert_expected

pa = helpers.pa
pytestmark = pytest.mark.gpu

PA_ERR_HIP, PA_ERR_UNSUPPORTED, PA_ERR_INTERNAL = -5, -8, -9   # include/pseudoaligner_amd.h
WORKER = helpers.ROOT / "tests" / "index_retry_worker.py"
CASES = [n for n in ic.NAMES if n != "retry"] + ["retry"]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if pa.lib().pa_device_count() < 1:
        raise RuntimeError("the gpu tier needs a GPU and the HIP library: %s" % pa.lib().pa_last_error().decode())


def device_build(words, tx_start, k, what):
    try:
        return pa.HostIndex.build_packed_device(words, tx_start, k, 0)
    except pa.PaError as e:
        if e.code == PA_ERR_HIP:
            pytest.exit("GPU index builder, %s: %s" % (what, e), returncode=3)
        raise


@pytest.mark.parametrize("name", CASES)
def test_case_on_the_device_builder(name):
    c = ic.case(name)
    ic.check(c)
    t0 = time.time()
    first = device_build(c.words, c.tx_start, c.k, name)
    t1 = time.time()
    second = device_build(c.words, c.tx_start, c.k, name)
    t2 = time.time()
    cpu = pa.HostIndex.build_packed(c.words, c.tx_start, c.k, 4)
    print("index edges %s: device builds %.3f s and %.3f s, CPU builder (4 threads) %.3f s" % (name, t1 - t0, t2 - t1, time.time() - t2))
    a, b = first.arrays(), second.arrays()
    for key in ("k", "num_nodes", "num_classes", "num_transcripts"):
        assert a[key] == b[key], "%s: two device builds, %s" % (name, key)
    for key in KEYS:
        assert a[key].tobytes() == b[key].tobytes(), "%s: two device builds differ in %s" % (name, key)
    assert_same_index(first, cpu, name)
    assert_expected(first, c, name + ", device builder")


def test_two_to_the_24_transcripts_are_refused_and_the_next_build_works():
    c = ic.id_edge(20, num_tx=1 << 24)
    assert c.num_tx == 1 << 24 and c.ids[-1] == (1 << 24) - 1
    with pytest.raises(pa.PaError) as e:
        device_build(c.words, c.tx_start, c.k, "2^24 transcripts")
    assert e.value.code == PA_ERR_UNSUPPORTED and "24 bits" in str(e.value), str(e.value)
    del c
    c = ic.case("empties-k8-empty")
    assert_expected(device_build(c.words, c.tx_start, c.k, "after the refusal"), c, "the build after the refusal")


# ---- the retry of the colour stage: one child process under the ibknobs build ----
_child = {}


def retry_results():
    """A child that ends by a signal, by abort or at its time limit may have left the GPU faulted: nothing more is started on it"""
    if not _child:
        so = helpers._build.build_ibknobs_variant()
        env = {k: v for k, v in os.environ.items() if k != "PA_IB_WEAK_ATTEMPTS"}
        env["PA_PRODUCT_SO"] = str(so)
        t0 = time.time()
        try:
            proc = subprocess.run([sys.executable, str(WORKER)], capture_output=True, text=True, env=env, timeout=180)
        except subprocess.TimeoutExpired:
            pytest.exit("index retry: the child did not end within 180 s", returncode=3)
        out = proc.stdout + proc.stderr
        if proc.returncode < 0 or proc.returncode in (124, 134, 137, 139) or re.search(r"illegal memory access|hip ?error|pseudoaligner_amd error -5|HSA_STATUS_ERROR|Memory access fault", out, re.I):
            pytest.exit("index retry: the child ended with %d\n%s" % (proc.returncode, out[-3000:]), returncode=3)
        assert proc.returncode == 0, out[-6000:]
        lines = [l for l in proc.stdout.splitlines() if l.startswith("RESULT ")]
        assert lines, out[-3000:]
        _child.update(json.loads(lines[-1][len("RESULT "):]))
        print("index retry child: %.1f s  %s" % (time.time() - t0, lines[-1]))
    return _child


@pytest.mark.parametrize("n", [0, 1, 2, 3])
def test_colliding_set_hashes_rerun_the_colour_stage(n):
    r = retry_results()["retry n=%d" % n]
    assert r["error"] == 0 and r["difference"] is None, r


def test_four_colliding_attempts_fail_the_build_and_the_next_one_works():
    res = retry_results()
    r = res["retry n=4"]
    assert r["error"] == PA_ERR_INTERNAL and "set hashes kept colliding" in r["message"], r
    assert "(%d k-mers)" % res["weak_failures"] in r["message"], (r, res["weak_failures"])   # the model's count of the k-mers that fail the content check
    r = res["retry n=0 after the failure"]
    assert r["error"] == 0 and r["difference"] is None, r


def test_the_rerun_over_a_segment_of_102000_records():
    r = retry_results()["hub n=1"]
    assert r["error"] == 0 and r["difference"] is None, r
