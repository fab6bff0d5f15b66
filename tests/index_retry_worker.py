"""Child process of tests/test_gpu_index_edges.py: loaded with the ibknobs test build of the product (PA_PRODUCT_SO), whose GPU index builder reads
PA_IB_WEAK_ATTEMPTS = n and keeps two bits of every addend of the set hash on its first n attempts of the colour stage. Case `retry` of
tests/index_cases.py (55 classes whose weak hashes collide on every attempt, by both exits of pa_ib_verify_kernel) is built with n = 0 ... 3 (n reruns
of the stage: dexts and dcnt passed as null, run_first allocated again, coltmp rewritten), with n = 4 (the build gives up), with n = 0 again in the
same process, and case `hub` with n = 1 (the rerun's segment kernel over the segment of 102 000 records).

Nothing is asserted here but the model's own conditions: the outcome of every step goes into one line "RESULT {json}" and the parent asserts on it. A
HIP error is not caught: the parent ends the session on it."""
import json
import os
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
for p in (str(ROOT), str(ROOT / "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import helpers  # noqa: E402
import index_cases as ic  # noqa: E402

pa = helpers.pa
KEYS = ("node_seq", "node_start", "node_len", "node_exts", "node_colour", "ec_offset", "ec_ids")
PA_ERR_HIP = -5


def difference(gpu, cpu):
    a, b = gpu.arrays(), cpu.arrays()
    for key in ("k", "num_nodes", "num_classes", "num_transcripts"):
        if a[key] != b[key]:
            return "%s %r != %r" % (key, a[key], b[key])
    for key in KEYS:
        if not np.array_equal(a[key], b[key]):
            return key + " differs"
    return None


def build(c, cpu, n):
    """one device build with the weak hash on the first n attempts -> what came of it"""
    os.environ["PA_IB_WEAK_ATTEMPTS"] = str(n)
    t0 = time.time()
    try:
        gpu = pa.HostIndex.build_packed_device(c.words, c.tx_start, c.k, 0)
    except pa.PaError as e:
        if e.code == PA_ERR_HIP:
            raise
        return dict(error=e.code, message=str(e), seconds=round(time.time() - t0, 3))
    return dict(error=0, difference=difference(gpu, cpu), seconds=round(time.time() - t0, 3))


def main():
    import torch  # noqa: F401  (before the product library initialises HIP: tests/conftest.py)
    out = {}
    c = ic.case("retry")
    ic.check(c)
    cpu = pa.HostIndex.build_packed(c.words, c.tx_start, c.k, 2)
    for n in (0, 1, 2, 3, 4):
        out["retry n=%d" % n] = build(c, cpu, n)
    out["retry n=0 after the failure"] = build(c, cpu, 0)
    out["weak_failures"] = ic.weak_failures(c)
    h = ic.case("hub")
    ic.check(h)
    out["hub n=1"] = build(h, pa.HostIndex.build_packed(h.words, h.tx_start, h.k, 4), 1)
    print("RESULT " + json.dumps(out))


if __name__ == "__main__":
    main()
