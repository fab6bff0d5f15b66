"""`-m gpu` tier: the launch paths of csrc/device_index.hip — the three device entry points are one path through the per-stream launch context, a released
context comes back, the timing calls answer for the launch they belong to, and a context created from a thread whose current device is another GPU
lands on the index's GPU. The index is gencode_small at K = 24, the reads come from pa_simulate_reads_device: 4 096 + 37 of 100 bases (a ragged last tile)."""
import math
import threading

import numpy as np
import pytest

import helpers

pa = helpers.pa
pytestmark = pytest.mark.gpu

N, READ_LEN, WPR, SEED, PPM, ALLOWED = 4096 + 37, 100, 4, 12, 15000, 2


@pytest.fixture(scope="module")
def aligner(small_index):
    if pa.lib().pa_device_count() < 1:
        raise RuntimeError("the gpu tier needs a GPU and the HIP library: %s" % pa.lib().pa_last_error().decode())
    return pa.Pseudoaligner(small_index(24), 0)


class Batch:
    """the reads on `device`, simulated on `stream`, and buffers for one launch on them"""

    def __init__(self, a, device, stream):
        import torch
        self.a, self.stream = a, stream
        self.dev = torch.device("cuda", device)
        self.tx = pa.Txome.from_host_index(a.host)
        self.d_tiles = torch.zeros(pa.lib().pa_tiles_words(N, WPR), dtype=torch.int64, device=self.dev)
        self.d_lens = torch.zeros(N, dtype=torch.int32, device=self.dev)
        self.tx.simulate_device(READ_LEN, SEED, N, self.d_tiles.data_ptr(), self.d_lens.data_ptr(), PPM, 0, WPR, device=device, stream=stream)
        pa.check(pa.lib().pa_stream_synchronize(stream or None))
        self.cap = a.arena_hint(N)
        self.d_res = torch.zeros(N * 4, dtype=torch.int32, device=self.dev)
        self.d_arena = torch.zeros(self.cap, dtype=torch.int32, device=self.dev)

    def launch(self, entry, n=N):
        """one launch through `entry` + pa_map_finish: (records, class offsets, class ids, arena_used, arena_needed, count table or None)"""
        import torch
        a, t, l, r, ar = self.a, self.d_tiles.data_ptr(), self.d_lens.data_ptr(), self.d_res.data_ptr(), self.d_arena.data_ptr()
        self.d_res.zero_()
        d_counts = None if entry == "map" else torch.zeros(a.counts_len(), dtype=torch.int64, device=self.dev)
        torch.cuda.synchronize(self.dev)
        if entry == "map":
            a.map_batch_device(t, l, n, WPR, r, ar, self.cap, ALLOWED, 0, self.stream)
        elif entry == "count":
            a.map_count_batch_device(t, l, n, WPR, r, ar, self.cap, d_counts.data_ptr(), ALLOWED, self.stream)
        else:
            a.map_count_batch_uniform_device(t, READ_LEN, n, WPR, r, ar, self.cap, d_counts.data_ptr(), ALLOWED, self.stream)
        used, need = a.map_finish(self.stream)
        res = self.d_res.cpu().numpy().view(pa.RESULT_DTYPE)[:n]
        coff, cids = pa.gather_classes(res, self.d_arena[: max(used, 1)].cpu().numpy().view(np.uint32), a.host)
        return res, coff, cids, used, need, None if d_counts is None else d_counts.cpu().numpy()


def same_records(got, want, what):
    """records and classes of two mappings of the same reads (an arena offset is where the launch happened to put the class: the ids are compared)"""
    res, coff, cids = got[:3]
    w_res, w_coff, w_cids = want[:3]
    for f in ("coverage", "mismatches", "class_len"):
        assert np.array_equal(res[f], w_res[f]), (what, f)
    by_ref = (w_res["class_off"] & pa.PA_CLASS_REF) != 0
    assert np.array_equal((res["class_off"] & pa.PA_CLASS_REF) != 0, by_ref), what
    assert np.array_equal(res["class_off"][by_ref], w_res["class_off"][by_ref]), what
    assert np.array_equal(coff, w_coff) and np.array_equal(cids, w_cids), what


@pytest.fixture(scope="module")
def reference(aligner):
    """the reads mapped the ordinary way: pa_map_batch of their ASCII on the null stream (records, class offsets, class ids)"""
    tx = pa.Txome.from_host_index(aligner.host)
    h_tiles, h_lens = tx.simulate_host(READ_LEN, SEED, N, PPM, 0, WPR)
    res, coff, cids = aligner.map_batch(pa.unpack_tiles(h_tiles, h_lens, WPR), ALLOWED)
    assert int((res["mismatches"] >> 31).sum()) > N // 2 and int((res["class_len"] > 1).sum()) > 0   # (not vacuous)
    return res, coff, cids


def test_three_entry_points_are_one_path_and_a_released_context_comes_back(aligner, reference):
    import torch
    a = aligner
    s = torch.cuda.Stream(device=torch.device("cuda", 0))
    assert s.cuda_stream != 0
    b = Batch(a, 0, s.cuda_stream)
    try:
        first = {e: b.launch(e) for e in ("map", "count", "uniform")}
        a.release_stream(s.cuda_stream)
        empty = b.launch("map", 0)   # the fresh context: nothing launched, nothing used
        assert (empty[3], empty[4]) == (0, 0)
        second = {e: b.launch(e) for e in ("map", "count", "uniform")}
    finally:
        a.release_stream(s.cuda_stream)
    want = first["map"]
    for rnd, runs in (("before", first), ("after", second)):
        for e, got in runs.items():
            what = "%s the release, %s" % (rnd, e)
            same_records(got, want, what)
            assert (got[3], got[4]) == (want[3], want[4]), (what, got[3:5], want[3:5])
            if e != "map":
                assert np.array_equal(got[5], first["count"][5]), what
    assert int(first["count"][5].sum()) == N
    # class_off of pa_map_batch points into its CSR: the reference is compared through its ids
    res, coff, cids = reference
    for f in ("coverage", "mismatches", "class_len"):
        assert np.array_equal(want[0][f], res[f]), f
    assert np.array_equal(want[1], coff) and np.array_equal(want[2], cids)


def test_timing_answers_for_the_last_launch_on_the_stream(aligner):
    import torch
    a = aligner
    s = torch.cuda.Stream(device=torch.device("cuda", 0))
    b = Batch(a, 0, s.cuda_stream)

    def no_timing():
        for call in (a.map_kernel_ms, a.map_stage_ms):
            with pytest.raises(pa.PaError) as e:
                call(s.cuda_stream)
            assert e.value.code == pa._ffi.PA_ERR_INVALID_ARG

    try:
        no_timing()   # no launch on this stream yet
        a.set_timing(True)
        b.launch("count")
        ms = a.map_stage_ms(s.cuda_stream)
        assert len(ms) == 3 and all(math.isfinite(x) and x >= 0 for x in ms), ms
        assert ms[0] == a.map_kernel_ms(s.cuda_stream)   # the same two events
        a.set_timing(False)
        b.launch("count")
        no_timing()   # the last launch was not timed
    finally:
        a.set_timing(False)
        a.release_stream(s.cuda_stream)


def test_context_of_a_new_stream_lands_on_the_index_device(small_index, reference):
    """the launch makes the index's device current BEFORE it looks the stream's context up (the lookup allocates the control block)"""
    import torch
    if pa.lib().pa_device_count() < 2:
        pytest.skip("needs two devices")
    a1 = pa.Pseudoaligner(small_index(24), 1)
    out, errors = [], []

    def worker():
        try:
            torch.cuda.set_device(0)
            torch.zeros(1, device="cuda:0")   # device 0 is this thread's current device, initialised
            s = torch.cuda.Stream(device=torch.device("cuda", 1))
            b = Batch(a1, 1, s.cuda_stream)
            torch.cuda.set_device(0)
            try:
                out.append(b.launch("map"))
            finally:
                a1.release_stream(s.cuda_stream)
        except Exception as e:   # noqa: BLE001
            errors.append(e)

    th = threading.Thread(target=worker)
    th.start()
    th.join()
    assert not errors, errors
    res, coff, cids = reference
    for f in ("coverage", "mismatches", "class_len"):
        assert np.array_equal(out[0][0][f], res[f]), f
    assert np.array_equal(out[0][1], coff) and np.array_equal(out[0][2], cids)
