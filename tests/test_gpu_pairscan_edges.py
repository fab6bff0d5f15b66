"""pa_pairs_gather_device (csrc/pair_scan.hip) on hand-written texts and record tables against tests/pairscan_model.py, bit for bit: the
gathered bytes of both mates, every offset, the whole control block. Both outputs are pre-filled with a canary byte and lie between 256
canary bytes on either side, and the whole buffers are compared, so a byte written outside [0, bytes) of an output fails the test; the
offset arrays carry sentinels behind their last entry. Every comparison is exact. A HIP error ends the session: nothing more is started on
a GPU that may have faulted."""
import numpy as np
import pytest

import helpers
import pairscan_model as pm

pytestmark = pytest.mark.gpu

GUARD, CANARY, OFF_SENTINEL = 256, 0xEE, 0x7A7A7A7A7A7A7A7A
WHOLE = pm.WHOLE_READ


@pytest.fixture(scope="module")
def torch_gpu():
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("the gpu tier needs a GPU")
    try:
        helpers.pa.lib()
    except ImportError:   # a tree that was never built
        helpers.build_all()
    return torch


def seqs(rng, lengths):
    return [bytes(rng.choice(np.frombuffer(b"ACGTN", np.uint8), n).tobytes()) for n in lengths]


def gather(torch, segments, prefix, cap1, cap2, n_off):
    """segments: (text1, rows1, text2, rows2, base) in call order -> (bytes1, off1, bytes2, off2, ctl) as numpy, guards and sentinels checked"""
    pa = helpers.pa
    bufs = [torch.full((GUARD + cap + GUARD,), CANARY, dtype=torch.uint8, device="cuda") for cap in (cap1, cap2)]
    offs = [torch.full((n_off + 8,), OFF_SENTINEL, dtype=torch.int64, device="cuda") for _ in range(2)]
    ctl = torch.full((8,), 0x5555, dtype=torch.int64, device="cuda")
    keep = []
    try:
        for text1, rows1, text2, rows2, base in segments:
            t = [torch.frombuffer(bytearray(x), dtype=torch.uint8).cuda() if x else torch.zeros(0, dtype=torch.uint8, device="cuda") for x in (text1, text2)]
            r = [torch.from_numpy(np.array(rows, np.uint32).reshape(-1, 4).view(np.int32).copy()).cuda() for rows in (rows1, rows2)]
            keep += t + r
            pa.pairs_gather_device(t[0], r[0], t[1], r[1], prefix, base, bufs[0][GUARD:GUARD + cap1], offs[0][:n_off], bufs[1][GUARD:GUARD + cap2], offs[1][:n_off], ctl)
        torch.cuda.synchronize()
    except (pa.PaError, RuntimeError) as e:
        pytest.exit("pair scan kernels: %s" % e, returncode=3)
    out = []
    for buf, off, cap in zip(bufs, offs, (cap1, cap2)):
        b, o = buf.cpu().numpy(), off.cpu().numpy().view(np.uint64)
        assert (b[:GUARD] == CANARY).all() and (b[GUARD + cap:] == CANARY).all(), "bytes were written outside an output buffer"
        assert (o[n_off:] == OFF_SENTINEL).all(), "offsets were written behind the array"
        out += [b[GUARD:GUARD + cap], o[:n_off]]
    return out[0], out[1], out[2], out[3], ctl.cpu().numpy().view(np.uint64)


def check(torch, segments, prefix, cap1=None, cap2=None):
    """one batch on the GPU and in the model: everything equal; returns the model"""
    n = max(base + len(rows1) for _, rows1, _, _, base in segments)
    need1 = sum(min(q[3], prefix) for _, rows1, _, _, _ in segments for q in rows1) + 37
    need2 = sum(q[3] for _, _, _, rows2, _ in segments for q in rows2) + 37
    cap1, cap2 = need1 if cap1 is None else cap1, need2 if cap2 is None else cap2
    model = pm.Batch(cap1, cap2, n + 1, CANARY)
    for text1, rows1, text2, rows2, base in segments:
        model.add_segment(text1, rows1, text2, rows2, prefix, base)
    b1, o1, b2, o2, ctl = gather(torch, segments, prefix, cap1, cap2, n + 1)
    assert ctl.tolist() == model.ctl_words() + [0, 0], (ctl.tolist(), model.ctl_words())
    for got, want, name in ((o1, model.off1, "off1"), (o2, model.off2, "off2")):
        want = [OFF_SENTINEL if w is None else w for w in want]
        assert got.tolist() == want, (name, [(i, g, w) for i, (g, w) in enumerate(zip(got.tolist(), want)) if g != w][:5])
    for got, want, name in ((b1, model.bytes1, "bytes1"), (b2, model.bytes2, "bytes2")):
        want = np.frombuffer(bytes(want), np.uint8)
        bad = np.flatnonzero(got != want)
        assert len(bad) == 0, (name, len(bad), bad[:5].tolist(), got[bad[:5]].tolist(), want[bad[:5]].tolist())
    return model


def segment(recs1, recs2, base=0, lead1=b"", lead2=b""):
    t1, r1 = pm.layout(recs1, lead=lead1)
    t2, r2 = pm.layout(recs2, lead=lead2)
    return (t1, r1, t2, r2, base)


@pytest.mark.parametrize("m", [0, 1, 63, 64, 65, 257])
def test_pair_counts(torch_gpu, m):
    rng = np.random.RandomState(m)
    s1, s2 = seqs(rng, rng.randint(28, 40, m)), seqs(rng, rng.randint(0, 200, m))
    recs1 = [(b"read%d/1" % i, s) for i, s in enumerate(s1)]
    recs2 = [(b"read%d/2" % i, s) for i, s in enumerate(s2)]
    model = check(torch_gpu, [segment(recs1, recs2, lead1=b"#", lead2=b"###")], 28)
    assert model.ctl["first_bad"] == pm.NONE and model.off1[m] == 28 * m


ID_CASES = [(b"read1", b"read1", True), (b"read1", b"read2", False), (b"read1", b"read10", False), (b"read10", b"read1", False), (b"a/1", b"a/2", True), (b"a/1", b"a", True),
            (b"a", b"a/2", True), (b"a/3", b"a/3", True), (b"a/3", b"a", False), (b"/1", b"", True), (b"/1", b"/2", True), (b"", b"", True), (b"", b"x", False), (b"x", b"x", True),
            (b"x", b"y", False), (b"1", b"1", True), (b"/", b"/", True), (b"/1", b"/", False), (b"a/1/1", b"a/1/2", True), (b"a/1/1", b"a/1", False)]   # (cut once, on both sides)


def test_ids_one_pair_at_a_time(torch_gpu):
    for id1, id2, same in ID_CASES:
        model = check(torch_gpu, [segment([(id1, b"ACGT")], [(id2, b"TTGCA")])], WHOLE)
        assert (model.ctl["first_bad"] == pm.NONE) == same, (id1, id2)
    # ... and all of them in one segment: the first pair that differs
    model = check(torch_gpu, [segment([(a, b"ACGT") for a, _, _ in ID_CASES], [(b, b"TT") for _, b, _ in ID_CASES])], WHOLE)
    assert model.ctl["first_bad"] == 1


@pytest.mark.parametrize("lead", range(16))
def test_id_lengths_at_every_address(torch_gpu, lead):
    rng = np.random.RandomState(100 + lead)
    for n in (15, 16, 17, 63, 64, 65):
        ident = bytes(rng.randint(ord("a"), ord("z") + 1, n).astype(np.uint8).tobytes())
        other = ident[:-1] + (b"A" if ident[-1:] != b"A" else b"B")      # the last byte only
        shorter = ident[:-1]                                             # the length only
        recs1 = [(ident, b"ACGT"), (ident, b"AC"), (ident, b"A"), (ident + b"/1", b"")]
        recs2 = [(ident, b"T"), (other, b"TT"), (shorter, b"TTT"), (ident + b"/2", b"TTTT")]
        for k in (3, 2, 1):     # the differing pairs dropped one by one from the front: first bad is pair 1 twice, then none
            a, b = recs1[:1] + recs1[4 - k:], recs2[:1] + recs2[4 - k:]
            model = check(torch_gpu, [segment(a, b, lead1=b"." * lead, lead2=b"." * ((lead * 7 + 3) % 16))], WHOLE)
            assert model.ctl["first_bad"] == (1 if k >= 2 else pm.NONE), (n, k)


def test_mismatch_positions(torch_gpu):
    rng = np.random.RandomState(7)
    s1, s2 = seqs(rng, [28] * 140), seqs(rng, rng.randint(30, 120, 140))
    for bad, first in (((5, 70, 130), 5), ((139,), 139), ((), pm.NONE)):
        recs1 = [(b"r%d/1" % i, s) for i, s in enumerate(s1)]
        recs2 = [(b"r%d/2" % i if i not in bad else b"r%dx/2" % i, s) for i, s in enumerate(s2)]
        assert check(torch_gpu, [segment(recs1, recs2)], 28).ctl["first_bad"] == first


@pytest.mark.parametrize("prefix", [2, 28, 32, WHOLE])
def test_r1_lengths_and_prefixes(torch_gpu, prefix):
    rng = np.random.RandomState(prefix & 0xFF)
    p = 32 if prefix == WHOLE else prefix
    lengths = [0, 1, p - 1, p, p + 1, 300] * 3
    recs1 = [(b"i%d" % i, s) for i, s in enumerate(seqs(rng, lengths))]
    recs2 = [(b"i%d" % i, s) for i, s in enumerate(seqs(rng, [7] * len(lengths)))]
    model = check(torch_gpu, [segment(recs1, recs2, lead1=b"..")], prefix)
    assert model.ctl["max_len1"] == (300 if prefix == WHOLE else prefix)


@pytest.mark.parametrize("lead", range(16))
def test_r2_lengths_at_every_address(torch_gpu, lead):
    """0 .. 513 bytes are gathered by eight lanes a pair, 70 000 bytes by a wave: sources at every address mod 16 (the lead), destinations
    wherever the lengths before them put them; R1's prefix pieces lie between them in their own output"""
    rng = np.random.RandomState(200 + lead)
    lengths = [0, 1, 2, 150, 511, 512, 513, 70000, 3, 1025, 1024]
    recs2 = [(b"p%d/2" % i, s) for i, s in enumerate(seqs(rng, lengths))]
    recs1 = [(b"p%d/1" % i, s) for i, s in enumerate(seqs(rng, [28 + (i % 3) for i in range(len(lengths))]))]
    model = check(torch_gpu, [segment(recs1, recs2, lead1=b"." * (15 - lead), lead2=b"." * lead)], 28)
    assert model.ctl["max_len2"] == 70000 and model.ctl["first_bad"] == pm.NONE


def test_long_r1_takes_the_wave_path_too(torch_gpu):
    rng = np.random.RandomState(3)
    recs1 = [(b"a", s) for s in seqs(rng, [5000, 1, 1025, 0, 2049])]
    recs2 = [(b"a", s) for s in seqs(rng, [1, 3000, 0, 1026, 5])]
    check(torch_gpu, [segment(recs1, recs2, lead1=b"...", lead2=b".")], WHOLE)
    check(torch_gpu, [segment(recs1, recs2, lead1=b"...", lead2=b".")], 1500)


def test_two_segments_of_one_batch(torch_gpu):
    rng = np.random.RandomState(11)
    n, cut = 37 + 100, 37                                    # the second segment lands at a base that is no multiple of 64
    recs1 = [(b"q%d/1" % i, s) for i, s in enumerate(seqs(rng, rng.randint(0, 60, n)))]
    recs2 = [(b"q%d/2" % i if i != 90 else b"other", s) for i, s in enumerate(seqs(rng, rng.randint(0, 300, n)))]
    one = check(torch_gpu, [segment(recs1, recs2)], 28)
    two = check(torch_gpu, [segment(recs1[:cut], recs2[:cut], 0, b".", b"....."), segment(recs1[cut:], recs2[cut:], cut, b"...........", b"..")], 28)
    assert (two.off1, two.off2, two.bytes1, two.bytes2, two.ctl) == (one.off1, one.off2, one.bytes1, one.bytes2, one.ctl) and two.ctl["first_bad"] == 90
    # an empty segment in between changes nothing; an empty first segment opens the batch
    check(torch_gpu, [segment([], [], 0), segment(recs1[:cut], recs2[:cut], 0), segment([], [], cut), segment(recs1[cut:], recs2[cut:], cut)], 28)


def test_rows_outside_their_text_and_outputs_that_are_too_small(torch_gpu):
    rng = np.random.RandomState(13)
    recs1 = [(b"k%d" % i, s) for i, s in enumerate(seqs(rng, [30] * 70))]
    recs2 = [(b"k%d" % i, s) for i, s in enumerate(seqs(rng, [90, 2000] * 35))]
    t1, r1, t2, r2, _ = segment(recs1, recs2)
    r1[66] = (r1[66][0], r1[66][1], r1[66][2], len(t1))               # a sequence that runs beyond the text
    r2[40] = (len(t2) - 1, 2, r2[40][2], r2[40][3])                   # an id that does
    r2[41] = (0xFFFFFFF0, 0x20, r2[41][2], r2[41][3])                 # offset + length beyond 32 bits
    model = check(torch_gpu, [(t1, r1, t2, r2, 0)], 28)
    assert model.ctl["first_outside"] == 40 and model.ctl["first_bad"] == pm.NONE
    t1, r1, t2, r2, _ = segment(recs1, recs2)
    small = check(torch_gpu, [(t1, r1, t2, r2, 0)], 28, cap1=28 * 33 + 5, cap2=90 * 20 + 2000 * 20 - 1)
    assert small.ctl["bytes1"] == 28 * 70 and small.ctl["bytes2"] == 35 * 2090


def test_a_repeat_gives_identical_bytes(torch_gpu):
    rng = np.random.RandomState(17)
    recs1 = [(b"z%d/1" % i, s) for i, s in enumerate(seqs(rng, rng.randint(0, 40, 300)))]
    recs2 = [(b"z%d/2" % i, s) for i, s in enumerate(seqs(rng, list(rng.randint(0, 400, 299)) + [4000]))]
    seg = segment(recs1, recs2, lead1=b".", lead2=b"..")
    n1 = sum(min(q[3], 28) for q in seg[1]) + 5
    n2 = sum(q[3] for q in seg[3]) + 5
    a = gather(torch_gpu, [seg], 28, n1, n2, 301)
    b = gather(torch_gpu, [seg], 28, n1, n2, 301)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    check(torch_gpu, [seg], 28)
