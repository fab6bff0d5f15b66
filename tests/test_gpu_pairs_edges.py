"""The paired-end stage (csrc/pairs.hip over csrc/pair_stage.hpp) at its edges, with no aligner in the loop: the tests write the mates' records and arenas by hand, so
every row of the pair rule, every list shape and both kernels' boundaries are chosen exactly. Everything is compared with the model
(tests/pairs_model.py) by CONTENT (which of reference / arena a result takes is the implementation's): all integers, equality."""
import numpy as np
import pytest

import helpers
import pairs_model as pm

pa = helpers.pa
pytestmark = pytest.mark.gpu

_cache = {}
GUARD = 16
SENTINEL = 0xDEADBEEF
# Where the combine stage hands a pair from a lane to a wave is its own business: the shorter list takes EVERY length from 1 to 33, so any
# cut up to 32 has its length and both neighbours here, next to 63 .. 65, 128, 129 and 1 025 (the blocks of 64 a wave works in).
SHORT_LENS = list(range(1, 34)) + [63, 64, 65, 128, 129, 1025]
LONG_LENS = [1, 15, 16, 17, 31, 32, 33, 64, 65, 1025]


def _setup(which):
    """(host index, aligner, arrays, number of transcripts): "small" = gencode_small at K = 20, "synth" = a synthetic index of >= 2 048 transcripts"""
    if which not in _cache:
        if which == "small":
            host = pa.build_index(str(helpers.FASTA), 20, 8)
        else:
            host = pa.HostIndex.from_txome(pa.Txome.synthesize(650, 2300, 3), 24, 8)
        a = host.arrays()
        assert which == "small" or a["num_transcripts"] >= 2048
        _cache[which] = (host, pa.Pseudoaligner(host), a, int(a["num_transcripts"]))
    return _cache[which]


def _up(a):
    import torch
    a = np.ascontiguousarray(a)
    t = torch.from_numpy(a.view(np.uint8).reshape(-1).copy() if a.size else np.zeros(16, np.uint8)).cuda()
    return t


def _down(t, dtype):
    return t.cpu().numpy().view(dtype).copy()


class Mates:
    """records + arena of one mate of every pair, written by hand"""

    def __init__(self, arrays):
        self.a = arrays
        self.rec, self.arena = [], [0xABCD0000 + j for j in range(3)]   # (offset 0 is not special: lists start behind three words of junk)

    def none(self):
        self.rec.append((0, 0, 0, 0))

    def ref(self, c, cov=40, mm=1):
        off = self.a["ec_offset"]
        self.rec.append((cov, mm | pm.MAPPED_BIT, pm.CLASS_REF | c, int(off[c + 1] - off[c])))

    def ids(self, ids, cov=50, mm=2):
        ids = sorted(set(int(x) for x in ids))
        self.rec.append((cov, mm | pm.MAPPED_BIT, len(self.arena) if ids else 0, len(ids)))
        self.arena += ids + [0xEEEE0000]   # (a word of junk between the lists)

    def arrays(self):
        return np.array(self.rec, pm.RESULT_DTYPE).reshape(-1) if self.rec else np.zeros(0, pm.RESULT_DTYPE), np.array(self.arena, np.uint32)


def _run(which, rec1, ar1, rec2, ar2, cap, counts=None, expect_full=False):
    """combine + finish on the GPU -> (results, arena[cap + GUARD], stats, used, need); a full arena is returned as need with stats, not raised"""
    import torch
    host, al, a, T = _setup(which)
    n = len(rec1)
    d = [_up(rec1), _up(ar1), _up(rec2), _up(ar2)]
    d_res = _up(np.full(4 * (n + 1), 0x5A5A5A5A, np.uint32))
    d_arena = _up(np.full(cap + GUARD, SENTINEL, np.uint32))
    sb = al.pairs_scratch_bytes(n)
    d_scr = torch.empty(sb + 256, dtype=torch.uint8, device="cuda")
    scr = (d_scr.data_ptr() + 255) & ~255
    torch.cuda.synchronize()
    al.pairs_combine_device(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), n, d_res.data_ptr(), d_arena.data_ptr() if cap else 0, cap,
                            scr, sb, d_counts=counts.data_ptr() if counts is not None else 0)
    try:
        stats, used, need = al.pairs_finish(scr)
        assert not expect_full
    except pa.PaError as e:
        assert e.code == pa._ffi.PA_ERR_ARENA_FULL and expect_full, e
        stats, used, need = e.stats, None, e.arena_needed
    res = _down(d_res, np.uint32).reshape(-1, 4)
    assert (res[n:] == 0x5A5A5A5A).all()                       # nothing behind the last record
    arena = _down(d_arena, np.uint32)
    assert (arena[cap:] == SENTINEL).all(), "a word behind arena_cap was written"
    return res[:n].copy().view(pm.RESULT_DTYPE).reshape(-1), arena, stats, used, need


def _check(which, m1, m2, counts=None, cap=None):
    """one batch against the model; returns the model's (results, coff, ids, stats) and the GPU's records"""
    host, al, a, T = _setup(which)
    rec1, ar1 = m1.arrays()
    rec2, ar2 = m2.arrays()
    want = pm.combine(pm.mates_from_records(rec1, ar1, a), pm.mates_from_records(rec2, ar2, a))
    w_res, w_coff, w_ids, w_st = want
    cap = int(w_coff[-1]) + 8 if cap is None else cap
    res, arena, st, used, need = _run(which, rec1, ar1, rec2, ar2, cap, counts)
    _same(which, res, arena[:cap], st, used, want)
    return want, res, arena, st, used, need


def _same(which, res, arena, st, used, want):
    host, al, a, T = _setup(which)
    w_res, w_coff, w_ids, w_st = want
    for f in ("coverage", "mismatches", "class_len"):
        assert np.array_equal(res[f], w_res[f]), (f, np.flatnonzero(res[f] != w_res[f])[:5])
    in_arena = ((res["mismatches"] >> 31) == 1) & (res["class_len"] > 0) & ((res["class_off"] & pm.CLASS_REF) == 0)
    assert (res["class_off"][in_arena].astype(np.int64) + res["class_len"][in_arena] <= used).all()   # (a lost record's offset is 2^31 - 1: beyond any `used`)
    unmapped_or_empty = res["class_len"] == 0
    assert (res["class_off"][unmapped_or_empty] == 0).all()
    coff, ids = pa.gather_classes(res, arena, host)
    assert np.array_equal(coff, w_coff) and np.array_equal(ids, w_ids)
    for k in ("pairs", "both_mapped", "mate1_only", "mate2_only", "neither", "both_mapped_empty"):
        assert st[k] == w_st[k], (k, st, w_st)
    pm.check_stats(st, res)
    assert st["in_arena"] == int(in_arena.sum()) and used >= int(res["class_len"][in_arena].sum())   # (a long result found to be an index class after it was written keeps its arena words)


# ---------------------------------------------------------------------------------------------- reverse complement
RC_LENS = [1, 2, 31, 32, 33, 63, 64, 65, 95, 96, 97, 150, 1000, 70000]


def test_revcomp_tiles():
    import torch
    host, al, a, T = _setup("small")
    rng = np.random.default_rng(7)
    n = 70                                                            # one full tile plus six reads
    lens = np.array([RC_LENS[i % len(RC_LENS)] for i in range(n)], np.uint32)
    lens[69] = 70000                                                  # the long one also in the ragged tile
    wpr = (int(lens.max()) + 31) // 32
    codes = [rng.integers(0, 4, int(l)).astype(np.uint8) for l in lens]
    tiles = rng.integers(0, 1 << 63, 2 * wpr * 64, dtype=np.uint64) | (rng.integers(0, 2, 2 * wpr * 64, dtype=np.uint64) << np.uint64(63))   # garbage everywhere ...
    t3 = tiles.reshape(2, wpr, 64)
    for i in range(n):                                                # ... the reads' bases written into it, the bits beyond a read's length left as garbage
        w = helpers.pack_bases(codes[i])[: (int(lens[i]) + 31) // 32]
        keep = np.full(len(w), 0xFFFFFFFFFFFFFFFF, np.uint64)
        if lens[i] & 31:
            keep[-1] = np.uint64((1 << (2 * int(lens[i] & 31))) - 1)
        col = t3[i >> 6, : len(w), i & 63]
        t3[i >> 6, : len(w), i & 63] = (col & ~keep) | (w & keep)
    words = len(tiles)
    d_in, d_lens = _up(tiles), _up(lens)
    d_out = _up(np.full(words + 1, 0x1234567812345678, np.uint64))
    d_back = _up(np.full(words + 1, 0x1234567812345678, np.uint64))
    torch.cuda.synchronize()
    al.revcomp_tiles_device(d_in.data_ptr(), d_lens.data_ptr(), n, wpr, d_out.data_ptr())
    al.revcomp_tiles_device(d_out.data_ptr(), d_lens.data_ptr(), n, wpr, d_back.data_ptr())
    al.revcomp_tiles_device(0, 0, 0, wpr, 0)                          # n = 0: a no-op, whatever the pointers
    torch.cuda.synchronize()
    out, back = _down(d_out, np.uint64), _down(d_back, np.uint64)
    assert out[words] == 0x1234567812345678 and back[words] == 0x1234567812345678   # the word behind the buffer
    got, clean = pm.tile_bases(out[:words], lens, wpr)
    assert clean, "bits beyond a read's length are not zero"
    for i in range(n):
        assert np.array_equal(got[i], pm.revcomp_codes(codes[i])), (i, int(lens[i]))
    assert np.array_equal(out[:words], pm.revcomp_tiles(tiles, lens, wpr))          # (the slots of reads 70..127 included: zero)
    got2, clean2 = pm.tile_bases(back[:words], lens, wpr)
    assert clean2 and all(np.array_equal(x, y) for x, y in zip(got2, codes))
    with pytest.raises(pa.PaError) as e:
        al.revcomp_tiles_device(d_in.data_ptr(), d_lens.data_ptr(), n, wpr, d_in.data_ptr())
    assert e.value.code == pa._ffi.PA_ERR_INVALID_ARG


# ---------------------------------------------------------------------------------------------- combine
def _class_pairs(a):
    """index classes for ref x ref: (same, nested -> an index class, strict subset of both that is an index class or None, novel, disjoint)"""
    off = a["ec_offset"].astype(np.int64)
    nc = a["num_classes"]
    sets = [frozenset(a["ec_ids"][off[c]:off[c + 1]].tolist()) for c in range(nc)]
    known = {s: c for c, s in enumerate(sets)}
    nested = strict = novel = disjoint = None
    order = sorted(range(nc), key=lambda c: -len(sets[c]))[:120]
    for x in order:
        for y in order:
            if x >= y:
                continue
            i = sets[x] & sets[y]
            if not i:
                disjoint = disjoint or (x, y)
            elif i == sets[x] or i == sets[y]:
                nested = nested or (x, y)
            elif i in known:
                strict = strict or (x, y)
            else:
                novel = novel or (x, y)
    return nested, strict, novel, disjoint


def _rule_rows(which):
    """every row of the rule table, every representation of the mates, the list shapes; -> (Mates 1, Mates 2)"""
    host, al, a, T = _setup(which)
    off = a["ec_offset"].astype(np.int64)
    cls = lambda c: a["ec_ids"][off[c]:off[c + 1]].tolist()
    m1, m2 = Mates(a), Mates(a)
    nested, strict, novel, disjoint = _class_pairs(a)
    assert nested and novel and disjoint, (nested, strict, novel, disjoint)
    big = int(np.argmax(off[1:] - off[:-1]))
    # neither / exactly one (by reference, in the arena, empty) / both with an empty mate
    m1.none(); m2.none()
    m1.ref(big); m2.none()
    m1.none(); m2.ref(big)
    m1.ids([0, 3, T - 1]); m2.none()
    m1.none(); m2.ids([1, 2])
    m1.ids([]); m2.none()
    m1.none(); m2.ids([])
    m1.ids([]); m2.ref(big)
    m1.ref(big); m2.ids([])
    m1.ids([]); m2.ids([])
    # reference x reference
    m1.ref(big, 33, 0); m2.ref(big, 44, 2)
    for pair in (nested, strict, novel, disjoint):
        if pair:
            m1.ref(pair[0]); m2.ref(pair[1])
            m1.ref(pair[1]); m2.ref(pair[0])
    # reference x arena, arena x reference, arena x arena: the class itself, a strict subset, a superset, disjoint
    ids = cls(big)
    for mk in (lambda x, y: (m1.ref(big), m2.ids(y)), lambda x, y: (m1.ids(y), m2.ref(big)), lambda x, y: (m1.ids(x), m2.ids(y))):
        mk(ids, ids)
        mk(ids, ids[::2])
        mk(ids, sorted(set(ids) | {0, T - 1}))
        mk(ids, [t for t in range(T) if t not in set(ids)][:5])
    # ids 0 and T - 1; identical, disjoint, nested, interleaved lists
    m1.ids([0]); m2.ids([0])
    m1.ids([T - 1]); m2.ids([T - 1])
    m1.ids([0, T - 1]); m2.ids([0, 1, T - 2, T - 1])
    m1.ids(range(0, 12)); m2.ids(range(0, 12))
    m1.ids(range(0, 12, 2)); m2.ids(range(1, 12, 2))
    m1.ids(range(2, 8)); m2.ids(range(0, 12))
    m1.ids(range(0, 24, 2)); m2.ids(range(0, 24, 3))
    return m1, m2


def _length_rows(which):
    """every list length of SHORT_LENS against every one of LONG_LENS (1 and 1 025 among them) — identical, nested, interleaved and disjoint for every
    combination (needs T >= 2 048)"""
    host, al, a, T = _setup(which)
    rng = np.random.default_rng(5)
    m1, m2 = Mates(a), Mates(a)
    for la in SHORT_LENS:
        for lb in LONG_LENS:
            lo, hi = min(la, lb), max(la, lb)
            long_ = np.sort(rng.choice(T, hi, replace=False))
            nested = np.sort(rng.choice(long_, lo, replace=False))
            half = np.sort(np.concatenate([rng.choice(long_, lo // 2, replace=False), rng.choice(np.setdiff1d(np.arange(T), long_), lo - lo // 2, replace=False)]))
            apart = np.sort(rng.choice(np.setdiff1d(np.arange(T), long_), lo, replace=False))
            for short in (nested, half, apart):
                x, y = (short, long_) if la <= lb else (long_, short)
                m1.ids(x); m2.ids(y)
            if la == lb:
                m1.ids(long_); m2.ids(long_)
    # the first and the last id, the last block of 64 partly filled, a survivor in every block
    m1.ids(range(0, 200)); m2.ids([0, 63, 64, 127, 128, 199] + list(range(300, 320)))
    m1.ids([0] + list(range(100, 130)) + [T - 1]); m2.ids([0] + list(range(500, 600)) + [T - 1])
    return m1, m2


def _join(x, y):
    """two Mates of one index, back to back"""
    out = Mates(x.a)
    out.rec, out.arena = list(x.rec), list(x.arena)
    base = len(out.arena)
    for cov, mm, off, ln in y.rec:
        out.rec.append((cov, mm, off if (off & pm.CLASS_REF) or ln == 0 else off + base, ln))
    out.arena += y.arena
    return out


def _batch(which):
    if ("batch", which) not in _cache:
        m1, m2 = _rule_rows(which)
        if which == "synth":
            l1, l2 = _length_rows(which)
            m1, m2 = _join(m1, l1), _join(m2, l2)
        _cache[("batch", which)] = (m1, m2)
    return _cache[("batch", which)]


@pytest.mark.parametrize("which", ["small", "synth"])
def test_rule_table_and_list_shapes(which):
    m1, m2 = _batch(which)
    want, res, arena, st, used, need = _check(which, m1, m2)
    w_res, w_coff, w_ids, w_st = want
    assert w_st["both_mapped_empty"] > 0 and w_st["neither"] > 0 and w_st["mate1_only"] > 0 and w_st["mate2_only"] > 0
    assert st["by_reference"] > 0 and st["in_arena"] > 0 and need == used
    if which == "synth":   # the shorter list of a pair with two lists takes every length up to 33, and 1 025
        r1, r2 = np.array(m1.rec), np.array(m2.rec)
        two = ((r1[:, 1] >> 31) & (r2[:, 1] >> 31)).astype(bool)
        short = np.minimum(r1[:, 3], r2[:, 3])[two]
        assert set(range(1, 34)) | {64, 65, 1025} <= set(short.tolist())


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65])
def test_small_batches(n):
    m1, m2 = _batch("synth")
    a = _setup("synth")[2]
    # the n pairs behind the trivial rows, so that even n = 1 has a list to intersect
    lo = 30
    s1, s2 = Mates(a), Mates(a)
    s1.rec, s1.arena, s2.rec, s2.arena = m1.rec[lo:lo + n], m1.arena, m2.rec[lo:lo + n], m2.arena
    _check("synth", s1, s2)


def test_more_long_pairs_than_the_grid_has_waves():
    host, al, a, T = _setup("synth")
    n = 5000                                   # the wave kernel's grid is at most 4 blocks of 4 waves per CU: 4 096 waves on 256 CUs
    rng = np.random.default_rng(9)
    m1, m2 = Mates(a), Mates(a)
    for i in range(n):
        base = int(rng.integers(0, T - 64))
        m1.ids(range(base, base + 17 + i % 5))
        m2.ids(range(base + i % 7, base + 30 + i % 3, 1 + i % 2))
    want, res, arena, st, used, need = _check("synth", m1, m2)
    assert st["in_arena"] + st["by_reference"] + st["both_mapped_empty"] == n


def test_arena_full_and_rerun():
    m1, m2 = _batch("synth")
    host, al, a, T = _setup("synth")
    rec1, ar1 = m1.arrays()
    rec2, ar2 = m2.arrays()
    want = pm.combine(pm.mates_from_records(rec1, ar1, a), pm.mates_from_records(rec2, ar2, a))
    ok_res, ok_arena, ok_st, ok_used, ok_need = _run("synth", rec1, ar1, rec2, ar2, int(want[1][-1]) + 8)
    assert ok_used == ok_need and ok_used > 1025
    for cap in (0, ok_need - 1):
        res, arena, st, used, need = _run("synth", rec1, ar1, rec2, ar2, cap, expect_full=True)    # (the guard words are checked in _run)
        assert need == ok_need
        listed = ((res["mismatches"] >> 31) == 1) & (res["class_len"] > 0) & ((res["class_off"] & pm.CLASS_REF) == 0)
        lost = listed & (res["class_off"] == pm.UNFIT)
        assert lost.any() and (cap != 0 or lost.sum() == listed.sum())
        kept = listed & ~lost
        assert (res["class_off"][kept].astype(np.int64) + res["class_len"][kept] <= cap).all()
        for f in ("coverage", "mismatches", "class_len"):
            assert np.array_equal(res[f], want[0][f])
        # what did fit is right
        sub = res.copy()
        sub["class_len"][lost] = 0
        coff, ids = pa.gather_classes(sub, arena[:cap], host)
        w_coff = want[1].astype(np.int64)
        for i in np.flatnonzero(~lost):
            assert np.array_equal(ids[int(coff[i]):int(coff[i + 1])], want[2][w_coff[i]:w_coff[i + 1]]), i
        res2, arena2, st2, used2, need2 = _run("synth", rec1, ar1, rec2, ar2, need)                # re-run with arena_needed
        _same("synth", res2, arena2[:need], st2, used2, want)


@pytest.mark.parametrize("which", ["small", "synth"])
def test_counts_overflow_and_twice(which):
    import torch
    host, al, a, T = _setup(which)
    m1, m2 = _batch(which)
    rec1, ar1 = m1.arrays()
    rec2, ar2 = m2.arrays()
    want = pm.combine(pm.mates_from_records(rec1, ar1, a), pm.mates_from_records(rec2, ar2, a))
    table, novel = pm.table_and_novel(want[0], want[1], want[2], host)
    nc = a["num_classes"]
    assert table[nc] > 0 and table[nc + 1] > 0 and table[nc + 2] > 0 and (table[:nc] > 0).sum() >= 2 and len(novel) >= 2
    cap = int(want[1][-1]) + 8
    counts = torch.zeros(al.counts_len(), dtype=torch.int64, device="cuda")
    # without an overflow table
    res, arena, st, used, need = _run(which, rec1, ar1, rec2, ar2, cap, counts)
    _same(which, res, arena[:cap], st, used, want)
    assert np.array_equal(counts.cpu().numpy(), table)
    # with one attached: the fetched records are the model's, their counts sum to the novel slot; a second launch doubles both
    ovf = pa.Overflow(0, 1 << 12, 1 << 18)
    al.set_overflow(ovf)
    try:
        counts.zero_()
        for times in (1, 2):
            _run(which, rec1, ar1, rec2, ar2, cap, counts)
            got = pa.parse_overflow(ovf.fetch())
            assert got == {k: times * v for k, v in novel.items()}
            assert np.array_equal(counts.cpu().numpy(), times * table) and sum(got.values()) == int(counts[nc].item())
    finally:
        al.set_overflow(None)


def test_arguments_are_checked():
    host, al, a, T = _setup("small")
    E = pa._ffi.PA_ERR_INVALID_ARG
    for call in (lambda: al.pairs_combine_device(0, 0, 0, 0, 1, 0, 0, 0, 256, 1 << 20),
                 lambda: al.pairs_combine_device(0, 0, 0, 0, 0, 0, 0, 0, 0, 1 << 20),
                 lambda: al.pairs_finish(0)):
        with pytest.raises(pa.PaError) as e:
            call()
        assert e.value.code == E
