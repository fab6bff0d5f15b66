"""The unstranded stage (csrc/strands.hip over csrc/pair_stage.hpp) at its edges, with no aligner in the loop: the tests write the two candidates' records and arenas by
hand (the Mates helper and the small indexes of tests/test_gpu_pairs_edges.py), so every row of the rule, every list shape and both kernels'
boundaries are chosen exactly. Everything is compared with the model (tests/strands_model.py) by CONTENT (which of reference / arena a
result takes is the implementation's): all integers, equality."""
import numpy as np
import pytest

import helpers
import pairs_model as pm
import strands_model as sm
import test_gpu_pairs_edges as pe

pa = helpers.pa
pytestmark = pytest.mark.gpu

_cache = {}
GUARD, SENTINEL = pe.GUARD, pe.SENTINEL
Mates, _setup, _up, _down = pe.Mates, pe._setup, pe._up, pe._down
# Where the stage hands an item from a lane to a wave is its own business: one list takes EVERY length from 1 to 33 (and 63 .. 65, 128, 129, 1 025),
# the other the lengths below, so any cut on either length or on their sum up to 66 has its value and both neighbours here.
ONE_LENS = pe.SHORT_LENS
OTHER_LENS = pe.LONG_LENS


def _run(which, recS, arS, recR, arR, cap, counts=None, expect_full=False):
    """merge + finish on the GPU -> (results, arena[cap + GUARD], stats, used, need); a full arena is returned as need with stats, not raised"""
    import torch
    host, al, a, T = _setup(which)
    n = len(recS)
    d = [_up(recS), _up(arS), _up(recR), _up(arR)]
    d_res = _up(np.full(4 * (n + 1), 0x5A5A5A5A, np.uint32))
    d_arena = _up(np.full(cap + GUARD, SENTINEL, np.uint32))
    sb = al.strands_scratch_bytes(n)
    d_scr = torch.empty(sb + 256, dtype=torch.uint8, device="cuda")
    scr = (d_scr.data_ptr() + 255) & ~255
    torch.cuda.synchronize()
    al.strands_merge_device(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), n, d_res.data_ptr(), d_arena.data_ptr() if cap else 0, cap,
                            scr, sb, d_counts=counts.data_ptr() if counts is not None else 0)
    try:
        stats, used, need = al.strands_finish(scr)
        assert not expect_full
    except pa.PaError as e:
        assert e.code == pa._ffi.PA_ERR_ARENA_FULL and expect_full, e
        stats, used, need = e.stats, None, e.arena_needed
    res = _down(d_res, np.uint32).reshape(-1, 4)
    assert (res[n:] == 0x5A5A5A5A).all()                       # nothing behind the last record
    arena = _down(d_arena, np.uint32)
    assert (arena[cap:] == SENTINEL).all(), "a word behind arena_cap was written"
    return res[:n].copy().view(pm.RESULT_DTYPE).reshape(-1), arena, stats, used, need


def _want(which, cS, cR):
    a = _setup(which)[2]
    recS, arS = cS.arrays()
    recR, arR = cR.arrays()
    return sm.merge(pm.mates_from_records(recS, arS, a), pm.mates_from_records(recR, arR, a))


def _same(which, res, arena, st, used, want):
    host = _setup(which)[0]
    w_res, w_coff, w_ids, w_st, _ = want
    for f in ("coverage", "mismatches", "class_len"):
        assert np.array_equal(res[f], w_res[f]), (f, np.flatnonzero(res[f] != w_res[f])[:5])
    in_arena = ((res["mismatches"] >> 31) == 1) & (res["class_len"] > 0) & ((res["class_off"] & pm.CLASS_REF) == 0)
    # every result in the arena lies inside the words the launch took: none reaches into a candidate's arena or the junk between its lists
    assert (res["class_off"][in_arena].astype(np.int64) + res["class_len"][in_arena] <= used).all()
    assert (res["class_off"][res["class_len"] == 0] == 0).all()
    coff, ids = pa.gather_classes(res, arena, host)
    assert np.array_equal(coff, w_coff) and np.array_equal(ids, w_ids)
    for k in ("items", "both_mapped", "sense_only", "antisense_only", "neither", "ties"):
        assert st[k] == w_st[k], (k, st, w_st)
    sm.check_stats(st, res)
    assert st["in_arena"] == int(in_arena.sum()) and used >= int(res["class_len"][in_arena].sum())   # (a long result found to be an index class after it was written keeps its arena words)


def _check(which, cS, cR, counts=None, cap=None):
    """one batch against the model; returns the model's tuple and the GPU's records"""
    recS, arS = cS.arrays()
    recR, arR = cR.arrays()
    want = _want(which, cS, cR)
    cap = int(want[1][-1]) + 8 if cap is None else cap
    res, arena, st, used, need = _run(which, recS, arS, recR, arR, cap, counts)
    _same(which, res, arena[:cap], st, used, want)
    return want, res, arena, st, used, need


def _rule_rows(which):
    """every row of the rule, every representation of the candidates; -> (Mates S, Mates R)"""
    host, al, a, T = _setup(which)
    off = a["ec_offset"].astype(np.int64)
    cls = lambda c: a["ec_ids"][off[c]:off[c + 1]].tolist()
    S, R = Mates(a), Mates(a)
    nested, strict, novel, disjoint = pe._class_pairs(a)
    assert nested and novel and disjoint, (nested, strict, novel, disjoint)
    big = int(np.argmax(off[1:] - off[:-1]))
    ids = cls(big)
    assert len(ids) >= 4
    other = [t for t in range(T) if t not in set(ids)][:5]
    # neither / exactly one (by reference, in the arena, empty)
    S.none(); R.none()
    S.ref(big); R.none()
    S.none(); R.ref(big)
    S.ids([0, 3, T - 1]); R.none()
    S.none(); R.ids([1, 2])
    S.ids([]); R.none()
    S.none(); R.ids([])
    both_ways = lambda f, g: (f(S), g(R), g(S), f(R))
    # both mapped, a winner. An empty class loses to a non-empty one whatever the coverage ...
    both_ways(lambda m: m.ids([], 150, 0), lambda m: m.ref(big, 32, 2))
    both_ways(lambda m: m.ids([], 150, 0), lambda m: m.ids([1, 2, 7], 32, 2))
    # ... then coverage decides (the winner by reference, in the arena, equal to an index class in the arena, empty) ...
    both_ways(lambda m: m.ref(big, 150, 2), lambda m: m.ids(other, 32, 0))
    both_ways(lambda m: m.ids([0, 5, T - 1], 150, 2), lambda m: m.ref(big, 32, 0))
    both_ways(lambda m: m.ids(ids, 150, 2), lambda m: m.ids(other, 149, 0))
    both_ways(lambda m: m.ids([], 100, 3), lambda m: m.ids([], 90, 0))
    # ... then fewer mismatches
    both_ways(lambda m: m.ref(big, 100, 1), lambda m: m.ids(other, 100, 2))
    both_ways(lambda m: m.ids(other, 100, 0), lambda m: m.ref(big, 100, 1))
    both_ways(lambda m: m.ids([], 100, 0), lambda m: m.ids([], 100, 1))
    # ties: two empties; the same reference twice; two references (nested, a union that is no class, disjoint)
    S.ids([], 64, 1); R.ids([], 64, 1)
    S.ref(big, 77, 1); R.ref(big, 77, 1)
    for pair in (nested, strict, novel, disjoint):
        if pair:
            both_ways(lambda m: m.ref(pair[0], 80, 0), lambda m: m.ref(pair[1], 80, 0))
    # ties of a reference and a list, of two lists: the class itself, a strict subset, a superset, disjoint
    for mk in (lambda x, y: (S.ref(big, 90, 2), R.ids(y, 90, 2)), lambda x, y: (S.ids(y, 90, 2), R.ref(big, 90, 2)), lambda x, y: (S.ids(x, 90, 2), R.ids(y, 90, 2))):
        mk(ids, ids)
        mk(ids, ids[::2])
        mk(ids, sorted(set(ids) | {0, T - 1}))
        mk(ids, other)
    # a union that equals an index class, from two lists that are none
    S.ids(ids[::2], 70, 0); R.ids(ids[1:], 70, 0)
    S.ids(ids[:1], 70, 0); R.ids(ids[1:], 70, 0)
    # ids 0 and T - 1; identical, disjoint, nested, interleaved lists
    S.ids([0], 50, 2); R.ids([0], 50, 2)
    S.ids([T - 1], 50, 2); R.ids([0], 50, 2)
    S.ids([0, T - 1], 50, 2); R.ids([0, 1, T - 2, T - 1], 50, 2)
    S.ids(range(0, 12), 50, 2); R.ids(range(0, 12), 50, 2)
    S.ids(range(0, 12, 2), 50, 2); R.ids(range(1, 12, 2), 50, 2)
    S.ids(range(2, 8), 50, 2); R.ids(range(0, 12), 50, 2)
    S.ids(range(0, 24, 2), 50, 2); R.ids(range(0, 24, 3), 50, 2)
    return S, R


def _length_rows(which):
    """ties of a list of every length of ONE_LENS with one of every length of OTHER_LENS — disjoint, nested (identical when the lengths are equal),
    interleaved, sharing only the first or only the last id — and a copied winner of every length (needs T >= 2 050)"""
    host, al, a, T = _setup(which)
    rng = np.random.default_rng(6)
    S, R = Mates(a), Mates(a)
    flip = 0
    for la in ONE_LENS:
        for lb in OTHER_LENS:
            pool = rng.permutation(np.arange(1, T - 1))
            A, B = np.sort(pool[:la]), np.sort(pool[la:la + lb])                  # disjoint
            lo, hi = min(la, lb), max(la, lb)
            long_ = np.sort(pool[:hi])
            nested = np.sort(rng.choice(long_, lo, replace=False))               # (lo == hi: identical)
            half = np.sort(np.concatenate([rng.choice(long_, lo // 2, replace=False), pool[hi:hi + lo - lo // 2]]))
            shapes = [(A, B), (nested, long_) if la <= lb else (long_, nested), (half, long_) if la <= lb else (long_, half),
                      (np.concatenate([[0], A[1:]]), np.concatenate([[0], B[1:]])),                          # only the first id shared
                      (np.concatenate([A[:-1], [T - 1]]), np.concatenate([B[:-1], [T - 1]]))]                # only the last
            for x, y in shapes:
                assert len(set(x.tolist())) == la and len(set(y.tolist())) == lb
                (S if flip & 1 == 0 else R).ids(x, 120, 1)
                (R if flip & 1 == 0 else S).ids(y, 120, 1)
                flip += 1
    for l in sorted(set(ONE_LENS + OTHER_LENS)):                                  # the winner's list copied: S wins, then R
        x = np.sort(rng.choice(T, l, replace=False))
        S.ids(x, 140, 0); R.ids(x[::-1][: max(1, l // 2)], 75, 0)
        S.ids([5, 6], 75, 2); R.ids(x, 140, 1)
    # the first and the last id, the last block of 64 partly filled, common ids in every block
    S.ids(range(0, 200), 99, 0); R.ids([0, 63, 64, 127, 128, 199] + list(range(300, 320)), 99, 0)
    S.ids([0] + list(range(100, 130)) + [T - 1], 99, 0); R.ids([0] + list(range(500, 600)) + [T - 1], 99, 0)
    return S, R


def _batch(which):
    if which not in _cache:
        S, R = _rule_rows(which)
        if which == "synth":
            lS, lR = _length_rows(which)
            S, R = pe._join(S, lS), pe._join(R, lR)
        _cache[which] = (S, R, _want(which, S, R))
    return _cache[which]


@pytest.mark.parametrize("which", ["small", "synth"])
def test_rule_rows_and_union_shapes(which):
    S, R, want = _batch(which)
    got, res, arena, st, used, need = _check(which, S, R)
    fates = want[4]
    for f in ("neither", "sense_only", "antisense_only", "sense_wins", "antisense_wins", "tie"):
        assert fates.count(f) >= 1, (f, fates.count(f))
    assert st["by_reference"] > 0 and st["in_arena"] > 0 and need == used
    if which == "synth":   # ties over every length of one list, the copied winners too
        rs, rr = np.array(S.rec), np.array(R.rec)
        tie = np.array([f == "tie" for f in fates])
        assert set(ONE_LENS) <= set(rs[tie, 3].tolist()) | set(rr[tie, 3].tolist())
        assert set(ONE_LENS) <= set(res["class_len"][~tie].tolist())


def test_results_that_equal_an_index_class_are_counted_in_its_slot():
    """a union and a copied winner that equal an index class, short (a lane's) and long (a wave's): the table has them in the class's slot"""
    import torch
    host, al, a, T = _setup("small")
    off = a["ec_offset"].astype(np.int64)
    lens = off[1:] - off[:-1]
    short, long_ = int(np.flatnonzero((lens >= 3) & (lens <= 8))[0]), int(np.argmax(lens))
    assert lens[long_] > 40                     # (a wave's: the cut is at most 33 ids)
    S, R = Mates(a), Mates(a)
    for c in (short, long_):
        ids = a["ec_ids"][off[c]:off[c + 1]].tolist()
        S.ids(ids[::2], 70, 0); R.ids(ids[1:], 70, 0)       # the union is the class
        S.ids(ids, 150, 0); R.ids(ids[:1], 32, 0)            # the winner's copy is
        S.ids([0], 32, 0); R.ids(ids, 150, 0)
    counts = torch.zeros(al.counts_len(), dtype=torch.int64, device="cuda")
    want, res, arena, st, used, need = _check("small", S, R, counts)
    table = counts.cpu().numpy()
    assert table[short] == 3 and table[long_] == 3 and table.sum() == 6
    assert np.array_equal(table, sm.table_and_novel(want[0], want[1], want[2], host)[0])


@pytest.mark.parametrize("n", [0, 1, 64, 65])
def test_small_batches(n):
    S, R, _ = _batch("synth")
    a = _setup("synth")[2]
    lo = 60                                    # behind the trivial rows, so that even n = 1 has a union to make
    s, r = Mates(a), Mates(a)
    s.rec, s.arena, r.rec, r.arena = S.rec[lo:lo + n], S.arena, R.rec[lo:lo + n], R.arena
    want, res, arena, st, used, need = _check("synth", s, r)
    assert n == 0 or want[4][0] == "tie"


def test_more_long_ties_than_the_grid_has_waves():
    """a wave goes round its item loop a second time: the ids common to both lists, and those counted in the chunks done, start from zero for every item"""
    host, al, a, T = _setup("synth")
    n = 5000                                   # the wave kernel's grid is at most 4 blocks of 4 waves per CU: 4 096 waves on 256 CUs
    rng = np.random.default_rng(9)
    S, R = Mates(a), Mates(a)
    for i in range(n):                         # two runs with an overlap that varies in size and in shape (every id, every other id)
        base = int(rng.integers(0, T - 64))
        S.ids(range(base, base + 24 + i % 5))
        R.ids(range(base + 10 + i % 7, base + 50 + i % 3, 1 + i % 2))
    want, res, arena, st, used, need = _check("synth", S, R)
    assert want[4].count("tie") == n and (res["class_len"] > 32).all()    # every union is a wave's, whatever the cut at or below 32
    assert st["ties"] == n and st["in_arena"] + st["by_reference"] == n


def test_arena_full_and_rerun():
    S, R, want = _batch("synth")
    host, al, a, T = _setup("synth")
    recS, arS = S.arrays()
    recR, arR = R.arrays()
    ok_res, ok_arena, ok_st, ok_used, ok_need = _run("synth", recS, arS, recR, arR, int(want[1][-1]) + 8)
    assert ok_used == ok_need and ok_used > 2050
    for cap in (0, ok_need - 1):
        res, arena, st, used, need = _run("synth", recS, arS, recR, arR, cap, expect_full=True)    # (the guard words are checked in _run)
        assert need == ok_need
        listed = ((res["mismatches"] >> 31) == 1) & (res["class_len"] > 0) & ((res["class_off"] & pm.CLASS_REF) == 0)
        lost = listed & (res["class_off"] == pm.UNFIT)
        assert lost.any() and (cap != 0 or lost.sum() == listed.sum())
        kept = listed & ~lost
        assert (res["class_off"][kept].astype(np.int64) + res["class_len"][kept] <= cap).all()
        for f in ("coverage", "mismatches", "class_len"):
            assert np.array_equal(res[f], want[0][f])
        sub = res.copy()                                       # what did fit is right
        sub["class_len"][lost] = 0
        coff, ids = pa.gather_classes(sub, arena[:cap], host)
        w_coff = want[1].astype(np.int64)
        for i in np.flatnonzero(~lost):
            assert np.array_equal(ids[int(coff[i]):int(coff[i + 1])], want[2][w_coff[i]:w_coff[i + 1]]), i
    res2, arena2, st2, used2, need2 = _run("synth", recS, arS, recR, arR, ok_need)                  # the exact capacity
    _same("synth", res2, arena2[:ok_need], st2, used2, want)
    assert used2 == need2 == ok_need
    # two runs are equal by content (offsets may differ: the order of the atomics is free)
    c1, c2 = pa.gather_classes(ok_res, ok_arena[:ok_used], host), pa.gather_classes(res2, arena2[:ok_need], host)
    assert np.array_equal(c1[0], c2[0]) and np.array_equal(c1[1], c2[1]) and st2 == ok_st


@pytest.mark.parametrize("which", ["small", "synth"])
def test_counts_overflow_and_twice(which):
    import torch
    host, al, a, T = _setup(which)
    S, R, want = _batch(which)
    recS, arS = S.arrays()
    recR, arR = R.arrays()
    table, novel = sm.table_and_novel(want[0], want[1], want[2], host)
    nc = a["num_classes"]
    assert table[nc] > 0 and table[nc + 1] > 0 and table[nc + 2] > 0 and (table[:nc] > 0).sum() >= 2 and len(novel) >= 2
    cap = int(want[1][-1]) + 8
    counts = torch.zeros(al.counts_len(), dtype=torch.int64, device="cuda")
    # without an overflow table
    res, arena, st, used, need = _run(which, recS, arS, recR, arR, cap, counts)
    _same(which, res, arena[:cap], st, used, want)
    assert np.array_equal(counts.cpu().numpy(), table)
    # with one attached: the fetched records are the model's, their counts sum to the novel slot; a second launch doubles both
    ovf = pa.Overflow(0, 1 << 13, 1 << 20)
    al.set_overflow(ovf)
    try:
        counts.zero_()
        for times in (1, 2):
            _run(which, recS, arS, recR, arR, cap, counts)
            got = pa.parse_overflow(ovf.fetch())
            assert got == {k: times * v for k, v in novel.items()}
            assert np.array_equal(counts.cpu().numpy(), times * table) and sum(got.values()) == int(counts[nc].item())
    finally:
        al.set_overflow(None)


def test_arguments_are_checked():
    host, al, a, T = _setup("small")
    E = pa._ffi.PA_ERR_INVALID_ARG
    for call in (lambda: al.strands_merge_device(0, 0, 0, 0, 1, 0, 0, 0, 256, 1 << 20),
                 lambda: al.strands_merge_device(0, 0, 0, 0, 0, 0, 0, 0, 0, 1 << 20),
                 lambda: al.strands_finish(0)):
        with pytest.raises(pa.PaError) as e:
            call()
        assert e.value.code == E
