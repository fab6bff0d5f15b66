"""pa_resolve_kernel (csrc/resolve.hip) on DESIGNED deferred-entry streams, driven through tests/resolve/resolve_probe.hip: one validated
launch_resolve on host arrays, every output pre-filled and guarded. The index is designed with tests/resolve_model.py (one isolated unitig
per class; window classes that fill a line of the window table and spill into the next, once through line 0; window-less classes that share
a slot of the class-list table, once through slot 0) and the read-back of both tables proves that the design reached them. Every comparison
is exact, against the model: records, arena words, arena_top, count keys by position, colours, the novel slot, the novel list, guards. A HIP
error ends the session: nothing more is started on a GPU that may have faulted.

What only the atomics' order decides — which slice of the arena a wave gets — is measured, not modelled: all entries of one take must agree
on its base, the slices must be pairwise disjoint and lie in [top0, arena_top)."""
import ctypes as C
from collections import Counter

import numpy as np
import pytest

import helpers
import resolve_model as rm

pytestmark = pytest.mark.gpu
pa = helpers.pa
ERR_HIP, ERR_INVALID = -5, -1   # PA_ERR_HIP, PA_ERR_INVALID_ARG of include/pseudoaligner_amd.h
NO_KEYS, NO_COLOUR, NO_NOVEL = 1, 2, 4
SWEEP = 4096                     # entries one sweep of a grid of 4 blocks covers


def ok(rc, what):
    """a pa_status of the probe: a HIP error ends the session, any other failure is a PaError with the library's message"""
    if rc == ERR_HIP:
        pytest.exit("resolve, %s: %s" % (what, (pa.lib().pa_last_error() or b"").decode("utf-8", "replace")), returncode=3)
    pa._ffi.check(rc)


class Ctx:
    pass


@pytest.fixture(scope="module")
def X():
    if pa.lib().pa_device_count() < 1:
        raise RuntimeError("the gpu tier needs a GPU")
    x = Ctx()
    x.L = helpers.resolve_lib()
    x.host = helpers.index_from_node_set(rm.design_nodes(), 20, rm.NUM_TX, seed=5)
    x.aligner = pa.Pseudoaligner(x.host, 0)
    a = x.host.arrays()
    off = a["ec_offset"].astype(np.int64)
    x.classes = [tuple(int(i) for i in a["ec_ids"][off[c]:off[c + 1]]) for c in range(int(a["num_classes"]))]
    x.class_of = {ids: c for c, ids in enumerate(x.classes)}
    x.nc = len(x.classes)
    x.f = rm.table_features(x.classes)
    x.FILL, x.FILL64, x.GUARD = x.L.rsp_fill(), x.L.rsp_fill64(), x.L.rsp_guard()
    wb, size, nc, cus = C.c_uint32(), C.c_uint64(), C.c_uint32(), C.c_int()
    ok(x.L.rsp_tables(x.aligner._h, C.byref(wb), C.byref(size), C.byref(nc), C.byref(cus), None, None), "tables")
    x.wtable, x.ctable = np.zeros((wb.value, 16), np.uint32), np.zeros(size.value, np.uint32)
    ok(x.L.rsp_tables(x.aligner._h, None, None, None, None, x.wtable.ctypes.data, x.ctable.ctypes.data), "tables")
    x.device_nc, x.num_cus = nc.value, cus.value
    assert x.L.rsp_arena_chunk() == rm.ARENA_CHUNK
    x.pool = Pool(x)
    return x


# ------------------------------------------------------------------------------------------------ the designed entries
class Pool:
    """every designed entry once, without rid: (words 3 .. 7, labels). List entries point into `arena` (ids between pre-fill words)."""

    def __init__(self, x):
        self.items, words = [], [x.FILL] * 3
        windowed = [c for c in range(x.nc) if c in x.f["lines"]]
        shapes = {ids for pair in rm.SHAPES.values() for ids in pair}
        for c in windowed:                                                       # window entries equal to an index class
            ps = rm.presentations(x.classes[c])
            for w, kinds in (ps if x.classes[c] in shapes or c in x.f["spilled"] else ps[:6]):
                self.add_window(w, ["class"] + kinds)
        novels = list(rm.NOVEL_SETS.values())
        novels += [(400, 403), (400, 403, 410, 412), (420, 425, 460), (540, 572), (600, 610, 663, 664), (0, 40), (rm.NUM_TX - 41, rm.NUM_TX - 1), (0,), (rm.NUM_TX - 1,),
                   (740, 748, 765, 781), (1300, 1331), (500, 507, 531, 532), (500, 507, 532)]
        full_lines = {home for home, line, pos in x.f["lines"].values() if line != home}
        for line in sorted(full_lines):                                          # novel sets at home in a full line: the walk passes the following lines too
            novels.append(next((a, a + d) for a in range(40, 1300) for d in range(1, 32) if rm.home_line(rm.windows_of((a, a + d)), x.f["wbuckets"]) == line and (a, a + d) not in x.class_of))
        assert not any(s in x.class_of for s in novels)
        for s in novels:
            for w, kinds in rm.presentations(s):
                self.add_window(w, ["novel"] + kinds)
        lists = [(x.classes[c], "list_windowless_class") for c in x.f["windowless"]] + [(x.classes[c], "list_windowed_class") for c in windowed[::3]]
        big = x.classes[max(x.f["windowless"], key=lambda c: len(x.classes[c]))]
        lists += [(big[:-1], "list_prefix"), (big + (rm.NUM_TX - 2,), "list_plus_one"), ((5, 100), "list_prefix"), ((5, 100, 300, 302), "list_plus_one"),
                  (rm.NOVEL_SETS[2], "list_novel"), (big[1:], "list_novel")]
        for ids, kind in lists:
            assert (ids in x.class_of) == kind.endswith("class")
            self.items.append(([rm.DEFER_LIST | len(ids), len(words), 0xDEAD0001, 0xDEAD0002, 0xDEAD0003], [kind]))
            words += list(ids) + [x.FILL]
        self.arena = np.array(words, np.uint32)
        self.kinds = Counter(k for _, ks in self.items for k in ks)

    def add_window(self, w, kinds):
        b1, m1, b2, m2 = w
        self.items.append(([rm.DEFER_WINDOW | (bin(m1).count("1") + bin(m2).count("1")), b1, m1, b2 & 0xFFFFFFFF, m2], kinds))

    def stream(self, n, first=0, pad=(), seed=1, step=1):
        """n entries: every `step`-th item of the pool from item `first` on, cyclically, padding at the positions `pad`; rids a seeded permutation of [0, n + 7)"""
        rids = np.random.RandomState(seed).permutation(n + 7)[:n]
        E = np.zeros((n, 8), np.uint32)
        for i in range(n):
            E[i] = [rids[i], 30 + i % 200, i % 4] + self.items[(first + step * i) % len(self.items)][0]
        for i in pad:
            E[i] = rm.PAD_ENTRY
        return E


def novel_windows(n, counts, seed=2, base=1000):
    """n entries, padding but for the positions of `counts` ({position: ids}): canonical window entries of base .. base + ids - 1 (no class:
    NOVEL_SETS' ranges). rids a permutation."""
    rids = np.random.RandomState(seed).permutation(n + 7)[:n]
    E = np.tile(np.array(rm.PAD_ENTRY, np.uint32), (n, 1))
    for i, c in counts.items():
        E[i] = rm.window_entry(int(rids[i]), 40 + i % 100, i % 3, *rm.windows_of(tuple(range(base, base + c))))
    return E


# ------------------------------------------------------------------------------------------------ one launch and its checks
def launch(x, E, arena=None, top0=None, arena_cap=None, defer_top=None, defer_cap=None, keys_top=5, keys_cap=None, novel_cap=None, novel_ctr0=3, num_cus=1,
           flags=0, n_results=None, checked=True):
    E = np.ascontiguousarray(E, np.uint32).reshape(-1, 8)
    arena = x.pool.arena if arena is None else np.ascontiguousarray(arena, np.uint32)
    r = Ctx()
    r.E, r.arena_in, r.flags, r.num_cus, r.novel_ctr0 = E, arena, flags, num_cus, novel_ctr0
    r.top0 = len(arena) if top0 is None else top0
    r.defer_top = len(E) if defer_top is None else defer_top
    r.defer_cap = len(E) if defer_cap is None else defer_cap
    r.n = min(r.defer_top, r.defer_cap)
    r.keys_top, r.keys_cap = keys_top, keys_top + 11 if keys_cap is None else keys_cap
    r.n_results = len(E) + 7 if n_results is None else n_results
    r.x = rm.expect(E, arena, x.class_of, r.n, num_cus) if checked else dict(used=rm.ARENA_CHUNK, novel=[True] * len(E))   # (unchecked: a launch the probe must refuse)
    r.arena_cap = r.top0 + r.x["used"] + 9 if arena_cap is None else arena_cap
    r.novel_cap = sum(r.x["novel"]) + 5 + novel_ctr0 if novel_cap is None else novel_cap
    r.arena_n, r.keys_n = max(len(arena), r.arena_cap), r.keys_cap + r.defer_cap
    G = x.GUARD
    r.results, r.arena, r.keys = np.zeros(4 * r.n_results + G, np.uint32), np.zeros(r.arena_n + G, np.uint32), np.zeros(r.keys_n + G, np.uint32)
    r.colour, r.counts, r.novel, r.ctl = np.zeros(r.n_results + G, np.uint32), np.zeros(x.nc + 3 + G, np.uint64), np.zeros(2 * r.novel_cap + G, np.uint32), np.zeros(4, np.uint64)
    rc = x.L.rsp_resolve(x.aligner._h, E.ctypes.data, len(E), r.defer_top, r.defer_cap, arena.ctypes.data, len(arena), r.top0, r.arena_cap, r.n_results, r.keys_top,
                         r.keys_cap, r.novel_cap, novel_ctr0, num_cus, flags, rm.NUM_TX, r.results.ctypes.data, r.arena.ctypes.data, r.keys.ctypes.data,
                         r.colour.ctypes.data, r.counts.ctypes.data, r.novel.ctypes.data, r.ctl.ctypes.data)
    if not checked:
        return rc
    ok(rc, "launch")
    r.arena_top, r.status, r.novel_ctr, r.novel_status = (int(v) for v in r.ctl)
    return r


def same(got, want, what):
    bad = np.flatnonzero(got != want)
    assert len(bad) == 0, "%s: %d words differ; first at %d: got %#x, want %#x" % (what, len(bad), bad[0], int(got[bad[0]]), int(want[bad[0]]))


def check(x, r):
    """everything a launch must leave behind, exactly; -> the positions of the window entries that lost their ids to a full arena"""
    m, E, n, FILL = r.x, r.E, r.n, x.FILL
    assert x.device_nc == x.nc
    assert r.arena_top == r.top0 + m["used"], "arena_top %d, the model's takes end at %d" % (r.arena_top, r.top0 + m["used"])
    rid = E[:n, 0].astype(np.int64)
    colour, novel, window = np.array(m["colour"], np.uint32).reshape(-1), np.array(m["novel"], bool).reshape(-1), m["window"]
    placed = np.flatnonzero(m["slice_of"] >= 0)                      # the novel window entries
    assert np.array_equal(placed, np.flatnonzero(window & novel))
    off = r.results.reshape(-1, 4)[rid[placed], 2].astype(np.int64) if len(placed) else np.zeros(0, np.int64)
    # slices: one base per take, inside [top0, arena_top), pairwise disjoint
    base = off - m["rel"][placed]
    bases = {}
    for k, b in zip(m["slice_of"][placed].tolist(), base.tolist()):
        assert bases.setdefault(k, b) == b, "two entries of take %d disagree on its base: %d, %d" % (k, bases[k], b)
    assert len(bases) == len(m["slices"])
    spans = sorted((b, b + m["slices"][k]["take"]) for k, b in bases.items())
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])) and (not spans or (spans[0][0] >= r.top0 and spans[-1][1] <= r.arena_top)), spans[:4]
    cnt = m["count"][placed]
    lost = off + cnt > r.arena_cap
    # records
    want = np.full(4 * r.n_results + x.GUARD, FILL, np.uint32)
    w4 = want[:4 * r.n_results].reshape(-1, 4)
    wi = np.flatnonzero(window)
    w4[rid[wi], 0], w4[rid[wi], 1], w4[rid[wi], 3] = E[wi, 1], E[wi, 2] | rm.MAPPED_BIT, m["count"][wi]
    w4[rid[wi], 2] = rm.CLASS_REF | colour[wi]
    w4[rid[placed], 2] = off
    same(r.results, want, "results")
    # arena: the ids of the entries that were not lost, ascending, and not one other word
    want = np.full(r.arena_n + x.GUARD, FILL, np.uint32)
    want[:len(r.arena_in)] = r.arena_in
    for i, o in zip(placed[~lost].tolist(), off[~lost].tolist()):
        want[o:o + len(m["ids"][i])] = m["ids"][i]
    same(r.arena, want, "arena")
    assert r.status == (rm.STATUS_ARENA_FULL if lost.any() else 0)
    # keys by position, colours by rid, the novel slot
    counting = not r.flags & NO_KEYS
    want = np.full(r.keys_n + x.GUARD, FILL, np.uint32)
    if counting:
        kt = min(r.keys_top, r.keys_cap)
        want[kt:kt + n] = np.array(m["keys"], np.uint32).reshape(-1)
    same(r.keys, want, "keys")
    want = np.full(r.n_results + x.GUARD, FILL, np.uint32)
    if not r.flags & NO_COLOUR:
        live = np.flatnonzero(E[:n, 0] != rm.PAD_RID)
        want[rid[live]] = colour[live]
    same(r.colour, want, "colours")
    want = x.FILL64 + np.arange(x.nc + 3 + x.GUARD, dtype=np.uint64)
    if counting:
        want[x.nc] += np.uint64(int(novel.sum()))
    same(r.counts, want, "counts")
    # the novel list: {arena offset, count} of every novel entry that has its ids in the arena
    want = np.full(2 * r.novel_cap + x.GUARD, FILL, np.uint32)
    if r.flags & NO_NOVEL:
        same(r.novel, want, "novel list")
        assert r.novel_ctr == r.novel_ctr0 and r.novel_status == 0
    else:
        lost_at = set(placed[lost].tolist())
        listed = [i for i in np.flatnonzero(novel).tolist() if i not in lost_at]
        where = dict(zip(placed.tolist(), off.tolist()))
        pairs = Counter((where[i] if window[i] else int(E[i, 4]), len(m["ids"][i])) for i in listed)
        assert r.novel_ctr == r.novel_ctr0 + len(listed)
        lo, hi = min(r.novel_ctr0, r.novel_cap), min(r.novel_ctr, r.novel_cap)
        got = Counter(map(tuple, r.novel[2 * lo:2 * hi].reshape(-1, 2).tolist()))
        assert not got - pairs, "listed pairs that are no novel entry: %r" % sorted((got - pairs).items())[:4]
        assert hi < r.novel_ctr or got == pairs
        content = Counter(tuple(int(v) for v in r.arena[o:o + c]) for o, c in got.elements())
        assert not content - Counter(m["ids"][i] for i in listed) and (hi < r.novel_ctr or content == Counter(m["ids"][i] for i in listed))
        same(r.novel[:2 * lo], want[:2 * lo], "novel list below the counter")
        same(r.novel[2 * hi:], want[2 * hi:], "novel list behind what was listed")
        assert r.novel_status == (rm.NOVEL_LIST_FULL if r.novel_ctr > r.novel_cap else 0)
    r.lost = placed[lost].tolist()
    return r.lost


def normal(x, r):
    """the outputs of a launch with the slice bases taken out: records with the ids in place of an arena offset, the novel list as a Counter"""
    rec = {}
    for i in range(r.n):
        if r.x["window"][i]:
            c, o, k = (int(v) for v in r.results.reshape(-1, 4)[int(r.E[i, 0])][[0, 2, 3]])
            rec[i] = (c, o if o & rm.CLASS_REF else tuple(r.arena[o:o + k].tolist()), k)
    lo, hi = min(r.novel_ctr0, r.novel_cap), min(r.novel_ctr, r.novel_cap)
    listed = Counter(tuple(r.arena[o:o + c].tolist()) for o, c in r.novel[2 * lo:2 * hi].reshape(-1, 2).tolist())
    return rec, listed, r.keys.tolist(), r.colour.tolist(), r.counts.tolist(), r.arena_top, r.status, r.novel_ctr, r.novel_status


# ------------------------------------------------------------------------------------------------ the design reached its tables
def test_the_designed_tables(X):
    f, wt = X.f, X.wtable
    assert len(wt) == f["wbuckets"] and len(X.ctable) == f["size"]
    want = np.zeros((f["wbuckets"], 16), np.uint32)
    want[:, [4, 9, 14]] = rm.NO_CLASS
    for c, (home, line, pos) in f["lines"].items():
        want[line, 5 * pos:5 * pos + 5] = list(rm.windows_of(X.classes[c])) + [c]
    assert np.array_equal(wt, want), "the window table is not where the model puts it"
    want = np.full(f["size"], rm.NO_CLASS, np.uint32)
    for c, (home, slot) in f["slots"].items():
        want[slot] = c
    assert np.array_equal(X.ctable, want), "the class-list table is not where the model puts it"
    # a full home line and a class in the following line; a chain from the last line through line 0; all three positions of a line
    nxt = [c for c in f["spilled"] if f["lines"][c][1] == (f["lines"][c][0] + 1) % f["wbuckets"]]
    assert nxt and all((wt[f["lines"][c][0], [4, 9, 14]] != rm.NO_CLASS).all() for c in f["spilled"])
    assert any(f["lines"][c][0] == f["wbuckets"] - 1 and f["lines"][c][1] < f["lines"][c][0] for c in f["wrapped"])
    assert f["positions"] == {0, 1, 2}
    # two window-less classes of one home slot; a chain through slot 0; more than 64 ids; ids more than 64 apart
    wl = f["windowless"]
    assert f["shared_slots"] and any(f["slots"][c][0] == f["size"] - 1 and f["slots"][c][1] < f["size"] - 1 for c in f["slot_wrapped"])
    assert any(len(X.classes[c]) > 64 for c in wl) and any(b - a > 64 for c in wl for a, b in zip(X.classes[c], X.classes[c][1:]))
    # every shape and its sibling is a window class of the index
    for name, pair in rm.SHAPES.items():
        assert all(X.class_of[ids] in f["lines"] for ids in pair), name
    spans = {name: max(pair[0]) - min(pair[0]) for name, pair in rm.SHAPES.items()}
    assert spans["span31"] == 31 and spans["span32"] == 32 and spans["span63"] == 63 and 0 in rm.SHAPES["id0"][0] and rm.NUM_TX - 1 in rm.SHAPES["last_id"][0]


def test_the_pool_holds_every_presentation(X):
    k = X.pool.kinds
    need = ["canonical", "m1zero", "stale_b2", "wholly", "partly", "none", "gap1", "gap31", "gap32", "m2tz", "class", "novel", "list_windowless_class",
            "list_windowed_class", "list_prefix", "list_plus_one", "list_novel"] + ["z%d" % z for z in range(1, 32)]
    assert all(k[n] for n in need), [n for n in need if not k[n]]
    for kind in ("class", "novel"):                                  # each presentation for classes and for novel sets alike
        have = {n for _, ks in X.pool.items if kind in ks for n in ks}
        assert have >= set(need[:10]) | {"z%d" % z for z in range(1, 32)}, (kind, sorted(set(need[:10]) - have))
    counts = {it[0] & rm.COUNT_MASK for it, ks in X.pool.items if "novel" in ks}
    assert counts >= {1, 2, 32, 33, 64}
    assert len(X.pool.items) < SWEEP                                 # one sweep of four blocks holds the whole pool


def test_the_whole_pool(X):
    n = len(X.pool.items)
    r = launch(X, X.pool.stream(n))
    assert check(X, r) == [] and r.x["sweeps"] == 1
    # every class entry got its class, every novel one none: said here once more by label, not through the model's dictionary
    for i, (it, ks) in enumerate(X.pool.items):
        assert (r.colour[r.E[i, 0]] != rm.NO_CLASS) == ("class" in ks or ks[0].endswith("_class")), (i, ks)
    assert {int(c) for c in r.colour[r.E[:, 0]]} >= set(X.f["spilled"]) | set(X.f["slot_wrapped"]) | set(X.f["windowless"])


# ------------------------------------------------------------------------------------------------ shapes
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 3 * 4096 + 5])
def test_stream_lengths(X, n):
    pad = [i for i in (0, 1, 2, 40, n - 2, n - 1) if 0 <= i < n] if n > 64 else []
    r = launch(X, X.pool.stream(n, first=7 * n, pad=pad, seed=n) if n else np.zeros((0, 8), np.uint32))
    assert check(X, r) == []
    assert r.x["sweeps"] == (n + SWEEP - 1) // SWEEP
    if n == 0:
        assert r.arena_top == r.top0 and r.novel_ctr == r.novel_ctr0


def test_padding_alone_in_runs_and_at_both_ends(X):
    E = X.pool.stream(700, first=100, pad=[0, 1, 2, 3, 64, 130] + list(range(200, 330)) + list(range(600, 700)))
    r = launch(X, E)
    assert check(X, r) == []
    r = launch(X, np.tile(np.array(rm.PAD_ENTRY, np.uint32), (300, 1)))          # nothing but padding: padding keys, nothing else
    assert check(X, r) == [] and r.arena_top == r.top0 and r.novel_ctr == r.novel_ctr0
    assert (r.keys[r.keys_top:r.keys_top + 300] == rm.NO_KEY).all()


def test_one_sweep_at_the_devices_own_grid(X):
    """a million entries on an MI355X: the pool at both ends and in the middle (the first, a middle and the last workgroup), one known class
    elsewhere, so that the host's side of the comparison stays in numpy"""
    n, p = 4 * X.num_cus * 256 * 4, len(X.pool.items)
    block = X.pool.stream(p, seed=3)
    E = np.tile(rm.window_entry(0, 77, 1, *rm.windows_of(rm.SHAPES["span32"][1])), (n, 1)).astype(np.uint32)
    for at in (0, (n // 2 // 1024) * 1024 + 5, n - p):
        E[at:at + p] = block
    E[:, 0] = np.random.RandomState(4).permutation(n)
    r = launch(X, E, num_cus=X.num_cus, n_results=n)
    assert check(X, r) == [] and r.x["sweeps"] == 1
    waves = {s["wave"] for s in r.x["slices"]}
    span = p // 256 + 1                                               # waves a copy of the pool covers
    assert min(waves) < span and max(waves) >= n // 256 - span and any(abs(w - n // 512) <= span for w in waves)
    assert all(s["iteration"] == 0 for s in r.x["slices"])


def test_more_than_a_chunk_in_one_iteration(X):
    r = launch(X, novel_windows(256, {i: 64 for i in range(256)}))
    assert check(X, r) == []
    assert [s["take"] for s in r.x["slices"]] == [256 * 64] and 256 * 64 > rm.ARENA_CHUNK and r.arena_top == r.top0 + 256 * 64
    first = r.results.reshape(-1, 4)[r.E[[0, 64, 1], 0], 2]
    assert list(first) == [r.top0, r.top0 + 64, r.top0 + 256]                    # one wave: lane 0 (j = 0, 1, 2, 3), then lane 1


def test_slices_run_out_in_later_iterations(X):
    """four waves of a grid of 4 blocks, three sweeps: wave 0 exhausts its slice in its second iteration, wave 1 in its third (its second still
    fits), wave 2 fills its slice to the last word in its second and takes a new one in its third, wave 3 meets nothing novel at all"""
    c = {}
    c.update({0 * 256 + i: 64 for i in range(10)})                   # wave 0: 640, then 448 > 384 left
    c.update({SWEEP + i: 64 for i in range(7)})
    c.update({1 * 256 + i: 64 for i in range(5)})                    # wave 1: 320, 320, then 33 + 64 x 6 = 417 > 384 left
    c.update({SWEEP + 256 + 64 * j + 9: 64 for j in range(4)})
    c[SWEEP + 256 + 200] = 64
    c.update({2 * SWEEP + 256 + i: 64 for i in range(6)})
    c[2 * SWEEP + 256 + 255] = 33
    c.update({2 * 256 + i: 64 for i in range(15)})                   # wave 2: 960, then exactly the 64 left, then 1
    c[SWEEP + 2 * 256 + 17] = 64
    c[2 * SWEEP + 2 * 256 + 130] = 1
    n = 2 * SWEEP + 4 * 256
    r = launch(X, novel_windows(n, c))
    assert check(X, r) == [] and r.x["sweeps"] == 3
    takes = sorted((s["wave"], s["iteration"], s["take"]) for s in r.x["slices"])
    assert takes == [(0, 0, 1024), (0, 1, 1024), (1, 0, 1024), (1, 2, 1024), (2, 0, 1024), (2, 2, 1024)], takes
    assert r.arena_top == r.top0 + 6 * 1024
    res = r.results.reshape(-1, 4)
    at = lambda i: int(res[r.E[i, 0], 2])
    # the second iteration goes on where the first ended: lane 8 (entry 200 = 64 * 3 + 8), then lane 9
    assert at(SWEEP + 256 + 200) == at(256) + 320 and at(SWEEP + 256 + 9) == at(256) + 384 and at(SWEEP + 2 * 256 + 17) == at(2 * 256) + 960


def test_a_launch_with_nothing_novel_takes_nothing(X):
    known = [i for i, (it, ks) in enumerate(X.pool.items) if "class" in ks or ks[0].endswith("_class")]
    E = X.pool.stream(600)
    for i in range(600):
        E[i, 3:] = X.pool.items[known[i % len(known)]][0]
    r = launch(X, E)
    assert check(X, r) == [] and r.arena_top == r.top0 and r.x["slices"] == [] and r.novel_ctr == r.novel_ctr0
    assert int(r.counts[X.nc]) == X.FILL64 + X.nc


@pytest.mark.parametrize("how", ["defer_at_cap", "defer_beyond_cap", "keys_at_cap", "keys_beyond_cap"])
def test_stream_heads_at_and_beyond_their_capacities(X, how):
    E = X.pool.stream(500, first=33)
    if how == "defer_at_cap":
        r = launch(X, E, defer_top=500, defer_cap=500)
    elif how == "defer_beyond_cap":                                  # the map kernel counted chunks it could not write: only defer_cap entries are read
        r = launch(X, E[:300], defer_top=500, defer_cap=300, n_results=507)
        assert r.n == 300
    elif how == "keys_at_cap":
        r = launch(X, E, keys_top=40, keys_cap=40)
    else:
        r = launch(X, E, keys_top=1 << 33, keys_cap=40)
        assert (r.keys[:40] == X.FILL).all() and (r.keys[40:540] != X.FILL).all()
    assert check(X, r) == []


@pytest.mark.parametrize("flags", [NO_KEYS, NO_COLOUR, NO_NOVEL, NO_KEYS | NO_COLOUR | NO_NOVEL])
def test_optional_outputs(X, flags):
    r = launch(X, X.pool.stream(900, first=11, pad=[5, 899], step=7), flags=flags)
    assert check(X, r) == [] and sum(r.x["novel"]) > 100
    if flags & NO_KEYS:                                               # records are still written
        assert (r.keys == X.FILL).all() and int(r.counts[X.nc]) == X.FILL64 + X.nc and (r.results[:4 * 900] != X.FILL).any()


def test_two_runs_agree(X):
    E = X.pool.stream(2 * SWEEP + 77, first=5, pad=[9, 4096])
    a, b = launch(X, E), launch(X, E)
    assert check(X, a) == [] and check(X, b) == []
    assert normal(X, a) == normal(X, b)


# ------------------------------------------------------------------------------------------------ capacity edges
def one_wave(X):
    """256 entries of the pool, a wave's worth: where every id lies is fully determined"""
    E = X.pool.stream(256, first=3, pad=[17], seed=8, step=29)
    x = rm.expect(E, X.pool.arena, X.class_of, 256, 1)
    total = int(x["count"][x["slice_of"] >= 0].sum())
    assert len(x["slices"]) == 1 and x["slices"][0]["take"] == max(total, rm.ARENA_CHUNK) and total > 64
    assert sum(1 for i in range(256) if x["novel"][i] and not x["window"][i]) > 0       # novel lists among them
    return E, x, total


def test_arena_exactly_large_enough_and_one_word_less(X):
    E, x, total = one_wave(X)
    top0 = len(X.pool.arena)
    r = launch(X, E, arena_cap=top0 + total, novel_ctr0=0)
    assert check(X, r) == [] and r.status == 0 and r.arena_top == top0 + max(total, rm.ARENA_CHUNK)
    assert all(int(r.results.reshape(-1, 4)[r.E[i, 0], 2]) == top0 + rel for i, rel in x["slices"][0]["entries"])   # one wave, one take: the base is top0
    r = launch(X, E, arena_cap=top0 + total - 1, novel_ctr0=0)
    last = x["slices"][0]["entries"][-1][0]                          # the last novel window entry in lane-then-j order
    assert check(X, r) == [last] and r.status == rm.STATUS_ARENA_FULL
    assert r.keys[r.keys_top + last] == rm.NO_KEY and int(r.counts[X.nc]) == X.FILL64 + X.nc + sum(x["novel"])
    assert r.novel_ctr == sum(x["novel"]) - 1 and (r.arena[top0 + total - 1:] == X.FILL).all()
    rec = r.results.reshape(-1, 4)[r.E[last, 0]]
    assert int(rec[2]) + int(rec[3]) == top0 + total and int(rec[3]) == len(x["ids"][last])


def test_a_full_arena_loses_every_novel_window_and_nothing_else(X):
    E = X.pool.stream(SWEEP + 300, first=3, pad=[0, 4100])
    top0 = len(X.pool.arena)
    r = launch(X, E, arena_cap=top0)
    lost = check(X, r)
    m = r.x
    assert lost == np.flatnonzero(m["window"] & np.array(m["novel"])).tolist() and len(lost) > 500 and r.status == rm.STATUS_ARENA_FULL
    assert np.array_equal(r.arena[:top0], X.pool.arena) and (r.arena[top0:] == X.FILL).all()
    lists = sum(1 for i in range(r.n) if m["novel"][i] and not m["window"][i])
    assert lists >= 6 and r.novel_ctr == r.novel_ctr0 + lists        # novel list entries are still listed
    # the arena_needed promise: a rerun with the arena_top the full run reported loses nothing
    again = launch(X, E, arena_cap=r.arena_top)
    assert check(X, again) == [] and again.status == 0 and again.arena_top == r.arena_top


@pytest.mark.parametrize("short", [1, "all_but_one", 0])
def test_novel_list_capacity(X, short):
    E, x, total = one_wave(X)
    novel = sum(x["novel"])
    assert novel > 8
    cap = novel if short == 0 else 1 if short == 1 else novel - 1
    r = launch(X, E, novel_cap=cap, novel_ctr0=0)
    assert check(X, r) == []
    assert r.novel_ctr == novel and r.novel_status == (0 if cap == novel else rm.NOVEL_LIST_FULL)
    written = r.novel[:2 * cap].reshape(-1, 2)
    assert (written[:, 1] != X.FILL).all() and (r.novel[2 * cap:] == X.FILL).all()   # exactly min(novel, cap) pairs


def test_a_counter_that_starts_beyond_the_list(X):
    E, x, total = one_wave(X)
    r = launch(X, E, novel_cap=4, novel_ctr0=9)                      # the map kernel overran the list already: nothing more is written
    assert check(X, r) == [] and r.novel_ctr == 9 + sum(x["novel"]) and (r.novel == X.FILL).all() and r.novel_status == rm.NOVEL_LIST_FULL


# ------------------------------------------------------------------------------------------------ the probe refuses what could leave its buffers
def test_the_probe_validates_its_input(X):
    good = X.pool.stream(40)
    assert check(X, launch(X, good)) == []

    def refused(E, **kw):
        rc = launch(X, E, checked=False, **kw)
        assert rc == ERR_INVALID, rc

    E = good.copy(); E[3, 0] = E[4, 0]; refused(E)                                   # two entries of one rid
    E = good.copy(); E[3, 0] = 47; refused(E)                                        # a rid outside the results (40 + 7 of them)
    w = next(i for i in range(40) if good[i, 3] & rm.DEFER_WINDOW)
    E = good.copy(); E[w, 3] += 1; refused(E)                                        # count is not the bits of the masks
    E = good.copy(); E[w, 3:8] = [rm.DEFER_WINDOW | 2, 100, 1, 131, 1]; refused(E)    # window 2 starts inside window 1
    E = good.copy(); E[w, 4:8] = [rm.NUM_TX - 1, 3, 0, 0]; E[w, 3] = rm.DEFER_WINDOW | 2; refused(E)   # an id that is no transcript
    E = good.copy(); E[w, 4:8] = [0, 1, rm.NUM_TX - 31, 0x80000000]; E[w, 3] = rm.DEFER_WINDOW | 2; refused(E)
    E = good.copy(); E[w, 3] = rm.DEFER_WINDOW; E[w, 5] = E[w, 7] = 0; refused(E)      # an empty window entry
    E = good.copy(); E[w, 3] = 2; refused(E)                                         # neither kind
    arena = X.pool.arena
    E = good.copy(); E[w, 3:8] = [rm.DEFER_LIST | 3, len(arena) - 2, 0, 0, 0]; refused(E)   # a list that runs past the arena
    bad = arena.copy(); bad[3:6] = [7, 7, 9]
    E = good.copy(); E[w, 3:8] = [rm.DEFER_LIST | 3, 3, 0, 0, 0]; refused(E, arena=bad)     # not strictly ascending
    bad[3:6] = [7, 9, rm.NUM_TX]
    refused(E, arena=bad)                                                            # an id that is no transcript
    refused(good[:30], defer_top=40, defer_cap=40, n_results=47)                                  # fewer entries than defer_top and defer_cap promise
    refused(good, defer_top=40, defer_cap=30)                                        # more than defer_cap holds
