"""tests/resolve_model.py on the CPU tier: the hashes and table rules it restates, on values worked out step by step here; the meaning of an
entry and the labels of a presentation on hand-made windows; the arena accounting on streams small enough to follow by hand; and the
designed classes, which must show their table features in whatever order an index numbers them."""
import numpy as np
import pytest

import overflow_model as om
import resolve_model as rm

M64 = (1 << 64) - 1


def fmix_by_hand(x):
    x ^= x >> 33
    x = x * 0xFF51AFD7ED558CCD & M64
    x ^= x >> 33
    x = x * 0xC4CEB9FE1A85EC53 & M64
    return x ^ x >> 33


def test_mix64_and_window_hash():
    assert om.fmix64(0) == 0 and om.fmix64(1) == 0xB456BCFC34C2CB2C                  # murmur3's finaliser, its published value for 1
    assert rm.window_hash(5, 1, 0, 0) == fmix_by_hand(0x500000001) >> 32 == 0x1E1D760C   # one window: the inner mix is of 0
    inner = fmix_by_hand(40 << 32 | 3)
    assert rm.window_hash(5, 0x80000001, 40, 3) == fmix_by_hand((5 << 32 | 0x80000001) ^ inner) >> 32 == 0x60D00DE0
    assert rm.window_hash(5, 1, 0, 0) != rm.window_hash(0, 0, 5, 1)                 # the windows are not interchangeable


def test_line_rule_and_sizes():
    assert rm.home_line((5, 1, 0, 0), 19) == 0x1E1D760C * 19 >> 32 == 2
    assert rm.home_line((5, 1, 0, 0), 1) == 0 and rm.home_line((5, 0x80000001, 40, 3), 19) == 0x60D00DE0 * 19 >> 32 == 7
    assert [rm.wbuckets_for(n) for n in (0, 1, 2, 3, 28, 30)] == [1, 1, 2, 3, 19, 21]   # nwin / 1.5 + 1, truncated
    assert rm.class_table_size(0) == 16 and rm.class_table_size(37) == 90
    assert om.list_hash((1, 2, 3)) == 0x399E6AF19BDFF770 and rm.home_slot((1, 2, 3), 90) == 0x399E6AF19BDFF770 % 90


def test_windows_of_a_class():
    assert rm.windows_of((5, 9, 36)) == (5, 0x80000011, 0, 0)                        # span 31: one window
    assert rm.windows_of((540, 547, 572)) == (540, 0x81, 572, 1)                     # span 32: window 2 at the first id beyond window 1
    assert rm.windows_of((600, 610, 663)) == (600, 0x401, 663, 1)
    assert rm.windows_of((600, 610, 640, 671)) == (600, 0x401, 640, 0x80000001) and rm.windows_of((600, 610, 640, 672)) is None
    assert rm.windows_of(tuple(range(800, 864))) == (800, 0xFFFFFFFF, 832, 0xFFFFFFFF)
    assert rm.windows_of(()) is None and rm.windows_of((5, 100, 300)) is None and rm.windows_of((0,)) == (0, 1, 0, 0)


def test_insertion_order_of_both_tables(monkeypatch):
    five = [(10 * c, 10 * c + 1) for c in range(5)] + [(5, 100, 300)]                # five window classes: 5 / 1.5 + 1 = 4 lines
    monkeypatch.setattr(rm, "window_hash", lambda *w: 0xFFFFFFFF)                    # every class at home in the last line
    wb, where = rm.place_windows(five)
    assert wb == 4 and where == {0: (3, 3, 0), 1: (3, 3, 1), 2: (3, 3, 2), 3: (3, 0, 0), 4: (3, 0, 1)}
    monkeypatch.setattr(rm, "window_hash", lambda b1, *w: 0x40000000 * (b1 // 10 % 2))  # classes 0, 2, 4 in line 0, classes 1, 3 in line 1
    assert rm.place_windows(five)[1] == {0: (0, 0, 0), 1: (1, 1, 0), 2: (0, 0, 1), 3: (1, 1, 1), 4: (0, 0, 2)}
    monkeypatch.setattr(om, "list_hash", lambda ids: 21 + 22 * len(ids))             # 2 * 3 + 16 = 22 slots, everything at home in the last
    assert rm.place_lists([(1,), (2, 3), (4, 5, 6)]) == (22, {0: (21, 21), 1: (21, 0), 2: (21, 1)})


def test_meaning_of_an_entry():
    e = rm.window_entry(7, 100, 2, 540, 0x81, 572, 1)
    assert e == [7, 100, 2, 0x80000003, 540, 0x81, 572, 1] and rm.is_window(e) and rm.ids_of(e, None) == (540, 547, 572)
    assert rm.ids_of(rm.window_entry(7, 1, 0, 509, 0x80000000, 541, 0x80000040), None) == (540, 547, 572)
    assert rm.ids_of(rm.window_entry(7, 1, 0, 99, 0, 540, 0x81), None) == (540, 547)  # window 1 empty: its base means nothing
    arena = np.array([9, 9, 5, 100, 300, 9], np.uint32)
    l = rm.list_entry(3, 50, 1, 2, 3)
    assert l[:5] == [3, 50, 1, 0x40000003, 2] and not rm.is_window(l) and rm.ids_of(l, arena) == (5, 100, 300)
    assert rm.is_pad(rm.PAD_ENTRY) and not rm.is_window(rm.PAD_ENTRY)


def test_presentations_by_hand():
    s31, two, merge = rm.SHAPES["span31"][0], rm.SHAPES["two_windows"][0], rm.SHAPES["merge"][0]
    assert rm.present(s31, 500, 0) == (500, 0x80000081, 0, 0) and rm.presentation_kind(s31, (500, 0x80000081, 0, 0)) == {"canonical"}
    assert rm.presentation_kind(s31, (500, 0x80000081, 77, 0)) == {"stale_b2"}
    w = rm.present(s31, 490, 522)                                                    # 531 lies in window 2 and, seen from 500, in window 1
    assert w == (490, 0x20400, 522, 0x200) and rm.presentation_kind(s31, w) == {"z10", "gap22", "wholly"}
    w = rm.present(merge, 730, 762)                                                  # 765 falls into window 1, 780 stays: bit 18 of a window at 762, 12 zeros below it at 772
    assert w == (730, 0x40400, 762, 0x40008) and rm.presentation_kind(merge, w) == {"z10", "gap22", "partly", "m2tz"}
    assert rm.presentation_kind(two, rm.present(two, 419, 451)) == {"z1", "gap31", "none", "m2tz"}
    assert rm.presentation_kind(two, rm.present(two, 420, 452)) == {"gap32", "none", "m2tz"} and rm.present(two, 420, 460) == rm.windows_of(two)
    g1 = rm.SHAPES["gap1"][0]
    assert rm.present(g1, 1269, 1301) == (1269, 0x80000000, 1301, 0x80000000) and rm.presentation_kind(g1, rm.present(g1, 1269, 1301)) == {"z31", "gap1", "none"}
    assert rm.present(s31, 400, 500) == (400, 0, 500, 0x80000081) and rm.presentation_kind(s31, rm.present(s31, 400, 500)) == {"m1zero"}
    assert rm.present(two, 420, 440) is None and rm.present(two, 410, 441) is None    # do not fit; window 2 inside window 1
    for ids in [c for pair in rm.SHAPES.values() for c in pair] + list(rm.NOVEL_SETS.values()):
        ps = rm.presentations(ids)
        assert ps and all(rm.ids_of(rm.window_entry(0, 0, 0, *w), None) == tuple(ids) for w, _ in ps)
        assert all(w[3] == 0 or w[2] >= w[0] + 32 for w, _ in ps)
    kinds = {k for ids in (s31, two, merge, g1) for _, ks in rm.presentations(ids) for k in ks}
    assert kinds >= {"canonical", "m1zero", "stale_b2", "wholly", "partly", "none", "gap1", "gap31", "gap32", "m2tz"} | {"z%d" % z for z in range(1, 32)}


def novel_stream(n, at):
    """n canonical window entries, rid = position; those listed in `at` ({position: ids}) hold a novel set, the others class (400, 403, 410)"""
    known = rm.windows_of(rm.SHAPES["one_window"][0])
    return [rm.window_entry(i, 1, 0, *(rm.windows_of(at[i]) if i in at else known)) for i in range(n)]


CLASS_OF = {rm.SHAPES["one_window"][0]: 4}
N64 = rm.NOVEL_SETS[64]


def test_arena_accounting_by_hand():
    two = rm.NOVEL_SETS[2]
    x = rm.expect(novel_stream(300, {0: two, 64: two, 1: two, 299: N64}), None, CLASS_OF, 300, 1)
    assert x["sweeps"] == 1 and x["used"] == 2048 and x["colour"][2] == 4 and x["keys"][0] == rm.NO_KEY and x["novel"][:3] == [True, True, False]
    by_wave = {s["wave"]: s for s in x["slices"]}
    assert by_wave[0]["entries"] == [(0, 0), (64, 2), (1, 4)] and by_wave[1]["entries"] == [(299, 0)] and by_wave[1]["take"] == 1024   # lane, then j
    # 16 x 64 ids fill a slice to its last word: the next iteration of that wave takes a new one, one id less and it does not
    full = {i: N64 for i in range(16)}
    x = rm.expect(novel_stream(4098, {**full, 4097: two}), None, CLASS_OF, 4098, 1)
    assert x["sweeps"] == 2 and [(s["wave"], s["iteration"], s["take"]) for s in x["slices"]] == [(0, 0, 1024), (0, 1, 1024)]
    x = rm.expect(novel_stream(4098, {**full, 15: N64[:62], 4097: two}), None, CLASS_OF, 4098, 1)
    assert [(s["iteration"], s["take"]) for s in x["slices"]] == [(0, 1024)] and x["slices"][0]["entries"][-1] == (4097, 1022) and x["used"] == 1024
    x = rm.expect(novel_stream(4098, {**full, 15: N64[:63], 4097: two}), None, CLASS_OF, 4098, 1)   # one word left, two wanted: the word stays unused
    assert [(s["iteration"], s["take"]) for s in x["slices"]] == [(0, 1024), (1, 1024)] and x["used"] == 2048
    x = rm.expect(novel_stream(256, {i: N64 for i in range(17)}), None, CLASS_OF, 256, 1)   # more than a chunk at once: exactly that much
    assert [s["take"] for s in x["slices"]] == [17 * 64] and x["slices"][0]["entries"][16] == (16, 1024)
    x = rm.expect(novel_stream(4097, {}), None, CLASS_OF, 4097, 1)                  # nothing novel: nothing taken
    assert x["slices"] == [] and x["used"] == 0 and x["sweeps"] == 2
    x = rm.expect(novel_stream(300, {0: two}) , None, CLASS_OF, 200, 1)             # only n entries are read
    assert len(x["ids"]) == 200 and x["used"] == 1024
    padded = [rm.PAD_ENTRY] + novel_stream(3, {1: two})
    x = rm.expect(padded, None, CLASS_OF, 4, 1)
    assert x["ids"][0] is None and x["keys"] == [rm.NO_KEY, 4, rm.NO_KEY, 4] and x["novel"] == [False, False, True, False]
    assert rm.waves_of(4097, 1)[:2] == [(0, 0, 0), (0, 1, 4096)] and len(rm.waves_of(4097, 1)) == 17 and len(rm.waves_of(4096 * 2, 2)) == 32
    assert rm.lane_order(0, 130)[:5] == [0, 64, 128, 1, 65] and rm.lane_order(256, 258) == [256, 257]


@pytest.mark.parametrize("seed", range(6))
def test_designed_classes_show_their_features_in_any_order(seed):
    classes = rm.design_classes()
    rng = np.random.RandomState(seed)
    order = [classes[i] for i in rng.permutation(len(classes))]
    f = rm.table_features(order)
    assert f["wbuckets"] == rm.wbuckets_for(sum(rm.windows_of(c) is not None for c in classes)) and f["size"] == 2 * len(classes) + 16
    assert f["spilled"] and f["wrapped"] and f["positions"] == {0, 1, 2} and f["shared_slots"] and f["slot_wrapped"]
    assert any(len(order[c]) > 64 for c in f["windowless"]) and any(b - a > 64 for c in f["windowless"] for a, b in zip(order[c], order[c][1:]))
    assert len({seq for seq, _, _, _ in rm.design_nodes()}) == len(classes)
