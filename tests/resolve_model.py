"""Model of pa_resolve_kernel (csrc/resolve.hip) in plain Python and numpy; no product code. tests/test_gpu_resolve_edges.py drives the
kernel through tests/resolve/resolve_probe.hip and compares with this, exactly; tests/test_resolve_model.py pins the model on the CPU tier.

MEANING of a deferred entry, by sets only: a window entry is {b1 + i : m1 bit i} U {b2 + i : m2 bit i}, a list entry the ids at its arena
offset. Its class is a dict lookup of the sorted tuple among the index's classes, or none: window_canon is NOT restated here, so a
canonicalisation that goes wrong shows as a mismatch. What the kernel must leave behind (records, count keys, colours, the novel slot, the
novel list) follows from that and from the ARENA ACCOUNTING, which is exact: wave w of a grid of 4 num_cus blocks of 256 handles entries
[i0, i0 + 256) for i0 = 256 w, stepping by 4 * grid lanes, lane l entry i0 + 64 j + l (j < 4); per iteration `total` is the sum of the ids of
its novel window entries, a wave whose slice cannot hold it takes max(total, PA_ARENA_CHUNK) fresh words, and inside an iteration the
offsets follow lane order, then j. So the final arena_top is exact, and so is every offset relative to the slice it lies in.

Restated ONLY TO DESIGN inputs (the tests prove by read-back that a design reached what it was made for): pa_mix64, window_hash and the
line rule of the window table (hash * wbuckets >> 32, three entries per 64-byte line), the flattener's windows and insertion order, the
list hash (overflow_model) and the class-list table of 2 num_classes + 16 slots."""
from collections import Counter

import numpy as np

import overflow_model as om

NO_CLASS = NO_KEY = PAD_RID = 0xFFFFFFFF
DEFER_WINDOW, DEFER_LIST, COUNT_MASK = 0x80000000, 0x40000000, 0x3FFFFFFF
MAPPED_BIT = CLASS_REF = 0x80000000
ARENA_CHUNK = 1024
BLOCK, WAVE, PER_LANE = 256, 64, 4
WAVE_ENTRIES = WAVE * PER_LANE
STATUS_ARENA_FULL, NOVEL_LIST_FULL = 1, 4
CLASS_WINDOW = 32
WT_ENTRIES = 3
M32 = 0xFFFFFFFF


# ------------------------------------------------------------------------------------------------ entries and what they mean
def window_entry(rid, cov, mm, b1, m1, b2, m2):
    return [rid, cov, mm, DEFER_WINDOW | (bin(m1).count("1") + bin(m2).count("1")), b1 & M32, m1, b2 & M32, m2]


def list_entry(rid, cov, mm, off, count, tail=(0, 0, 0)):
    return [rid, cov, mm, DEFER_LIST | count, off] + list(tail)


PAD_ENTRY = [PAD_RID, 0, 0, 0, 0, 0, 0, 0]


def is_pad(e):
    return int(e[0]) == PAD_RID


def is_window(e):
    return not is_pad(e) and bool(int(e[3]) & DEFER_WINDOW)


def ids_of(e, arena):
    """the id set of a live entry as a sorted tuple"""
    if is_window(e):
        b1, m1, b2, m2 = (int(x) for x in e[4:8])
        s = {b1 + i for i in range(32) if m1 >> i & 1} | {b2 + i for i in range(32) if m2 >> i & 1}
        return tuple(sorted(s))
    off, n = int(e[4]), int(e[3]) & COUNT_MASK
    return tuple(int(x) for x in arena[off:off + n])


def present(ids, b1, b2):
    """the window entry words (b1, m1, b2, m2) of `ids` with window 1 at b1 and window 2 at b2: ids in [b1, b1 + 32) go to mask 1, the others to
    mask 2; None when they do not fit or the producer could not leave it (window 2 with ids must start at b1 + 32 or beyond)"""
    m1 = m2 = 0
    for i in ids:
        if 0 <= i - b1 < 32:
            m1 |= 1 << (i - b1)
        elif 0 <= i - b2 < 32:
            m2 |= 1 << (i - b2)
        else:
            return None
    if m2 and b2 < b1 + 32:
        return None
    return (b1, m1, b2, m2)


def presentation_kind(ids, w):
    """what a presentation exercises of the canonicalisation, from the sets alone: a set of labels among canonical, z<k> (mask 1 has k trailing
    zeros), m1zero, stale_b2, wholly / partly / none (ids of window 2 that lie within 32 of the smallest id), gap<g>, m2tz"""
    b1, m1, b2, m2 = w
    out = set()
    if w == windows_of(ids):
        out.add("canonical")
    if m1 == 0:
        out.add("m1zero")
        return out
    lo = min(ids)
    if lo > b1:
        out.add("z%d" % (lo - b1))
    if m2 == 0:
        if b2 != 0:
            out.add("stale_b2")
        return out
    w2 = [i for i in ids if not 0 <= i - b1 < 32]
    falls = [i for i in w2 if i < lo + 32]
    out.add("wholly" if len(falls) == len(w2) else "partly" if falls else "none")
    out.add("gap%d" % (b2 - lo))
    rest = [i for i in w2 if i >= lo + 32]
    if rest and min(rest) > max(b2, lo + 32):
        out.add("m2tz")
    return out


def presentations(ids, stale=(1, 0xFFFFFFFF)):
    """every way the producer can leave `ids` as two windows, one (words, labels) per distinct set of labels: window 1 from 31 ids below the
    smallest id up to it, window 2 from where it may start up to the first id it has to hold; window 1 empty; a stale base 2"""
    lo, out = min(ids), {}

    def add(w):
        if w is not None and (w[3] == 0 or w[2] + 31 < 1 << 32):
            kinds = presentation_kind(ids, w)
            key = frozenset(k for k in kinds if not k.startswith("gap") or k in ("gap1", "gap31", "gap32"))   # the other gaps: one of each is enough
            if key not in out:
                out[key] = (w, kinds)

    for b1 in range(max(0, lo - 31), lo + 1):
        rest = [i for i in ids if i - b1 >= 32]
        if not rest:
            for b2 in (0,) + tuple(stale) + (b1 + 7,):
                add(present(ids, b1, b2))
        else:
            for b2 in range(b1 + 32, rest[0] + 1):
                add(present(ids, b1, b2))
    if max(ids) - lo < 32:
        for b2 in {max(32, lo - t) for t in (0, 1, 5)} | {max(ids) - 31}:
            if 32 <= b2 <= lo and max(ids) - b2 < 32:
                for b1 in {0, b2 - 32}:
                    add(present(ids, b1, b2))
    return [(w, sorted(kinds)) for w, kinds in out.values()]


# ------------------------------------------------------------------------------------------------ restated to design inputs only
def window_hash(b1, m1, b2, m2):
    return om.fmix64((b1 << 32 | m1) ^ om.fmix64(b2 << 32 | m2)) >> 32


def windows_of(ids):
    """the flattener's windows of a class (device_flatten.cpp): window 1 at the smallest id, window 2 at the first id beyond it; None for a
    class of three or more windows (or none)"""
    ids = sorted(ids)
    if not ids:
        return None
    b1 = ids[0]
    rest = [i for i in ids if i - b1 >= CLASS_WINDOW]
    if rest and rest[-1] - rest[0] >= CLASS_WINDOW:
        return None
    b2 = rest[0] if rest else 0
    return (b1, sum(1 << (i - b1) for i in ids if i - b1 < CLASS_WINDOW), b2, sum(1 << (i - b2) for i in rest))


def wbuckets_for(nwin):
    return max(1, int(nwin / (WT_ENTRIES * 0.5)) + 1)


def home_line(w, wbuckets):
    return window_hash(*w) * wbuckets >> 32


def place_windows(classes):
    """classes (id tuples in class-id order) -> (wbuckets, {class id: (home line, line, position)}) as the flattener fills the window table"""
    wins = [(c, windows_of(ids)) for c, ids in enumerate(classes)]
    wins = [(c, w) for c, w in wins if w is not None]
    wb = wbuckets_for(len(wins))
    fill, where = [0] * wb, {}
    for c, w in wins:
        home = line = home_line(w, wb)
        while fill[line] == WT_ENTRIES:
            line = (line + 1) % wb
        where[c] = (home, line, fill[line])
        fill[line] += 1
    return wb, where


def class_table_size(num_classes):
    return 2 * num_classes + 16


def home_slot(ids, size):
    return om.list_hash(ids) % size


def place_lists(classes):
    """-> (size, {class id: (home slot, slot)}) of the class-list table (device_index.hip: every class, in class-id order, linear probing)"""
    size = class_table_size(len(classes))
    taken, where = set(), {}
    for c, ids in enumerate(classes):
        home = s = home_slot(ids, size)
        while s in taken:
            s = (s + 1) % size
        taken.add(s)
        where[c] = (home, s)
    return size, where


# ------------------------------------------------------------------------------------------------ the designed index
NUM_TX = 1400
SHAPES = {   # window-class shapes, each with a sibling that differs in one id
    "one_window": ((400, 403, 410), (400, 403, 411)),
    "two_windows": ((420, 425, 460, 470), (420, 425, 460, 471)),
    "span31": ((500, 507, 531), (500, 508, 531)),
    "span32": ((540, 547, 572), (540, 548, 572)),
    "span63": ((600, 610, 663), (600, 611, 663)),
    "id0": ((0, 3, 40), (0, 4, 40)),
    "last_id": ((NUM_TX - 41, NUM_TX - 5, NUM_TX - 1), (NUM_TX - 41, NUM_TX - 6, NUM_TX - 1)),
    "single": ((700,), (701,)),
    "merge": ((740, 748, 765, 780), (740, 748, 766, 780)),      # ids within 32 of the smallest that a shifted presentation leaves in window 2
    "gap1": ((1300, 1332), (1300, 1333)),                       # the one shape whose window 2 can start one id behind the smallest id
    "full": (tuple(range(800, 864)), tuple(i for i in range(800, 864) if i != 815)),
}
WINDOWLESS = [tuple(range(3, 3 + 3 * 70, 3)), (5, 100, 300), (5, 100, 301), (7, 72, 137, 202), tuple(range(900, 1000))]
NOVEL_SETS = {1: (702,), 2: (702, 703), 32: tuple(range(1000, 1032)), 33: tuple(range(1000, 1033)), 64: tuple(range(1000, 1064))}
FILL_LINES, FILL_SLOTS = 4, 2   # window classes sought per designed home line; window-less classes per designed home slot


def design_classes():
    """The designed classes (id tuples, a set: the index numbers them). Besides SHAPES and WINDOWLESS: four two-id window classes whose home line
    is the LAST line of the window table and four for a line in the middle (a full line and a class in the following one, once through line 0),
    and two window-less three-id classes for the last slot of the class-list table and two for a slot in the middle. The table sizes depend on
    the class counts only, which are fixed before the search."""
    fixed = [c for pair in SHAPES.values() for c in pair]
    nwin = len(fixed) + 2 * FILL_LINES
    nc = nwin + len(WINDOWLESS) + 2 * FILL_SLOTS
    wb, size = wbuckets_for(nwin), class_table_size(nc)
    assert all(windows_of(c) for c in fixed) and not any(windows_of(c) for c in WINDOWLESS)
    out = list(fixed)
    for line in (wb - 1, wb // 2):
        found = []
        for a in range(1100, 1300):
            for d in range(1, 32):
                if len(found) < FILL_LINES and home_line(windows_of((a, a + d)), wb) == line and all(a not in f and a + d not in f for f in found):
                    found.append((a, a + d))
        assert len(found) == FILL_LINES, "no %d window classes for line %d" % (FILL_LINES, line)
        out += found
    out += WINDOWLESS
    for slot in (size - 1, size // 2):
        found = []
        for a in range(10, 400):
            for d in range(70, 90):
                ids = (a, a + d, a + 2 * d + 1)
                if len(found) < FILL_SLOTS and home_slot(ids, size) == slot and all(a != f[0] for f in found):
                    found.append(ids)
        assert len(found) == FILL_SLOTS, "no %d window-less classes for slot %d" % (FILL_SLOTS, slot)
        out += found
    assert len(set(out)) == len(out) == nc and all(i < NUM_TX for c in out for i in c)
    assert not any(s in out for s in NOVEL_SETS.values())
    return out


def design_nodes(k=20, seed=11):
    """one isolated unitig per designed class: (sequence, ids, no left extension, no right extension), what helpers.index_from_node_set takes"""
    rng = np.random.RandomState(seed)
    return {("".join("ACGT"[c] for c in rng.randint(0, 4, k + 3)), ids, "", "") for ids in design_classes()}


def table_features(classes):
    """what the designed tables must show, from the placement the model computes for `classes` in class-id order: -> dict of
    spilled (window classes that sit in the line after their full home line), wrapped (those whose walk went from the last line through line
    0), positions (the line positions in use), shared_slots (home slots that two window-less classes share), slot_wrapped (window-less classes
    whose walk went through slot 0)"""
    wb, wl = place_windows(classes)
    size, sl = place_lists(classes)
    spilled = [c for c, (home, line, pos) in wl.items() if line != home]
    wrapped = [c for c in spilled if wl[c][1] < wl[c][0]]
    wless = [c for c in range(len(classes)) if c not in wl]
    homes = Counter(sl[c][0] for c in wless)
    return dict(wbuckets=wb, lines=wl, size=size, slots=sl, spilled=spilled, wrapped=wrapped, positions={p for _, _, p in wl.values()},
                shared_slots=[h for h, m in homes.items() if m > 1], slot_wrapped=[c for c in wless if sl[c][1] < sl[c][0]], windowless=wless)


# ------------------------------------------------------------------------------------------------ what a launch must leave behind
def waves_of(n, num_cus):
    """[(wave, iteration, first entry)] of every wave iteration that handles an entry below n, in the order a wave runs its own"""
    step = 4 * num_cus * BLOCK * PER_LANE
    out = []
    for w in range(4 * num_cus * BLOCK // WAVE):
        out += [(w, it, i0) for it, i0 in enumerate(range(w * WAVE_ENTRIES, n, step))]
    return out


def lane_order(i0, n):
    """the entries of the wave iteration at i0 in the order their arena offsets follow: lane, then j"""
    return [i0 + WAVE * j + lane for lane in range(WAVE) for j in range(PER_LANE) if i0 + WAVE * j + lane < n]


LANE_ORDER = (np.arange(WAVE)[:, None] + WAVE * np.arange(PER_LANE)[None, :]).ravel()   # offsets of a wave iteration's entries, lane by lane


def expect(entries, arena, class_of, n, num_cus):
    """entries[:n] are what the kernel reads (n = min(*defer_top, defer_cap)). class_of: {id tuple: class id} of the index. ->
    dict(ids (sorted tuples; None for padding), colour (NO_CLASS for none and padding), novel, keys, count, window: one per entry;
         slices = [dict(wave, iteration, take, entries=[(entry, offset inside the slice)])] in no particular order between waves (the entry
         lists only up to 65536 entries), slice_of / rel: per entry the slice that holds its ids (-1: none) and its offset inside the slice,
         used = sum of the takes, sweeps = iterations of wave 0)"""
    E = np.asarray(entries, np.uint32).reshape(-1, 8)[:n]
    live = E[:, 0] != PAD_RID
    window = live & ((E[:, 3] & DEFER_WINDOW) != 0)
    rows = E[:, 3:8].copy()
    rows[~window, 2:] = 0                                  # a list entry means its offset and count alone
    rows[~live] = 0
    with np.errstate(over="ignore"):                       # distinct rows through a 64-bit mix of each, then checked word for word
        mixed = (rows.astype(np.uint64) * np.array([0x9E3779B97F4A7C15, 0xBF58476D1CE4E5B9, 0x94D049BB133111EB, 0xFF51AFD7ED558CCD, 0xC4CEB9FE1A85EC53], np.uint64)).sum(axis=1, dtype=np.uint64)
    _, first, inv = np.unique(mixed, return_index=True, return_inverse=True)
    inv = inv.reshape(-1)
    uniq = rows[first]
    assert np.array_equal(uniq[inv], rows), "two different entries share a mix"
    u_ids = [ids_of([0, 0, 0] + [int(x) for x in r], arena) if r[0] else None for r in uniq]
    u_colour = np.array([NO_CLASS if s is None else class_of.get(s, NO_CLASS) for s in u_ids], np.uint32).reshape(-1)
    colour = np.where(live, u_colour[inv], NO_CLASS).astype(np.uint32) if n else np.zeros(0, np.uint32)
    novel = live & (colour == NO_CLASS)
    count = (E[:, 3] & COUNT_MASK).astype(np.int64)
    want = np.where(window & novel, count, 0)
    slice_of, rel = np.full(n, -1, np.int64), np.zeros(n, np.int64)
    slices, cur = [], {}
    for w, it, i0 in waves_of(n, num_cus):
        idx = i0 + LANE_ORDER
        idx = idx[idx < n]
        wv = want[idx]
        total = int(wv.sum())
        if not total:
            continue
        at, end, k = cur.get(w, (0, 0, -1))
        if at + total > end:
            k, at, end = len(slices), 0, max(total, ARENA_CHUNK)
            slices.append(dict(wave=w, iteration=it, take=end, entries=[]))
        sel = wv > 0
        rel[idx[sel]] = at + (np.cumsum(wv) - wv)[sel]
        slice_of[idx[sel]] = k
        if n <= 65536:
            slices[k]["entries"] += [(int(i), int(rel[i])) for i in idx[sel]]
        cur[w] = (at + total, end, k)
    return dict(ids=[u_ids[j] if l else None for j, l in zip(inv.tolist(), live.tolist())], colour=colour.tolist(), novel=novel.tolist(),
                keys=colour.tolist(), count=count, window=window, slices=slices, slice_of=slice_of, rel=rel,
                used=sum(s["take"] for s in slices), sweeps=len(range(0, n, 4 * num_cus * BLOCK * PER_LANE)))
