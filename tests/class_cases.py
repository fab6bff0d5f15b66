"""Designed class sets for the map kernel's class intersection (src/pseudoaligner.rs:323-356, nodes_to_eq_class + intersect).
Pure Python + numpy, no product code: the expected class of a read is a Python set intersection.

A case is a list of CHAINS. A chain is one random backbone cut into consecutive nodes (number of k-mers, id set): node i is
backbone[p_i : p_{i+1} + k - 1], its left / right extension letters are the backbone's neighbouring bases — a unitig cut only by
colour. A read over the nodes a..b is backbone[p_a + lo : p_{b+1} + k - 1 - hi] (lo / hi k-mers inside the first / last node), its
expected class the intersection of the id sets of the nodes a..b, its coverage its length, its mismatches 0.

case(name, k) -> (node set, k, num_tx, reads, expected id lists, target per read, bitmap_min). The node set is what
helpers.index_from_node_set takes. A TARGET names the way the read has to take through the product (what tests/emu reports,
helpers.Emu.map_tiles(want_path=True)):
    path      "window"  two-window AND only (ST_F_BITS)
              "masked"  window mode with window-less classes pending (ST_F_MASK)
              "lists"   only window-less classes: restarted in list mode (restart_lists)
    tier      list mode: what isect_pick chooses — 0 ST_F_LIGHT, 1 ST_F_SCAN, 2 ST_F_COOP
    ncol      list mode: distinct classes collected        npend   window mode: pending (window-less) classes
    base_len  list mode: ids of the base (a shortest) list
    kind      "ref" by reference / "class" an index class found by content / "novel" / "empty"; None = whatever it is
The targets of the reads a row is ABOUT are written out in the tables below; target_of() derives the same fields from the class
structure alone (the flattener's rule for windows, isect_pick's rule for the tier) for the sub-reads of a chain, and the module
asserts that both agree."""
import numpy as np

CLASS_WINDOW = 32

# src/pseudoaligner.rs:544-559, the reference's own vectors for `intersect` (tests/test_oracle_intersect.py runs them on the oracle)
VECS = [
    [1, 2, 3, 4, 5, 6, 7, 8, 9], [1, 2, 3], [1, 4, 5], [7, 8, 9], [9], [], [1, 2, 3, 6, 7, 8, 9], [1, 7, 8, 9, 10],
    [10, 15, 20], [21, 22, 23], [0], [0, 1000, 5000], [0, 1000, 1000001], [5], [100000000], [1, 23, 45, 1000001, 100000000],
]

CASES = ("seams", "vectors", "pending32768", "pending32783", "nobitmap", "lists")


def has_windows(ids):
    """the index keeps a class as two windows when its ids lie in [min, min + 32) U [x, x + 32), x = the first id beyond window 1"""
    ids = sorted(ids)
    if not ids:
        return False
    rest = [x for x in ids if x - ids[0] >= CLASS_WINDOW]
    return not rest or rest[-1] - rest[0] < CLASS_WINDOW


def T(path, tier=-1, ncol=0, npend=0, base_len=0, kind=None):
    return dict(path=path, tier=tier, ncol=ncol, npend=npend, base_len=base_len, kind=kind)


def target_of(sets):
    """path / counts of a read over nodes with these id sets, from the class structure alone (kind is not derived)"""
    wl = [not has_windows(s) for s in sets]
    if not any(wl):
        return T("window")
    if not all(wl):
        return T("masked", npend=sum(wl))
    distinct = list(dict.fromkeys(tuple(sorted(s)) for s in sets))
    lens = [len(s) for s in distinct]
    base = min(lens)
    tier = 0 if len(distinct) == 1 or (len(distinct) <= 3 and max(lens) <= 7) else 1 if base <= 8 else 2
    return T("lists", tier, len(distinct), 0, base)


class Builder:
    def __init__(self, k, seed, tail=0):
        self.k, self.rng, self.tail = k, np.random.RandomState(seed), tail
        self.nodes, self.reads, self.expected, self.target = set(), [], [], []

    def chain(self, sets, nk=2):
        """nodes of nk k-mers each (an int, or one per node); with self.tail a last node of that many k-mers and the class of the one before"""
        sets = [tuple(sorted(s)) for s in sets]
        nks = [nk] * len(sets) if isinstance(nk, int) else list(nk)
        if self.tail:
            sets, nks = sets + [sets[-1]], nks + [self.tail]
        p = np.concatenate([[0], np.cumsum(nks)]).astype(np.int64)
        bb = "".join("ACGT"[c] for c in self.rng.randint(0, 4, int(p[-1]) + self.k - 1))
        for i, s in enumerate(sets):
            self.nodes.add((bb[p[i]: p[i + 1] + self.k - 1], s, bb[p[i] - 1] if i else "", bb[p[i + 1] + self.k - 1] if i + 1 < len(sets) else ""))
        return bb, p, sets, nks

    def read(self, ch, a, b, want=None, lo=0, hi=0):
        bb, p, sets, nks = ch
        if self.tail and b == len(sets) - 2:   # a read that reaches the chain's end runs on through the tail: same class, other length
            b, hi = b + 1, 0
        assert lo < nks[a] and hi < nks[b]
        got = target_of(sets[a: b + 1]) if not self.tail else None
        if want is not None and got is not None:
            assert {f: want[f] for f in got if f != "kind"} == {f: got[f] for f in got if f != "kind"}, (want, got)
        exp = set(sets[a])
        for s in sets[a + 1: b + 1]:
            exp &= set(s)
        self.reads.append(bb[p[a] + lo: p[b + 1] + self.k - 1 - hi])
        self.expected.append(sorted(exp))
        self.target.append(want or got)

    def row(self, sets, want, nk=2, subreads=True):
        """the chain, the read over all of it (the one the row is about), and its sub-reads: every single node, the read that starts and
        ends one k-mer inside its end nodes, and the read without the first node"""
        ch = self.chain(sets, nk)
        n = len(sets)
        self.read(ch, 0, n - 1, want)
        if subreads and not self.tail:
            if ch[3][0] > 1 and ch[3][n - 1] > 1 and (n > 1 or ch[3][0] > 2):
                self.read(ch, 0, n - 1, want and dict(want, kind=None), lo=1, hi=1)
            if n > 1:
                self.read(ch, 1, n - 1)
                for i in range(min(n, 3)):
                    self.read(ch, i, i)
        return ch


def far(start, n, step=40):
    """n ids no two of which share a window"""
    return [start + step * i for i in range(n)]


# ------------------------------------------------------------------------------------------------ window seams (ST_F_BITS, resolve.hip)
def _seams(b):
    W, R, C, N, E = T("window"), T("window", kind="ref"), T("window", kind="class"), T("window", kind="novel"), T("window", kind="empty")
    b.row([{5, 9, 36}, {5, 36}], R)                               # max - min = 31: one window, base 5 (no multiple of 32)
    b.row([{105, 109, 137}, {105, 137}], R)                       # max - min = 32: two windows, the second at the first id beyond window 1
    b.row([{205, 236, 237, 268}, {205, 237, 268}], R)             # window 2 = [237, 269): its last id
    b.row([{305, 340, 380}], T("lists", 0, 1, 0, 3, "ref"))       # a third window of one id: no windows at all
    b.row([{405, 409, 440, 445}, {440, 445, 500}], N)             # empties window 1, keeps window 2: window_canon moves it; no class
    b.row([{505, 509, 540, 545}, {540, 545, 600}, ], C)           # ... and {540, 545} is a class of a node the read does not visit
    b.row([{540, 545}], R)
    b.row([{605, 620, 630, 640, 645}, {620, 630, 640, 645, 651}], N)   # window 2's ids fall into the re-based window 1 (gap = 20 < 32), none stay
    b.row([{705, 730, 740, 770, 771}, {730, 740, 770, 771, 799}], N)   # gap = 10: id 740 moves to window 1, 770 and 771 stay in a re-based window 2
    b.row([{805, 830, 840, 870, 871}, {830, 840, 870, 871, 899}], C)   # ... and that is a class elsewhere
    b.row([{830, 840, 870, 871}], R)
    b.row([{905, 937}, {905, 937, 940}, {905, 906, 937}], R)      # the result is the first class seen (gap = 32 exactly)
    b.row([{1005, 1006, 1037}, {1005, 1037, 1040}, {1005, 1037}], R)    # ... the last class seen
    b.row([{1105, 1110}, {1140, 1150}], E)                        # disjoint: empty
    b.row([{1205, 1236}, {1237, 1268}], E)                        # neighbours across both seams: empty
    b.row([{1305, 1336, 1337}, {1336, 1337, 1368}], N)            # ids on both sides of the seam survive
    b.row([{1400 + i for i in range(32)} | {1432 + i for i in range(32)}, {1400, 1431, 1432, 1463}], R)   # two full windows
    b.row([{0, 31}, {0, 31, 32}], R)                              # id 0, base 0
    b.row([{0, 31, 32, 63}, {31, 32, 63, 64}], N)
    b.row([{1505, 1509}, {1505, 1509}, {1505, 1509, 1511}], R, nk=[1, 3, 2])     # the same class twice, a node of one k-mer
    return 1600


# ------------------------------------------------------------------------------------------------ the reference's intersect vectors
def _vectors(b):
    vals = sorted({v for vec in VECS for v in vec})
    rank = {v: i for i, v in enumerate(vals)}
    # two monotone maps of the values (intersections are kept): ranks three apart from 7 on (the vectors span one, two and three
    # windows), and the values themselves from 29 on while they are small (so that 1..9 straddle id 32), 40 apart beyond
    maps = (lambda v: 7 + 3 * rank[v], lambda v: 29 + v if v <= 23 else 60 + 40 * (rank[v] - rank[23]))
    top = 0
    for f in maps:
        for x in VECS:
            for y in VECS:
                sx, sy = {f(v) for v in x}, {f(v) for v in y}
                top = max([top] + list(sx | sy))
                b.row([sx, sy], dict(target_of([sx, sy]), kind=None), subreads=False)
    return top + 1


# ------------------------------------------------------------------------------------------------ pending classes (ST_F_MASK, window_hits)
def _pending_class(w_part, n, pool):
    """a window-less class of n ids: w_part and ids of `pool` (far from every window class, no two in one window)"""
    ids = sorted(set(w_part) | set(pool[: n - len(set(w_part))]))
    assert len(ids) == n and not has_windows(ids), ids
    return ids


def _multi_pending(b, w, n, pool, psize, at):
    """a window class w and n DIFFERENT pending classes of psize ids each, every one holding all of w but: the first lacks w[2], the last
    w[4], the 65th (the whole-wave loop's second round) w[5]. w is node `at` of the walk (0 first, -1 last, else in the middle)."""
    w = sorted(w)
    ps = []
    for i in range(n):
        drop = {w[2]} if i == 0 else set()
        if i == n - 1 and n > 1:
            drop.add(w[4])
        if i == 64:
            drop.add(w[5])
        ps.append(_pending_class(set(w) - drop, psize, [pool[0] + 40 * i + 1] + pool[1:]))
    pos = 0 if at == 0 else n if at == -1 else n // 2
    sets = ps[:pos] + [w] + ps[pos:]
    b.row(sets, T("masked", npend=n, kind="novel"), subreads=False)


def _pending(b, num_tx, sizes=(3, 15, 16, 64, 65), counts=(1, 2, 5, 40, 63, 64, 65, 130), pool_at=None):
    """window class W + window-less classes P of `sizes` ids that hold some, none and all of W; `counts` pending classes in one read"""
    pool = far(pool_at or num_tx // 2, 140, 40)          # far ids, shared by the pending classes
    base = 64
    for n in sizes:
        for share in ("some", "none", "all"):
            for order in (0, 1):
                w = [base + 3, base + 10, base + 43] if n > 3 or share != "all" else [base + 3, base + 43]
                part = {"some": w[1:2] + w[2:3] if n > 3 else w[1:2], "none": [], "all": w}[share]
                p = _pending_class(part, n, pool)
                kind = {"some": "novel", "none": "empty", "all": "ref"}[share]
                b.row([w, p] if order == 0 else [p, w], T("masked", npend=1, kind=kind))
                base += 128
    for n in counts:
        for at in (0, -1, 1):
            w = [base + 1, base + 2, base + 9, base + 31, base + 40, base + 71]
            _multi_pending(b, w, n, pool, 20 if at == 1 else 9, at)   # (20 ids: classes with a bitmap)
            base += 128
    # the same class pending twice (it is noted once per node), a window class between
    w = [base + 3, base + 10, base + 43]
    p = _pending_class(w[:2], 16, pool)
    b.row([p, w, p], T("masked", npend=2, kind="novel"))
    base += 128
    # the end of the id range: a bitmap class that holds id_span - 1, a running window whose base lies within the last 32 ids (the
    # bitmap's spare words) and one whose second window does
    last = num_tx - 1
    for w in ([last - 5, last - 2, last], [last - 31, last], [last - 60, last - 31, last - 1, last], [last]):
        for n in (16, 33):
            p = _pending_class([last], n, pool)
            b.row([w, p], T("masked", npend=1, kind="class" if len(w) > 1 else "ref"))   # ({last} is the class of the last of these rows)
            b.row([p, w, _pending_class([last - 1 if last - 1 in w else last], n, pool[1:])], T("masked", npend=2, kind=None))
    assert base < pool[0] - 64 and pool[-1] + 200 < num_tx - 200
    return num_tx


def _nobitmap(b, num_tx=1 << 27):
    """an index whose bitmaps at 16 ids would take more than 4 GiB: more than 256 window-less classes of 64 ids and more over 2^27
    transcripts give bitmap_min = 128 (the six of 130 ids keep a bitmap of 16 MiB each). window_hits then reads lists of more than 64 ids by binary search."""
    rng = b.rng
    nclasses = [0, 0]

    def far_ids(n, lo, hi):
        out = np.zeros(0, np.int64)
        while len(out) < n:   # randint + unique, and no two ids in one window
            c = np.unique(np.concatenate([out, rng.randint(lo // 64, hi // 64, 2 * n) * 64 + rng.randint(0, 32, 2 * n)]))
            c = c[np.concatenate([[True], c[1:] // 64 != c[:-1] // 64])]
            out = c if len(c) <= n else rng.permutation(c)[:n]
        return sorted(int(x) for x in out)

    def pclass(w_part, n, nlow, wlo, whi):
        """n ids: w_part, nlow far ids below the window class, the rest above it"""
        nhigh = n - len(w_part) - nlow
        ids = sorted(set(far_ids(nlow, 4096, wlo - 4096)) | set(w_part) | set(far_ids(nhigh, whi + 4096, num_tx - 4096)))
        assert len(ids) == n and not has_windows(ids)
        nclasses[n >= 128] += 1
        return ids

    base = 1 << 20
    # the sought window before the first id, after the last, in the last chunk, and at every position of a 4-id chunk
    for n in (64, 65, 66, 127, 130):
        full = [base + i for i in range(32)]
        two = full + [base + 40 + i for i in range(32)]
        few = n >= 128                                   # (these keep a bitmap of num_tx / 8 bytes each: six of them)
        for nlow in [0, n - 32] if few else list(range(0, 9)) + [n - 32]:
            if nlow + 32 <= n:
                # all 32 ids of the window are in the list: the last of them sits in the last chunk the search has to scan
                p = pclass(full, n, nlow, base, base + 128)
                b.row([full, p], T("masked", npend=1, kind="ref"), subreads=False)
                base += 1 << 12
        for nlow in (1,) if few else (0, 1, n - 64):
            if n > 64:
                p = pclass(two, n, nlow, base, base + 128)
                b.row([p, two], T("masked", npend=1, kind="ref"), subreads=False)
                base += 1 << 12
        w = [base + 3, base + 10, base + 43]
        for nlow, part, kind in ((0, [], "empty"), (n, [], "empty"), (0, w[:2], "novel"), (n - 2, w[1:], "novel"), (n - 3, w, "ref"),
                                 (n // 2, w[1:2], "novel"), (1, [w[0], w[2]], "novel"))[4 if few else 0:]:
            p = pclass(part, n, nlow, base, base + 128)
            b.row([w, p] if nlow & 1 else [p, w], T("masked", npend=1, kind=kind), subreads=False)
            base += 1 << 12
    # 1 .. 130 pending lists of 64 / 65 ids in one read
    for n, psize in ((1, 65), (2, 64), (5, 70), (40, 65), (63, 66), (64, 65), (65, 64), (130, 65)):
        w = [base + 1, base + 2, base + 9, base + 31, base + 40, base + 71]
        # (the first id of the pool is where every class gets an id of its own; a third of the others lie below the window class)
        pool = [base + 2048] + far_ids(psize // 3, 4096, base - 4096) + far_ids(psize, base + 8192, num_tx - 4096)
        nclasses[0] += n
        _multi_pending(b, w, n, pool, psize, 1)
        base += 1 << 12
    for _ in range(24):                      # random lists of 64 .. 127 ids, the window anywhere
        w = sorted(base + int(x) for x in rng.choice(72, 6, replace=False))
        w = [x for x in w if x - w[0] < 32 or x - w[0] >= 40]
        assert has_windows(w)
        n = int(rng.randint(64, 128))
        part = [x for x in w if rng.rand() < 0.6]
        p = pclass(part, n, int(rng.randint(0, n - len(part) + 1)), base, base + 128)
        b.row([w, p] if rng.rand() < 0.5 else [p, w], T("masked", npend=1), subreads=False)
        base += 1 << 12
    assert nclasses[1] < 256 <= nclasses[0] + nclasses[1]
    return num_tx


# ------------------------------------------------------------------------------------------------ list mode (ST_F_LIGHT / _SCAN / _COOP)
def _lists(b):
    state = {"next": 4096}

    def fresh(n):
        out = far(state["next"], n, 40)
        state["next"] += 40 * n + 40
        return out

    filler = far(400000, 140, 40)   # ids only the OTHER lists hold

    def family(ncls, base_len, other_len, tier, kind):
        """a base list of base_len ids and ncls - 1 other lists of other_len ids. kind: "ref" every other list holds the whole base;
        "novel" / "class" the first other list lacks one base id, the last another; "empty" none holds a base id."""
        if kind == "ref" and other_len == base_len and ncls > 1:
            return                                  # (every other list holds the base and an id of its own)
        base = fresh(base_len)
        others = []
        for i in range(ncls - 1):
            if kind == "ref":
                part = list(base)
            elif kind == "empty":
                part = []
            else:
                part = [x for j, x in enumerate(base) if not (i == 0 and j == 1) and not (i == ncls - 2 and j == base_len - 1 and ncls > 2)]
            uniq = fresh(1)
            others.append(sorted(set(part) | set(uniq) | set(filler[: other_len - len(part) - 1])))
            assert len(others[-1]) == other_len and other_len >= base_len, (other_len, base_len)
        pos = (ncls - 1) // 2                       # the base in the middle of the walk
        sets = others[:pos] + [base] + others[pos:]
        if kind == "class":                         # the result as the class of a node of another chain
            res = set(base)
            for o in others:
                res &= set(o)
            b.row([res], None, subreads=False)
        b.row(sets, T("lists", tier, ncls, 0, base_len, kind if ncls > 1 else "ref"), subreads=ncls <= 5)

    for ncls in (1, 2, 3):                          # ST_F_LIGHT: registers only
        for kind in ("ref", "novel", "class", "empty"):
            family(ncls, 3, 7, 0, kind)
            family(ncls, 7, 7, 0, kind)
    for kind in ("ref", "novel", "class", "empty"):
        family(4, 3, 7, 1, kind)                    # four short lists: no longer ST_F_LIGHT; all inline (LDS_CLASSES)
        family(5, 3, 7, 1, kind)                    # the fifth class is in the spill row
        family(2, 7, 8, 1, kind)                    # <= 3 classes, a list of 8 ids: ST_F_LIGHT hands over to ST_F_SCAN
        family(3, 8, 9, 1, kind)                    # base of 8 ids: the eighth id comes from the third quad
        family(5, 8, 12, 1, kind)
        family(2, 9, 9, 2, kind)                    # base of 9 ids: ST_F_COOP (through ST_F_LIGHT)
        family(5, 9, 20, 2, kind)                   # ... and directly
    for ncls in (40, 63, 64, 65, 130):              # ST_F_SCAN: the packed pass, the pass that fills the wave, the whole-wave loop and its second round
        for kind in ("novel", "ref", "empty"):
            family(ncls, 7 if ncls & 1 else 8, 9, 1, kind)
    family(64, 3, 64, 1, "class")
    family(65, 5, 65, 1, "class")                   # long other lists under the scan
    for base_len in (9, 64, 65, 130):               # ST_F_COOP: one base id per lane, a second round of base ids beyond 64
        for other_len in (64, 65):                  # ... other lists scanned (<= 64 ids) or searched
            if other_len >= base_len:
                for kind in ("novel", "ref", "class", "empty"):
                    family(3, base_len, other_len, 2, kind)
        for kind in ("novel", "ref", "empty"):
            family(5, base_len, 135, 2, kind)
    family(66, 9, 12, 2, "novel")                   # more than 64 lists under ST_F_COOP
    family(130, 10, 11, 2, "class")
    # the same class met twice (dedupe), two classes of equal shortest length (the first is the base)
    a, c = fresh(5), fresh(5)
    b.row([a, sorted(set(a[:3]) | set(c[:4])), a], T("lists", 0, 2, 0, 5, "novel"))
    b.row([sorted(a[:4] + c[:1]), sorted(a[:4] + c[1:2])], T("lists", 0, 2, 0, 5, "novel"))
    x, y = fresh(9), fresh(9)
    b.row([sorted(x[:8] + y[:1]), sorted(x[:8] + y[1:2]), sorted(x[:7] + y[2:4])], T("lists", 2, 3, 0, 9, "novel"))
    assert state["next"] < filler[0] - 64
    return filler[-1] + 64


_FAMILIES = {
    "seams": (_seams, 16), "vectors": (_vectors, 16), "pending32768": (lambda b: _pending(b, 32768), 16),
    "pending32783": (lambda b: _pending(b, 32783), 16), "nobitmap": (_nobitmap, 128), "lists": (_lists, 16),
}


def case(name, k, tail=0, seed=0):
    """-> (node set, k, num_tx, reads, expected id lists, target per read, bitmap_min of the index). tail: every chain gets a last node
    of that many k-mers with the class of the node before it, and the reads that reach a chain's end run through it (targets are None then)"""
    fn, bitmap_min = _FAMILIES[name]
    b = Builder(k, 1000 * CASES.index(name) + seed + k, tail)
    num_tx = fn(b)
    assert all(i < num_tx for e in b.expected for i in e)
    return b.nodes, k, num_tx, b.reads, b.expected, b.target, bitmap_min
