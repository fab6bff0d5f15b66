"""Hand-made count tables that put the abundance kernels (csrc/quant.hip, csrc/quant_boot.hip) on their bin, batch and draw edges.
A serialised overflow record is any sorted id list with a 64-bit count, so a table whose class counts are zero and whose records are
written by hand is any incidence we like. Nothing here needs a GPU: the properties of every case are asserted where the case is made,
from the numpy models (tests/quant_model.py, tests/boot_model.py). Used by tests/test_quant_cases.py (CPU),
tests/test_gpu_quant_edges.py and tests/test_gpu_quant_boot_edges.py."""
import copy

import numpy as np

import boot_model as bm
import helpers
import quant_model as qm
from test_index_build import pack

pa = helpers.pa

# ---- what the kernels say, restated once: a change there means a change here ----
# csrc/quant_state.hpp: bin_min_len() and bin_group() (a block has QB = 256 threads: QB / bin_group(k) rows or transcripts share a block)
BIN_MIN = (1025, 17, 9, 5, 1)
GROUP = (256, 64, 16, 8, 4)
PER_BLOCK = (1, 4, 16, 32, 64)
# every threshold and every lane-group size, each with its two neighbours; 2049: a 256-lane group goes round its row nine times
EDGE = [1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 1026, 2049]
# csrc/quant_boot.hip: COARSE (the LDS copy of every step-th cumulative count, step = ceil(rows / COARSE): 1 up to 1024 rows, 2 up to
# 2048, 3 beyond), HT_SLOTS (the block's hash table; HT_PROBES = 4, then a direct atomic), QB * 2 draws of a workgroup per round
# (a Philox block is two draws), DRAW_CHUNK * 2 draws of a workgroup; boot_grid(): the bootstrap passes take layout bins 0 and 1
# together on the long path, then <= 16 / <= 8 / <= 4, and 256 / stride entities share a block; stride_for(): 4, 8, 16, 32, 64
COARSE = 1024
HT_SLOTS = 4096
DRAWS_PER_ROUND = 512
DRAWS_PER_WORKGROUP = 16384
BATCHES = (1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 63, 64)

SEED = 0x1234567855AA33CC          # the seed of tests/test_gpu_quant_boot.py
HIGH = 2 ** 32 - 64
MEAN_READ_LEN = 60.0               # transcripts of 20 .. 400 bases: some at the floor (eff == 1), some above it
POOL = 2049
LADDER_BOOT_TARGET = 24500          # Case.scaled() of a ladder: N of about 20 000
BIG_T = 6100
_cache = {}


def edge_index(T):
    """(host index, HostIndex.arrays(), transcript lengths) of T random ACGT transcripts of 20 .. 400 bases, K = 16"""
    key = ("index", T)
    if key not in _cache:
        rng = np.random.default_rng(9000 + T)
        lens = rng.integers(20, 401, T)
        lut = np.frombuffer(b"ACGT", np.uint8)
        seqs = [lut[rng.integers(0, 4, int(n))].tobytes().decode() for n in lens]
        words, tx_start = pack(seqs)
        host = pa.HostIndex.build_packed(words, tx_start, 16, 4)
        arr = host.arrays()
        tx_len = np.diff(host.transcripts()[1].astype(np.int64))
        assert arr["num_transcripts"] == T and np.array_equal(tx_len, lens)
        class_len = np.diff(arr["ec_offset"].astype(np.int64))
        assert arr["num_classes"] >= 1 and class_len.min() >= 1 and class_len.max() <= 2       # singletons or pairs
        if T == BIG_T:
            eff = qm.effective_lengths(tx_len, MEAN_READ_LEN)
            assert (eff == 1.0).any() and (eff > 1.0).any()
        _cache[key] = (host, arr, tx_len)
    return _cache[key]


def words_in_order(records):
    """[(sorted ids, count)] -> serialised words in the GIVEN record order (quant_model.write_overflow sorts them: an empty record would
    come first)"""
    w = [0, 0]
    for ids, c in records:
        w += [len(ids), int(c) & 0xFFFFFFFF, int(c) >> 32] + [int(x) for x in ids]
    w[0], w[1] = len(records), len(w)
    return np.array(w, np.uint32)


class Case:
    """a count table over edge_index(T): class_counts u64[C + 3] and the serialised overflow words"""

    def __init__(self, name, T, counts, words):
        self.name, self.T, self.counts, self.words = name, T, counts, words
        self._problem = self._cand = None

    @classmethod
    def of_records(cls, name, T, records, in_order=False):
        """every class count zero: the table is its records"""
        C = edge_index(T)[1]["num_classes"]
        counts = np.zeros(C + 3, np.uint64)
        counts[C] = sum(int(c) for _, c in records)
        return cls(name, T, counts, words_in_order(records) if in_order else qm.write_overflow(records))

    @property
    def problem(self):
        if self._problem is None:
            _, arr, tx_len = edge_index(self.T)
            self._problem = qm.Problem.from_table(arr, tx_len, self.counts, self.words, mean_read_len=MEAN_READ_LEN)
        return self._problem

    @property
    def cand(self):
        """reads of every candidate in candidate order (boot_model.candidate_counts)"""
        if self._cand is None:
            self._cand = bm.candidate_counts(edge_index(self.T)[1], self.counts, self.words)
        return self._cand

    def with_counts(self, name, fn):
        """the same candidates with counts fn(count) where a candidate has reads"""
        C = len(self.counts) - 3
        counts = self.counts.copy()
        pos = counts[:C] > 0
        counts[:C][pos] = [fn(int(c)) for c in counts[:C][pos]]
        recs = [(ids, fn(c) if c and len(ids) else c) for ids, c in qm.read_overflow(self.words)]
        counts[C] = sum(c for _, c in recs)
        return Case(name, self.T, counts, words_in_order(recs))

    def scaled(self, target=20000):
        """every count c -> 1 + c (target - rows) // N: N' in (target - rows, target], no row lost"""
        p = self.problem
        assert target > len(p.rows)
        return self.with_counts(self.name + "/scaled", lambda c: 1 + c * (target - len(p.rows)) // p.N)

    def replicate_problem(self, rep):
        """the Problem of a replicate (counts per candidate) WITHOUT building it again: the rows of the table, a row the replicate left
        without reads stays with n = 0 and adds 0.0 to every sum it is in. step() is that of the table quant_model.Problem.from_table
        makes of the replicate, bit for bit (tests/test_quant_cases.py holds the two together)"""
        p = copy.copy(self.problem)
        p.n = np.asarray(rep, np.uint64)[np.flatnonzero(self.cand > 0)].astype(np.float64)
        assert len(p.n) == len(p.rows)
        p.N = int(np.asarray(rep, np.uint64).sum())
        return p

    def replicate_table(self, rep):
        """(class_counts, overflow counts) as pa_quant_bootstrap_counts gives them"""
        return bm.replicate_table(edge_index(self.T)[1], self.words, rep)


def layouts(p):
    """entities per bin of the row layout and of the transcript-slot layout of a Problem: ([rows in bin k], [transcripts in bin k])"""
    def bins(x):
        x = np.asarray(x)
        hi = (1 << 62,) + BIN_MIN[:-1]
        return [int(((x >= BIN_MIN[k]) & (x < hi[k])).sum()) for k in range(5)]
    return bins(p.lens), bins(p.degree[p.degree > 0])


def blocks(per_bin):
    """Layout.blk of quant_state.hpp from the entities per bin"""
    blk = [0]
    for k in range(5):
        blk.append(blk[-1] + (per_bin[k] + PER_BLOCK[k] - 1) // PER_BLOCK[k])
    return blk


def _cached(fn):
    def get(*args):
        key = (fn.__name__,) + args
        if key not in _cache:
            _cache[key] = fn(*args)
        return _cache[key]
    get.__name__, get.__doc__ = fn.__name__, fn.__doc__
    return get


@_cached
def ladder(seed):
    """every L of EDGE as a row length (records of exactly L ids from the pool [0, POOL)), every d of EDGE as a degree (a hub transcript
    outside the pool in exactly d records {x, hub}); counts in 1 .. 5000"""
    rng = np.random.default_rng(1000 + seed)
    recs = {}
    for L in EDGE:
        for _ in range(37 if L < 17 else 3):
            recs[tuple(sorted(rng.choice(POOL, L, replace=False).tolist()))] = int(rng.integers(1, 5001))
    for j, d in enumerate(EDGE):
        for x in rng.choice(POOL, d, replace=False).tolist():
            recs[(x, POOL + j)] = int(rng.integers(1, 5001))
    case = Case.of_records("ladder_%d" % seed, BIG_T, list(recs.items()))
    p = case.problem
    assert set(EDGE) <= set(p.lens.tolist()) and set(EDGE) <= set(p.degree.tolist())
    assert [int(p.degree[POOL + j]) for j in range(len(EDGE))] == EDGE
    rows, slots = layouts(p)
    assert all(rows) and all(slots) and sum(rows) == len(p.rows)
    assert p.m_max == 2049 and p.d_max == 2049
    return case


@_cached
def ladder_small(seed):
    """ladder(seed) with its counts scaled down to N of about 20 000: 64 replicates cost the numpy resampler under 1.3 M draws"""
    case = ladder(seed).scaled(LADDER_BOOT_TARGET)
    assert 19000 <= case.problem.N <= 20312 and np.array_equal(case.problem.lens, ladder(seed).problem.lens)
    return case


SINGLE_BIN_LENS = ([1025, 1026, 2049, 1500], [17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024], [9, 15, 16, 10, 12],
                   [5, 7, 8, 6], [1, 2, 3, 4])
SINGLE_BIN_MULT = (4, 5, 2, 2, 2)      # 4, 20, 32, 64, 128 rows: whole blocks; one more: a last block with one row


@_cached
def single_bin(k, extra=0):
    """every row lies in bin k: PER_BLOCK[k] * SINGLE_BIN_MULT[k] + extra rows whose lengths go round SINGLE_BIN_LENS[k]"""
    rng = np.random.default_rng(2000 + 10 * k + extra)
    n = PER_BLOCK[k] * SINGLE_BIN_MULT[k] + extra
    recs = {}
    i = 0
    while len(recs) < n:
        L = SINGLE_BIN_LENS[k][i % len(SINGLE_BIN_LENS[k])]
        ids = tuple(sorted(rng.choice(BIG_T, L, replace=False).tolist()))
        if ids not in recs:
            recs[ids] = int(rng.integers(1, 5001))
            i += 1
    case = Case.of_records("single_bin_%d+%d" % (k, extra), BIG_T, list(recs.items()))
    p = case.problem
    rows, _ = layouts(p)
    assert rows == [n if j == k else 0 for j in range(5)]
    assert blocks(rows) == [0] * (k + 1) + [SINGLE_BIN_MULT[k] + extra] * (5 - k)
    assert n % PER_BLOCK[k] == (extra if PER_BLOCK[k] > 1 else 0)
    assert set(SINGLE_BIN_LENS[k]) <= set(p.lens.tolist())
    return case


@_cached
def mixed_candidates(big=None):
    """counts on index classes and on overflow records; in the middle of the records one with count 0 and one without ids; a record whose
    ids are those of a counted index class; one record with all the other reads of N = 2^53 - 1 (big: that record's count instead)"""
    _, arr, _ = edge_index(BIG_T)
    rng = np.random.default_rng(3000)
    C = arr["num_classes"]
    eo, ei = arr["ec_offset"].astype(np.int64), arr["ec_ids"]
    counts = np.zeros(C + 3, np.uint64)
    picked = np.flatnonzero(rng.random(C) < 0.4)
    counts[picked] = rng.integers(1, 5001, len(picked)).astype(np.uint64)
    pair = int(picked[np.flatnonzero(np.diff(eo)[picked] == 2)[0]])         # a counted class of two transcripts

    def rec(lo, hi):
        return tuple(sorted(rng.choice(BIG_T, int(rng.integers(lo, hi + 1)), replace=False).tolist())), int(rng.integers(1, 5001))

    recs = [rec(1, 40) for _ in range(20)]
    zero_at, empty_at, same_at = len(recs), len(recs) + 1, len(recs) + 2
    recs += [(rec(4, 4)[0], 0), ((), 11), (tuple(int(x) for x in ei[eo[pair]:eo[pair + 1]]), 77)]
    recs += [rec(1, 40) for _ in range(20)]
    assert len({ids for ids, _ in recs}) == len(recs)
    rest = int(counts[:C].sum()) + sum(c for ids, c in recs if len(ids))
    big_at = len(recs)
    recs.append((rec(5, 5)[0], 2 ** 53 - 1 - rest if big is None else big))
    counts[C] = sum(c for _, c in recs)
    counts[C + 1], counts[C + 2] = 5, 9                                       # the tail slots never take part
    case = Case("mixed_candidates" if big is None else "mixed_candidates/%d" % big, BIG_T, counts, words_in_order(recs))
    case.at = dict(zero=zero_at, empty=empty_at, same=same_at, big=big_at, pair=pair)
    p = case.problem
    back = qm.read_overflow(case.words)
    assert back[zero_at][1] == 0 and len(back[zero_at][0]) == 4 and len(back[empty_at][0]) == 0 and back[empty_at][1] == 11
    assert 0 < zero_at < empty_at < len(recs) - 1
    assert counts[pair] > 0 and back[same_at][0].tolist() == ei[eo[pair]:eo[pair + 1]].tolist()
    assert len(p.rows) == len(picked) + len(recs) - 2 and (case.cand > 0).sum() == len(p.rows)
    assert p.N == (2 ** 53 - 1 if big is None else rest + big)
    return case


@_cached
def tiny(T, zero=False):
    """T = 1: one class with count 7, or the zero table; T = 2: rows {0}, {1}, {0, 1}"""
    _, arr, _ = edge_index(T)
    C = arr["num_classes"]
    eo, ei = arr["ec_offset"].astype(np.int64), arr["ec_ids"]
    counts = np.zeros(C + 3, np.uint64)
    if zero:
        return Case("tiny_%d_zero" % T, T, counts, qm.write_overflow([]))
    if T == 1:
        assert C == 1 and ei[eo[0]:eo[1]].tolist() == [0]
        counts[0] = 7
        case = Case("tiny_1", 1, counts, None)
        assert case.problem.N == 7 and [r.tolist() for r in case.problem.rows] == [[0]]
        return case
    assert T == 2
    case = Case.of_records("tiny_2", 2, [((0,), 30), ((1,), 5), ((0, 1), 100)])
    assert [r.tolist() for r in case.problem.rows] == [[0], [0, 1], [1]] and case.problem.N == 135
    return case


DRAW_ROWS = (1, 2, 1023, 1024, 1025, 2047, 2048, 2049, 4096, 4097, 6000)
DRAW_READS = (1, 2, 3, 511, 512, 513, 16383, 16384, 16385, 32769)
DRAW_CASES = [("rows", R, v) for R in DRAW_ROWS for v in ("heavy", "threes")] + [("reads", N, v) for N in DRAW_READS for v in ("seven", "each")]
FALLBACK = ("rows", 6000, "threes")     # more than HT_SLOTS distinct rows in a workgroup's draws: the direct atomics run


def _nth_ids(i):
    """distinct sorted id lists: the singletons {i}, then pairs"""
    if i < BIG_T:
        return (i,)
    j = i - BIG_T
    return (j % 6000, j % 6000 + 1 + j // 6000)


@_cached
def draw_table(kind, x, variant):
    """rows: x single-id records {t}, t < x, with count 1 and one heavy row in the middle (heavy), or all 3 (threes).
    reads: x reads over 7 records (seven; a record without reads where x < 7) or one read in each of x records (each)"""
    if kind == "rows":
        recs = [((t,), 3 if variant == "threes" else 1000 if t == x // 2 else 1) for t in range(x)]
        want_rows, want_N = x, 3 * x if variant == "threes" else x + 999
    elif variant == "seven":
        recs = [((t,), x // 7 + (1 if t < x % 7 else 0)) for t in range(7)]
        want_rows, want_N = min(x, 7), x
    else:
        recs = [(_nth_ids(i), 1) for i in range(x)]
        want_rows, want_N = x, x
    case = Case.of_records("draw_%s_%d_%s" % (kind, x, variant), BIG_T, recs)
    p = case.problem
    assert len(p.rows) == want_rows and p.N == want_N
    return case


def fallback_replicates():
    """the replicates the GPU tests draw of FALLBACK"""
    return sorted(set(range(5)) | {HIGH + k for k in range(5)} | {32, 62, 63})


def distinct_rows_of_the_first_workgroup(case, b):
    """distinct rows among the first DRAWS_PER_WORKGROUP draws of replicate b"""
    cand = case.cand
    N = int(cand.sum())
    p = bm.picks(bm.draw_values(SEED, b, min(N, DRAWS_PER_WORKGROUP)), N)
    cum = np.concatenate([[0], np.cumsum(cand, dtype=np.uint64)]).astype(np.uint64)
    return len(np.unique(np.searchsorted(cum, p, side="right") - 1))


def step_cases():
    """the cases of the point-estimate suite"""
    out = [ladder(0), ladder(1)] + [single_bin(k, e) for k in range(5) for e in (0, 1)] + [mixed_candidates(), tiny(1), tiny(1, True), tiny(2)]
    return {c.name: c for c in out}


STEP_CASE_NAMES = ["ladder_0", "ladder_1"] + ["single_bin_%d+%d" % (k, e) for k in range(5) for e in (0, 1)] + ["mixed_candidates", "tiny_1", "tiny_1_zero", "tiny_2"]
MIXED_BOOT_BIG = 30000
