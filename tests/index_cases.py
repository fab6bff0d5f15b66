"""Designed transcriptomes for the index builders (csrc/index_build.hip on the GPU, csrc/dbg_build.cpp on the CPU): pure Python / numpy, no product code.
Every case is built to take one named path of the GPU builder and carries the index it must give:

  long_unitig             one transcript whose k-mers are all distinct: more distinct k-mers than one trip of pa_ib_jump_kernel's capped grid covers, a
                          unitig of 2^21 k-mers (22 jump rounds). Closed form: one node that IS the transcript.
  long_unitig_and_cycles  the same beside a 2-cycle of joinable k-mers and a self-loop: cycle members keep moving while the chain resolves.
  id_edge                 2^24 - 1 transcripts, all empty but four; identical transcripts at ids 0 and 2^24 - 2, so that one class spans both ends.
  empties                 empty transcripts (and transcripts of k - 1 bases) first, last and in runs: the binary search of pa_ib_enum_kernel.
  lengths                 transcripts of k - 1, k, k + 1 and 2k - 1 bases; total_bases % 32 in {0, 1, 31}; the last k-mer ends on the last base; every
                          word behind the packed words is all ones.
  alignment               about 160 one-node transcripts: node_start % 32 takes all 32 values, first k-mers that spill into a second and third word.
  hub                     a poly-A tail: one k-mer with 102 000 occurrence records and a class of 600 ids.
  retry                   55 classes whose WEAK set hashes (2 bits per addend: the knobs build of index_build.hip) collide on each of four attempts.

The expectation comes from test_index_build.naive_graph (ids mapped where only a few transcripts are not empty) or from the closed form; where the graph has
no pure cycle, expected_arrays() also restates the builders' numbering (nodes by hash partition of the first k-mer, then by k-mer; classes in
lexicographic order of their id lists) and gives the flat index array for array. check(case) asserts, on the model's side, that the case has the shape it
was built for."""
from functools import lru_cache

import numpy as np

from test_index_build import naive_graph, random_txome

M64 = (1 << 64) - 1
GUARD_WORDS = 8                      # words of all ones behind the packed words of every case
ACGT = np.frombuffer(b"ACGT", np.uint8)
CODE_OF = np.zeros(256, np.uint8)
CODE_OF[ACGT] = np.arange(4, dtype=np.uint8)

# ---- the set hash of the colour stage (index_build.hip), restated; tests/test_index_cases.py reads the constants back from the source ----
SEED0 = 0x243f6a8885a308d3
ATTEMPTS = 4
WEAK_MASK = 3


def mix64(x):
    """murmur3 fmix64 (pa_mix64)"""
    x &= M64
    x ^= x >> 33
    x = (x * 0xff51afd7ed558ccd) & M64
    x ^= x >> 33
    x = (x * 0xc4ceb9fe1a85ec53) & M64
    x ^= x >> 33
    return x


def seeds():
    out = [SEED0]
    for a in range(ATTEMPTS - 1):
        out.append(mix64(out[-1] + a + 1))
    return out


def set_hash(ids, seed, mask=M64):
    return sum(mix64(t + seed) & mask for t in ids) & M64


# ---- packing ----
def codes_of(s):
    return CODE_OF[np.frombuffer(s.encode(), np.uint8)]


def text_of(codes):
    return ACGT[codes].tobytes().decode()


def pack_codes(codes):
    """-> a view of exactly (n + 31) // 32 words into a buffer whose following words are all ones; the unused high bits of the last word are zero"""
    n = len(codes)
    nw = (n + 31) // 32
    buf = np.full(nw + GUARD_WORDS, M64, np.uint64)
    padded = np.zeros(nw * 32, np.uint64)
    padded[:n] = codes
    if nw:
        buf[:nw] = np.bitwise_or.reduce(padded.reshape(nw, 32) << (np.arange(32, dtype=np.uint64) * np.uint64(2)), axis=1)
    return buf[:nw]


def unpack(words, start, n):
    pos = np.arange(start, start + n, dtype=np.int64)
    return ((words[pos >> 5] >> ((pos & 31) * 2).astype(np.uint64)) & np.uint64(3)).astype(np.uint8)


def kmer_words(codes, k):
    """(lo, hi) of every k-mer of `codes`: base j of the k-mer in bits 2j, as the builders hold it"""
    n = len(codes) - k + 1
    c = codes.astype(np.uint64)
    lo, hi = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
    for j in range(k):
        (lo if j < 32 else hi)[:] |= c[j:j + n] << np.uint64(2 * (j & 31))
    return lo, hi


def kmer_value(s):
    return sum(int(c) << (2 * j) for j, c in enumerate(codes_of(s)))


def partition_of(km, k, logp):
    """DKmer::hash >> (64 - logp): the hash partition that leads the node order"""
    h = mix64(km) if k <= 32 else mix64((km & M64) ^ ((mix64(km >> 64) * 0x9e3779b97f4a7c15) & M64))
    return h >> (64 - logp)


def logp_of(n_occ):
    logp = 4
    while logp < 12 and (n_occ >> logp) > (1 << 20):
        logp += 1
    return logp


# ---- a case ----
class Case:
    """placed = [(transcript id, sequence)], ids ascending; every other transcript of the num_tx is empty"""

    def __init__(self, name, k, placed, num_tx=None, nodes=None, cyc=None):
        self.name, self.k = name, k
        self.ids = [t for t, _ in placed]
        self.seqs = [s for _, s in placed]
        self.num_tx = len(placed) if num_tx is None else num_tx
        assert self.ids == sorted(set(self.ids)) and (not self.ids or self.ids[-1] < self.num_tx)
        lens = np.zeros(self.num_tx, np.uint64)
        lens[self.ids] = [len(s) for s in self.seqs]
        self.tx_start = np.zeros(self.num_tx + 1, np.uint64)
        np.cumsum(lens, out=self.tx_start[1:])
        self.codes = np.concatenate([codes_of(s) for s in self.seqs]) if self.seqs else np.zeros(0, np.uint8)
        self.total_bases = int(self.tx_start[-1])
        self.words = pack_codes(self.codes)
        self.n_occ = sum(max(0, len(s) - k + 1) for s in self.seqs)
        if nodes is None:
            nodes, cyc = naive_graph(self.seqs, k)
            nodes = {(s, tuple(self.ids[i] for i in cl), le, re) for s, cl, le, re in nodes}
        self.nodes, self.cyc = nodes, cyc
        self.arrays = expected_arrays(nodes, k, self.n_occ) if not cyc else None

    def classes(self):
        """k-mer -> sorted tuple of the transcripts that hold it"""
        col = {}
        for t, s in zip(self.ids, self.seqs):
            for p in range(len(s) - self.k + 1):
                col.setdefault(s[p:p + self.k], set()).add(t)
        return {km: tuple(sorted(v)) for km, v in col.items()}


def expected_arrays(nodes, k, n_occ):
    """the flat index of a node set without pure cycles, in the builders' numbering"""
    logp = logp_of(n_occ)
    keyed = sorted((partition_of(kmer_value(s[:k]), k, logp), kmer_value(s[:k]), s, cl, le, re) for s, cl, le, re in nodes)
    lists = sorted({cl for _, cl, _, _ in nodes})
    number = {cl: i for i, cl in enumerate(lists)}
    bits = lambda e: sum(1 << "ACGT".index(ch) for ch in e)
    node_len = np.array([len(s) for _, _, s, _, _, _ in keyed], np.uint32)
    node_start = np.zeros(len(keyed) + 1, np.uint64)
    np.cumsum(node_len, out=node_start[1:])
    seq = pack_codes(np.concatenate([codes_of(s) for _, _, s, _, _, _ in keyed]) if keyed else np.zeros(0, np.uint8))
    ec_offset = np.zeros(len(lists) + 1, np.uint64)
    np.cumsum([len(cl) for cl in lists], out=ec_offset[1:])
    return dict(node_seq=np.append(seq, np.uint64(0)), node_start=node_start, node_len=node_len,
                node_exts=np.array([bits(le) << 4 | bits(re) for _, _, _, _, le, re in keyed], np.uint8),
                node_colour=np.array([number[cl] for _, _, _, cl, _, _ in keyed], np.uint32), ec_offset=ec_offset,
                ec_ids=np.array([t for cl in lists for t in cl], np.uint32))


def graph_from_arrays(a):
    """test_index_build.graph_of for indexes with nodes of millions of bases: one vectorised decode -> [(sequence, id list, left exts, right exts)]"""
    text = text_of(unpack(a["node_seq"], 0, int(a["node_start"][-1])))
    out = []
    for n in range(a["num_nodes"]):
        s, c, e = int(a["node_start"][n]), int(a["node_colour"][n]), int(a["node_exts"][n])
        cl = tuple(a["ec_ids"][int(a["ec_offset"][c]):int(a["ec_offset"][c + 1])].tolist())
        out.append((text[s:s + int(a["node_len"][n])], cl, "".join("ACGT"[b] for b in range(4) if e >> (4 + b) & 1), "".join("ACGT"[b] for b in range(4) if e >> b & 1)))
    return out


def rand_seq(rng, n):
    return text_of(rng.integers(0, 4, n, dtype=np.uint8))


def all_kmers_distinct(seqs, k):
    kms = [s[p:p + k] for s in seqs for p in range(len(s) - k + 1)]
    return len(kms) == len(set(kms))


# ---- the cases ----
LONG = {31: (1 << 21) + 5000, 33: (1 << 18) + 77}
CYCLES = ["AC" * 40, "CA" * 37, "A" * 70]
ID_EDGE_TX = (1 << 24) - 1
EMPTIES_K = (8, 33)
LENGTHS_K = (8, 31, 32, 33, 63, 64)
LENGTHS_MOD = (0, 1, 31)
ALIGNMENT_K = (31, 32, 33, 63, 64)
HUB_TX, HUB_TAIL, HUB_MOTIF = 600, 200, 45


def long_transcript(k):
    return rand_seq(np.random.default_rng(1000 + k), LONG[k])


def one_node(s):
    return {(s, (0,), "", "")}


def long_unitig(k):
    s = long_transcript(k)
    return Case("long_unitig-k%d" % k, k, [(0, s)], nodes=one_node(s), cyc=set())


def long_unitig_and_cycles():
    s, k = long_transcript(31), 31
    nodes, cyc = naive_graph([""] + CYCLES, k)
    return Case("long_unitig_and_cycles", k, [(0, s)] + list(enumerate(CYCLES, 1)), nodes=one_node(s) | nodes, cyc=cyc)


def id_edge_segments(k):
    rng = np.random.default_rng(2000 + k)
    return [rand_seq(rng, n) for n in (90, 70, 120, 64)]


def id_edge(k, num_tx=ID_EDGE_TX):
    s0, s1, s2, s3 = id_edge_segments(k)
    return Case("id_edge-k%d" % k, k, [(0, s0 + s1), (1, s2), (num_tx - 2, s1 + s3), (num_tx - 1, s0 + s1)], num_tx=num_tx)


def empties(k, short):
    rng = np.random.default_rng(3000 + k)
    S, T = rand_seq(rng, 3 * k + 5), rand_seq(rng, 2 * k + 3)
    gap = (lambda: rand_seq(rng, k - 1)) if short else (lambda: "")
    seqs = [gap(), gap(), S, gap(), T, gap(), gap()]
    return Case("empties-k%d-%s" % (k, "short" if short else "empty"), k, list(enumerate(seqs)))


def lengths(k, mod):
    """filler, then the four lengths rotated so that a transcript of at least k bases comes last; the filler's length sets total_bases % 32"""
    rng = np.random.default_rng(4000 + 100 * k + mod)
    four = [rand_seq(rng, n) for n in (k - 1, k, k + 1, 2 * k - 1)]
    r = LENGTHS_MOD.index(mod)
    four = four[r + 2:] + four[:r + 2]          # last: k, k + 1, 2k - 1
    fill = (mod - sum(len(s) for s in four)) % 32 or 32
    seqs = [rand_seq(rng, fill)] + four
    return Case("lengths-k%d-mod%d" % (k, mod), k, list(enumerate(seqs)))


def alignment(k):
    """the node order follows the hashes of the first k-mers: the first seed whose order puts a node at every alignment"""
    for seed in range(5000 + k, 5000 + k + 100 * 50, 100):
        rng = np.random.default_rng(seed)
        c = Case("alignment-k%d" % k, k, list(enumerate(rand_seq(rng, k + (i % 41)) for i in range(160))))
        if len(set((c.arrays["node_start"][:-1] % np.uint64(32)).tolist())) == 32:
            return c
    raise AssertionError("alignment K=%d: no seed reaches all 32 alignments" % k)


def hub():
    rng = np.random.default_rng(6000)
    motif = rand_seq(rng, HUB_MOTIF)
    seqs = [rand_seq(rng, 40) + motif + "CGT"[i % 3] + "A" * HUB_TAIL for i in range(HUB_TX)]
    return Case("hub", 31, list(enumerate(seqs)))


def retry():
    return Case("retry", 16, list(enumerate(random_txome(np.random.RandomState(7), 25))))


NAMES = (["long_unitig-k31", "long_unitig-k33", "long_unitig_and_cycles"] + ["id_edge-k%d" % k for k in (20, 40)] +
         ["empties-k%d-%s" % (k, v) for k in EMPTIES_K for v in ("empty", "short")] + ["lengths-k%d-mod%d" % (k, m) for k in LENGTHS_K for m in LENGTHS_MOD] +
         ["alignment-k%d" % k for k in ALIGNMENT_K] + ["hub", "retry"])
BIG = ("long_unitig-k31", "long_unitig-k33", "long_unitig_and_cycles")   # decoded by graph_from_arrays


@lru_cache(maxsize=2)   # (id_edge holds 128 MB of tx_start)
def case(name):
    family, _, rest = name.partition("-")
    args = rest.split("-") if rest else []
    k = int(args[0][1:]) if args else None
    if family == "long_unitig":
        return long_unitig(k)
    if family == "id_edge":
        return id_edge(k)
    if family == "empties":
        return empties(k, args[1] == "short")
    if family == "lengths":
        return lengths(k, int(args[1][3:]))
    if family == "alignment":
        return alignment(k)
    return {"long_unitig_and_cycles": long_unitig_and_cycles, "hub": hub, "retry": retry}[family]()


# ---- the colour stage under the weak hash ----
def verify_model(classes, seed, mask):
    """pa_ib_verify_kernel on the runs of equal set hash: the run's representative is its smallest k-mer -> (k-mers whose count differs from the
    representative's, k-mers of the same count and another list, runs that hold different lists of one length, runs that mix lengths)"""
    h_of = {}
    runs = {}
    for km, cl in classes.items():
        if cl not in h_of:
            h_of[cl] = set_hash(cl, seed, mask)
        runs.setdefault(h_of[cl], []).append((kmer_value(km), cl))
    by_count = by_content = same_len = mixed = 0
    for members in runs.values():
        rep = min(members)[1]
        by_count += sum(1 for _, cl in members if len(cl) != len(rep))
        by_content += sum(1 for _, cl in members if len(cl) == len(rep) and cl != rep)
        lens = [len(cl) for cl in {cl for _, cl in members}]
        same_len += len(lens) > len(set(lens))
        mixed += len(set(lens)) > 1
    return by_count, by_content, same_len, mixed


# ---- the shape each case was built for ----
def check(c):
    family = c.name.partition("-")[0]
    k = c.k
    assert len(c.words) == (c.total_bases + 31) // 32 and (c.words.base[len(c.words):] == np.uint64(M64)).all() and len(c.words.base) - len(c.words) == GUARD_WORDS
    if c.total_bases % 32:
        assert int(c.words[-1]) >> (2 * (c.total_bases % 32)) == 0
    assert np.array_equal(unpack(c.words, 0, c.total_bases), c.codes)
    if family in ("long_unitig", "long_unitig_and_cycles"):
        L = LONG[k]
        lo, hi = kmer_words(c.codes[:L], k)
        assert L - k + 1 > 8192 * 256 or k == 33            # more distinct k-mers than one trip of the jump kernel's capped grid
        assert (k == 31) == (L - k + 1 >= 1 << 21)
        pairs = np.unique(lo) if k <= 32 else np.unique(np.stack([lo, hi], 1), axis=0)
        assert len(pairs) == L - k + 1                      # all distinct: one unitig
        a = expected_arrays(one_node(c.seqs[0]), k, L - k + 1)
        assert a["node_len"].tolist() == [L] and a["node_start"].tolist() == [0, L] and a["node_exts"].tolist() == [0] and a["node_colour"].tolist() == [0]
        assert a["ec_offset"].tolist() == [0, 1] and a["ec_ids"].tolist() == [0] and np.array_equal(a["node_seq"][:-1], pack_codes(c.codes[:L]))
        if family == "long_unitig":
            assert not c.cyc and all(np.array_equal(a[key], c.arrays[key]) for key in a)
        else:
            rest = {kmer_value(s[p:p + k]) for s in CYCLES for p in range(len(s) - k + 1)}
            assert not np.isin(np.array(sorted(rest), np.uint64), lo).any()     # the long node shares no k-mer with the rest
            assert c.cyc == {("AC" * 16)[:31], ("CA" * 16)[:31]} and ("A" * k, (3,), "A", "A") in c.nodes and len(c.nodes) == 2
    elif family == "id_edge":
        assert c.num_tx == (1 << 24) - 1 and c.ids == [0, 1, (1 << 24) - 3, (1 << 24) - 2] and c.seqs[0] == c.seqs[3]
        assert [len(s) for s in c.seqs] == [160, 120, 134, 160] and not c.cyc
        assert any(cl[0] == 0 and cl[-1] == (1 << 24) - 2 for _, cl, _, _ in c.nodes)   # a class that spans both ends
        assert any(cl == (0, (1 << 24) - 3, (1 << 24) - 2) for _, cl, _, _ in c.nodes)  # (S1: three of the four)
        assert int(c.arrays["ec_ids"].max()) == (1 << 24) - 2
    elif family == "empties":
        lens = [len(s) for s in c.seqs]
        assert [n >= k for n in lens] == [False, False, True, False, True, False, False] and not c.cyc
        assert set(lens) - {lens[2], lens[4]} == ({k - 1} if c.name.endswith("short") else {0})
        assert {t for _, cl, _, _ in c.nodes for t in cl} == {2, 4}
    elif family == "lengths":
        lens = [len(s) for s in c.seqs]
        assert sorted(lens[1:]) == [k - 1, k, k + 1, 2 * k - 1] and lens[-1] >= k and 1 <= lens[0] <= 32
        assert c.total_bases % 32 == int(c.name.rpartition("mod")[2]) and all_kmers_distinct(c.seqs, k) and not c.cyc
        assert {s for s, _, _, _ in c.nodes} == {s for s in c.seqs if len(s) >= k}     # every transcript of k bases or more is one node
        assert c.seqs[-1][-k:] == text_of(c.codes[-k:])                                # the last k-mer ends on the last base
    elif family == "alignment":
        assert [len(s) for s in c.seqs] == [k + i % 41 for i in range(160)] and all_kmers_distinct(c.seqs, k) and not c.cyc
        assert {s for s, _, _, _ in c.nodes} == set(c.seqs)
        starts = c.arrays["node_start"][:-1].astype(np.int64)
        assert set((starts % 32).tolist()) == set(range(32))
        assert (starts % 32 + min(k, 32) > 32).any()                                   # a first k-mer spills into the next word
        if k > 32:   # ... and into a third (33 bases never do: 31 + 33 = 64; there the 33rd base always lies in the word after the first base's)
            assert ((starts % 32 + k - 1) // 32 == 2).any() if k > 33 else ((starts % 32 + k - 1) // 32 == 1).all()
    elif family == "hub":
        cls = c.classes()
        poly, motif = "A" * k, c.seqs[0][40:40 + HUB_MOTIF]
        assert sum(s.count("A" * HUB_TAIL) for s in c.seqs) == HUB_TX and c.n_occ == HUB_TX * (40 + HUB_MOTIF + 1 + HUB_TAIL - k + 1)
        assert sum(1 for s in c.seqs for p in range(len(s) - k + 1) if s[p:p + k] == poly) == HUB_TX * (HUB_TAIL - k + 1) == 102000
        everyone = tuple(range(HUB_TX))
        assert cls[poly] == everyone and [cls[motif[p:p + k]] for p in range(HUB_MOTIF - k + 1)] == [everyone] * 15
        assert kmer_value(poly) == 0 and not c.cyc        # A^31 sorts first: the representative of its run; its self-loop is no cycle (y != x)
        assert len(c.nodes) > 900
        by_count, by_content, _, _ = verify_model(cls, seeds()[0], WEAK_MASK)
        assert by_count + by_content > 0                  # the weak hash sends it into a second attempt
        assert verify_model(cls, seeds()[1], M64)[:2] == (0, 0)
    elif family == "retry":
        cls = c.classes()
        assert len(set(cls.values())) == 55
        got = [verify_model(cls, s, WEAK_MASK) for s in seeds()]
        assert all(bc > 0 and bt > 0 for bc, bt, _, _ in got), got      # both exits of the verify kernel, on every weak attempt
        assert [g[2] for g in got] == [6, 6, 9, 7] and [g[3] for g in got] == [7, 5, 7, 9], got
        assert all(verify_model(cls, s, M64) == (0, 0, 0, 0) for s in seeds())
    else:
        raise KeyError(c.name)


def weak_failures(c):
    """k-mers that fail the content check on the last weak attempt: the number the builder's error message names"""
    bc, bt, _, _ = verify_model(c.classes(), seeds()[ATTEMPTS - 1], WEAK_MASK)
    return bc + bt
