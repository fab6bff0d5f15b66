"""The abundance EM over equivalence classes, in numpy, written from the rules in include/pseudoaligner_amd.h (section "transcript
abundances") and from nothing else: the yardstick of tests/test_gpu_quant.py. Twice: in float64, and in np.longdouble (x87 extended
on x86-64, 64-bit mantissa) so that the float64 model's own order noise can be measured. Also: a reader of the serialised overflow
format and a seeded generator of count tables over a host index."""
import math

import numpy as np

DEFAULTS = dict(mean_read_len=0.0, alpha_limit=1e-7, alpha_change_limit=1e-2, alpha_change=1e-2, min_iters=50, max_iters=10000, check_every=10)
EPS = 2.0 ** -53


def read_overflow(words):
    """serialised overflow words -> [(ids uint32 array, count)] in record order"""
    if words is None or len(words) < 2:
        return []
    words = np.asarray(words, np.uint32)
    out, p = [], 2
    for _ in range(int(words[0])):
        n = int(words[p])
        out.append((words[p + 3:p + 3 + n].copy(), int(words[p + 1]) | (int(words[p + 2]) << 32)))
        p += 3 + n
    assert p == int(words[1]) == len(words)
    return out


def write_overflow(records):
    """[(sorted ids, count)] -> serialised words, in the canonical (lexicographic) order"""
    w = [0, 0]
    for ids, c in sorted(((tuple(int(x) for x in i), int(c)) for i, c in records)):
        w += [len(ids), c & 0xFFFFFFFF, c >> 32] + list(ids)
    w[0], w[1] = len(records), len(w)
    return np.array(w, np.uint32)


def effective_lengths(tx_len, mean_read_len=0.0):
    tx_len = np.asarray(tx_len, np.float64)
    return np.maximum(tx_len - mean_read_len + 1.0, 1.0) if mean_read_len > 0 else np.maximum(tx_len, 1.0)


class Problem:
    """the reduced problem: rows (id lists, counts) over T transcripts with effective lengths eff"""

    def __init__(self, rows, counts, eff):
        keep = [i for i, (r, c) in enumerate(zip(rows, counts)) if c > 0 and len(r) > 0]
        self.rows = [np.asarray(rows[i], np.int64) for i in keep]
        self.n = np.array([counts[i] for i in keep], np.float64)            # exact below 2^53
        assert all(counts[i] < 2 ** 53 for i in keep)
        self.eff = np.asarray(eff, np.float64)
        self.T = len(self.eff)
        self.lens = np.array([len(r) for r in self.rows], np.int64)
        self.off = np.concatenate([[0], np.cumsum(self.lens)]).astype(np.int64)
        self.ids = np.concatenate(self.rows).astype(np.int64) if self.rows else np.zeros(0, np.int64)
        self.row_of = np.repeat(np.arange(len(self.rows)), self.lens)
        self.N = int(sum(counts[i] for i in keep))
        self.degree = np.bincount(self.ids, minlength=self.T)
        self.m_max = int(self.lens.max()) if len(self.rows) else 0
        self.d_max = int(self.degree.max()) if len(self.rows) else 0

    @classmethod
    def from_table(cls, arrays, tx_len, class_counts, overflow_words=None, mean_read_len=0.0):
        """arrays: HostIndex.arrays(); the tail slots never take part, the novel slot only through the overflow records"""
        C = arrays["num_classes"]
        assert len(class_counts) == C + 3
        eo, ei = arrays["ec_offset"].astype(np.int64), arrays["ec_ids"]
        rows = [ei[eo[c]:eo[c + 1]] for c in np.flatnonzero(np.asarray(class_counts[:C]) > 0)]
        counts = [int(class_counts[c]) for c in np.flatnonzero(np.asarray(class_counts[:C]) > 0)]
        if overflow_words is not None:
            recs = read_overflow(overflow_words)
            assert sum(c for _, c in recs) == int(class_counts[C]), "overflow total != novel slot"
            rows += [r for r, _ in recs]
            counts += [c for _, c in recs]
        return cls(rows, counts, effective_lengths(tx_len, mean_read_len))

    def start(self):
        return np.where(self.degree > 0, self.N / self.T, 0.0) if self.N else np.zeros(self.T)

    def step(self, alpha, dtype=np.float64):
        """one iteration from alpha, every operation in dtype"""
        if not len(self.rows):
            return np.zeros(self.T, dtype)
        alpha = np.asarray(alpha, dtype)
        w = alpha / self.eff.astype(dtype)
        d = np.add.reduceat(w[self.ids], self.off[:-1])
        with np.errstate(divide="ignore", invalid="ignore"):
            q = np.where(d > 0, self.n.astype(dtype) / d, dtype(0))
        s = np.zeros(self.T, dtype)
        if dtype == np.float64:
            s = np.bincount(self.ids, weights=q[self.row_of], minlength=self.T)
        else:
            np.add.at(s, self.ids, q[self.row_of])
        return w * s

    def step_exact_sums(self, alpha):
        """one iteration in long double with correctly rounded row and column sums (math.fsum over hi + lo parts); small problems only"""
        L = np.longdouble
        w = np.asarray(alpha, L) / self.eff.astype(L)
        q = np.zeros(len(self.rows), L)
        for r, ids in enumerate(self.rows):
            d = fsum_ld(w[ids])
            q[r] = L(self.n[r]) / d if d > 0 else L(0)
        out = np.zeros(self.T, L)
        by_t = [[] for _ in range(self.T)]
        for r, ids in enumerate(self.rows):
            for t in ids:
                by_t[t].append(q[r])
        for t in range(self.T):
            out[t] = w[t] * fsum_ld(by_t[t]) if by_t[t] else L(0)
        return out

    def iterate(self, n_iters, dtype=np.float64, alpha=None):
        a = np.asarray(self.start() if alpha is None else alpha, dtype)
        for _ in range(n_iters):
            a = self.step(a, dtype)
        return a

    def loglik(self, alpha):
        """sum n_c log d_c of a float64 alpha, evaluated in long double, summed with math.fsum"""
        L = np.longdouble
        w = np.asarray(alpha, L) / self.eff.astype(L)
        d = np.add.reduceat(w[self.ids], self.off[:-1])
        terms = self.n.astype(L) * np.log(d)
        return fsum_ld(terms)

    def step_bound(self):
        """relative error bound of one computed alpha'_t against the exact one"""
        return (self.m_max + self.d_max + 4) * EPS


def fsum_ld(values):
    """sum of long doubles: math.fsum over their float64 high and low parts (exact up to the final rounding and the 2^-106 tails)"""
    v = np.asarray(values, np.longdouble)
    hi = v.astype(np.float64)
    lo = (v - hi.astype(np.longdouble)).astype(np.float64)
    return np.longdouble(math.fsum(hi)) + np.longdouble(math.fsum(lo))


def stop_rule_holds(prev, new, alpha_change_limit=1e-2, alpha_change=1e-2):
    """no transcript has both new > alpha_change_limit and |new - prev| / new > alpha_change"""
    prev, new = np.asarray(prev, np.float64), np.asarray(new, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        moved = (new > alpha_change_limit) & (np.abs(new - prev) / new > alpha_change)
    return not moved.any()


def tpm(alpha, eff):
    """the denominator summed in transcript order"""
    den = 0.0
    w = np.asarray(alpha, np.float64) / np.asarray(eff, np.float64)
    for x in w:
        den += float(x)
    return 1e6 * w / den if den > 0 else np.zeros(len(w))


def random_table(arrays, seed, class_fraction=0.3, n_overflow=60, max_count=5000, hub=None, hub_records=0, overflow_len=(2, 6)):
    """seeded count table over a host index: counts on a fraction of the index classes + random sorted id sets as overflow records
    (hub / hub_records: that many further records all holding transcript `hub`: a transcript of very large degree).
    -> (class_counts u64[C + 3], overflow words)"""
    rng = np.random.default_rng(seed)
    C, T = arrays["num_classes"], arrays["num_transcripts"]
    counts = np.zeros(C + 3, np.uint64)
    picked = np.flatnonzero(rng.random(C) < class_fraction)
    counts[picked] = rng.integers(1, max_count, len(picked)).astype(np.uint64)
    recs = {}
    while len(recs) < n_overflow and T >= overflow_len[0]:
        k = int(rng.integers(overflow_len[0], min(overflow_len[1], T) + 1))
        recs[tuple(sorted(rng.choice(T, k, replace=False).tolist()))] = int(rng.integers(1, max_count))
    target = len(recs) + hub_records
    while len(recs) < target:
        k = int(rng.integers(1, 4))
        recs[tuple(sorted(set(rng.choice(T, k, replace=False).tolist()) | {int(hub)}))] = int(rng.integers(1, max_count))
    counts[C] = sum(recs.values())
    counts[C + 1], counts[C + 2] = rng.integers(0, 1000, 2).astype(np.uint64)
    return counts, write_overflow(list(recs.items()))


def multi_fraction(arrays, counts, words):
    """share of the counted reads that lie in rows of at least two transcripts"""
    C = arrays["num_classes"]
    lens = np.diff(arrays["ec_offset"].astype(np.int64))
    recs = read_overflow(words)
    multi = int(counts[:C][lens >= 2].sum()) + sum(c for r, c in recs if len(r) >= 2)
    total = int(counts[:C].sum()) + sum(c for _, c in recs)
    return multi / max(total, 1)
