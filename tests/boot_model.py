"""The bootstrap resampler in numpy, written from the rules in include/pseudoaligner_amd.h (section "bootstrap replicates") and from
nothing else: Philox4x32-10, the draws of a replicate, its counts per candidate, and the replicate as a table that quant_model.Problem
reads. Everything is integer: the GPU's counts must equal these bit for bit (tests/test_gpu_quant_boot.py)."""
import numpy as np

import quant_model as qm

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)


def philox4x32_10(counter, key):
    """counter: four arrays (or scalars) of 32-bit words, key: two 32-bit words -> four uint64 arrays holding 32-bit words"""
    c = [np.atleast_1d(np.asarray(x, np.uint64)) & MASK for x in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]                        # 32 x 32 bits: exact in 64
        c = [(p1 >> S32) ^ c[1] ^ np.uint64(k0), p1 & MASK, (p0 >> S32) ^ c[3] ^ np.uint64(k1), p0 & MASK]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return c


def draw_values(seed, b, N):
    """x_j for j = 0 .. N - 1 of replicate b (uint64): block j >> 1, even j the low pair, odd j the high pair"""
    blocks = (N + 1) // 2
    i = np.arange(blocks, dtype=np.uint64)
    o = philox4x32_10((i & MASK, i >> S32, b, 0), (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    x = np.empty(2 * blocks, np.uint64)
    x[0::2] = o[0] | (o[1] << S32)
    x[1::2] = o[2] | (o[3] << S32)
    return x[:N]


def picks(x, N):
    """(x * N) >> 64 for N < 2^32, in 64-bit pieces: x = h 2^32 + l  ->  (h N + (l N >> 32)) >> 32 (no piece overflows)"""
    assert 0 < N < 2 ** 32
    x = np.asarray(x, np.uint64)
    n = np.uint64(N)
    return ((x >> S32) * n + (((x & MASK) * n) >> S32)) >> S32


def candidate_counts(arrays, class_counts, overflow_words):
    """the reads of every candidate in candidate order (the index classes ascending, then the overflow records in record order); a
    candidate without entries owns none"""
    C = arrays["num_classes"]
    lens = np.diff(arrays["ec_offset"].astype(np.int64))
    n = np.where(lens > 0, np.asarray(class_counts[:C], np.uint64), np.uint64(0)).astype(np.uint64)
    recs = qm.read_overflow(overflow_words) if overflow_words is not None else []
    o = np.array([c if len(ids) else 0 for ids, c in recs], np.uint64)
    return np.concatenate([n, o]).astype(np.uint64)


def resample(cand, seed, b):
    """counts per candidate of replicate b of a table with the candidate counts `cand`"""
    cand = np.asarray(cand, np.uint64)
    N = int(cand.sum())
    if N == 0:
        return np.zeros(len(cand), np.uint64)
    return counts_of_picks(cand, picks(draw_values(seed, b, N), N))


def counts_of_picks(cand, p):
    cum = np.concatenate([[0], np.cumsum(np.asarray(cand, np.uint64), dtype=np.uint64)]).astype(np.uint64)
    owner = np.searchsorted(cum, np.asarray(p, np.uint64), side="right") - 1       # the last candidate with cum_i <= p: it is never an empty one
    return np.bincount(owner, minlength=len(cand)).astype(np.uint64)[: len(cand)]


def replicate_table(arrays, overflow_words, rep):
    """counts per candidate -> (class_counts u64[C + 3], overflow counts u64[records]) as pa_quant_bootstrap_counts gives them"""
    C = arrays["num_classes"]
    cc = np.zeros(C + 3, np.uint64)
    cc[:C] = rep[:C]
    oc = np.asarray(rep[C:], np.uint64)
    cc[C] = oc.sum()
    return cc, oc


def overflow_with_counts(words, counts):
    """the serialised overflow records with other counts (the order of the records stays)"""
    if words is None:
        return None
    w = np.array(words, np.uint32)
    p = 2
    for r in range(int(w[0])):
        w[p + 1], w[p + 2] = int(counts[r]) & 0xFFFFFFFF, int(counts[r]) >> 32
        p += 3 + int(w[p])
    return w
