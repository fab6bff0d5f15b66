"""Read families for the forward step's STAY-IN-BLOCK rule (lane_steps.hpp, fwd_next_block): a lane that goes on in its chain keeps the
128-byte block it holds — window position x up to 255, its node's slot known — when the rest of the read fits the block's 256-base
window, and re-bases to the block 64 bases further otherwise. Which block a base is read from must not be observable, so every family
is mapped by the code under test (emulator / GPU) and compared with the oracle bit for bit. Shared by tests/test_emu_stay_in_block.py
and tests/test_gpu_stay_in_block.py."""
import numpy as np

import helpers

pa = helpers.pa

# chain positions of node ENDS (colour-only cuts): on and around the seams of the 64-base block stride and the block window's last
# sequence word (224..255) and end (256), as seen from block 0 — and, for reads that start 64 / 128 bases later, from blocks 1 and 2
NODE_ENDS = [63, 64, 65, 191, 192, 223, 224, 255, 256, 319, 320]
FORK_ENDS = [255, 256, 257, 319, 320, 321]
SHORT_B = 20          # k-mers of the middle node B of a triple: A | B | C in ONE block, a third node for the step after A and B
TX_LEN = 720          # > 130 (start offsets) + 513 (the longest read)
READ_LENS = [100, 150, 192, 193, 300, 513]


def _rnd(rng, n):
    return "".join(rng.choice(list("ACGT"), n))


def _sub(c, rng):
    return "ACGT"[("ACGT".index(c) + 1 + rng.randint(3)) % 4]


def hand_built_txome(k, tmp_path, seed=1):
    """Transcript triples T, T[c:], T[c + SHORT_B:] — two colour changes, so the chain of T is the nodes A | B | C with A ending at chain
    position e = c + k - 1 and B at e + SHORT_B, for every e of NODE_ENDS that k allows — and FORKS P + X / P + Y whose node P (a chain's
    last node, with right edges) ends at e of FORK_ENDS: its edge slot lies in a block's window only where e - 64 j < 256.
    Returns (host index, [(T, e_A, e_B)], [(P + X, e)])."""
    rng = np.random.RandomState(52000 + 97 * k + seed)
    txs, triples, forks = [], [], []
    for e in NODE_ENDS:
        c = e - (k - 1)
        if c < 1:
            continue
        t = _rnd(rng, TX_LEN)
        txs += [t, t[c:], t[c + SHORT_B:]]
        triples.append((t, e, e + SHORT_B))
    for e in FORK_ENDS:
        p = _rnd(rng, e)
        a, b = "A" + _rnd(rng, 300), "C" + _rnd(rng, 300)
        txs += [p + a, p + a, p + b]                   # (the first branch is the favoured one)
        forks.append((p + a, e))
        forks.append((p + b, e))
    fa = tmp_path / ("stay_k%d.fa" % k)
    fa.write_text("".join(">t%d|g%d\n%s\n" % (i, i, s) for i, s in enumerate(txs)))
    return pa.HostIndex.build_fasta(str(fa), k, 3), triples, forks


def sweep_reads(k, triples, forks, seed=2, offsets=range(0, 131)):
    """Error-free reads of every triple's T from start offsets 0..130 (the first k-mer at window position p = offset & 63 of block
    offset >> 6), of the READ_LENS and of the lengths that put x + rest — constant over a walk in one chain: p + L — at 255, 256 and
    257: stays, stays, re-bases. Also reads with ONE substitution (tolerated or not, by `allowed` of the caller) on the last base of A, on
    the base the extension test at A's end looks at, on the one at B's end, and on the first base compared in C. Reads over the forks
    that end one base before, at, and one and two bases beyond the last node's end."""
    rng = np.random.RandomState(seed)
    reads = []
    for t, e_a, e_b in triples:
        for s in offsets:
            p = s & 63
            lens = set(READ_LENS) | {255 - p, 256 - p, 257 - p}
            for n in sorted(lens):
                if n < k or s + n > len(t):
                    continue
                r = t[s:s + n]
                reads.append(r)
                if n in (150, 256 - p, 300):
                    for pos in (e_a - 1, e_a, e_b, e_b + 1):
                        if s + k <= pos < s + n:          # behind the read's first k-mer (which has to be found), inside the read
                            reads.append(r[:pos - s] + _sub(r[pos - s], rng) + r[pos - s + 1:])
    for t, e in forks:
        for s in offsets:
            for end in (e - 1, e, e + 1, e + 2, e + 40):
                if end - s >= k:
                    reads.append(t[s:end])
    return reads


def case_reads(host_reads, k_of, n_max, seed=3):
    """the reads of a helpers.*_case cut to the lengths of READ_LENS from swept start offsets (the cases' own reads start anywhere)"""
    rng = np.random.RandomState(seed)
    out = []
    for r in host_reads:
        for n in READ_LENS:
            if len(r) >= n >= k_of:
                o = int(rng.randint(0, len(r) - n + 1))
                out.append(r[o:o + n])
    if len(out) > n_max:
        out = [out[i] for i in rng.choice(len(out), n_max, replace=False)]
    return out
