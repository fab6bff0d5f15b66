"""The hand-made abundance cases of tests/quant_cases.py on the CPU: every property a case claims (each edge present as a row length
and as a degree, the bins full, ragged or absent, N = 2^53 - 1, more distinct rows in a workgroup's draws than its hash table holds),
and the proof that the numpy models themselves stay inside the limits the GPU tests apply to the kernels."""
import numpy as np
import pytest

import boot_model as bm
import quant_cases as qc
import quant_model as qm


@pytest.fixture(autouse=True, scope="module")
def _library(built):
    """the cases build their indexes with the product's host builder"""


def test_restated_constants_are_those_of_the_sources():
    """the lines the constants of quant_cases.py restate are still in csrc/"""
    import helpers
    src = helpers.ROOT / "rust-pseudoaligner_amd" / "csrc"
    state, boot = (src / "quant_state.hpp").read_text(), (src / "quant_boot.hip").read_text()
    assert "return k == 0 ? %du : k == 1 ? %du : k == 2 ? %du : k == 3 ? %du : %du; }" % qc.BIN_MIN in state
    assert "return k == 0 ? %du : k == 1 ? %du : k == 2 ? %du : k == 3 ? %du : %du; }" % qc.GROUP in state
    assert "constexpr int QB = 256;" in state and tuple(256 // g for g in qc.GROUP) == qc.PER_BLOCK
    assert "constexpr uint32_t COARSE = %d;" % qc.COARSE in boot and "HT_SLOTS = %d," % qc.HT_SLOTS in boot and "HT_PROBES = 4;" in boot
    assert "constexpr uint32_t DRAW_BLOCKS_PER_LANE = 32;" in boot and "constexpr uint32_t DRAW_CHUNK = QB * DRAW_BLOCKS_PER_LANE;" in boot
    assert qc.DRAWS_PER_ROUND == 2 * 256 and qc.DRAWS_PER_WORKGROUP == 2 * 256 * 32
    assert "constexpr uint32_t LONG_REPS = 4;" in boot
    for x in qc.BIN_MIN + qc.GROUP:                                                    # every threshold and group size with both neighbours,
        assert {x - 1, x, x + 1} - {0, 6, 10, 18} <= set(qc.EDGE), x                   # but for 6, 10 and 18: no lane group ends beside them
    assert list(qc.step_cases()) == qc.STEP_CASE_NAMES
    import test_gpu_quant_boot as tb
    assert (qc.SEED, qc.HIGH) == (tb.SEED, tb.HIGH)


def test_edge_indexes():
    for T in (1, 2, qc.BIG_T):
        host, arr, tx_len = qc.edge_index(T)                                           # (the properties are asserted where it is built)
        assert host.num_transcripts == T and tx_len.min() >= 20 and tx_len.max() <= 400
    eff = qm.effective_lengths(qc.edge_index(qc.BIG_T)[2], qc.MEAN_READ_LEN)
    print("T = %d: %d transcripts at the floor, %d above" % (qc.BIG_T, int((eff == 1).sum()), int((eff > 1).sum())))


def test_ladder_holds_every_edge_and_leaves_every_bin_ragged_once():
    ragged = np.zeros((2, 5), bool)
    for seed in (0, 1):
        p = qc.ladder(seed).problem
        rows, slots = qc.layouts(p)
        print("ladder %d: %d rows, %d ids, N = %d, rows per bin %s, transcripts per bin %s" % (seed, len(p.rows), len(p.ids), p.N, rows, slots))
        assert set(qc.EDGE) <= set(p.lens.tolist()) and set(qc.EDGE) <= set(p.degree.tolist())
        assert all(rows) and all(slots)
        ragged[0] |= [rows[k] % qc.PER_BLOCK[k] != 0 for k in range(5)]
        ragged[1] |= [slots[k] % qc.PER_BLOCK[k] != 0 for k in range(5)]
        s = qc.ladder_small(seed).problem
        assert 19000 <= s.N <= 20312 and len(s.rows) == len(p.rows) and np.array_equal(s.degree, p.degree)   # 64 replicates: under 1.3 M draws
    assert ragged[:, 1:].all()                                                         # (bin 0 has one entity in a block: no ragged block)


def test_single_bin_layouts():
    for k in range(5):
        for extra in (0, 1):
            p = qc.single_bin(k, extra).problem
            rows, _ = qc.layouts(p)
            n = qc.PER_BLOCK[k] * qc.SINGLE_BIN_MULT[k] + extra
            assert rows[k] == n == len(p.rows) and sum(rows) == n
            blk = qc.blocks(rows)
            assert blk[:k + 1] == [0] * (k + 1) and len(set(blk[k + 1:])) == 1
            assert (n % qc.PER_BLOCK[k] == 0) == (extra == 0 or k == 0)


def test_mixed_candidates_and_tiny_and_draw_tables():
    c = qc.mixed_candidates()
    assert c.problem.N == 2 ** 53 - 1 and float(c.problem.n.max()) == float(int(c.problem.n.max()))
    recs = qm.read_overflow(c.words)
    assert recs[c.at["zero"]][1] == 0 and len(recs[c.at["empty"]][0]) == 0
    assert c.cand[len(c.counts) - 3 + c.at["zero"]] == 0 and c.cand[len(c.counts) - 3 + c.at["empty"]] == 0
    small = qc.mixed_candidates(qc.MIXED_BOOT_BIG)
    assert small.problem.N < 2 ** 32 and np.array_equal(small.cand > 0, c.cand > 0)
    assert qc.tiny(1).problem.N == 7 and qc.tiny(1, True).problem.N == 0 and qc.tiny(2).problem.N == 135
    assert np.array_equal(qc.tiny(1).problem.iterate(200), [7.0])                      # the model keeps 7.0 exactly
    for d in qc.DRAW_CASES:
        p = qc.draw_table(*d).problem
        assert p.N < 2 ** 32 and (len(p.rows) if d[0] == "rows" or d[2] == "each" else p.N) == d[1]


def test_the_fallback_table_overfills_the_hash_table():
    case = qc.draw_table(*qc.FALLBACK)
    assert case.problem.N == 18000 and len(case.problem.rows) == 6000
    for b in qc.fallback_replicates():
        d = qc.distinct_rows_of_the_first_workgroup(case, b)
        print("replicate %d: %d distinct rows in the first %d draws" % (b, d, qc.DRAWS_PER_WORKGROUP))
        assert d > qc.HT_SLOTS


SMALL = ["single_bin_%d+%d" % (k, e) for k in range(5) for e in (0, 1)] + ["tiny_1", "tiny_2"]


@pytest.mark.parametrize("name", SMALL)
def test_model_step_against_exact_sums(name):
    p = qc.step_cases()[name].problem
    a = p.start()
    for _ in range(3):
        got, want = p.step(a), p.step_exact_sums(a)
        ok = want > 0
        assert np.all(np.abs(got[ok].astype(np.longdouble) - want[ok]) <= p.step_bound() * want[ok]) and not got[~ok].any()
        a = got


def _all_cases():
    out = dict(qc.step_cases())
    for s in (0, 1):
        c = qc.ladder_small(s)
        out[c.name] = c
    c = qc.mixed_candidates(qc.MIXED_BOOT_BIG)
    out[c.name] = c
    for d in qc.DRAW_CASES:
        c = qc.draw_table(*d)
        out[c.name] = c
    return out


def test_every_case_keeps_its_reads():
    """one model step from the start sums to N within step_bound() * N; a resampled replicate sums to N (where the model can draw: N
    below 2^32; the 24 M draws of a whole ladder once)"""
    for name, c in _all_cases().items():
        p = c.problem
        if p.N:
            assert abs(float(qm.fsum_ld(p.step(p.start()))) - p.N) <= p.step_bound() * p.N, name
        else:
            assert not p.step(p.start()).any()
        if p.N < 2 ** 32 and name != "ladder_1":
            rep = bm.resample(c.cand, qc.SEED, 3)
            assert int(rep.sum()) == p.N and not rep[c.cand == 0].any(), name


def test_replicate_problem_is_the_table_of_the_replicate():
    for c in (qc.ladder_small(0), qc.mixed_candidates(qc.MIXED_BOOT_BIG), qc.tiny(2)):
        rep = bm.resample(c.cand, qc.SEED, 1)
        fast = c.replicate_problem(rep)
        cc, oc = c.replicate_table(rep)
        _, arr, tx_len = qc.edge_index(c.T)
        slow = qm.Problem.from_table(arr, tx_len, cc, bm.overflow_with_counts(c.words, oc), mean_read_len=qc.MEAN_READ_LEN)
        assert fast.N == slow.N
        a = c.problem.start()
        for _ in range(3):
            assert fast.step(a).tobytes() == slow.step(a).tobytes()
            a = slow.step(a)
