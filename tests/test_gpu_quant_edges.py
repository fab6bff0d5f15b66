"""The abundance kernels (csrc/quant.hip) on the hand-made tables of tests/quant_cases.py: every bin threshold and lane-group size as
a row length and as a degree, every bin alone with a full and with a ragged last block, candidates without reads or without ids,
N = 2^53 - 1, T = 1 and T = 2, and one object moved between tables of different shape. The yardstick is tests/quant_model.py with the
limits of tests/test_gpu_quant.py: one step within _step_tolerance (derived), 200 steps within 16 x the float64 model's own deviation
from the long-double model; every integer and every byte comparison is exact."""
import numpy as np
import pytest

import helpers
import quant_cases as qc
import quant_model as qm
import test_gpu_quant as tq

pa = helpers.pa
pytestmark = pytest.mark.gpu

STEP_POINTS = (0, 1, 2, 10, 49)
_cache = {}


def aligner(T):
    """(host index, its Pseudoaligner) of quant_cases.edge_index(T)"""
    if T not in _cache:
        host = qc.edge_index(T)[0]
        _cache[T] = (host, pa.Pseudoaligner(host))
    return _cache[T]


def quantifier(case, **params):
    host, a = aligner(case.T)
    params.setdefault("mean_read_len", qc.MEAN_READ_LEN)
    q = pa.Quantifier(a, host, **params)
    q.set_counts(case.counts, case.words)
    return q


def model_stats(case):
    p = case.problem
    return dict(rows=len(p.rows), ids=len(p.ids), transcripts_with_a_row=int((p.degree > 0).sum()), longest_row=p.m_max, largest_degree=p.d_max,
                reads_used=p.N, novel_reads_left_out=0 if case.words is not None else int(case.counts[-3]))


def assert_stats(q, case):
    st = q.stats()
    want = model_stats(case)
    assert {k: st[k] for k in want} == want, case.name
    return st


def assert_step_is_the_em_map(name, got, want, tol, what):
    tiny = want < 1e-290
    worst = float(np.max(np.abs(got[~tiny] - want[~tiny]) / np.where(want[~tiny] > 0, want[~tiny], 1.0))) if (~tiny).any() else 0.0
    print("%s %s: worst relative deviation %.3g (bound %.3g)" % (name, what, worst, tol))
    assert np.all(np.abs(got[~tiny] - want[~tiny]) <= tol * want[~tiny]), (name, what, worst, tol)
    assert np.all(got[tiny] < 1e-289)


@pytest.mark.parametrize("name", qc.STEP_CASE_NAMES)
def test_stats_and_single_steps(name):
    case = qc.step_cases()[name]
    p = case.problem
    q = quantifier(case)
    st = assert_stats(q, case)
    tol = tq._step_tolerance(st)
    assert np.array_equal(q.alpha(), p.start())
    done = 0
    for i in STEP_POINTS:
        q.step(i - done)
        done = i
        before = q.alpha()
        want = p.step(before)                                                      # one model step from the GPU's own alpha_i
        q.step(1)
        done += 1
        assert_step_is_the_em_map(name, q.alpha(), want, tol, "step %d" % i)
    assert q.stats()["iterations"] == (done if p.N else 0)


@pytest.mark.parametrize("name", qc.STEP_CASE_NAMES)
def test_200_steps_against_the_long_double_model(name):
    """GPU deviation <= 16 x D_ref, D_ref = the float64 model's deviation from the long-double model (floored at 2^-50), over the
    transcripts with alpha >= alpha_change_limit"""
    case = qc.step_cases()[name]
    p = case.problem
    q = quantifier(case)
    q.step(200)
    got = q.alpha()
    if not p.N:
        assert not got.any() and q.stats()["iterations"] == 0
        return
    a64 = p.iterate(200)
    a80 = p.iterate(200, np.longdouble)
    sel = np.asarray(a80, np.float64) >= 1e-2
    assert sel.any()
    ref = a80[sel]
    d_ref = max(float(np.max(np.abs(a64[sel].astype(np.longdouble) - ref) / ref)), 2.0 ** -50)
    d_gpu = float(np.max(np.abs(got[sel].astype(np.longdouble) - ref) / ref))
    print("%s: D_ref %.3g, GPU %.3g" % (name, d_ref, d_gpu))
    assert d_gpu <= 16 * d_ref, (name, d_gpu, d_ref)


@pytest.mark.parametrize("name", qc.STEP_CASE_NAMES)
def test_repeats_are_bit_identical(name):
    case = qc.step_cases()[name]
    q1, q2 = quantifier(case), quantifier(case)
    q1.step(200)
    q2.step(200)
    a1 = q1.alpha()
    assert a1.tobytes() == q2.alpha().tobytes()
    q1.set_counts(case.counts, case.words)
    assert q1.stats()["iterations"] == 0
    q1.step(200)
    assert q1.alpha().tobytes() == a1.tobytes()


def test_one_object_through_tables_of_different_shape():
    """pa_quant_set_counts allocates anew: after every table the moved object is a fresh one, byte for byte"""
    zero = qc.Case("zero", qc.BIG_T, np.zeros(len(qc.ladder(0).counts), np.uint64), qm.write_overflow([]))   # no reads, as tiny(1, True), over this index
    walk = [qc.ladder(0), zero, qc.single_bin(0), qc.mixed_candidates(), qc.ladder(0)]
    assert not zero.problem.N
    q = quantifier(walk[0])
    seen = []
    for i, case in enumerate(walk):
        if i:
            q.set_counts(case.counts, case.words)
        q.step(20)
        fresh = quantifier(case)
        fresh.step(20)
        assert q.alpha().tobytes() == fresh.alpha().tobytes(), (i, case.name)
        assert q.stats() == fresh.stats() and q.stats()["iterations"] == (20 if case.problem.N else 0), (i, case.name)
        assert_stats(q, case)
        seen.append(q.alpha().tobytes())
    assert seen[4] == seen[0] and not np.frombuffer(seen[1]).any() and len({seen[0], seen[2], seen[3]}) == 3


def test_one_transcript():
    case = qc.tiny(1)
    q = quantifier(case)
    assert q.num_transcripts == 1 and q.alpha().tolist() == [7.0]
    for n in (1, 1, 2, 10, 50, 137):
        q.step(n)
        assert q.alpha().tolist() == [7.0]
    q.set_counts(case.counts, case.words)
    iters, converged = q.run()
    assert converged and iters == q.params.min_iters and q.alpha().tolist() == [7.0]
    est, tpm, eff = q.fetch()
    assert est.tolist() == [7.0] and np.array_equal(tpm, qm.tpm(est, eff)) and abs(tpm[0] - 1e6) <= 1e6 * 2.0 ** -52 and eff.tolist() == case.problem.eff.tolist()
    zero = qc.tiny(1, True)
    q.set_counts(zero.counts, zero.words)
    assert q.run() == (0, True) and q.alpha().tolist() == [0.0] and q.stats()["iterations"] == 0
    q.step(5)
    assert q.alpha().tolist() == [0.0] and not q.fetch()[1].any()
