"""The bootstrap kernels (csrc/quant_boot.hip) on the hand-made tables of tests/quant_cases.py: every batch size at which the stride
changes (4, 8, 16, 32, 64 and the sizes on both sides of each step) over a table that holds every bin threshold as a row length and as
a degree; the resampler's two-level search at 1024 and 2048 rows, its hash table beyond 4096 distinct rows of a workgroup (the direct
atomics), a lane's and a workgroup's last draw; candidates without reads or ids; T = 1 and T = 2; one object moved between tables and
batch sizes. Counts equal tests/boot_model.py bit for bit; a batched step is the EM map of tests/quant_model.py per replicate within
test_gpu_quant._step_tolerance; every other comparison is of bytes."""
import numpy as np
import pytest

import boot_model as bm
import helpers
import quant_cases as qc
import test_gpu_quant as tq
from test_gpu_quant_edges import assert_step_is_the_em_map, quantifier

pa = helpers.pa
pytestmark = pytest.mark.gpu

SEED, HIGH = qc.SEED, qc.HIGH
_cache = {}


def model_rep(case, b):
    """candidate counts of global replicate b (memoised: the batches overlap)"""
    key = (case.name, b)
    if key not in _cache:
        _cache[key] = bm.resample(case.cand, SEED, b)
    return _cache[key]


def assert_counts_are_the_models(q, case, first, n, look=None):
    N = case.problem.N
    for k in range(n):
        cc, oc = q.bootstrap_counts(k)
        assert int(cc[:-3].sum()) + int(oc.sum()) == N and int(cc[-3]) == int(oc.sum()) and not cc[-2:].any(), (case.name, first, n, k)
        if look is None or k in look:
            want_cc, want_oc = case.replicate_table(model_rep(case, first + k))
            assert np.array_equal(cc, want_cc) and np.array_equal(oc, want_oc), (case.name, first, n, k)


def _batch_is_the_models(case, n, points):
    """a batch of n from replicate 0: the counts are the model's, the start is N / T where the ORIGINAL table has a row, and one batched
    step from the GPU's own alpha is the EM map of every replicate, at the steps `points`"""
    p = case.problem
    q = quantifier(case)
    st = q.stats()
    assert (st["rows"], st["reads_used"], st["longest_row"], st["largest_degree"]) == (len(p.rows), p.N, p.m_max, p.d_max)
    tol = tq._step_tolerance(st)
    q.bootstrap_draw(SEED, 0, n)
    assert_counts_are_the_models(q, case, 0, n)
    probs = [case.replicate_problem(model_rep(case, k)) for k in range(n)]
    start = np.where(p.degree > 0, p.N / p.T, 0.0)
    got = q.bootstrap_fetch()[0]
    assert got.shape == (n, p.T) and all(np.array_equal(a, start) for a in got)
    done = 0
    for i in points:
        q.bootstrap_step(i - done)
        before = q.bootstrap_fetch()[0]
        q.bootstrap_step(1)
        done = i + 1
        got = q.bootstrap_fetch()[0]
        worst = 0.0
        for k in range(n):
            want = probs[k].step(before[k])
            ok = want >= 1e-290
            worst = max(worst, float(np.max(np.abs(got[k][ok] - want[ok]) / want[ok])))
            assert np.all(np.abs(got[k][ok] - want[ok]) <= tol * want[ok]), (case.name, n, k, i, worst, tol)
            assert np.all(got[k][~ok] < 1e-289)
        print("%s batch of %d step %d: worst relative deviation of a replicate %.3g (bound %.3g)" % (case.name, n, i, worst, tol))


@pytest.mark.parametrize("n", qc.BATCHES)
def test_batch_sizes(n):
    case = qc.ladder_small(0)
    assert (case.problem.m_max, case.problem.d_max) == (2049, 2049)
    _batch_is_the_models(case, n, (0, 1, 10))


@pytest.mark.parametrize("extra", (0, 1))
@pytest.mark.parametrize("k", range(5))
def test_every_bin_alone(k, extra):
    """the bootstrap passes group the bins anew (0 and 1 on the long path, then <= 16 / <= 8 / <= 4 entries): each alone, with a full
    and with a ragged last block at the strides 8 and 64"""
    _batch_is_the_models(qc.single_bin(k, extra), 5, (0, 1))
    _batch_is_the_models(qc.single_bin(k, extra), 64, (0,))


def _outputs(q, first, n, ks):
    q.bootstrap_draw(SEED, first, n)
    counts = [np.concatenate(q.bootstrap_counts(k)).tobytes() for k in ks]
    q.bootstrap_step(50)
    stepped = q.bootstrap_fetch()[0]
    q.bootstrap_draw(SEED, first, n)
    iters, conv = q.bootstrap_run()
    est, tpm = q.bootstrap_fetch()
    return [(counts[j], stepped[k].tobytes(), est[k].tobytes(), tpm[k].tobytes(), int(iters[k]), bool(conv[k])) for j, k in enumerate(ks)]


def _stride_case(name):
    return qc.ladder_small(0) if name == "ladder" else qc.single_bin(int(name[-1]))


@pytest.mark.parametrize("n", (4, 5, 8, 9, 16, 17, 32, 33, 64))
@pytest.mark.parametrize("name", ["ladder", "single_bin_0", "single_bin_4"])
def test_replicates_3_and_4_do_not_depend_on_the_stride(name, n):
    case = _stride_case(name)
    key = ("pair", name)
    if key not in _cache:
        _cache[key] = _outputs(quantifier(case), 3, 2, [0, 1])
        print("%s: replicates 3 and 4 stop after %d and %d iterations" % (name, _cache[key][0][4], _cache[key][1][4]))
    pair = _cache[key]
    assert pair[0][0] != pair[1][0]
    ks = [3, 4] if n > 4 else [3]
    assert _outputs(quantifier(case), 0, n, ks) == pair[:len(ks)]


@pytest.mark.parametrize("kind,x,variant", qc.DRAW_CASES)
def test_draw_tables(kind, x, variant):
    case = qc.draw_table(kind, x, variant)
    q = quantifier(case)
    assert q.stats()["reads_used"] == case.problem.N and q.stats()["rows"] == len(case.problem.rows)
    for first in (0, HIGH):
        q.bootstrap_draw(SEED, first, 5)
        assert_counts_are_the_models(q, case, first, 5)
    if (kind, x, variant) == qc.FALLBACK:                                              # (tests/test_quant_cases.py: every one of these overfills the hash table)
        q.bootstrap_draw(SEED, 0, 64)
        assert_counts_are_the_models(q, case, 0, 64, look=(0, 1, 32, 62, 63))


def test_mixed_candidates():
    case = qc.mixed_candidates(qc.MIXED_BOOT_BIG)
    C, N = len(case.counts) - 3, case.problem.N
    q = quantifier(case)
    assert q.stats()["reads_used"] == N < 2 ** 32
    q.bootstrap_draw(SEED, 0, 5)
    assert_counts_are_the_models(q, case, 0, 5)
    tables = [q.bootstrap_counts(k) for k in range(5)]
    for cc, oc in tables:
        assert not cc[:C][case.counts[:C] == 0].any() and oc[case.at["zero"]] == 0 and oc[case.at["empty"]] == 0
        assert len(oc) == int(case.words[0]) == 44                                     # record order: one count for every record
    for cc, oc in tables[:2]:
        q.set_counts(cc, bm.overflow_with_counts(case.words, oc))                      # a table pa_quant_set_counts accepts
        assert q.stats()["reads_used"] == N and q.stats()["novel_reads_left_out"] == 0


def test_tiny():
    one = qc.tiny(1)
    q = quantifier(one)
    q.bootstrap_draw(SEED, HIGH, 64)
    for k in range(64):
        cc, oc = q.bootstrap_counts(k)
        assert cc.tolist() == [7, 0, 0, 0] and len(oc) == 0
    assert np.array_equal(q.bootstrap_fetch()[0], np.full((64, 1), 7.0))
    q.bootstrap_step(33)
    assert np.array_equal(q.bootstrap_fetch()[0], np.full((64, 1), 7.0))
    iters, conv = q.bootstrap_run()
    assert conv.all() and np.array_equal(q.bootstrap_fetch()[0], np.full((64, 1), 7.0))
    zero = qc.tiny(1, True)
    q.set_counts(zero.counts, zero.words)
    q.bootstrap_draw(SEED, 0, 3)
    assert not q.bootstrap_counts(2)[0].any() and not q.bootstrap_fetch()[0].any() and q.bootstrap_run()[0].tolist() == [0, 0, 0]
    two = qc.tiny(2)
    q = quantifier(two)
    tol = tq._step_tolerance(q.stats())
    q.bootstrap_draw(SEED, 0, 5)
    assert_counts_are_the_models(q, two, 0, 5)
    before = q.bootstrap_fetch()[0]
    assert np.array_equal(before, np.full((5, 2), 135 / 2))
    q.bootstrap_step(1)
    got = q.bootstrap_fetch()[0]
    for k in range(5):
        assert_step_is_the_em_map("tiny_2", got[k], two.replicate_problem(model_rep(two, k)).step(before[k]), tol, "replicate %d step 0" % k)


def test_one_object_through_tables_and_batch_sizes():
    """QuantBoot::drop() keeps some buffers and pa_quant_bootstrap_draw resizes others: the moved object's batch is a fresh object's"""
    def batch(q, n):
        q.bootstrap_draw(SEED, 0, n)
        counts = [np.concatenate(q.bootstrap_counts(k)).tobytes() for k in range(n)]
        q.bootstrap_step(20)
        return counts, q.bootstrap_fetch()[0].tobytes()

    first, second = qc.ladder_small(0), qc.single_bin(2)
    q = quantifier(first)
    big = batch(q, 64)
    q.set_counts(second.counts, second.words)
    assert batch(q, 5) == batch(quantifier(second), 5)
    assert batch(q, 64) == batch(quantifier(second), 64)                               # the same table, a wider stride: the buffers grow
    assert batch(q, 3) == batch(quantifier(second), 3)                                 # and shrink
    q.set_counts(first.counts, first.words)
    assert batch(q, 64) == big
