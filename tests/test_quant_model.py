"""The numpy model of the abundance EM (tests/quant_model.py) against closed forms, and the entry points of pa_quant_* that answer
without a device. No GPU here."""
import ctypes as C

import numpy as np
import pytest

import helpers
import quant_model as qm

pa = helpers.pa


def _random_problem(seed, T=40, rows=120):
    rng = np.random.default_rng(seed)
    r = [np.sort(rng.choice(T, int(rng.integers(1, 7)), replace=False)) for _ in range(rows)]
    return qm.Problem(r, [int(x) for x in rng.integers(1, 10000, rows)], rng.integers(200, 5000, T).astype(np.float64))


def test_disjoint_singletons_keep_their_counts():
    n = [7, 0, 123456, 1, 99]
    p = qm.Problem([[t] for t in range(5)], n, [1000.0, 50.0, 3.0, 777.0, 1.0])
    a = p.start()
    for _ in range(3):
        a = p.step(a)
        assert np.allclose(a, n, rtol=4 * qm.EPS, atol=0)
    assert a[1] == 0.0 and p.N == sum(n)


def test_two_transcripts_share_a_class_evenly():
    a_, c_ = 300, 101
    p = qm.Problem([[0], [1], [0, 1]], [a_, a_, c_], [500.0, 500.0])
    a = p.start()
    for _ in range(5):                                   # from the first iteration on
        a = p.step(a)
        assert np.allclose(a, a_ + c_ / 2, rtol=8 * qm.EPS, atol=0)
    assert np.allclose(np.asarray(p.step(p.start(), np.longdouble), np.float64), a_ + c_ / 2, rtol=8 * qm.EPS)
    assert np.allclose(np.asarray(p.step_exact_sums(p.start()), np.float64), a_ + c_ / 2, rtol=8 * qm.EPS)


@pytest.mark.parametrize("seed", range(4))
def test_mass_is_kept_and_the_likelihood_does_not_fall(seed):
    p = _random_problem(seed)
    bound = p.step_bound()
    a = p.start()
    ll = p.loglik(a)
    for _ in range(60):
        a = p.step(a)
        assert abs(float(qm.fsum_ld(a)) - p.N) <= bound * p.N
        ll2 = p.loglik(a)
        assert float(ll2 - ll) >= -4 * p.N * bound
        ll = ll2


def test_float64_and_long_double_models_agree(seed=5):
    p = _random_problem(seed)
    a64, a80 = p.iterate(100), p.iterate(100, np.longdouble)
    big = a64 >= 1e-2
    assert big.any() and np.max(np.abs(a64[big] - np.asarray(a80[big], np.float64)) / a64[big]) < 1e-10
    one = p.step(a64)
    exact = np.asarray(p.step_exact_sums(a64), np.float64)
    assert np.all(np.abs(one - exact) <= 2 * p.step_bound() * exact)


def test_empty_problem_and_transcripts_without_a_row():
    p = qm.Problem([[0, 1]], [0], [10.0, 10.0, 10.0])
    assert p.N == 0 and not p.start().any() and not p.step(p.start()).any()
    p = qm.Problem([[0, 1]], [6], [10.0, 10.0, 10.0])
    assert p.start().tolist() == [2.0, 2.0, 0.0]          # N / T where there is a row, 0 where there is none
    assert p.step(p.start()).tolist() == [3.0, 3.0, 0.0]


def test_overflow_words_round_trip_and_generator(small_index):
    host = small_index(24)
    arr = host.arrays()
    counts, words = qm.random_table(arr, 3, 0.3, 60)
    recs = qm.read_overflow(words)
    assert len(recs) == 60 and sum(c for _, c in recs) == int(counts[arr["num_classes"]])
    assert np.array_equal(qm.write_overflow(recs), words) and pa.parse_overflow(words) == {tuple(int(x) for x in r): c for r, c in recs}
    assert all(np.all(np.diff(r.astype(np.int64)) > 0) for r, _ in recs)
    counts2, words2 = qm.random_table(arr, 3, 0.3, 60)
    assert np.array_equal(counts, counts2) and np.array_equal(words, words2)
    tx_len = np.diff(host.transcripts()[1].astype(np.int64))
    p = qm.Problem.from_table(arr, tx_len, counts, words, mean_read_len=100.0)
    assert p.N == int(counts[: arr["num_classes"] + 1].sum()) and np.array_equal(p.eff, np.maximum(tx_len - 100.0 + 1, 1.0))
    assert qm.Problem.from_table(arr, tx_len, counts, None).N == int(counts[: arr["num_classes"]].sum())


def test_stop_rule_in_numpy():
    assert qm.stop_rule_holds([1.0, 5e-3], [1.005, 1e-2])           # 0.5 % on the large one; the small one is not above the limit
    assert not qm.stop_rule_holds([1.0, 5e-3], [1.02, 1e-2])
    assert np.isclose(qm.tpm([1.0, 3.0], [10.0, 10.0]).sum(), 1e6)


def test_default_params_and_checks_that_need_no_device(built, small_index):
    lib = pa.lib()
    p = pa._ffi.QuantParams()
    lib.pa_quant_default_params(None)                                # a null pointer is ignored
    lib.pa_quant_default_params(C.byref(p))
    got = {n: getattr(p, n) for n, _ in pa._ffi.QuantParams._fields_}
    assert got == dict(qm.DEFAULTS, reserved=0)
    assert C.sizeof(pa._ffi.QuantParams) == 48
    host = small_index(24)
    q = C.c_void_p()
    assert lib.pa_quant_create(None, None, C.byref(p), C.byref(q)) == pa._ffi.PA_ERR_INVALID_ARG and not q
    assert lib.pa_quant_create(None, host._h, C.byref(p), None) == pa._ffi.PA_ERR_INVALID_ARG
    for field, bad in (("check_every", 0), ("alpha_change", -1.0), ("alpha_limit", float("nan")), ("mean_read_len", float("inf"))):
        b = pa._ffi.QuantParams()
        lib.pa_quant_default_params(C.byref(b))
        setattr(b, field, bad)
        assert lib.pa_quant_create(None, host._h, C.byref(b), C.byref(q)) == pa._ffi.PA_ERR_INVALID_ARG and not q, field
    counts = np.zeros(host.arrays()["num_classes"] + 3, np.uint64)
    assert lib.pa_quant_set_counts(None, counts.ctypes.data, len(counts), None, 0) == pa._ffi.PA_ERR_INVALID_ARG
    assert lib.pa_quant_step(None, 1) == pa._ffi.PA_ERR_INVALID_ARG and lib.pa_quant_stats(None, counts.ctypes.data) == pa._ffi.PA_ERR_INVALID_ARG
    lib.pa_quant_destroy(None)


def test_no_gpu_means_no_quantifier(built, small_index):
    if pa.lib().pa_device_count() > 0:
        pytest.skip("a GPU is present")
    host = small_index(24)
    q = C.c_void_p()
    assert pa.lib().pa_quant_create(None, host._h, None, C.byref(q)) == pa._ffi.PA_ERR_NO_DEVICE and not q
    with pytest.raises(pa.PaError) as e:
        pa.Quantifier(None, host)
    assert e.value.code == pa._ffi.PA_ERR_NO_DEVICE and "no CPU fallback" in str(e.value)
