"""Bootstrap replicates on the GPU (pa_quant_bootstrap_*) against the numpy models: the resampled counts bit for bit (tests/boot_model.py),
one batched step against the EM map per replicate, 200 steps against the long-double model, the stop rule and the freeze per replicate,
independence of a replicate from its batch, and that nothing of the point estimate moves. The tables are those of tests/test_gpu_quant.py
plus three made by hand: one class with 3 000 000 reads among classes with one read each, a table with one read, one with 37."""
import json
import os

import numpy as np
import pytest

import boot_model as bm
import helpers
import quant_model as qm
import test_gpu_quant as tq

pa = helpers.pa
pytestmark = pytest.mark.gpu

SEED = 0x1234567855AA33CC
HIGH = 2 ** 32 - 64
_cache = {}


def _case(name):
    """(index name, class_counts, overflow words or None, mean_read_len)"""
    key = ("boot case", name)
    if key in _cache:
        return _cache[key]
    if name in ("skewed", "one_read", "odd"):
        index, counts, words, mrl = tq._case("gencode_0")
        arr = tq._index(index)[2]
        C = arr["num_classes"]
        lens = np.diff(arr["ec_offset"].astype(np.int64))
        counted = np.flatnonzero(counts[:C] > 0)
        new = np.zeros(C + 3, np.uint64)
        if name == "skewed":       # adjacent rows of one read put every interval boundary in play; the heavy class sits in the middle
            new[counted] = 1
            new[counted[len(counted) // 2]] = 3_000_000
            recs = qm.read_overflow(words)
            words = bm.overflow_with_counts(words, np.ones(len(recs), np.uint64))
            new[C] = len(recs)
            new[C + 2] = 5
        elif name == "one_read":
            new[counted[3]] = 1
            words = None
        else:
            new[counted[:5]] = [1, 20, 3, 12, 1]
            words = None
        out = (index, new, words, mrl)
    else:
        out = tq._case(name)
    _cache[key] = out
    return out


def _quantifier(name, **params):
    index, counts, words, mrl = _case(name)
    host, a, arr, tx_len = tq._index(index)
    params.setdefault("mean_read_len", mrl)
    q = pa.Quantifier(a, host, **params)
    q.set_counts(counts, words)
    return q


def _model_counts(name, seed, b):
    """candidate counts of global replicate b (memoised: several tests look at the same replicates)"""
    key = ("rep", name, seed, b)
    if key not in _cache:
        index, counts, words, _ = _case(name)
        _cache[key] = bm.resample(bm.candidate_counts(tq._index(index)[2], counts, words), seed, b)
    return _cache[key]


def _problem(name, cc, oc):
    """quant_model.Problem of a replicate's table"""
    index, counts, words, mrl = _case(name)
    host, a, arr, tx_len = tq._index(index)
    return qm.Problem.from_table(arr, tx_len, cc, bm.overflow_with_counts(words, oc), mean_read_len=mrl)


COUNT_CASES = [("gencode_0", 64, 0), ("gencode_0", 5, HIGH), ("synth", 8, HIGH), ("synth", 1, 0), ("mapped", 5, 0), ("mapped", 64, HIGH), ("one_class", 1, 0),
               ("one_class", 8, 0), ("zero", 5, 0), ("skewed", 5, HIGH), ("skewed", 64, 0), ("one_read", 64, HIGH), ("one_read", 1, 0), ("odd", 8, 0), ("odd", 5, HIGH)]


@pytest.mark.parametrize("name,n,first", COUNT_CASES)
def test_counts_are_exact(name, n, first):
    """every replicate's table sums to N; against the model bit for bit: every replicate of the batch while the batch has at most 16 M
    draws (a draw costs the numpy model about 0.1 us), else the first two, the middle one and the last two"""
    index, counts, words, _ = _case(name)
    arr = tq._index(index)[2]
    cand = bm.candidate_counts(arr, counts, words)
    N = int(cand.sum())
    q = _quantifier(name)
    assert q.stats()["reads_used"] == N
    q.bootstrap_draw(SEED, first, n)
    look = range(n) if N * n <= 16_000_000 else sorted({0, 1, n // 2, n - 2, n - 1})
    for k in range(n):
        cc, oc = q.bootstrap_counts(k)
        assert int(cc[:-3].sum()) + int(oc.sum()) == N and int(cc[-3]) == int(oc.sum()) and not cc[-2:].any()
        if k in look:
            want_cc, want_oc = bm.replicate_table(arr, words, _model_counts(name, SEED, first + k))
            assert np.array_equal(cc, want_cc) and np.array_equal(oc, want_oc), (name, n, first, k)
    if name == "zero":
        assert not q.bootstrap_fetch()[0].any() and q.bootstrap_run()[0].tolist() == [0] * n
    else:
        cc, oc = q.bootstrap_counts(0)
        q.set_counts(cc, bm.overflow_with_counts(words, oc))                           # a table pa_quant_set_counts accepts
        assert q.stats()["reads_used"] == N


@pytest.mark.parametrize("name", ["gencode_0", "synth", "repeats"])
def test_one_step_is_the_em_map(name):
    n = 5
    q = _quantifier(name)
    st = q.stats()
    if name == "repeats":
        assert st["longest_row"] >= 2000 and st["largest_degree"] >= 2000              # the split-row path runs in both passes
    tol = tq._step_tolerance(st)
    q.bootstrap_draw(SEED, 0, n)
    probs = [_problem(name, *q.bootstrap_counts(k)) for k in range(n)]
    T = q.num_transcripts
    start = np.where(tq._quantifier(name)[1].degree > 0, st["reads_used"] / T, 0.0)
    assert all(np.array_equal(a, start) for a in q.bootstrap_fetch()[0])               # N / T where the ORIGINAL table has a row
    done = 0
    for i in (0, 1, 2, 10, 49):
        q.bootstrap_step(i - done)
        before = q.bootstrap_fetch()[0]
        q.bootstrap_step(1)
        done = i + 1
        got = q.bootstrap_fetch()[0]
        for k in range(n):
            want = probs[k].step(before[k])
            tiny = want < 1e-290
            worst = float(np.max(np.abs(got[k][~tiny] - want[~tiny]) / want[~tiny])) if (~tiny).any() else 0.0
            print("%s replicate %d step %d: worst relative deviation %.3g (bound %.3g)" % (name, k, i, worst, tol))
            assert np.all(np.abs(got[k][~tiny] - want[~tiny]) <= tol * want[~tiny]), (name, k, i, worst, tol)
            assert np.all(got[k][tiny] < 1e-289)


@pytest.mark.parametrize("name", ["gencode_0", "synth", "repeats"])
def test_200_steps_against_the_long_double_model(name):
    """per replicate: GPU deviation <= 16 x D_ref, D_ref = the float64 model's deviation from the long-double model (floored at 2^-50),
    over the transcripts with alpha >= alpha_change_limit; both models start from the GPU's start"""
    n = 3
    q = _quantifier(name)
    q.bootstrap_draw(SEED, 0, n)
    probs = [_problem(name, *q.bootstrap_counts(k)) for k in range(n)]
    start = q.bootstrap_fetch()[0]
    q.bootstrap_step(200)
    got = q.bootstrap_fetch()[0]
    for k in range(n):
        a64 = probs[k].iterate(200, alpha=start[k])
        a80 = probs[k].iterate(200, np.longdouble, alpha=start[k])
        sel = np.asarray(a80, np.float64) >= 1e-2
        assert sel.any()
        ref = a80[sel]
        d_ref = max(float(np.max(np.abs(a64[sel].astype(np.longdouble) - ref) / ref)), 2.0 ** -50)
        d_gpu = float(np.max(np.abs(got[k][sel].astype(np.longdouble) - ref) / ref))
        print("%s replicate %d: D_ref %.3g, GPU %.3g, ratio %.3g" % (name, k, d_ref, d_gpu, d_gpu / d_ref))
        out = os.environ.get("PA_QUANT_BOOT_PARITY_JSON")
        if out:
            rec = json.load(open(out)) if os.path.exists(out) else {}
            rec["%s/%d" % (name, k)] = dict(d_ref=d_ref, d_gpu=d_gpu, ratio=d_gpu / d_ref, transcripts=int(sel.sum()))
            json.dump(rec, open(out, "w"), indent=1, sort_keys=True)
        assert d_gpu <= 16 * d_ref, (name, k, d_gpu, d_ref)


def _model_stop(p, start, par):
    a, i = start, 0
    while i < par.max_iters:
        new = p.step(a)
        i += 1
        if ((i >= par.min_iters and i % par.check_every == 0) or i == par.max_iters) and qm.stop_rule_holds(a, new, par.alpha_change_limit, par.alpha_change) and i >= par.min_iters:
            return i
        a = new
    return i


STOP_CASE, STOP_SEED, STOP_N = "gencode_0", SEED, 3   # the float64 model stops these three at 1110, 1040 and 1100


def test_stop_rule_and_freeze():
    name, n = STOP_CASE, STOP_N
    q = _quantifier(name)
    par = q.params
    q.bootstrap_draw(STOP_SEED, 0, n)
    start = q.bootstrap_fetch()[0]
    model_stops = [_model_stop(_problem(name, *q.bootstrap_counts(k)), start[k], par) for k in range(n)]
    print("float64 model stops:", model_stops)
    assert len(set(model_stops)) > 1                                                   # the replicates do not stop together: the freeze path runs
    iters, conv = q.bootstrap_run()
    final = q.bootstrap_fetch()[0]
    print("GPU stops:", iters.tolist())
    assert conv.all() and len(set(iters.tolist())) > 1
    for i in iters.tolist():
        assert i >= par.min_iters and (i % par.check_every == 0 or i == par.max_iters)
    assert np.all((final == 0) | (final >= par.alpha_limit / 10))
    # replay by determinism: one walk over every iterate that is needed
    need = set()
    for v in set(iters.tolist()):
        need |= {v - 1, v}
        if v - par.check_every >= par.min_iters:
            need |= {v - par.check_every - 1, v - par.check_every}
    q.bootstrap_draw(STOP_SEED, 0, n)
    snap, cur = {}, 0
    for i in sorted(need):
        q.bootstrap_step(i - cur)
        cur = i
        snap[i] = q.bootstrap_fetch()[0]
    for k in range(n):
        v = int(iters[k])
        prev, last = snap[v - 1][k], snap[v][k]
        assert qm.stop_rule_holds(prev, last, par.alpha_change_limit, par.alpha_change), k
        assert np.where(last < par.alpha_limit / 10, 0.0, last).tobytes() == final[k].tobytes(), k      # frozen at its own stop, untouched since
        if v - par.check_every >= par.min_iters:                                       # the check before did not hold
            assert not qm.stop_rule_holds(snap[v - par.check_every - 1][k], snap[v - par.check_every][k], par.alpha_change_limit, par.alpha_change), k


def test_max_iters_ends_unconverged_replicates():
    q = _quantifier("gencode_1", max_iters=7)
    q.bootstrap_draw(SEED, 0, 5)
    iters, conv = q.bootstrap_run()
    assert iters.tolist() == [7] * 5 and not conv.any()
    q.bootstrap_draw(SEED, 0, 5)
    q.bootstrap_step(7)
    last = q.bootstrap_fetch()[0]
    q.bootstrap_draw(SEED, 0, 5)
    q.bootstrap_run()
    assert np.array_equal(np.where(last < q.params.alpha_limit / 10, 0.0, last), q.bootstrap_fetch()[0])


@pytest.mark.parametrize("name", ["gencode_0", "repeats"])
def test_a_replicate_does_not_depend_on_its_batch(name):
    def outputs(q, first, n, ks):
        q.bootstrap_draw(SEED, first, n)
        counts = [np.concatenate(q.bootstrap_counts(k)).tobytes() for k in ks]
        q.bootstrap_step(200)
        stepped = q.bootstrap_fetch()[0]
        q.bootstrap_draw(SEED, first, n)
        iters, conv = q.bootstrap_run()
        est, tpm = q.bootstrap_fetch()
        return [(counts[j], stepped[k].tobytes(), est[k].tobytes(), tpm[k].tobytes(), int(iters[k]), bool(conv[k])) for j, k in enumerate(ks)]

    q = _quantifier(name)
    pair = outputs(q, 3, 2, [0, 1])
    assert pair == outputs(q, 0, 8, [3, 4])
    assert pair == outputs(q, 0, 64, [3, 4])
    assert pair == outputs(_quantifier(name), 3, 2, [0, 1])                            # another object: the same bytes
    assert pair[0][0] != pair[1][0]
    q.bootstrap_draw(SEED + 1, 3, 2)
    assert np.concatenate(q.bootstrap_counts(0)).tobytes() != pair[0][0]               # another seed: other counts


def test_nothing_of_the_point_estimate_moves():
    q1, q2 = _quantifier("gencode_2"), _quantifier("gencode_2")
    q1.step(3)
    q2.step(3)
    q1.bootstrap_draw(SEED, 0, 5)
    q1.bootstrap_step(4)
    q1.bootstrap_run()
    q1.bootstrap_fetch()
    assert q1.alpha().tobytes() == q2.alpha().tobytes() and q1.stats() == q2.stats()
    assert q1.run() == q2.run()
    assert q1.alpha().tobytes() == q2.alpha().tobytes() and q1.stats() == q2.stats()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(q1.fetch(), q2.fetch()))


def test_errors():
    E = pa._ffi
    index, counts, words, _ = _case("gencode_2")
    q = _quantifier("gencode_2")

    def fails(code, fn, *args):
        with pytest.raises(pa.PaError) as e:
            fn(*args)
        assert e.value.code == code, e.value
        return str(e.value)

    for fn, args in ((q.bootstrap_step, (1,)), (q.bootstrap_run, ()), (q.bootstrap_fetch, ()), (q.bootstrap_counts, (0,))):
        assert "no bootstrap batch drawn" in fails(E.PA_ERR_INVALID_ARG, fn, *args)
    fails(E.PA_ERR_INVALID_ARG, q.bootstrap_draw, SEED, 0, 0)
    fails(E.PA_ERR_INVALID_ARG, q.bootstrap_draw, SEED, 0, E.PA_QUANT_BOOT_MAX_BATCH + 1)
    fails(E.PA_ERR_INVALID_ARG, q.bootstrap_draw, SEED, 2 ** 32 - 4, 5)
    q.bootstrap_draw(SEED, 2 ** 32 - 5, 5)
    q.bootstrap_step(2)
    before = q.bootstrap_fetch()[0]
    fails(E.PA_ERR_INVALID_ARG, q.bootstrap_counts, 5)
    fails(E.PA_ERR_INVALID_ARG, q.bootstrap_draw, SEED, 0, 65)                         # a failed call leaves the batch as it was
    assert q.bootstrap_fetch()[0].tobytes() == before.tobytes()
    cc = np.zeros(len(counts) - 1, np.uint64)
    assert pa.lib().pa_quant_bootstrap_counts(q._h, 0, cc.ctypes.data, len(cc), None, 0) == E.PA_ERR_INVALID_ARG
    q.set_counts(counts, words)                                                        # drops the batch
    assert "no bootstrap batch drawn" in fails(E.PA_ERR_INVALID_ARG, q.bootstrap_fetch)
    big = counts.copy()
    big[int(np.flatnonzero(counts[:-3] > 0)[0])] = 2 ** 32
    q.set_counts(big, words)
    fails(E.PA_ERR_UNSUPPORTED, q.bootstrap_draw, SEED, 0, 1)
    iters, converged = q.run()                                                         # the point estimate of that table still works
    assert iters >= q.params.min_iters and converged


def test_outputs():
    name = "gencode_3"
    q = _quantifier(name)
    q.bootstrap_draw(SEED, 0, 5)
    q.bootstrap_run()
    est, tpm = q.bootstrap_fetch()
    eff = q.fetch()[2]
    N = q.stats()["reads_used"]
    for k in range(5):
        assert np.array_equal(tpm[k], qm.tpm(est[k], eff))
        assert abs(float(est[k].sum()) - N) <= 1e-6 * N
    got, iters, conv = q.bootstrap(20, SEED, batch=8)
    assert got.shape == (20, q.num_transcripts) and conv.all()
    for first, n in ((0, 8), (8, 8), (16, 4)):
        q.bootstrap_draw(SEED, first, n)
        it, _ = q.bootstrap_run()
        assert q.bootstrap_fetch()[0].tobytes() == got[first:first + n].tobytes() and it.tolist() == iters[first:first + n].tolist()
    assert got[:5].tobytes() == est.tobytes()


def test_c_client_runs_the_bootstrap_calls(tmp_path):
    import subprocess
    exe = helpers._build.build_abi_check()
    src = (helpers.ROOT / "integration" / "c" / "abi_check.c").read_text()
    for fn in ("draw", "counts", "step", "run", "fetch"):
        assert "pa_quant_bootstrap_%s(qq" % fn in src
    out = subprocess.run([str(exe), str(helpers.FASTA), str(helpers.FASTQ), str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "device halves ok" in out.stdout and "0 failures" in out.stdout, out.stdout + out.stderr
