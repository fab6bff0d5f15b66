"""Transcript abundances on the GPU (pa_quant_*) against the numpy model of tests/quant_model.py: one step is the EM map (a derived
bound), 200 steps against the long-double model (16 x the float64 model's own order noise), the stop rule on the GPU's own iterates,
bit-identical repeats, outputs, errors. Inputs: 12 seeded tables over gencode_small (K = 24), the synthetic transcriptome of
test_gpu_cells.py, a repeat-family transcriptome with a row and a degree beyond 2 000, an empty table, a table with one class, and
the table + overflow of a real mapping of 200 k simulated reads."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import helpers
import quant_model as qm

pa = helpers.pa
pytestmark = pytest.mark.gpu

EPS = 2.0 ** -53
STEP_POINTS = (0, 1, 2, 10, 49, 200)
_cache = {}


def _index(name):
    """(host index, aligner, HostIndex.arrays(), transcript lengths)"""
    if name not in _cache:
        if name == "gencode":
            host = pa.build_index(str(helpers.FASTA), 24, 8)
        elif name == "synth":
            host = pa.HostIndex.from_txome(pa.Txome.synthesize(120, 400, 11), 24, 8)
        else:   # one repeat family, no divergence, in every gene: its k-mers are shared by thousands of transcripts
            tx = pa.Txome.synthesize_repeats(1500, 5000, 5, families=1, element_len=300, div_lo_ppm=0, div_hi_ppm=0, young_families=0,
                                             gene_fraction_ppm=1000000, low_complexity_genes=0)
            host = pa.HostIndex.from_txome(tx, 24, 8)
        _cache[name] = (host, pa.Pseudoaligner(host), host.arrays(), np.diff(host.transcripts()[1].astype(np.int64)))
    return _cache[name]


def _real_mapping():
    """200 k simulated reads of gencode_small with 1 % substitutions through map_count_batch_device with an overflow attached; the table
    is the oracle's (as in test_gpu_parity.py) and the overflow records are the oracle's novel classes"""
    import torch
    host, a, arr, _ = _index("gencode")
    tx = pa.Txome.from_host_index(host)
    n, wpr = 200_000, 4
    dev = torch.device("cuda", 0)
    h_tiles, h_lens = tx.simulate_host(100, 11, n, 10000, 0, wpr)
    d_tiles = torch.from_numpy(h_tiles.view(np.int64)).to(dev)
    d_lens = torch.from_numpy(h_lens.view(np.int32)).to(dev)
    cap = a.arena_hint(n)
    d_res = torch.zeros(n * 4, dtype=torch.int32, device=dev)
    d_arena = torch.zeros(cap, dtype=torch.int32, device=dev)
    d_counts = torch.zeros(a.counts_len(), dtype=torch.int64, device=dev)
    ovf = pa.Overflow(0, 1 << 16, 1 << 22)
    a.set_overflow(ovf)
    try:
        a.map_count_batch_device(d_tiles.data_ptr(), d_lens.data_ptr(), n, wpr, d_res.data_ptr(), d_arena.data_ptr(), cap, d_counts.data_ptr(), 2)
        a.map_finish()
        counts = d_counts.cpu().numpy().astype(np.uint64)
        words = ovf.fetch()
    finally:
        a.set_overflow(None)
    o_res, o_coff, o_ids, _ = helpers.Oracle(host).map_tiles(h_tiles, h_lens, wpr, 2, 8)
    assert np.array_equal(counts, helpers.counts_reference(o_res, o_coff, o_ids, host).astype(np.uint64))
    want = helpers.novel_reference(o_res, o_coff, o_ids, host)
    assert len(want) > 0 and pa.parse_overflow(words) == want and sum(want.values()) == int(counts[-3])
    return counts, words


def _case(name):
    """(index name, class_counts, overflow words or None, mean_read_len); every named property is checked here, on the CPU"""
    key = ("case", name)
    if key in _cache:
        return _cache[key]
    if name.startswith("gencode_"):
        arr = _index("gencode")[2]
        counts, words = qm.random_table(arr, 100 + int(name.split("_")[1]), 0.5, 60)
        assert qm.multi_fraction(arr, counts, words) >= 0.30 and len(qm.read_overflow(words)) >= 50
        out = ("gencode", counts, words, 75.0)
    elif name == "synth":
        arr = _index("synth")[2]
        counts, words = qm.random_table(arr, 7, 0.4, 80)
        out = ("synth", counts, words, 0.0)
    elif name == "repeats":
        arr = _index("repeats")[2]
        lens = np.diff(arr["ec_offset"].astype(np.int64))
        assert lens.max() >= 2000, "longest class %d" % lens.max()
        counts, words = qm.random_table(arr, 9, 0.2, 60, hub=3, hub_records=2400)
        counts[int(np.argmax(lens))] = 12345                               # the family's class is counted
        out = ("repeats", counts, words, 100.0)
    elif name == "zero":
        arr = _index("gencode")[2]
        out = ("gencode", np.zeros(arr["num_classes"] + 3, np.uint64), qm.write_overflow([]), 0.0)
    elif name == "one_class":
        arr = _index("gencode")[2]
        counts = np.zeros(arr["num_classes"] + 3, np.uint64)
        lens = np.diff(arr["ec_offset"].astype(np.int64))
        counts[int(np.flatnonzero(lens >= 2)[0])] = 1000
        counts[-1] = 17                                                    # unmapped reads never take part
        out = ("gencode", counts, None, 0.0)
    else:
        assert name == "mapped"
        counts, words = _real_mapping()
        out = ("gencode", counts, words, 100.0)
    _cache[key] = out
    return out


CASES = ["gencode_%d" % i for i in range(12)] + ["synth", "repeats", "zero", "one_class", "mapped"]
LIGHT = ["gencode_0", "gencode_5", "synth", "repeats", "one_class", "mapped"]


def _quantifier(name, **params):
    index, counts, words, mrl = _case(name)
    host, a, arr, tx_len = _index(index)
    params.setdefault("mean_read_len", mrl)
    q = pa.Quantifier(a, host, **params)
    q.set_counts(counts, words)
    return q, qm.Problem.from_table(arr, tx_len, counts, words, mean_read_len=params["mean_read_len"])


def _step_tolerance(st):
    return 4 * (st["longest_row"] + st["largest_degree"] + 4) * EPS


@pytest.mark.parametrize("name", CASES)
def test_one_step_is_the_em_map(name):
    q, p = _quantifier(name)
    st = q.stats()
    assert (st["rows"], st["ids"], st["reads_used"], st["longest_row"], st["largest_degree"]) == (len(p.rows), len(p.ids), p.N, p.m_max, p.d_max)
    assert st["transcripts_with_a_row"] == int((p.degree > 0).sum()) and st["novel_reads_left_out"] == (0 if _case(name)[2] is not None else int(_case(name)[1][-3]))
    if name == "repeats":
        assert st["longest_row"] >= 2000 and st["largest_degree"] >= 2000          # the workgroup-per-row path runs in both passes
    tol = _step_tolerance(st)
    assert np.array_equal(q.alpha(), p.start())
    done = 0
    for i in STEP_POINTS:
        q.step(i - done)
        done = i
        before = q.alpha()
        want = p.step(before)                                                      # one model step from the GPU's own alpha_i
        q.step(1)
        done += 1
        got = q.alpha()
        tiny = want < 1e-290
        worst = float(np.max(np.abs(got[~tiny] - want[~tiny]) / np.where(want[~tiny] > 0, want[~tiny], 1.0))) if (~tiny).any() else 0.0
        print("%s step %d: worst relative deviation %.3g (bound %.3g)" % (name, i, worst, tol))
        assert np.all(np.abs(got[~tiny] - want[~tiny]) <= tol * want[~tiny]), (name, i, worst, tol)
        assert np.all(got[tiny] < 1e-289)
    assert q.stats()["iterations"] == (done if p.N else 0)                         # N = 0: no iteration is ever run


@pytest.mark.parametrize("name", CASES)
def test_200_steps_against_the_long_double_model(name):
    """GPU deviation <= 16 x D_ref, D_ref = the float64 model's deviation from the long-double model (floored at 2^-50), over the
    transcripts with alpha >= alpha_change_limit"""
    q, p = _quantifier(name)
    q.step(200)
    got = q.alpha()
    a64 = p.iterate(200)
    a80 = p.iterate(200, np.longdouble)
    sel = np.asarray(a80, np.float64) >= 1e-2
    if not p.N:
        assert not got.any() and q.stats()["iterations"] == 0
        return
    assert sel.any()
    ref = a80[sel]
    d_ref = max(float(np.max(np.abs(a64[sel].astype(np.longdouble) - ref) / ref)), 2.0 ** -50)
    d_gpu = float(np.max(np.abs(got[sel].astype(np.longdouble) - ref) / ref))
    print("%s: D_ref %.3g, GPU %.3g" % (name, d_ref, d_gpu))
    out = os.environ.get("PA_QUANT_PARITY_JSON")
    if out:
        rec = json.load(open(out)) if os.path.exists(out) else {}
        rec[name] = dict(d_ref=d_ref, d_gpu=d_gpu, rows=len(p.rows), ids=len(p.ids), longest_row=p.m_max, largest_degree=p.d_max, transcripts=int(sel.sum()))
        json.dump(rec, open(out, "w"), indent=1, sort_keys=True)
    assert d_gpu <= 16 * d_ref, (name, d_gpu, d_ref)


@pytest.mark.parametrize("name", LIGHT)
def test_stop_rule(name):
    q, p = _quantifier(name)
    par = q.params
    iters, converged = q.run()
    final = q.alpha()
    assert iters >= par.min_iters and (iters % par.check_every == 0 or iters == par.max_iters) and converged
    assert np.all((final == 0) | (final >= par.alpha_limit / 10))
    index, counts, words, _ = _case(name)
    q.set_counts(counts, words)                                                    # back to the start: determinism makes the replay legitimate
    q.step(iters - 1)
    prev = q.alpha()
    q.step(1)
    last = q.alpha()
    assert np.array_equal(np.where(last < par.alpha_limit / 10, 0.0, last), final)
    assert qm.stop_rule_holds(prev, last, par.alpha_change_limit, par.alpha_change)
    if iters - par.check_every >= par.min_iters:                                   # the check before did not stop the run
        q.set_counts(counts, words)
        q.step(iters - par.check_every - 1)
        prev = q.alpha()
        q.step(1)
        assert not qm.stop_rule_holds(prev, q.alpha(), par.alpha_change_limit, par.alpha_change)


def test_max_iters_ends_an_unconverged_run():
    q, p = _quantifier("gencode_1", max_iters=7)
    iters, converged = q.run()
    assert iters == 7 and not converged
    a = p.start()
    for _ in range(6):
        a = p.step(a)
    assert not qm.stop_rule_holds(a, p.step(a))                                     # the table does need more
    q2, _ = _quantifier("zero")
    assert q2.run() == (0, True) and not q2.alpha().any() and not q2.fetch()[1].any()


@pytest.mark.parametrize("name", ["gencode_2", "repeats", "mapped"])
def test_repeats_are_bit_identical(name):
    q1, _ = _quantifier(name)
    q2, _ = _quantifier(name)
    q1.step(200)
    q2.step(200)
    a1 = q1.alpha()
    assert a1.tobytes() == q2.alpha().tobytes()
    index, counts, words, _ = _case(name)
    q1.set_counts(counts, words)
    assert q1.stats()["iterations"] == 0
    q1.step(200)
    assert q1.alpha().tobytes() == a1.tobytes()


@pytest.mark.parametrize("name", ["gencode_3", "synth", "mapped"])
def test_outputs(name, tmp_path):
    q, p = _quantifier(name)
    q.run()
    est, tpm, eff = q.fetch()
    host = _index(_case(name)[0])[0]
    assert np.array_equal(eff, p.eff) and np.array_equal(est, q.alpha())
    assert abs(float(qm.fsum_ld(est)) - p.N) <= p.step_bound() * p.N + p.T * q.params.alpha_limit / 10     # (+ what the truncation may remove)
    assert abs(float(qm.fsum_ld(tpm)) - 1e6) <= p.T * 2.0 ** -52 * 1e6
    assert np.array_equal(tpm, qm.tpm(est, eff))
    tx_gene, names = host.genes()
    g_est, g_tpm = q.genes()
    want_e, want_t = np.zeros(len(names)), np.zeros(len(names))
    if names:                                                                      # (a synthesized transcriptome carries no gene names: no genes)
        np.add.at(want_e, tx_gene, est)                                            # transcript order
        np.add.at(want_t, tx_gene, tpm)
    else:
        assert name == "synth"
    assert np.array_equal(g_est, want_e) and np.array_equal(g_tpm, want_t)
    path = tmp_path / "abundance.tsv"
    q.write_tsv(str(path))
    lines = path.read_text().split("\n")
    assert lines[0] == "target_id\tlength\teff_length\test_counts\ttpm" and lines[-1] == "" and len(lines) == p.T + 2
    tx_names, tx_len = host.tx_names(), np.diff(host.transcripts()[1].astype(np.int64))
    for t, line in enumerate(lines[1:-1]):
        f = line.split("\t")
        assert f[0] == tx_names[t] and int(f[1]) == tx_len[t] and "e" not in line.lower().split("\t", 1)[1]
        assert (float(f[2]), float(f[3]), float(f[4])) == (eff[t], est[t], tpm[t])


def test_quantify_from_a_device_table():
    import torch
    index, counts, words, _ = _case("gencode_4")
    host, a, arr, tx_len = _index(index)
    d_counts = torch.from_numpy(counts.view(np.int64)).to("cuda:0")
    q = a.quantify(d_counts.data_ptr(), None, mean_read_len=50.0)
    assert q.converged and q.stats()["novel_reads_left_out"] == int(counts[-3])
    p = qm.Problem.from_table(arr, tx_len, counts, None, mean_read_len=50.0)
    assert abs(float(q.fetch()[0].sum()) - p.N) <= 1e-6 * p.N


def test_errors_leave_the_quantifier_usable():
    q, p = _quantifier("gencode_6")
    index, counts, words, _ = _case("gencode_6")
    host, a, arr, _ = _index(index)
    q.step(3)
    before = q.alpha()
    E = pa._ffi

    def fails(code, c, w):
        with pytest.raises(pa.PaError) as e:
            q.set_counts(c, w)
        assert e.value.code == code, e.value
        assert np.array_equal(q.alpha(), before) and q.stats()["iterations"] == 3  # as it was

    bad = counts.copy()
    bad[-3] += 1
    fails(E.PA_ERR_INVALID_ARG, bad, words)                                          # overflow total != novel slot
    fails(E.PA_ERR_INVALID_ARG, counts[:-1], words)                                  # counts_len != pa_counts_len
    recs = qm.read_overflow(words)
    recs[0] = (np.array([0, arr["num_transcripts"]], np.uint32), recs[0][1])
    fails(E.PA_ERR_INVALID_ARG, counts, qm.write_overflow(recs))                     # a record id >= T
    big = counts.copy()
    big[0] = 1 << 53
    fails(E.PA_ERR_UNSUPPORTED, big, words)
    other = pa.build_index(str(helpers.FASTA), 20, 8)
    with pytest.raises(pa.PaError) as e:
        pa.Quantifier(a, other)                                                      # h of another index
    assert e.value.code == E.PA_ERR_INVALID_ARG
    with pytest.raises(pa.PaError) as e:
        pa.Quantifier(None, host)
    assert e.value.code == E.PA_ERR_INVALID_ARG
    tol = _step_tolerance(q.stats())                                                 # still usable: its next steps are the EM map
    for _ in range(2):
        want = p.step(q.alpha())
        q.step(1)
        assert np.all(np.abs(q.alpha() - want) <= tol * want)
    assert q.stats()["iterations"] == 5


def test_c_client_runs_the_new_calls(tmp_path):
    import subprocess
    exe = helpers._build.build_abi_check()
    out = subprocess.run([str(exe), str(helpers.FASTA), str(helpers.FASTQ), str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "device halves ok" in out.stdout and "0 failures" in out.stdout, out.stdout + out.stderr
    assert (tmp_path / "abi_check_abundance.tsv").read_text().startswith("target_id\tlength\t")
    assert "pa_quant_run(" in (helpers.ROOT / "integration" / "c" / "abi_check.c").read_text()
