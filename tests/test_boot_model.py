"""The numpy model of the bootstrap resampler (tests/boot_model.py) against the rule text of include/pseudoaligner_amd.h: the Philox
known answers, the edges of the pick, the use of the last block, and a sanity check of the rule itself (CPU only)."""
import numpy as np

import boot_model as bm

KNOWN = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
         ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
         ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1")]


def test_philox_known_answers():
    for counter, key, want in KNOWN:
        got = bm.philox4x32_10(counter, key)
        assert " ".join("%08x" % int(w[0]) for w in got) == want
    # vectorised over counters: the same words as one at a time
    many = bm.philox4x32_10((np.arange(5), 0, 7, 0), (1, 2))
    for i in range(5):
        one = bm.philox4x32_10((i, 0, 7, 0), (1, 2))
        assert [int(w[i]) for w in many] == [int(w[0]) for w in one]


def test_header_states_the_known_answers():
    import helpers
    text = (helpers.ROOT / "include" / "pseudoaligner_amd.h").read_text()
    assert "bootstrap replicates" in text
    for _, _, want in KNOWN:
        assert want in text


def test_pick_edges():
    for N in (1, 2, 63, 1000, 2 ** 32 - 1):
        p = bm.picks(np.array([0, 2 ** 64 - 1, 2 ** 63], np.uint64), N)
        assert int(p[0]) == 0 and int(p[1]) == N - 1 and int(p[2]) == N // 2
    x = np.random.default_rng(1).integers(0, 2 ** 64, 2000, dtype=np.uint64)
    for N in (3, 12345, 2 ** 32 - 1):
        assert [int(v) for v in bm.picks(x, N)] == [(int(v) * N) >> 64 for v in x]      # against Python's integers


def test_counts_sum_to_n_and_stay_zero_where_the_table_is_zero():
    rng = np.random.default_rng(3)
    cand = rng.integers(0, 50, 400).astype(np.uint64)
    cand[rng.random(400) < 0.4] = 0
    cand[0] = cand[-1] = 0
    N = int(cand.sum())
    for b in (0, 1, 2 ** 32 - 1):
        rep = bm.resample(cand, 99, b)
        assert int(rep.sum()) == N and not rep[cand == 0].any()
    assert not np.array_equal(bm.resample(cand, 99, 0), bm.resample(cand, 99, 1))
    assert not np.array_equal(bm.resample(cand, 99, 0), bm.resample(cand, 100, 0))
    assert np.array_equal(bm.resample(cand, 99, 5), bm.resample(cand, 99, 5))
    assert not bm.resample(np.zeros(7, np.uint64), 1, 0).any()                         # N = 0


def test_interval_edges():
    cand = np.array([0, 3, 0, 0, 1, 2, 0], np.uint64)                                  # reads 0..2 -> 1, 3 -> 4, 4..5 -> 5
    got = bm.counts_of_picks(cand, np.arange(6, dtype=np.uint64))
    assert got.tolist() == [0, 3, 0, 0, 1, 2, 0]


def test_an_odd_n_uses_half_of_the_last_block():
    seed, b = 5, 9
    for N in (1, 7, 63):
        x = bm.draw_values(seed, b, N)
        assert len(x) == N
        last = bm.philox4x32_10(((N - 1) >> 1, 0, b, 0), (seed, 0))
        assert int(x[-1]) == int(last[0][0]) | (int(last[1][0]) << 32)                 # the even draw of block (N - 1) / 2: o0 | o1 << 32
        if N > 1:
            prev = bm.philox4x32_10(((N - 2) >> 1, 0, b, 0), (seed, 0))
            assert int(x[-2]) == int(prev[2][0]) | (int(prev[3][0]) << 32)             # an odd draw: o2 | o3 << 32
    big = bm.draw_values(seed | (3 << 32), b, 8)
    blk = bm.philox4x32_10((3, 0, b, 0), (seed, 3))                                    # the key is (lo32(seed), hi32(seed))
    assert int(big[6]) == int(blk[0][0]) | (int(blk[1][0]) << 32)


def test_n_equal_one_draws_the_candidate_of_read_zero():
    cand = np.array([0, 0, 1, 0], np.uint64)
    for b in range(8):
        assert bm.resample(cand, 1234, b).tolist() == [0, 0, 1, 0]


def test_replicate_means_stay_near_the_table():
    """64 replicates of a 300-row table with one row of 40 % of the reads: the mean of every non-empty row within 5 standard errors of
    n_r (a multinomial count has variance n_r (1 - n_r / N)); a fixed seed, so this is deterministic"""
    rng = np.random.default_rng(11)
    cand = rng.integers(1, 400, 300).astype(np.uint64)
    cand[rng.random(300) < 0.2] = 0
    rest = int(cand.sum())
    cand[17] = int(rest * 0.4 / 0.6)
    N = int(cand.sum())
    reps = np.stack([bm.resample(cand, 2024, b) for b in range(64)]).astype(np.float64)
    n = cand.astype(np.float64)
    se = np.sqrt(n * (1 - n / N) / 64)
    sel = cand > 0
    z = np.abs(reps.mean(axis=0)[sel] - n[sel]) / se[sel]
    print("worst deviation of a row's mean: %.2f standard errors" % z.max())
    assert z.max() <= 5.0 and not reps[:, ~sel].any()


def test_replicate_table_and_overflow_words():
    import quant_model as qm
    words = qm.write_overflow([((1, 2), 5), ((0, 3, 4), 7)])
    arrays = dict(num_classes=3, ec_offset=np.array([0, 1, 1, 3], np.uint64))
    cand = bm.candidate_counts(arrays, np.array([4, 9, 2, 12, 1, 1], np.uint64), words)
    assert cand.tolist() == [4, 0, 2, 7, 5]                                            # class 1 has no entries; the records in (canonical) record order
    cc, oc = bm.replicate_table(arrays, words, np.array([3, 0, 1, 9, 5], np.uint64))
    assert cc.tolist() == [3, 0, 1, 14, 0, 0] and oc.tolist() == [9, 5]
    assert [c for _, c in qm.read_overflow(bm.overflow_with_counts(words, oc))] == [9, 5]


def test_rust_quant_binding_matches_the_header(monkeypatch):
    """integration/rust/src/amd_quant_ffi.rs cannot be compiled here (no rustc): every prototype of it, the bootstrap calls among
    them, and its constants are compared with the header signature by signature, as tests/test_abi.py does for amd_ffi.rs"""
    import abi_sigs
    import helpers
    monkeypatch.setitem(abi_sigs.RUST_SCALARS, "PaQuant", "pa_quant")
    monkeypatch.setitem(abi_sigs.RUST_SCALARS, "PaQuantParams", "pa_quant_params")
    header = (helpers.ROOT / "include" / "pseudoaligner_amd.h").read_text()
    rust = (helpers.ROOT / "integration" / "rust" / "src" / "amd_quant_ffi.rs").read_text()
    hp, rp = abi_sigs.header_prototypes(header), abi_sigs.rust_prototypes(rust)
    for fn in ("draw", "counts", "step", "run", "fetch"):
        assert "pa_quant_bootstrap_" + fn in rp
    for name, sig in rp.items():
        assert hp.get(name) == sig, "%s: Rust says %s, the header %s" % (name, sig, hp.get(name))
    hc = abi_sigs.header_consts(header)
    for name, value in abi_sigs.rust_consts(rust).items():
        assert hc.get(name) == value, (name, value, hc.get(name))
    # not vacuous: a drifted bootstrap prototype is caught
    for bad_from, bad_to in (("seed: u64, first: u32, n: u32", "seed: u32, first: u32, n: u32"),
                             ("k: u32, class_counts: *mut u64, counts_len: u64", "class_counts: *mut u64, k: u32, counts_len: u64")):
        assert bad_from in rust
        assert any(hp[n] != s for n, s in abi_sigs.rust_prototypes(rust.replace(bad_from, bad_to, 1)).items())


def test_rust_bootstrap_wrapper_calls_what_the_binding_declares():
    """amd::quantify_bootstrap (uncompiled here): every pa_* it calls is declared in a binding file with that many arguments, and a
    batch's outputs go to the slices that start at its first replicate (iters[first..], est[first * t..])"""
    import re
    import abi_sigs
    import helpers
    src = helpers.ROOT / "integration" / "rust" / "src"
    text = (src / "amd.rs").read_text()
    body = text[text.index("pub fn quantify_bootstrap("):]
    body = body[: body.index("\n}\n") + 3]
    arity = {}
    for f in ("amd_ffi.rs", "amd_quant_ffi.rs"):
        decl = re.sub(r"//.*$", "", (src / f).read_text(), flags=re.M)
        for m in re.finditer(r"pub fn (pa_\w+)\s*\(([^)]*)\)", decl):
            arity[m.group(1)] = len(abi_sigs.split_args(m.group(2)))
    calls = re.findall(r"\b(pa_\w+)\(", body)
    assert [c for c in calls if c.startswith("pa_quant_bootstrap_")] == ["pa_quant_bootstrap_draw", "pa_quant_bootstrap_run", "pa_quant_bootstrap_fetch"]
    for m in re.finditer(r"\b(pa_\w+)\(", body):
        depth, i = 1, m.end()
        while depth:
            depth += {"(": 1, ")": -1}.get(body[i], 0)
            i += 1
        assert len(abi_sigs.split_args(body[m.end():i - 1])) == arity[m.group(1)], m.group(1)
    assert "iters[first as usize..].as_mut_ptr()" in body and "est[first as usize * t..].as_mut_ptr()" in body
    assert "vec![0f64; n as usize * t]" in body and "vec![0u32; n as usize]" in body and "first += m;" in body
