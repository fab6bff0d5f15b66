"""The paired-end model (tests/pairs_model.py) against itself and the oracle, without a GPU: the reverse complement is an involution, the
pair rule is the header's table, error-free FR pairs map to their transcript under "fr" and not all of them under "ff", and the
end-to-end cases of tests/test_gpu_pairs.py reach every fate on the model's side."""
import numpy as np
import pytest

import helpers
import pairs_model as pm


def test_revcomp_is_an_involution_and_keeps_padding_zero():
    rng = np.random.default_rng(1)
    for n in (1, 2, 31, 32, 33, 63, 64, 65, 95, 96, 97, 150, 1000):
        codes = rng.integers(0, 4, n).astype(np.uint8)
        words = helpers.pack_bases(codes)
        words[(n + 31) // 32:] = np.uint64(0xFFFFFFFFFFFFFFFF)            # garbage beyond the read's words ...
        if n & 31:
            words[n >> 5] |= np.uint64(0xFFFFFFFFFFFFFFFF) << np.uint64(2 * (n & 31))   # ... and beyond its length in the last one
        rc = pm.revcomp_packed(words, n)
        assert len(rc) == (n + 31) // 32
        got = helpers.unpack_bases(rc, n)
        assert np.array_equal(got, 3 - codes[::-1])
        if n & 31:
            assert int(rc[-1]) >> (2 * (n & 31)) == 0
        assert np.array_equal(helpers.unpack_bases(pm.revcomp_packed(rc, n), n), codes)
    assert pm.revcomp_text("ACGTTn") == "nAACGT"
    # an N the encoder packed as A comes out as T
    tiles, lens, wpr = helpers.pack_reads_tiles(["ACNT"])
    assert helpers.unpack_bases(pm.revcomp_tiles(tiles, lens, wpr).reshape(-1, wpr, 64)[0, :, 0], 4).tolist() == [0, 3, 2, 3]


def test_pair_rule_table():
    assert pm.pair_rule(None, None) is None
    assert pm.pair_rule(([1, 5], 40, 1), None) == ([1, 5], 40, 1)
    assert pm.pair_rule(None, ([], 33, 0)) == ([], 33, 0)
    assert pm.pair_rule(([1, 5, 9], 40, 1), ([0, 5, 9, 11], 50, 2)) == ([5, 9], 90, 3)
    assert pm.pair_rule(([1, 5], 40, 1), ([2, 6], 50, 2)) == ([], 90, 3)
    assert pm.pair_rule(([], 40, 0), ([2, 6], 50, 0)) == ([], 90, 0)
    m1 = [None, ([1, 5], 40, 1), None, ([1, 5, 9], 40, 1), ([1], 32, 0)]
    m2 = [None, None, ([7], 33, 2), ([5, 9], 50, 2), ([2], 32, 0)]
    res, coff, ids, st = pm.combine(m1, m2)
    assert coff.tolist() == [0, 0, 2, 3, 5, 5] and ids.tolist() == [1, 5, 7, 5, 9]
    assert (res["mismatches"] >> 31).tolist() == [0, 1, 1, 1, 1] and (res["mismatches"] & 0x7FFFFFFF).tolist() == [0, 1, 2, 3, 0]
    assert res["coverage"].tolist() == [0, 40, 33, 90, 64] and res["class_len"].tolist() == [0, 2, 1, 2, 0]
    assert st == dict(pairs=5, both_mapped=2, mate1_only=1, mate2_only=1, neither=1, both_mapped_empty=1, by_reference=0, in_arena=0)


def test_records_model_reads_both_forms(small_index):
    a = small_index(20).arrays()
    off = a["ec_offset"].astype(np.int64)
    c = int(np.argmax(off[1:] - off[:-1]))
    rec = np.zeros(3, pm.RESULT_DTYPE)
    rec[0] = (50, pm.MAPPED_BIT | 1, pm.CLASS_REF | c, off[c + 1] - off[c])
    rec[1] = (40, pm.MAPPED_BIT, 1, 2)
    m = pm.mates_from_records(rec, np.array([9, 3, 4], np.uint32), a)
    assert m[0] == (a["ec_ids"][off[c]:off[c + 1]].tolist(), 50, 1) and m[1] == ([3, 4], 40, 0) and m[2] is None


@pytest.mark.parametrize("k", [20, 31])
def test_error_free_fr_pairs_map_to_their_transcript(small_index, k):
    host = small_index(k)
    txs = pm.transcripts_text(host)
    r1, r2, src = pm.simulate_pairs(txs, 300, seed=3)
    res, coff, ids, st, m1, m2 = pm.model_pairs(host, r1, r2, "fr")
    coff = coff.astype(np.int64)
    assert st["both_mapped"] == 300
    for i in range(300):
        assert int(src[i]) in ids[coff[i]:coff[i + 1]], i
    # non-vacuity: the same pairs taken as "ff" leave mate 2 on the wrong strand
    res_ff, coff_ff, ids_ff, st_ff, _, _ = pm.model_pairs(host, r1, r2, "ff")
    assert st_ff["both_mapped"] < 300
    differ = [i for i in range(300) if ids_ff[int(coff_ff[i]):int(coff_ff[i + 1])].tolist() != ids[coff[i]:coff[i + 1]].tolist() or res_ff[i] != res[i]]
    assert differ


def test_end_to_end_cases_reach_every_fate(small_index):
    import pairs_cases
    for name in pairs_cases.CASES:
        host, r1, r2, orient = pairs_cases.case(name, small_index)
        res, coff, ids, st, m1, m2 = pm.model_pairs(host, r1, r2, orient)
        assert pm.fates(res, coff, ids, m1, m2, host) == pm.ALL_FATES, (name, pm.fates(res, coff, ids, m1, m2, host))
        pm.check_stats(dict(st, by_reference=0, in_arena=int(((res["mismatches"] >> 31) & (res["class_len"] > 0)).sum())), res)


def test_rust_pairs_binding_matches_the_header():
    """integration/rust/src/amd_pairs_ffi.rs cannot be compiled here: every prototype and constant of it against the header, as tests/test_abi.py
    does for amd_ffi.rs; and amd::map_pairs calls what it declares with that many arguments"""
    import re
    import abi_sigs
    src = helpers.ROOT / "integration" / "rust" / "src"
    header = (helpers.ROOT / "include" / "pseudoaligner_amd.h").read_text()
    rust = (src / "amd_pairs_ffi.rs").read_text()
    hp, rp = abi_sigs.header_prototypes(header), abi_sigs.rust_prototypes(rust)
    assert set(rp) == {"pa_revcomp_tiles_device", "pa_pairs_scratch_bytes", "pa_pairs_combine_device", "pa_pairs_finish", "pa_map_pairs", "pa_count_pairs"}
    for name, sig in rp.items():
        assert hp.get(name) == sig, "%s: Rust says %s, the header %s" % (name, sig, hp.get(name))
    hc = abi_sigs.header_consts(header)
    rc = {m.group(1): int(m.group(2)) for m in re.finditer(r"pub const (PA_\w+)\s*:\s*\w+\s*=\s*(\d+)\s*;", rust)}
    assert rc == {k: hc[k] for k in ("PA_PAIR_FR", "PA_PAIR_RF", "PA_PAIR_FF", "PA_PAIR_STATS")}
    drift = rust.replace("n_pairs: u64,\n                        orient: c_int", "n_pairs: u32,\n                        orient: c_int", 1)
    assert drift != rust and any(hp[n] != s for n, s in abi_sigs.rust_prototypes(drift).items())
    body = (src / "amd.rs").read_text()
    body = body[body.index("pub fn map_pairs("):]
    body = body[: body.index("\n}\n")]
    m = re.search(r"\bpa_map_pairs\(", body)
    depth, i = 1, m.end()
    while depth:
        depth += {"(": 1, ")": -1}.get(body[i], 0)
        i += 1
    assert len(abi_sigs.split_args(body[m.end():i - 1])) == len(rp["pa_map_pairs"][1])
    body = (src / "amd.rs").read_text()
    body = body[body.index("pub fn count_pairs<"):]
    body = body[: body.index("\n}\n")]
    m = re.search(r"\bpa_count_pairs\(", body)
    depth, i = 1, m.end()
    while depth:
        depth += {"(": 1, ")": -1}.get(body[i], 0)
        i += 1
    assert len(abi_sigs.split_args(body[m.end():i - 1])) == len(rp["pa_count_pairs"][1])
