"""CPU tier: the pair dictionary (csrc/device_layout.hpp, csrc/dict_slots.hpp) — mixing function and inverse, entry fields at their limits, the
choice of format, and the builder's edges (keys homed to one pair, runs of full pairs, the wrap, absent keys behind flagged and unflagged pairs,
the alias a carried key would have without its displacement, independence of the order of insertion) — driven by a stand-alone host program under
AddressSanitizer + UndefinedBehaviorSanitizer (tests/pairdict/); then the emulator's map of reads through a pair dictionary against the oracle."""
import importlib.util
import os
import subprocess

import pytest

import helpers


def test_pair_dictionary_format_and_builder_edges():
    spec = importlib.util.spec_from_file_location("pa_pairdict_build", str(helpers.ROOT / "tests" / "pairdict" / "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    exe = mod.build_check()
    env = {k: v for k, v in os.environ.items() if not k.startswith("PA_")}
    proc = subprocess.run([str(exe)], capture_output=True, text=True, env=env)
    assert proc.returncode == 0, proc.stdout + proc.stderr
    assert "pairdict ok" in proc.stdout


def _emu_check(host, read_len, ppm, n=4096):
    pa = helpers.pa
    tx = pa.Txome.from_host_index(host)
    tiles, lens = tx.simulate_host(read_len, 4, n, ppm)
    wpr = pa.lib().pa_words_per_read(read_len)
    o_res, o_coff, o_ids, ctr = helpers.Oracle(host).map_tiles(tiles, lens, wpr, 2, 4)
    r = helpers.Emu(host).map_tiles(tiles, lens, wpr, 2, 8)
    helpers.assert_same_as_oracle(r["results"], r["coff"], r["ids"], o_res, o_coff, o_ids, "emu, pair dictionary")
    return ctr, int(r["steps"][0])


@pytest.mark.parametrize("k", [24, 21])
@pytest.mark.parametrize("ppm", [0, 10000])
def test_emulator_maps_through_a_pair_dictionary(small_index, built, monkeypatch, k, ppm):
    """gencode_small (1.17 M k-mers at K = 24) through the pair dictionary the CPU flattener builds, forced to start from the smallest size
    (the emulator's flattener is a knobs build: it reads PA_PAIR_LOG2). A table of 2^b pairs can hold a key at most 2^(b - 20) - 2 pairs behind
    its home, so the builder doubles the table until every key fits: the retry path. Error-free reads make one dictionary probe per k-mer the
    reference looks up and one seek step per pair they look at, so the emulator's seek steps exceed the oracle's probes by exactly the
    second-pair probes: asserted above zero. 1 % substitutions make lanes probe past a miss, two positions per step."""
    monkeypatch.setenv("PA_PAIR_LOG2", "21")
    monkeypatch.delenv("PA_DICT_LOAD", raising=False)
    host = small_index(k) if k == 24 else helpers.pa.build_index(str(helpers.FASTA), k, 8)
    info = helpers.Emu(host).info()
    assert info["nbuckets"] in (1 << 22, 1 << 23)   # (pairs; the 16-byte format of this index would have some 1.2 M buckets, no power of two)
    ctr, seek_steps = _emu_check(host, 100, ppm)
    if ppm:
        assert ctr["reseeks"] > 0
    else:
        assert seek_steps > ctr["probes"], (seek_steps, ctr["probes"])   # probes that went on to a second pair
