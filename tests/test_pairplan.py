"""CPU tier: the arithmetic of the paired drivers' device path that needs no GPU — segment planning over two sequences of window record counts and the
order in which window slots are taken again (csrc/window_feed.hpp) — driven by a stand-alone host program under AddressSanitizer +
UndefinedBehaviorSanitizer (tests/pairplan/). It pins segment_pairs() and feed_slot_of(); the loop around them is the program's own."""
import importlib.util
import subprocess

import helpers


def test_segments_and_slots_keep_their_contract():
    spec = importlib.util.spec_from_file_location("pa_pairplan_build", str(helpers.ROOT / "tests" / "pairplan" / "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    exe = mod.build_check()
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stderr == "", (out.returncode, out.stdout[-3000:], out.stderr[-3000:])   # the sanitizers stay silent
    lines = out.stdout.splitlines()
    assert lines[-1] == "OK" and len(lines) == 11 and not any(l.startswith("MISS") for l in lines), out.stdout[-3000:]
