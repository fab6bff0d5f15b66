"""CPU tier: what of the window steps shared by pa_process_reads and the paired drivers' window feed (csrc/text_window.hpp) needs no GPU — copy_streaming
against memcpy for every destination offset 0-63, source offset 0-15 and length 0-200 plus 4096 + {0, 1, 63} with guard bytes on both sides, the window-size
rule over hand-written cases, host_tail_cut over made-up record starts — driven by a stand-alone host program under AddressSanitizer +
UndefinedBehaviorSanitizer (tests/winsteps/)."""
import importlib.util
import subprocess

import helpers


def test_window_steps_keep_their_contract():
    spec = importlib.util.spec_from_file_location("pa_winsteps_build", str(helpers.ROOT / "tests" / "winsteps" / "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    exe = mod.build_check()
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stderr == "", (out.returncode, out.stdout[-3000:], out.stderr[-3000:])   # the sanitizers stay silent
    lines = out.stdout.splitlines()
    assert lines[-1] == "OK" and len(lines) == 10 and not any(l.startswith("MISS") for l in lines), out.stdout[-3000:]
    assert lines[0] == "copy_streaming: %d copies" % (64 * 16 * (201 + 3))
