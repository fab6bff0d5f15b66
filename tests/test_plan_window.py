"""CPU tier: plan_window (csrc/fastq_text.cpp), the arithmetic that cuts the text of pa_process_reads into the windows the GPU scans, driven over made-up
plain and BGZF texts by a stand-alone host program under AddressSanitizer + UndefinedBehaviorSanitizer (tests/plan/)."""
import importlib.util
import subprocess

import helpers


def test_window_plans_keep_their_contract():
    spec = importlib.util.spec_from_file_location("pa_plan_build", str(helpers.ROOT / "tests" / "plan" / "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    exe = mod.build_check()
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stderr == "", (out.returncode, out.stdout[-3000:], out.stderr[-3000:])   # the sanitizers stay silent
    lines = out.stdout.splitlines()
    assert lines[-1] == "OK" and len(lines) == 12 and not any(l.startswith("MISS") for l in lines), out.stdout[-3000:]
