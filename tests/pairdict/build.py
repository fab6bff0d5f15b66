"""g++ recipe for tests/pairdict/pairdict_check.cpp: the pair dictionary's format and builder (csrc/device_layout.hpp, csrc/dict_slots.hpp, the choice
of format in csrc/device_flatten.cpp) as a stand-alone host program under AddressSanitizer + UndefinedBehaviorSanitizer (run as a child process by
tests/test_dict_pairs.py; never loaded into Python, never on a GPU). -DPA_DEBUG_KNOBS: the test-only sizing hooks are read."""
import subprocess
from pathlib import Path

HERE = Path(__file__).resolve().parent
ROOT = HERE.parent.parent
CSRC = ROOT / "rust-pseudoaligner_amd" / "csrc"
SRC = HERE / "pairdict_check.cpp"
EXE = HERE / "_build" / "pairdict_check"


def build_check(force: bool = False) -> Path:
    srcs = [SRC] + [CSRC / s for s in ("host_index.cpp", "dbg_build.cpp", "device_flatten.cpp")]
    deps = srcs + [Path(__file__), ROOT / "include" / "pseudoaligner_amd.h"] + list(CSRC.glob("*.hpp"))
    if force or not EXE.exists() or any(d.stat().st_mtime > EXE.stat().st_mtime for d in deps):
        EXE.parent.mkdir(parents=True, exist_ok=True)
        cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wno-unused-function", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
               "-fno-omit-frame-pointer", "-DPA_DEBUG_KNOBS", "-I", str(CSRC)] + [str(s) for s in srcs] + ["-pthread", "-o", str(EXE)]
        proc = subprocess.run(cmd, capture_output=True, text=True)
        if proc.returncode != 0:
            raise RuntimeError("pairdict_check build failed:\n" + proc.stderr)
    return EXE


if __name__ == "__main__":
    print(build_check(True))
