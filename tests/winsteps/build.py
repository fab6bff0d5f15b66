"""g++ recipe for tests/winsteps/winsteps_check.cpp: the arithmetic and the streaming copy of csrc/text_window.hpp as a stand-alone host program under
AddressSanitizer + UndefinedBehaviorSanitizer (run as a child process by tests/test_winsteps.py; never loaded into Python, never on a GPU). Only inline
functions of the header are used; the HIP headers it includes come from the ROCm tree that holds hipcc."""
import importlib
import subprocess
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
ROOT = HERE.parent.parent
CSRC = ROOT / "rust-pseudoaligner_amd" / "csrc"
SRC = HERE / "winsteps_check.cpp"
EXE = HERE / "_build" / "winsteps_check"


def build_check(force: bool = False) -> Path:
    deps = [SRC, Path(__file__), ROOT / "include" / "pseudoaligner_amd.h"] + list(CSRC.glob("*.hpp"))
    if force or not EXE.exists() or any(d.stat().st_mtime > EXE.stat().st_mtime for d in deps):
        if str(ROOT) not in sys.path:
            sys.path.insert(0, str(ROOT))
        rocm = Path(importlib.import_module("rust-pseudoaligner_amd._build").hipcc_path()).resolve().parent.parent
        EXE.parent.mkdir(parents=True, exist_ok=True)
        cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-Wno-unused-function", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
               "-fno-omit-frame-pointer", "-D__HIP_PLATFORM_AMD__", "-I", str(rocm / "include"), "-I", str(CSRC), str(SRC), "-pthread", "-o", str(EXE)]
        proc = subprocess.run(cmd, capture_output=True, text=True)
        if proc.returncode != 0:
            raise RuntimeError("winsteps_check build failed:\n" + proc.stderr)
    return EXE


if __name__ == "__main__":
    print(build_check(True))
