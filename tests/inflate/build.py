"""g++ recipe for tests/inflate/inflate_host_check.cpp: the DEFLATE decoder of csrc/inflate_core.hpp as a stand-alone host program under
AddressSanitizer + UndefinedBehaviorSanitizer (run as a child process by tests/test_bgzf_cases.py; never loaded into Python, never on a GPU)."""
import subprocess
from pathlib import Path

HERE = Path(__file__).resolve().parent
ROOT = HERE.parent.parent
CSRC = ROOT / "rust-pseudoaligner_amd" / "csrc"
SRC = HERE / "inflate_host_check.cpp"
EXE = HERE / "_build" / "inflate_host_check"


def build_check(force: bool = False) -> Path:
    deps = [SRC, CSRC / "inflate_core.hpp", ROOT / "include" / "pseudoaligner_amd.h", Path(__file__)]
    if force or not EXE.exists() or any(d.stat().st_mtime > EXE.stat().st_mtime for d in deps):
        EXE.parent.mkdir(parents=True, exist_ok=True)
        cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
               "-I", str(CSRC), str(SRC), "-o", str(EXE)]
        proc = subprocess.run(cmd, capture_output=True, text=True)
        if proc.returncode != 0:
            raise RuntimeError("inflate_host_check build failed:\n" + proc.stderr)
    return EXE


if __name__ == "__main__":
    print(build_check(True))
