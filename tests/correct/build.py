"""g++ recipe for tests/correct/correct_host_check.cpp: csrc/bus_correct_host.cpp (the host half of the BUS barcode correction, free of HIP)
as a stand-alone host program under AddressSanitizer + UndefinedBehaviorSanitizer (run as a child process by tests/test_correct_host.py;
never loaded into Python, never on a GPU)."""
import subprocess
from pathlib import Path

HERE = Path(__file__).resolve().parent
ROOT = HERE.parent.parent
CSRC = ROOT / "rust-pseudoaligner_amd" / "csrc"
SRC = HERE / "correct_host_check.cpp"
EXE = HERE / "_build" / "correct_host_check"


def build_check(force: bool = False) -> Path:
    deps = [SRC, CSRC / "bus_correct_host.cpp", CSRC / "bus_correct_host.hpp", CSRC / "bus_records_host.hpp", CSRC / "pa_common.hpp", Path(__file__), ROOT / "include" / "pseudoaligner_amd.h"]
    if force or not EXE.exists() or any(d.stat().st_mtime > EXE.stat().st_mtime for d in deps):
        EXE.parent.mkdir(parents=True, exist_ok=True)
        cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-Wno-unused-function", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
               "-fno-omit-frame-pointer", "-I", str(CSRC), str(SRC), str(CSRC / "bus_correct_host.cpp"), "-o", str(EXE)]
        proc = subprocess.run(cmd, capture_output=True, text=True)
        if proc.returncode != 0:
            raise RuntimeError("correct_host_check build failed:\n" + proc.stderr)
    return EXE


if __name__ == "__main__":
    print(build_check(True))
