"""g++ recipe for tests/knee/knee_host_check.cpp: csrc/bus_knee_host.cpp, the host half of the cell calling on BUS records, as a stand-alone host
program under AddressSanitizer + UndefinedBehaviorSanitizer (run as a child process by tests/test_knee_host.py; never loaded into Python, never on
a GPU). The source is free of HIP, and the record walk it calls is header-only (csrc/bus_records_host.hpp). -ffp-contract=off: the curve's products and differences are
single operations, as the clang pragma of the source asks of the product's compiler."""
import subprocess
from pathlib import Path

HERE = Path(__file__).resolve().parent
ROOT = HERE.parent.parent
CSRC = ROOT / "rust-pseudoaligner_amd" / "csrc"
SRC = HERE / "knee_host_check.cpp"
EXE = HERE / "_build" / "knee_host_check"
SOURCES = [CSRC / "bus_knee_host.cpp"]


def build_check(force: bool = False) -> Path:
    deps = [SRC, CSRC / "bus_knee_host.hpp", CSRC / "bus_records_host.hpp", CSRC / "pa_common.hpp", Path(__file__), ROOT / "include" / "pseudoaligner_amd.h"] + SOURCES
    if force or not EXE.exists() or any(d.stat().st_mtime > EXE.stat().st_mtime for d in deps):
        EXE.parent.mkdir(parents=True, exist_ok=True)
        cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-Wno-unused-function", "-ffp-contract=off", "-fsanitize=address,undefined",
               "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-I", str(CSRC), str(SRC)] + [str(s) for s in SOURCES] + ["-o", str(EXE)]
        proc = subprocess.run(cmd, capture_output=True, text=True)
        if proc.returncode != 0:
            raise RuntimeError("knee_host_check build failed:\n" + proc.stderr)
    return EXE


if __name__ == "__main__":
    print(build_check(True))
