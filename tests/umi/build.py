"""g++ recipe for tests/umi/umi_host_check.cpp: csrc/bus_umi_host.cpp (the host half of the UMI correction, free of HIP) with the gene counter's
host half it reuses (csrc/genes_host.cpp) as a stand-alone host program under AddressSanitizer + UndefinedBehaviorSanitizer (run as a child
process by tests/test_umi_host.py; never loaded into Python, never on a GPU)."""
import os
import subprocess
from pathlib import Path

HERE = Path(__file__).resolve().parent
ROOT = HERE.parent.parent
CSRC = ROOT / "rust-pseudoaligner_amd" / "csrc"
SRC = HERE / "umi_host_check.cpp"
EXE = HERE / "_build" / "umi_host_check"


def build_check(force: bool = False) -> Path:
    deps = [SRC, CSRC / "bus_umi_host.cpp", CSRC / "bus_umi_host.hpp", CSRC / "genes_host.cpp", CSRC / "genes_host.hpp", CSRC / "bus_records_host.hpp", CSRC / "pa_common.hpp",
            Path(__file__), ROOT / "include" / "pseudoaligner_amd.h"]
    if force or not EXE.exists() or any(d.stat().st_mtime > EXE.stat().st_mtime for d in deps):
        EXE.parent.mkdir(parents=True, exist_ok=True)
        cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-Wno-unused-function", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
               "-fno-omit-frame-pointer", "-I", str(CSRC), str(SRC), str(CSRC / "bus_umi_host.cpp"), str(CSRC / "genes_host.cpp"), "-o"]
        tmp = EXE.with_name("%s.%d.tmp" % (EXE.name, os.getpid()))   # (built beside and renamed: test workers that run side by side never see half a program)
        proc = subprocess.run(cmd + [str(tmp)], capture_output=True, text=True)
        if proc.returncode != 0:
            raise RuntimeError("umi_host_check build failed:\n" + proc.stderr)
        os.replace(tmp, EXE)
    return EXE


if __name__ == "__main__":
    print(build_check(True))
