"""hipcc recipe for the probe of csrc/device_prims.hpp (tests/prims/prims_probe.hip: one export per wrapper instantiation the product
makes; a checker for tests/test_gpu_prims.py, never part of the product). gfx950 and the product's own flags."""
import importlib.util
import subprocess
from pathlib import Path

HERE = Path(__file__).resolve().parent
ROOT = HERE.parent.parent
PKG = ROOT / "rust-pseudoaligner_amd"
CSRC = PKG / "csrc"
PROBE_SRC = HERE / "prims_probe.hip"
PROBE_SO = HERE / "_build" / "libpa_prims_probe.so"


def _product_recipe():
    spec = importlib.util.spec_from_file_location("pa_product_build", str(PKG / "_build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def build_probe(force: bool = False) -> Path:
    deps = [PROBE_SRC, Path(__file__)] + list(CSRC.glob("*.hpp")) + [ROOT / "include" / "pseudoaligner_amd.h"]
    if force or not PROBE_SO.exists() or any(s.stat().st_mtime > PROBE_SO.stat().st_mtime for s in deps):
        PROBE_SO.parent.mkdir(parents=True, exist_ok=True)
        cmd = [_product_recipe().hipcc_path(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-pthread", "-Wall", "-Wno-unused-function", "-shared",
               "-x", "hip", str(PROBE_SRC), "-o", str(PROBE_SO)]
        proc = subprocess.run(cmd, capture_output=True, text=True)
        if proc.returncode != 0:
            raise RuntimeError("device_prims probe build failed:\n" + proc.stderr)
    return PROBE_SO


if __name__ == "__main__":
    print(build_probe(True))
