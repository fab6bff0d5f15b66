"""hipcc recipe for the probe of the text kernels of process_reads (tests/text/text_probe.hip: host arrays in and out around the launch
functions of csrc/fastq_scan.hip and csrc/render.hip, and the host's scan of csrc/fastq_text.cpp; a checker for
tests/test_gpu_text_kernels.py and tests/test_text_model.py, never part of the product). The product's sources are compiled as the
product compiles them: its hipcc, gfx950, its flags. `csrc`: another directory to take the three product sources from."""
import importlib.util
import subprocess
from pathlib import Path

HERE = Path(__file__).resolve().parent
ROOT = HERE.parent.parent
PKG = ROOT / "rust-pseudoaligner_amd"
CSRC = PKG / "csrc"
PROBE_SRC = HERE / "text_probe.hip"
PROBE_SO = HERE / "_build" / "libpa_text_probe.so"
PRODUCT_SOURCES = ["fastq_scan.hip", "render.hip", "fastq_text.cpp"]


def _product_recipe():
    spec = importlib.util.spec_from_file_location("pa_product_build", str(PKG / "_build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def build_probe(force: bool = False, csrc: Path = None, out: Path = None) -> Path:
    so = Path(out) if out else PROBE_SO
    srcs = [PROBE_SRC] + [(Path(csrc) if csrc else CSRC) / s for s in PRODUCT_SOURCES]
    deps = srcs + [Path(__file__)] + list(CSRC.glob("*.hpp")) + [ROOT / "include" / "pseudoaligner_amd.h"]
    if force or not so.exists() or any(s.stat().st_mtime > so.stat().st_mtime for s in deps):
        so.parent.mkdir(parents=True, exist_ok=True)
        # -Bsymbolic: the probe's copies of the launch functions are the ones it calls, whatever else the process has loaded
        cmd = [_product_recipe().hipcc_path(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-pthread", "-Wall", "-Wno-unused-function", "-shared",
               "-Wl,-Bsymbolic", "-Wl,--no-undefined", "-I", str(CSRC), "-I", str(ROOT / "include")]
        for s in srcs:
            cmd += ["-x", "hip", str(s)]
        cmd += ["-lz", "-o", str(so)]
        proc = subprocess.run(cmd, capture_output=True, text=True)
        if proc.returncode != 0:
            raise RuntimeError("text probe build failed:\n" + proc.stderr)
    return so


if __name__ == "__main__":
    print(build_probe(True))
