"""hipcc recipe for the probe of the resolve kernel (tests/resolve/resolve_probe.hip, which includes csrc/resolve.hip; a checker for
tests/test_gpu_resolve_edges.py, never part of the product). resolve.hip is compiled as the product compiles it: its hipcc, gfx950, its
flags; the rest of the host runtime comes from the product library, which the probe is linked against. `csrc`: another directory to take
resolve.hip and the headers it includes from (a mutated copy of the whole of csrc/, when the tests themselves are tested)."""
import importlib.util
import subprocess
from pathlib import Path

HERE = Path(__file__).resolve().parent
ROOT = HERE.parent.parent
PKG = ROOT / "rust-pseudoaligner_amd"
CSRC = PKG / "csrc"
PROBE_SRC = HERE / "resolve_probe.hip"
PROBE_SO = HERE / "_build" / "libpa_resolve_probe.so"


def _product_recipe():
    spec = importlib.util.spec_from_file_location("pa_product_build", str(PKG / "_build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def build_probe(force: bool = False, csrc: Path = None, out: Path = None) -> Path:
    so = Path(out) if out else PROBE_SO
    recipe = _product_recipe()
    product = recipe.PRODUCT_SO if recipe.PRODUCT_SO.exists() and not force else recipe.build_product()   # (a built library is taken as it is)
    src_dir = Path(csrc) if csrc else CSRC
    deps = [PROBE_SRC, src_dir / "resolve.hip", Path(__file__), product] + list(src_dir.glob("*.hpp")) + [ROOT / "include" / "pseudoaligner_amd.h"]
    if force or not so.exists() or any(s.stat().st_mtime > so.stat().st_mtime for s in deps):
        so.parent.mkdir(parents=True, exist_ok=True)
        # -Bsymbolic: the probe's copy of launch_resolve is the one it calls, although the product library it needs has one too
        cmd = [recipe.hipcc_path(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-pthread", "-Wall", "-Wno-unused-function", "-shared",
               "-Wl,-Bsymbolic", "-Wl,--no-undefined", "-I", str(src_dir), "-I", str(CSRC), "-I", str(ROOT / "include"), "-x", "hip", str(PROBE_SRC),
               "-L", str(PKG), "-l:" + product.name, "-Wl,-rpath,$ORIGIN/../../../" + PKG.name, "-Wl,-rpath," + str(PKG), "-ldl", "-o", str(so)]
        proc = subprocess.run(cmd, capture_output=True, text=True)
        if proc.returncode != 0:
            raise RuntimeError("resolve probe build failed:\n" + proc.stderr)
    return so


if __name__ == "__main__":
    print(build_probe(True))
