"""Build recipe of the product library (hipcc, gfx950), in-tree so that the .so travels with the repository snapshot."""
from __future__ import annotations

import os
import shutil
import subprocess
from pathlib import Path

PKG = Path(__file__).resolve().parent
ROOT = PKG.parent
CSRC = PKG / "csrc"

PRODUCT_SO = PKG / "libpseudoaligner_amd.so"

HOST_SOURCES = ["host_index.cpp", "dbg_build.cpp", "device_flatten.cpp", "synth.cpp", "fastq_text.cpp", "fastq_reads.cpp", "pair_reader.cpp", "fastq_cells.cpp", "fastq_pairs.cpp", "record_stream.cpp", "host_batch.cpp", "bgzf.cpp", "bus_host.cpp", "bus_correct_host.cpp", "bus_knee_host.cpp", "genes_host.cpp", "bus_umi_host.cpp", "window_feed.cpp", "text_window.cpp", "pairs_host.cpp"]
HIP_SOURCES = ["kernels.hip", "map_pool.hip", "device_index.hip", "map_batch.hip", "device_plumbing.hip", "collective.hip", "barcode_counts.hip", "index_build.hip", "index_fill.hip", "count_sort.hip", "resolve.hip", "render.hip", "fastq_scan.hip", "compact.hip", "quant.hip", "quant_boot.hip", "pairs.hip", "strands.hip", "inflate.hip", "bus.hip", "pair_scan.hip", "genes.hip", "bus_correct.hip", "bus_knee.hip", "bus_umi.hip"]


# flags of single sources. map_pool.hip: without LLVM's machine-sinking pass the mapping kernel is 1 % faster at config 3 (7.608 -> 7.536 ms, three interleaved
# pairs on one box), 0.2 % at config 5, 0.5-1.7 % at config3r (profiles/r06_compiler_flags_ab.txt; eight other scheduler / if-conversion flags: within noise or slower)
EXTRA_FLAGS = {"map_pool.hip": ["-mllvm", "-disable-machine-sink"]}


def _stale(target: Path, sources) -> bool:
    if not target.exists():
        return True
    t = target.stat().st_mtime
    return any(Path(s).stat().st_mtime > t for s in sources)


def _run(cmd):
    proc = subprocess.run(cmd, capture_output=True, text=True)
    if proc.returncode != 0:
        raise RuntimeError("build failed: %s\n%s\n%s" % (" ".join(map(str, cmd)), proc.stdout, proc.stderr))
    return proc


def hipcc_path() -> str:
    for cand in (shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found: the product library cannot be built")


OBJ_DIR = PKG / "_build"   # per-source objects (git-ignored): only what changed is recompiled


def _deps_of(src: Path):
    """the source plus every header it can see (all of csrc/*.hpp and the public header: coarse, always safe)"""
    return [src] + list(CSRC.glob("*.hpp")) + list(CSRC.glob("*.inc")) + [ROOT / "include" / "pseudoaligner_amd.h", Path(__file__)]


def build_product(force: bool = False) -> Path:
    """hipcc --offload-arch=gfx950: HIP kernels + C ABI + host runtime -> libpseudoaligner_amd.so (one object per source,
    compiled in parallel, then linked)"""
    from concurrent.futures import ThreadPoolExecutor
    srcs = [CSRC / s for s in HOST_SOURCES + HIP_SOURCES]
    OBJ_DIR.mkdir(exist_ok=True)
    hipcc = hipcc_path()
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-pthread", "-Wall", "-Wno-unused-function"]
    jobs = []
    for s in srcs:
        obj = OBJ_DIR / (s.name + ".o")
        if force or _stale(obj, _deps_of(s)):
            jobs.append([hipcc] + flags + EXTRA_FLAGS.get(s.name, []) + ["-x", "hip", "-c", str(s), "-o", str(obj)])
    if jobs:
        with ThreadPoolExecutor(max_workers=min(len(jobs), os.cpu_count() or 1)) as ex:
            list(ex.map(_run, jobs))
    objs = [OBJ_DIR / (s.name + ".o") for s in srcs]
    if jobs or _stale(PRODUCT_SO, objs):
        _run([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-pthread"] + [str(o) for o in objs] + ["-ldl", "-lz", "-o", str(PRODUCT_SO)])
    return PRODUCT_SO


MAXBINS_SO = OBJ_DIR / "libpseudoaligner_amd_maxbins2.so"


def build_maxbins_variant(force: bool = False) -> Path:
    """A TEST build of the product: count_sort.hip compiled with -DPA_MAX_BINS=2, everything else the product's own objects. A class-count table
    of more than 65 536 slots is then "beyond MAX_BINS" and takes the plain-atomics path of count_sort.hip for batches of ANY size — the path
    that in the product only tables beyond 8.4 M classes take for large batches (tests/test_gpu_scale.py loads it through PA_PRODUCT_SO)."""
    build_product()
    hipcc = hipcc_path()
    src = CSRC / "count_sort.hip"
    obj = OBJ_DIR / "count_sort.maxbins2.o"
    if force or _stale(obj, _deps_of(src)):
        _run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-pthread", "-Wall", "-Wno-unused-function", "-DPA_MAX_BINS=2", "-x", "hip", "-c", str(src), "-o", str(obj)])
    objs = [OBJ_DIR / (s + ".o") for s in HOST_SOURCES + HIP_SOURCES if s != "count_sort.hip"] + [obj]
    if force or _stale(MAXBINS_SO, objs):
        _run([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-pthread"] + [str(o) for o in objs] + ["-ldl", "-lz", "-o", str(MAXBINS_SO)])
    return MAXBINS_SO


PAIRKNOBS_SO = OBJ_DIR / "libpseudoaligner_amd_pairknobs.so"


def build_pairknobs_variant(force: bool = False) -> Path:
    """A TEST build of the product: device_flatten.cpp compiled with -DPA_DEBUG_KNOBS, everything else the product's own objects. The choice of the
    dictionary's format and size (dict_pair_log2, used by the CPU flattener and the GPU filler alike) then reads the test-only sizing hooks
    PA_PAIR_LOG2 / PA_PAIR_MAX_BLOCKS (tests/test_gpu_dict_pairs.py loads it in a child process through PA_PRODUCT_SO)."""
    build_product()
    hipcc = hipcc_path()
    src = CSRC / "device_flatten.cpp"
    obj = OBJ_DIR / "device_flatten.pairknobs.o"
    if force or _stale(obj, _deps_of(src)):
        _run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-pthread", "-Wall", "-Wno-unused-function", "-DPA_DEBUG_KNOBS", "-x", "hip", "-c", str(src), "-o", str(obj)])
    objs = [OBJ_DIR / (s + ".o") for s in HOST_SOURCES + HIP_SOURCES if s != "device_flatten.cpp"] + [obj]
    if force or _stale(PAIRKNOBS_SO, objs):
        _run([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-pthread"] + [str(o) for o in objs] + ["-ldl", "-lz", "-o", str(PAIRKNOBS_SO)])
    return PAIRKNOBS_SO


DICTKNOBS_SO = OBJ_DIR / "libpseudoaligner_amd_dictknobs.so"


def build_dictknobs_variant(force: bool = False) -> Path:
    """A TEST build of the product: device_flatten.cpp AND index_fill.hip compiled with -DPA_DEBUG_KNOBS, everything else the product's own objects.
    The CPU flattener and the GPU filler then read PA_DICT_LOAD, the load the 16-byte slots (K <= 32; K <= 24 too: a named load refuses the pair
    format) and the two-word lines (K > 32) are built at, so that a test can have DENSE tables: keys in named slots, chains of several buckets, the
    builders' retry (tests/test_dict_model.py and tests/test_gpu_dict_dense.py load it in child processes through PA_PRODUCT_SO)."""
    build_product()
    hipcc = hipcc_path()
    knob_objs = []
    for name in ("device_flatten.cpp", "index_fill.hip"):
        src, obj = CSRC / name, OBJ_DIR / (name.rsplit(".", 1)[0] + ".dictknobs.o")
        if force or _stale(obj, _deps_of(src)):
            _run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-pthread", "-Wall", "-Wno-unused-function", "-DPA_DEBUG_KNOBS", "-x", "hip", "-c", str(src), "-o", str(obj)])
        knob_objs.append(obj)
    objs = [OBJ_DIR / (s + ".o") for s in HOST_SOURCES + HIP_SOURCES if s not in ("device_flatten.cpp", "index_fill.hip")] + knob_objs
    if force or _stale(DICTKNOBS_SO, objs):
        _run([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-pthread"] + [str(o) for o in objs] + ["-ldl", "-lz", "-o", str(DICTKNOBS_SO)])
    return DICTKNOBS_SO


IBKNOBS_SO = OBJ_DIR / "libpseudoaligner_amd_ibknobs.so"


def build_ibknobs_variant(force: bool = False) -> Path:
    """A TEST build of the product: index_build.hip compiled with -DPA_DEBUG_KNOBS, everything else the product's own objects. The GPU index builder
    then reads PA_IB_WEAK_ATTEMPTS = n: on its first n attempts the colour stage keeps two bits of every addend of the set hash, so that different id
    lists share a hash, the content check fails and the stage runs again with another seed — four times, then the build fails
    (tests/test_gpu_index_edges.py loads it in a child process through PA_PRODUCT_SO)."""
    build_product()
    hipcc = hipcc_path()
    src = CSRC / "index_build.hip"
    obj = OBJ_DIR / "index_build.ibknobs.o"
    if force or _stale(obj, _deps_of(src)):
        _run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-pthread", "-Wall", "-Wno-unused-function", "-DPA_DEBUG_KNOBS", "-x", "hip", "-c", str(src), "-o", str(obj)])
    objs = [OBJ_DIR / (s + ".o") for s in HOST_SOURCES + HIP_SOURCES if s != "index_build.hip"] + [obj]
    if force or _stale(IBKNOBS_SO, objs):
        _run([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-pthread"] + [str(o) for o in objs] + ["-ldl", "-lz", "-o", str(IBKNOBS_SO)])
    return IBKNOBS_SO


UMIHBM_SO = OBJ_DIR / "libpseudoaligner_amd_umihbm.so"


def build_umi_hbm_variant(force: bool = False) -> Path:
    """A TEST build of the product: bus_umi.hip compiled with -DPA_UMI_FORCE_HBM, everything else the product's own objects. The barcodes of the UMI
    correction's block bin (more than UM_LANE_MAX molecules, up to UM_LDS_CAP) then take the HBM variant of the neighbour search, so that the two can be
    timed on the same barcodes (tools/bench_umi.py loads it in a child process through PA_PRODUCT_SO)."""
    build_product()
    hipcc = hipcc_path()
    src = CSRC / "bus_umi.hip"
    obj = OBJ_DIR / "bus_umi.umihbm.o"
    if force or _stale(obj, _deps_of(src)):
        _run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-pthread", "-Wall", "-Wno-unused-function", "-DPA_UMI_FORCE_HBM", "-x", "hip", "-c", str(src), "-o", str(obj)])
    objs = [OBJ_DIR / (s + ".o") for s in HOST_SOURCES + HIP_SOURCES if s != "bus_umi.hip"] + [obj]
    if force or _stale(UMIHBM_SO, objs):
        _run([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-pthread"] + [str(o) for o in objs] + ["-ldl", "-lz", "-o", str(UMIHBM_SO)])
    return UMIHBM_SO


ABI_CHECK_SRC = ROOT / "integration" / "c" / "abi_check.c"
ABI_CHECK_BIN = ROOT / "integration" / "c" / "abi_check"


def build_abi_check(force: bool = False) -> Path:
    """gcc -Wall -Werror: the plain-C client that calls every entry point of include/pseudoaligner_amd.h (type check of the
    header from C; the tests run it)"""
    if force or _stale(ABI_CHECK_BIN, [ABI_CHECK_SRC, ROOT / "include" / "pseudoaligner_amd.h", PRODUCT_SO]):
        _run(["gcc", "-std=c11", "-O1", "-Wall", "-Wextra", "-Werror", "-I", str(ROOT / "include"), str(ABI_CHECK_SRC), "-L", str(PKG),
              "-lpseudoaligner_amd", "-Wl,-rpath," + str(PKG), "-Wl,-rpath,$ORIGIN/../../rust-pseudoaligner_amd", "-o", str(ABI_CHECK_BIN)])
    return ABI_CHECK_BIN


if __name__ == "__main__":
    import sys
    if "--list" in sys.argv:   # one line per source of the product, its extra flags behind it (tools/build_variant.sh reads this)
        for s in HOST_SOURCES + HIP_SOURCES:
            print(" ".join([s] + EXTRA_FLAGS.get(s, [])))
    else:
        print(build_product("--force" in sys.argv))
