# build tools/baseline/<name>.so = the product library compiled under extra flags, for same-box A/B runs (PA_PRODUCT_SO=...).
# Every variant is built with -DPA_DEBUG_KNOBS: the A/B knobs of DESIGN.md §8 (PA_MAP_ABLATE, PA_MAP_STATS, PA_POOL_SLOTS, ...)
# exist in these builds only, never in the shipped library.
# usage: bash tools/build_variant.sh <name> [-DPA_NT=5 ...]
set -e
name=$1; shift
cd "$(dirname "$0")/.."
mkdir -p tools/baseline _build/variant_$name
src=rust-pseudoaligner_amd/csrc
pids=""
while read -r f extra; do   # the product's sources and their extra flags: rust-pseudoaligner_amd/_build.py is the one list
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -pthread -Wall -Wno-unused-function -DPA_DEBUG_KNOBS $extra "$@" -x hip -c $src/$f -o _build/variant_$name/$f.o &
  pids="$pids $!"
done < <(python3 rust-pseudoaligner_amd/_build.py --list)
for p in $pids; do wait $p || { echo "compile failed"; exit 1; }; done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -pthread _build/variant_$name/*.o -ldl -lz -o tools/baseline/$name.so
echo tools/baseline/$name.so
