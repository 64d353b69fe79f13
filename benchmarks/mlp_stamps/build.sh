#!/bin/bash
# Builds benchmarks/mlp_stamps/build/libfv3hip_stamps_<phase>.so: libfv3hip.so with mlp_fused_kernel's cycle stamps compiled in
# (-DMLP_STAMPS -DMLP_STAMP_PHASE=<phase>), flagship instantiations only, one library per per-slot phase.  The product
# library is not touched.  Needs the objects of a normal build (make -C fv3net_amd/csrc).
#   usage: build.sh [phase ...]     default: 0 2 3 4 10 20   (see MLP_STAMP_PHASE in mlp.hip)
#   MLP_SRC=<file> builds another mlp.hip (a checkout of the parent commit, say) against this tree's other objects,
#   MLP_STAMPS_OUT=<dir> puts the libraries somewhere else.
set -e
here=$(cd "$(dirname "$0")" && pwd)
csrc="$here/../../fv3net_amd/csrc"
src=${MLP_SRC:-$csrc/mlp.hip}
out=${MLP_STAMPS_OUT:-$here/build}
mkdir -p "$out"
phases=${*:-0 2 3 4 10 20}
objs=$(ls "$csrc"/*.o | grep -v '/mlp\.o$')
pids=()
for p in $phases; do
    (hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=off -Wno-unused-value -Wno-invalid-offsetof -Wno-inline-asm \
           -mllvm -pragma-unroll-threshold=262144 -I"$csrc" -DMLP_FAST_BUILD -DMLP_STAMPS -DMLP_STAMP_PHASE=$p -c "$src" -o "$out/mlp_stamps_$p.o" &&
     hipcc --offload-arch=gfx950 -shared -fPIC -o "$out/libfv3hip_stamps_$p.so" $objs "$out/mlp_stamps_$p.o") &
    pids+=($!)
done
for pid in "${pids[@]}"; do wait "$pid"; done
