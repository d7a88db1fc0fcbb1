#!/bin/bash
# Builds the library's host code WITH the map cache -- the files of map-merge_amd/csrc/host_sources.sh (runtime.cpp, capi.cpp,
# pair_estimate.cpp, the driver_*.cpp, host_pipeline.cpp, linalg.cpp, devices.cpp) and map_cache.cpp, unchanged -- with a sanitizer
# against tests/host_san's fake HIP runtime and fake device layer (read from there, not copied) plus this directory's fake of the one entry point of map_cache.hip, into tests/host_san_cache/_build/san_<kind>
# (git-ignored):
#   tests/host_san_cache/build.sh thread | address
set -euo pipefail
KIND=${1:-thread}
cd "$(dirname "$0")"
CSRC=../../map-merge_amd/csrc
FAKES=../host_san
CLANG=${CLANG:-/opt/rocm/lib/llvm/bin/clang++}
[ "$KIND" = thread ] && SAN="-fsanitize=thread" || SAN="-fsanitize=address,undefined -fno-sanitize-recover=undefined"
FLAGS="-x hip --cuda-host-only -nogpulib -std=c++17 -O1 -g -fno-omit-frame-pointer -ffp-contract=off -I/opt/rocm/include -I$CSRC -Wno-unused-function -Wno-option-ignored -Wno-unused-command-line-argument $SAN"
. $CSRC/host_sources.sh
mkdir -p _build
objs=""
pids=()
for f in $(printf "$CSRC/%s " $MM3D_HOST_SOURCES) $CSRC/map_cache.cpp \
         $FAKES/fake_hip.cpp $FAKES/fake_rccl.cpp $FAKES/fake_device.cpp fake_digest.cpp cache_main.cpp; do
  o=_build/$(basename "${f%.*}")_$KIND.o
  objs="$objs $o"
  ( $CLANG $FLAGS -c "$f" -o "$o" ) &
  pids+=($!)
done
for p in "${pids[@]}"; do wait "$p"; done
$CLANG $SAN -rdynamic -o _build/san_$KIND $objs -lpthread -ldl
echo "built $(pwd)/_build/san_$KIND"
