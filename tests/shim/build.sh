#!/bin/bash
# TEST infrastructure: compiles the reference-side binding (include/map_merge_3d_shim.hpp) as one
# translation unit against the reference's OWN public headers where they lie (R/include, read-only,
# nothing is copied) plus the stand-ins of tests/shim/mock, and links it against libmm3d.so with
# --no-undefined.  Output: oracle/_ref/shim_check.o and oracle/_ref/shim_check (git-ignored, like everything built
# from the reference; `make -C oracle shim` runs this).
set -euo pipefail
cd "$(dirname "$0")"
REF=${MM3D_REFERENCE:-/root/reference/map_merge_3d}
[ -d "$REF/include/map_merge_3d" ] || { echo "reference headers absent: shim_check not rebuilt"; exit 0; }
OUT=../../oracle/_ref
mkdir -p $OUT
g++ -std=c++14 -O1 -Wall -Wextra -Werror -Wno-unused-parameter -I"$REF/include" -Imock -I../../include -c shim_check.cpp -o $OUT/shim_check.o
g++ $OUT/shim_check.o -o $OUT/shim_check -L../../map-merge_amd -lmm3d -Wl,-rpath,'$ORIGIN/../../map-merge_amd' -Wl,--no-undefined
echo "built $(cd $OUT && pwd)/shim_check"
