#!/bin/bash
# hmsg_kmeans_batch under AddressSanitizer, as a stand-alone host program: the kernel simulator's objects (every HIP kernel
# compiled for the host, device memory = heap blocks) built with -fsanitize=address and linked with
# tests/host_c/kmeans_batch_asan.cpp.  Nothing is loaded into Python and no GPU is involved.
#   scripts/kmeans_asan.sh [build dir]
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
CL=${HOSTCXX:-/opt/rocm/lib/llvm/bin/clang++}
OUT=${1:-/tmp/kmeans_asan}
mkdir -p $OUT
FLAGS="-fsanitize=address -fno-omit-frame-pointer"
for f in $ROOT/holoagent_amd/csrc/*.hip; do
  b=$(basename $f .hip)
  ( $CL -x c++ -O1 -g -std=c++17 -fPIC -ffp-contract=off -mf16c -mavx2 $FLAGS -I$ROOT/tests/emu/include -Wno-unused-value -c $f -o $OUT/$b.o ) &
done
wait
$CL -O1 -g -std=c++17 $FLAGS $ROOT/tests/host_c/kmeans_batch_asan.cpp $OUT/*.o -o $OUT/kmeans_batch_asan -ldl -lpthread
ASAN_OPTIONS=detect_leaks=0:halt_on_error=1 HMSG_DEBUG_EXACT_ALLOC=1 exec $OUT/kmeans_batch_asan
