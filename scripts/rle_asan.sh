#!/bin/bash
# The run-length mask decode under AddressSanitizer and UBSan, as a stand-alone host program: hmsg_rle.hip compiled for the kernel
# simulator (device memory = heap blocks, one allocation per buffer with HMSG_DEBUG_EXACT_ALLOC) and linked with
# tests/host_c/rle_asan.cpp.  Nothing is loaded into Python and no GPU is involved.
#   scripts/rle_asan.sh [build dir]
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
CL=${HOSTCXX:-/opt/rocm/lib/llvm/bin/clang++}
OUT=${1:-/tmp/rle_asan}
mkdir -p $OUT
$CL -x c++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-omit-frame-pointer -ffp-contract=off -mf16c -mavx2 \
    -I$ROOT/tests/emu/include -Wno-unused-value $ROOT/holoagent_amd/csrc/hmsg_rle.hip $ROOT/tests/host_c/rle_asan.cpp -o $OUT/rle_asan -ldl
# (the refusals' messages, two hundred of them, go to a file with whatever a sanitizer has to say; shown when the run fails)
if ASAN_OPTIONS=detect_leaks=0:halt_on_error=1 UBSAN_OPTIONS=halt_on_error=1 HMSG_DEBUG_EXACT_ALLOC=1 $OUT/rle_asan 2> $OUT/stderr.log; then
  exit 0
fi
grep -v "^hmsg_rle_to_" $OUT/stderr.log | tail -40
exit 1
