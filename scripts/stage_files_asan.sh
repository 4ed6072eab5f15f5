#!/bin/bash
# The host-side parsing and validation behind hmsg_read_ply / hmsg_restore_stage (holoagent_amd/csrc/hmsg_stage_files.h) under
# AddressSanitizer + UndefinedBehaviorSanitizer, as a stand-alone host program (tests/host_c/stage_files_asan.cpp): truncated and
# over-long PLY headers, counts a file cannot hold, bad offsets.  Nothing is loaded into Python and no GPU is involved.
#   scripts/stage_files_asan.sh [build dir]
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
CL=${HOSTCXX:-/opt/rocm/lib/llvm/bin/clang++}
OUT=${1:-/tmp/stage_files_asan}
mkdir -p $OUT/files
$CL -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer \
    $ROOT/tests/host_c/stage_files_asan.cpp -o $OUT/stage_files_asan
ASAN_OPTIONS=halt_on_error=1 exec $OUT/stage_files_asan $OUT/files
