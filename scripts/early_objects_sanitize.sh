#!/bin/bash
# The object stage beside the pooling under the host's AddressSanitizer, in a stand-alone program (no Python in the process, no
# GPU): the kernel simulator's objects (tests/emu) are compiled with -fsanitize=address and linked straight into
# tests/host_cpp/early_objects_lifetime.cpp, which runs begin -> pool -> finish with the stage on and off and the order / lifetime
# cases.  The input scene is written by an unsanitized Python first (the file tests/test_c_host.py hands to its C host).
# ThreadSanitizer is not offered: the simulator switches between the threads of a workgroup with a hand-written stack switch
# (tests/emu/include/hip/hip_runtime.h: fiber_switch), which it cannot follow.
#   scripts/early_objects_sanitize.sh
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
CL=/opt/rocm/lib/llvm/bin/clang++
OUT=${TMPDIR:-/tmp}/early_objects_asan
mkdir -p $OUT
SRC=$ROOT/holoagent_amd/csrc
FLAGS="-fsanitize=address -fno-omit-frame-pointer"
for f in $SRC/*.hip; do
  b=$(basename $f .hip)
  ( $CL -x c++ -O1 -g -std=c++17 -fPIC -ffp-contract=off -mf16c -mavx2 $FLAGS -I$ROOT/tests/emu/include -Wno-unused-value -c $f -o $OUT/$b.o ) &
done
wait
$CL -O1 -g -std=c++17 $FLAGS -I$ROOT/include $ROOT/tests/host_cpp/early_objects_lifetime.cpp $OUT/*.o -o $OUT/early_objects_lifetime -ldl -lpthread
cd $ROOT
python - "$OUT/in.bin" <<'EOF'
import sys
import numpy as np
from tests import parity_common as PC
from tests.test_c_host import _scene
spec, frames, text = _scene()
S = PC.stack_frames(frames)
F, (H, W), M, D = len(frames), frames[0]["depth"].shape, S["masks"].shape[1], spec.feat_dim
with open(sys.argv[1], "wb") as f:
    np.array([F, H, W, M, D, 0, 0, 40, 8, 500], np.int32).tofile(f)
    for a, t in ((S["K"], np.float64), (S["rgb"], np.uint8), (S["depth"], np.uint16), (S["pose"], np.float64), (S["masks"], np.uint8),
                 (S["n_masks"], np.int32), (S["f_g"], np.float32), (S["f_masked"], np.float32), (S["f_crop"], np.float32)):
        np.ascontiguousarray(a, t).tofile(f)
EOF
ASAN_OPTIONS=detect_leaks=0:halt_on_error=1 HMSG_DEBUG_EXACT_ALLOC=1 $OUT/early_objects_lifetime $OUT/in.bin
