"""The host-side parsing and validation of the stage artefacts (holoagent_amd/csrc/hmsg_stage_files.h: the PLY reader behind hmsg_load and
hmsg_read_ply, the offset check of hmsg_restore_stage) under AddressSanitizer + UndefinedBehaviorSanitizer: a stand-alone program with
its own main (tests/host_c/stage_files_asan.cpp) that includes the header alone, built and run here as a child process.  Nothing
sanitized is loaded into Python, and no GPU is involved."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host_c", "stage_files_asan.cpp")


def test_stage_file_parsing_is_clean_under_the_sanitizers(tmp_path):
    cxx = next((c for c in (os.environ.get("HOSTCXX"), "/opt/rocm/lib/llvm/bin/clang++", shutil.which("clang++"), shutil.which("g++")) if c and os.path.exists(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "stage_files_asan")
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", SRC, "-o", exe],
                   check=True, capture_output=True)
    files = tmp_path / "files"
    files.mkdir()
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([exe, str(files)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "stage_files_asan ok" in r.stdout, r.stdout + r.stderr
