"""Routes from C (tests/host_c/hmsg_host_route.c, strict C99 against include/hmsg.h ALONE): the host computes the clearance of a
rooms-and-doors map, is told by the first hmsg_nav_route how long the path list has to be and repeats the call; what it writes
equals the same calls made through the Python binding and the restatement of tests/navroute_reference.py.  CPU: the kernel
simulator; -m gpu: libhmsg.so."""
import os
import subprocess

import numpy as np
import pytest

from tests import navroute_cases as NC
from tests import navroute_reference as RR
from tests import parity_common as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host_c", "hmsg_host_route.c")
INC = os.path.join(ROOT, "include")
LIB = os.path.join(ROOT, "holoagent_amd", "libhmsg.so")


def _compile(lib_path, out):
    cmd = ["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-O1", "-I", INC, SRC, "-o", out, lib_path,
           "-Wl,-rpath," + os.path.dirname(lib_path), "-Wl,-rpath,/opt/rocm/lib", "-Wl,--allow-shlib-undefined"]
    subprocess.run(cmd, check=True, capture_output=True)
    return out


def _run(lib_path, tmp_path):
    from holoagent_amd._lib import HmsgLib, nav_clearance, nav_route
    L = HmsgLib(lib_path)
    m = np.ascontiguousarray(NC.rooms_map())
    rng = np.random.default_rng(21)
    goals = np.ascontiguousarray(np.c_[rng.integers(-5, 135, 25), rng.integers(-5, 195, 25)].astype(np.int32))
    start, minc = (64, 95), 10
    want = nav_route(m, start, goals, lib_=L, min_clearance=minc)
    ref = RR.route(m, start, goals, min_clearance=minc)
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        np.array([m.shape[0], m.shape[1], len(goals), minc, start[0], start[1]], np.int32).tofile(f)
        m.tofile(f)
        goals.tofile(f)
    exe = _compile(lib_path, str(tmp_path / "hmsg_host_route"))
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    raw = open(fout, "rb").read()
    cells, n = m.size, len(goals)
    start_cell = tuple(int(v) for v in np.frombuffer(raw, np.int32, 2))
    start_d2, n_path = (int(v) for v in np.frombuffer(raw, np.int64, 2, 8))
    o = 24
    clr = np.frombuffer(raw, np.int32, cells, o).reshape(m.shape); o += 4 * cells
    got = dict(start_cell=start_cell, start_d2=start_d2)
    got["passable"] = np.frombuffer(raw, np.uint8, cells, o).reshape(m.shape); o += cells
    got["goal_cell"] = np.frombuffer(raw, np.int32, n * 2, o).reshape(n, 2); o += 8 * n
    got["goal_d2"] = np.frombuffer(raw, np.int64, n, o); o += 8 * n
    got["goal_dist"] = np.frombuffer(raw, np.int32, n, o); o += 4 * n
    got["path_off"] = np.frombuffer(raw, np.int64, n + 1, o); o += 8 * (n + 1)
    got["path_rc"] = np.frombuffer(raw, np.int32, n_path * 2, o).reshape(n_path, 2); o += 8 * n_path
    assert o == len(raw) and n_path > 1                                    # (the host's first list of one cell was too short)
    NC.compare_route(got, ref)
    NC.compare_route(got, want)
    assert np.array_equal(clr, RR.clearance(m)) and np.array_equal(clr, nav_clearance(m, lib_=L))
    assert "path cells %d" % n_path in r.stdout


@pytest.mark.skipif(not os.path.exists(PC.EMU_PATH), reason="kernel simulator not built")
def test_c_host_route_on_the_simulator(tmp_path):
    _run(PC.EMU_PATH, tmp_path)


@pytest.mark.gpu
def test_c_host_route_gpu(tmp_path):
    _run(LIB, tmp_path)
