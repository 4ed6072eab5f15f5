"""Viewpoints from C (tests/host_c/hmsg_host_view.c, strict C99 against include/hmsg.h ALONE) on the wall that the old snap goes
through (tests/navview_cases.py, case 3), without and with the door: the host calls hmsg_nav_view_route -- told by the first call
how long the path list has to be where there is a path -- and then hmsg_nav_viewpoints on the passable map and the field that
call returned; what it writes equals the restatement of tests/navview_reference.py.  CPU: the kernel simulator; -m gpu:
libhmsg.so."""
import os
import subprocess

import numpy as np
import pytest

from tests import navview_cases as VC
from tests import navview_reference as VR
from tests import parity_common as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host_c", "hmsg_host_view.c")
INC = os.path.join(ROOT, "include")
LIB = os.path.join(ROOT, "holoagent_amd", "libhmsg.so")


def _compile(lib_path, out):
    cmd = ["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-O1", "-I", INC, SRC, "-o", out, lib_path,
           "-Wl,-rpath," + os.path.dirname(lib_path), "-Wl,-rpath,/opt/rocm/lib", "-Wl,--allow-shlib-undefined"]
    subprocess.run(cmd, check=True, capture_output=True)
    return out


def _run(lib_path, tmp_path):
    exe = _compile(lib_path, str(tmp_path / "hmsg_host_view"))
    for door in (False, True):
        m, blk, start, goals = VC.wall_map(door)
        ref = VR.view_route(m, blk, start, goals, *VC.WALL_BAND, min_clearance=VC.MINC)
        views = VR.viewpoints(blk, ref["passable"], goals, *VC.WALL_BAND, ref["field"], 0, want_visible=True)
        fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
        with open(fin, "wb") as f:
            np.array([m.shape[0], m.shape[1], len(goals), VC.MINC, start[0], start[1]], np.int32).tofile(f)
            np.array(VC.WALL_BAND, np.int64).tofile(f)
            m.tofile(f)
            blk.tofile(f)
            goals.tofile(f)
        r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        raw = open(fout, "rb").read()
        cells, n = m.size, len(goals)
        got = dict(start_cell=tuple(int(v) for v in np.frombuffer(raw, np.int32, 2)))
        got["start_d2"], n_path = (int(v) for v in np.frombuffer(raw, np.int64, 2, 8))
        o = 24
        got["passable"] = np.frombuffer(raw, np.uint8, cells, o).reshape(m.shape); o += cells
        got["goal_cell"] = np.frombuffer(raw, np.int32, n * 2, o).reshape(n, 2); o += 8 * n
        got["goal_d2"] = np.frombuffer(raw, np.int64, n, o); o += 8 * n
        got["goal_dist"] = np.frombuffer(raw, np.int32, n, o); o += 4 * n
        got["n_visible"] = np.frombuffer(raw, np.int32, n, o); o += 4 * n
        got["path_off"] = np.frombuffer(raw, np.int64, n + 1, o); o += 8 * (n + 1)
        got["path_rc"] = np.frombuffer(raw, np.int32, n_path * 2, o).reshape(n_path, 2); o += 8 * n_path
        v = {}
        v["view_rc"] = np.frombuffer(raw, np.int32, n * 2, o).reshape(n, 2); o += 8 * n
        v["view_d2"] = np.frombuffer(raw, np.int64, n, o); o += 8 * n
        v["view_dist"] = np.frombuffer(raw, np.int32, n, o); o += 4 * n
        v["n_visible"] = np.frombuffer(raw, np.int32, n, o); o += 4 * n
        v["visible"] = np.frombuffer(raw, np.uint8, n * cells, o).reshape((n,) + m.shape); o += n * cells
        assert o == len(raw)
        VC.compare_view_route(got, ref)
        VC.compare_views(v, views)
        assert np.array_equal(v["view_rc"], got["goal_cell"]) and np.array_equal(v["n_visible"], got["n_visible"])
        if door:
            assert n_path > 1 and got["goal_cell"][0, 0] <= 16 and v["visible"][0].sum() == got["n_visible"][0] > 0
        else:
            assert n_path == 0 and tuple(got["goal_cell"][0]) == (-1, -1) and not v["visible"].any()
        assert "path cells %d" % n_path in r.stdout


@pytest.mark.skipif(not os.path.exists(PC.EMU_PATH), reason="kernel simulator not built")
def test_c_host_view_on_the_simulator(tmp_path):
    _run(PC.EMU_PATH, tmp_path)


@pytest.mark.gpu
def test_c_host_view_gpu(tmp_path):
    _run(LIB, tmp_path)
