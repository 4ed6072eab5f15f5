"""Sight over furniture from C (tests/host_c/hmsg_host_sight.c, strict C99 against include/hmsg.h ALONE) on the motivating case of
tests/navsight_cases.py given as a cloud: a point per cell on the floor and one at the top of every wall and table cell, heights in
units of 1 / 32 m so that every division is exact.  The host makes the height map (hmsg_nav_grid, hmsg_nav_height_map), walks on its
cells of height 0, calls hmsg_nav_view_route_h -- told by the first call how long the path list has to be -- and then
hmsg_nav_viewpoints_h on the passable map and the field that call returned; what it writes equals the restatement of
tests/navsight_reference.py, with the case's counts.  CPU: the kernel simulator; -m gpu: libhmsg.so."""
import os
import subprocess

import numpy as np
import pytest

from tests import navsight_cases as SC
from tests import navsight_reference as SR
from tests import navview_cases as VC
from tests import parity_common as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host_c", "hmsg_host_sight.c")
INC = os.path.join(ROOT, "include")
LIB = os.path.join(ROOT, "holoagent_amd", "libhmsg.so")
CELL, UNIT, TOP_MAX, ZERO = 0.25, 1.0 / 32, 10.0, -1.5


def _compile(lib_path, out):
    cmd = ["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-O1", "-I", INC, SRC, "-o", out, lib_path,
           "-Wl,-rpath," + os.path.dirname(lib_path), "-Wl,-rpath,/opt/rocm/lib", "-Wl,--allow-shlib-undefined"]
    subprocess.run(cmd, check=True, capture_output=True)
    return out


def _run(lib_path, tmp_path):
    exe = _compile(lib_path, str(tmp_path / "hmsg_host_sight"))
    top, pas, g, band = SC.motivating_map()
    r, c = np.nonzero(np.ones_like(top))
    floor = np.c_[c * CELL, np.full(len(r), ZERO), r * CELL]
    r, c = np.nonzero(top)
    tops = np.c_[c * CELL, ZERO + top[r, c] * UNIT, r * CELL]
    rng = np.random.default_rng(5)
    pts = np.concatenate([floor, tops])
    pts = np.ascontiguousarray(pts[rng.permutation(len(pts))])
    ref_top, ref_known = SR.height_map_np(pts, ZERO, CELL, UNIT, TOP_MAX, 0)
    assert np.array_equal(ref_top, top) and ref_known.all()
    goals, gh, gr2 = np.array([g, g, (3, 30)], np.int32), np.array([90, 40, 60], np.int32), np.array([-1, -1, 2], np.int64)
    start, eye = (10, 5), 150
    ref = SR.view_route_h(pas, top, start, goals, eye, gh, gr2, *band)
    views = SR.viewpoints_h(top, ref["passable"], goals, *band, eye, gh, gr2, ref["field"], 0, want_visible=True)
    assert list(views["n_visible"][:2]) == [520, 379] and ref["goal_cell"][0, 1] < 20 < ref["goal_cell"][1, 1]       # over the table from west of the wall
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        np.array([len(pts), len(goals)], np.int64).tofile(f)
        np.array([ZERO, CELL, UNIT, TOP_MAX], np.float64).tofile(f)
        np.array([0, 0, eye, 0, start[0], start[1]], np.int32).tofile(f)
        np.array(band, np.int64).tofile(f)
        pts.tofile(f)
        goals.tofile(f)
        gh.tofile(f)
        gr2.tofile(f)
    run = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    raw = open(fout, "rb").read()
    cells, n = top.size, len(goals)
    grid = np.frombuffer(raw, np.int32, 2)
    assert (int(grid[1]), int(grid[0])) == top.shape
    got = dict(start_cell=tuple(int(v) for v in np.frombuffer(raw, np.int32, 2, 8)))
    got["start_d2"], n_path = (int(v) for v in np.frombuffer(raw, np.int64, 2, 16))
    o = 32
    assert np.array_equal(np.frombuffer(raw, np.uint16, cells, o).reshape(top.shape), top); o += 2 * cells
    assert np.array_equal(np.frombuffer(raw, np.uint8, cells, o).reshape(top.shape), ref_known); o += cells
    got["passable"] = np.frombuffer(raw, np.uint8, cells, o).reshape(top.shape); o += cells
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
    v["visible"] = np.frombuffer(raw, np.uint8, n * cells, o).reshape((n,) + top.shape); o += n * cells
    assert o == len(raw)
    VC.compare_view_route(got, ref)
    VC.compare_views(v, views)
    assert np.array_equal(v["view_rc"], got["goal_cell"]) and np.array_equal(v["n_visible"], got["n_visible"]) and n_path > 1
    assert "path cells %d" % n_path in run.stdout


@pytest.mark.skipif(not os.path.exists(PC.EMU_PATH), reason="kernel simulator not built")
def test_c_host_sight_on_the_simulator(tmp_path):
    _run(PC.EMU_PATH, tmp_path)


@pytest.mark.gpu
def test_c_host_sight_gpu(tmp_path):
    _run(LIB, tmp_path)
