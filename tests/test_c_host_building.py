"""Routes across storeys from C (tests/host_c/hmsg_host_building.c, strict C99 against include/hmsg.h ALONE): the host builds the
fields of one start over three storeys, is told by the first hmsg_nav_building_route how long the path list has to be and repeats
the call; what it writes equals the same calls made through the Python binding and the restatement of
tests/navbuilding_reference.py.  CPU: the kernel simulator; -m gpu: libhmsg.so."""
import os
import subprocess

import numpy as np
import pytest

from tests import navbuilding_cases as BC
from tests import navbuilding_reference as RB
from tests import navroute_cases as NC
from tests import navroute_reference as RR
from tests import parity_common as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host_c", "hmsg_host_building.c")
INC = os.path.join(ROOT, "include")
LIB = os.path.join(ROOT, "holoagent_amd", "libhmsg.so")


def _compile(lib_path, out):
    cmd = ["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-O1", "-I", INC, SRC, "-o", out, lib_path,
           "-Wl,-rpath," + os.path.dirname(lib_path), "-Wl,-rpath,/opt/rocm/lib", "-Wl,--allow-shlib-undefined"]
    subprocess.run(cmd, check=True, capture_output=True)
    return out


def _run(lib_path, tmp_path):
    from holoagent_amd._lib import HmsgLib, nav_building_route
    L = HmsgLib(lib_path)
    maps = [np.ascontiguousarray(m) for m in (NC.rooms_map(), BC.open_map(67, 70), BC.two_rooms())]
    clear = tuple(int(v) for v in np.argwhere(RR.clearance(maps[0]) >= 10)[40])        # a cell that keeps its link at min_clearance 10
    links = np.array([(0,) + clear + (1, 35, 45, 27), (1, 5, 5, 2, 35, 20, 19), (1, 60, 60, 2, 35, 70, 19)], np.int32)
    rng = np.random.default_rng(21)
    goals = np.ascontiguousarray(np.c_[rng.integers(0, 3, 25), rng.integers(-5, 135, 25), rng.integers(-5, 195, 25)].astype(np.int32))
    start, minc = (2, 35, 25), 10
    want = nav_building_route(maps, links, start, goals, lib_=L, min_clearance=minc)
    ref, B = RB.route(maps, links, start, goals, min_clearance=minc)
    plain_fields, plain_reached = RB.Building(maps, links).fields(start)
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        np.array([3, len(links), len(goals), minc] + list(start), np.int32).tofile(f)
        np.array([m.shape[0] for m in maps], np.int32).tofile(f)
        np.array([m.shape[1] for m in maps], np.int32).tofile(f)
        for m in maps:
            m.tofile(f)
        links.tofile(f)
        goals.tofile(f)
    exe = _compile(lib_path, str(tmp_path / "hmsg_host_building"))
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    raw = open(fout, "rb").read()
    n = len(goals)
    got = dict(start_cell=tuple(int(v) for v in np.frombuffer(raw, np.int32, 3)))
    got["start_d2"], n_path = (int(v) for v in np.frombuffer(raw, np.int64, 2, 12))
    o = 28
    reached = np.frombuffer(raw, np.int64, 3, o); o += 24
    fields = []
    for m in maps:
        fields.append(np.frombuffer(raw, np.int32, m.size, o).reshape(m.shape)); o += 4 * m.size
    got["passable"] = []
    for m in maps:
        got["passable"].append(np.frombuffer(raw, np.uint8, m.size, o).reshape(m.shape)); o += m.size
    got["goal_cell"] = np.frombuffer(raw, np.int32, n * 3, o).reshape(n, 3); o += 12 * n
    got["goal_d2"] = np.frombuffer(raw, np.int64, n, o); o += 8 * n
    got["goal_dist"] = np.frombuffer(raw, np.int32, n, o); o += 4 * n
    got["path_off"] = np.frombuffer(raw, np.int64, n + 1, o); o += 8 * (n + 1)
    got["path_src"] = np.frombuffer(raw, np.int32, n_path * 3, o).reshape(n_path, 3); o += 12 * n_path
    assert o == len(raw) and n_path > 1                                    # (the host's first list of one cell was too short)
    BC.compare_route(got, ref)
    BC.compare_route(got, want)
    B.check_walk(ref["fields"], ref["path_off"], ref["path_src"])
    assert np.array_equal(reached, plain_reached) and all(np.array_equal(a, b) for a, b in zip(fields, plain_fields))
    assert len({int(t[0]) for t in got["path_src"]}) == 3 and "path cells %d" % n_path in r.stdout


@pytest.mark.skipif(not os.path.exists(PC.EMU_PATH), reason="kernel simulator not built")
def test_c_host_building_on_the_simulator(tmp_path):
    _run(PC.EMU_PATH, tmp_path)


@pytest.mark.gpu
def test_c_host_building_gpu(tmp_path):
    _run(LIB, tmp_path)
