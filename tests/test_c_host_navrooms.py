"""Rooms on a free map from C (tests/host_c/hmsg_host_navrooms.c, strict C99 against include/hmsg.h ALONE): the host is told by the
first hmsg_nav_room_doors how long the door lists have to be and repeats the call, then counts and fetches the legs of a path list;
what it writes equals the same calls made through the Python binding and the restatement of tests/navrooms_reference.py.  CPU: the
kernel simulator; -m gpu: libhmsg.so.  (tests/host_c/hmsg_host_rooms.c is the host of N1, the rooms of a storey as a label image.)"""
import os
import subprocess

import numpy as np
import pytest

from tests import navroute_cases as NC
from tests import navroute_reference as RR
from tests import navrooms_cases as GC
from tests import navrooms_reference as GR
from tests import parity_common as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host_c", "hmsg_host_navrooms.c")
INC = os.path.join(ROOT, "include")
LIB = os.path.join(ROOT, "holoagent_amd", "libhmsg.so")


def _compile(lib_path, out):
    cmd = ["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-O1", "-I", INC, SRC, "-o", out, lib_path,
           "-Wl,-rpath," + os.path.dirname(lib_path), "-Wl,-rpath,/opt/rocm/lib", "-Wl,--allow-shlib-undefined"]
    subprocess.run(cmd, check=True, capture_output=True)
    return out


def _run(lib_path, tmp_path):
    from holoagent_amd._lib import HmsgLib, nav_path_rooms, nav_room_doors
    L = HmsgLib(lib_path)
    m = np.ascontiguousarray(NC.rooms_map())
    seeds = list(GC.room_seeds("third"))
    minc = 10
    off = np.concatenate([[0], np.cumsum([len(s) for s in seeds])]).astype(np.int64)
    rc = np.ascontiguousarray(np.concatenate(seeds).astype(np.int32))
    pas = ((m != 0) & (RR.clearance(m) >= minc)).astype(np.uint8)
    lab, _, _ = GR.labels(pas, seeds)
    ref = GR.doors(pas, lab, len(seeds))
    src = NC.first_free(pas, (60, 90))
    f, _ = RR.field(pas, [src])
    poff, prc = RR.paths(pas, f, np.argwhere(f != U_)[::701])
    legs = GR.legs(lab, poff, prc)
    want = nav_room_doors(m, seeds, lib_=L, min_clearance=minc)
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as fh:
        np.array([m.shape[0], m.shape[1], len(seeds), minc, len(poff) - 1, 0], np.int32).tofile(fh)
        m.tofile(fh)
        off.tofile(fh)
        rc.tofile(fh)
        poff.tofile(fh)
        np.ascontiguousarray(prc).tofile(fh)
    exe = _compile(lib_path, str(tmp_path / "hmsg_host_navrooms"))
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    raw = open(fout, "rb").read()
    cells, n = m.size, len(seeds)
    nd, nc, nl = (int(v) for v in np.frombuffer(raw, np.int64, 3))
    o = 24
    got = {}
    for key, dt, count, shape in (("label", np.int32, cells, m.shape), ("passable", np.uint8, cells, m.shape), ("other", np.int32, cells, m.shape),
                                  ("door_pair", np.int32, nd * 2, (nd, 2)), ("door_off", np.int64, nd + 1, (nd + 1,)),
                                  ("door_rc", np.int32, nc * 2, (nc, 2)), ("adjacency", np.int32, n * n, (n, n)),
                                  ("leg_off", np.int64, len(poff), (len(poff),)), ("leg_room", np.int32, nl, (nl,)), ("leg_first", np.int64, nl, (nl,))):
        got[key] = np.frombuffer(raw, dt, count, o).reshape(shape)
        o += count * np.dtype(dt).itemsize
    assert o == len(raw) and nd > 1 and nc > 1                             # (the host's first lists of one entry were too short)
    assert np.array_equal(got["label"], lab) and np.array_equal(got["passable"], pas)
    for k in ("other", "door_pair", "door_off", "door_rc", "adjacency"):
        assert np.array_equal(got[k], ref[k]) and np.array_equal(got[k], want[k]), k
    for k, v in zip(("leg_off", "leg_room", "leg_first"), legs):
        assert np.array_equal(got[k], v), k
    for a, b in zip(nav_path_rooms(lab, poff, prc, lib_=L), legs):
        assert np.array_equal(a, b)
    assert "doors %d door cells %d legs %d" % (nd, nc, nl) in r.stdout


U_ = RR.UNREACHED


@pytest.mark.skipif(not os.path.exists(PC.EMU_PATH), reason="kernel simulator not built")
def test_c_host_navrooms_on_the_simulator(tmp_path):
    _run(PC.EMU_PATH, tmp_path)


@pytest.mark.gpu
def test_c_host_navrooms_gpu(tmp_path):
    _run(LIB, tmp_path)
