"""hmsg_lsap (include/hmsg.h; holoagent_amd/csrc/hmsg_lsap_host.h) against scipy.optimize.linear_sum_assignment, INDEX FOR INDEX.

The evaluator's association matrices are mostly zeros, so most of its assignments are ties, and object_semantics_eval_tp_auc walks
every assigned pair, the zero-overlap ones included: the library has to return the very assignment scipy returns, not one of equal
cost.  The matrices: tie-free, 90 % zeros with values of one decimal, all zeros, wide, tall, one row, one column, up to 60 x 60,
both values of `maximize`.  The solver runs on the host: any build of the library serves (the simulator's here).  The header is also
built into a program of its own (tests/host_cpp/eval_lsap_host.cpp), plain and under the host compiler's address and
undefined-behaviour sanitizers, and driven with the same kinds of matrices."""
import os
import shutil
import subprocess

import numpy as np
import pytest
from scipy.optimize import linear_sum_assignment

from tests import parity_common as PC

needs_emu = pytest.mark.skipif(not os.path.exists(PC.EMU_PATH), reason="kernel simulator not built")

SHAPES = [(1, 1), (1, 7), (7, 1), (2, 2), (3, 5), (5, 3), (8, 8), (13, 21), (21, 13), (30, 30), (17, 60), (60, 17), (60, 60), (59, 60), (60, 59)]


@pytest.fixture(scope="module")
def L():
    from holoagent_amd._lib import HmsgLib
    return HmsgLib(PC.EMU_PATH)


def matrices(kind, seed):
    rng = np.random.default_rng(seed)
    for nr, nc in SHAPES:
        if kind == "tie_free":
            m = rng.permutation(nr * nc).astype(np.float64).reshape(nr, nc) + rng.random((nr, nc)) * 0.25
        elif kind == "sparse_decimal":                     # what an association matrix looks like
            m = np.round(rng.random((nr, nc)), 1) * (rng.random((nr, nc)) < 0.1)
        elif kind == "zeros":
            m = np.zeros((nr, nc))
        elif kind == "few_values":
            m = rng.integers(0, 3, (nr, nc)).astype(np.float64)
        else:
            raise KeyError(kind)
        yield m


def same_as_scipy(L, m, maximize):
    from holoagent_amd._lib import lsap
    r0, c0 = linear_sum_assignment(m, maximize=maximize)
    r1, c1 = lsap(m, maximize=maximize, lib_=L)
    assert np.array_equal(r0, r1) and np.array_equal(c0, c1), (m.shape, maximize, r0.tolist(), c0.tolist(), r1.tolist(), c1.tolist())


@needs_emu
@pytest.mark.parametrize("maximize", [False, True])
@pytest.mark.parametrize("kind", ["tie_free", "sparse_decimal", "zeros", "few_values"])
def test_lsap_equals_scipy(L, kind, maximize):
    n = 0
    for seed in range(6):
        for m in matrices(kind, 100 * seed + 7):
            same_as_scipy(L, m, maximize)
            n += 1
    assert n == 6 * len(SHAPES)


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g", "-O1"]], ids=["plain", "asan_ubsan"])
def test_lsap_host_header_stand_alone(tmp_path, flags):
    """tests/host_cpp/eval_lsap_host.cpp: the header alone, in a program of its own, plain and under the host sanitizers (nothing of it
    is loaded into Python), on tie-heavy matrices"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ is needed to build tests/host_cpp/eval_lsap_host.cpp")
    exe = str(tmp_path / "eval_lsap_host")
    r = subprocess.run([cxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(root, "holoagent_amd", "csrc"),
                        os.path.join(root, "tests", "host_cpp", "eval_lsap_host.cpp"), "-o", exe] + flags, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    mats = []
    for kind in ("sparse_decimal", "zeros", "few_values", "tie_free"):
        for seed in (1, 2):
            mats += [(m, mx) for m in matrices(kind, seed) for mx in (0, 1)]
    mats.append((np.array([[np.inf, 1.0], [np.inf, 2.0]]), 0))          # infeasible
    mats.append((np.array([[0.0, np.nan]]), 1))                         # invalid
    text = "\n".join("M %d %d %d\n%s" % (m.shape[0], m.shape[1], mx, " ".join(float(v).hex() for v in m.ravel())) for m, mx in mats) + "\n"
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.strip().split("\n")
    assert len(lines) == len(mats)
    for (m, mx), line in zip(mats[:-2], lines):
        v = [int(x) for x in line.split()]
        r0, c0 = linear_sum_assignment(m, maximize=bool(mx))
        assert v[0] == 0 and v[1] == len(r0) and v[2::2] == r0.tolist() and v[3::2] == c0.tolist(), (m.shape, mx)
    assert lines[-2].split()[0] == "-1" and lines[-1].split()[0] == "-2"


@needs_emu
def test_lsap_non_contiguous_and_integer_input(L):
    rng = np.random.default_rng(3)
    m = rng.integers(0, 4, (12, 18))
    same_as_scipy(L, m[:, ::2], True)
    same_as_scipy(L, m.T, False)


@needs_emu
def test_lsap_empty_and_invalid(L, capfd):
    from holoagent_amd._lib import HmsgError, lsap
    for shape in ((0, 4), (4, 0), (0, 0)):
        r, c = lsap(np.zeros(shape), lib_=L)
        assert len(r) == 0 and len(c) == 0
    bad = np.zeros((3, 3))
    bad[1, 1] = np.nan
    with pytest.raises(HmsgError):
        lsap(bad, lib_=L)
    with pytest.raises(ValueError):
        linear_sum_assignment(bad)
    inf = np.full((2, 2), np.inf)                          # no feasible assignment: scipy raises as well
    with pytest.raises(HmsgError):
        lsap(inf, lib_=L)
    with pytest.raises(ValueError):
        linear_sum_assignment(inf)
    part = np.array([[np.inf, 1.0, 2.0], [0.5, np.inf, np.inf]])         # +inf entries beside a feasible assignment are allowed
    same_as_scipy(L, part, False)
    assert "hmsg_lsap" in capfd.readouterr().err
    with pytest.raises(HmsgError):
        lsap(np.zeros(4), lib_=L)
