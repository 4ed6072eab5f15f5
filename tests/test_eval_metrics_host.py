"""The evaluator's metrics (holoagent_amd/csrc/hmsg_eval_metrics_host.h: evaluate_floors, the threshold sweep, np.trapz, the hydra
means, top-k accuracies from ranks) against numpy itself -- tests/eval_reference.py, the reference's lines restated --, every float64
bit for bit.

The header is built into a program of its own (tests/host_cpp/eval_metrics_host.cpp) with the host compiler, plain and under its
address and undefined-behaviour sanitizers (nothing of it is loaded into Python), and fed a few hundred random matrices with
assignments (square, P != G, all zero, TP = 0 at every threshold, entries exactly at a threshold), hydra matrices, floors of 1, 2
and 3 storeys, unequal floor counts, rank lists for class tables of 3 to 1030 names (np.trapz over more than 8 and -- with its own
records -- more than 128 samples, where numpy's pairwise sum changes its order)."""
import os
import shutil
import subprocess

import numpy as np
import pytest
from scipy.optimize import linear_sum_assignment

from tests import eval_reference as R


def hx(v):
    return " ".join(float(x).hex() for x in np.asarray(v, np.float64).reshape(-1))


def box_vertices(rng, lo, hi):
    """eight vertices of a box from y = lo to hi, in a shuffled order"""
    x0, x1, z0, z1 = rng.uniform(-5, 0), rng.uniform(0, 5), rng.uniform(-5, 0), rng.uniform(0, 5)
    v = np.array([(x, y, z) for x in (x0, x1) for y in (lo, hi) for z in (z0, z1)])
    return v[rng.permutation(8)]


def records():
    """-> list of (text, expected line)"""
    rng = np.random.default_rng(77)
    out = []

    def matrix(P, G, kind):
        if kind == "zero":                                  # nothing above the first threshold: TP = 0 everywhere
            M = np.zeros((P, G))
        elif kind == "tenths":                              # entries exactly AT the thresholds (`>` is strict; 0.3 is not linspace's 0.30000000000000004)
            M = rng.integers(0, 11, (P, G)) / 10.0 * (rng.random((P, G)) < 0.6)
        elif kind == "linspace":
            M = np.linspace(0, 1, 11)[rng.integers(0, 11, (P, G))]
        else:
            M = rng.random((P, G)) * (rng.random((P, G)) < rng.choice([0.1, 0.5, 1.0]))
        return np.ascontiguousarray(M)

    def m_record(M, row, col):
        P, G = M.shape
        s = R.sweep(M, row, col, P, G)
        c = R.counts_at(M, row, col, P, G)
        text = "M %d %d %d\n%s\n%s\n" % (P, G, len(row), hx(M), " ".join("%d %d" % (r, c_) for r, c_ in zip(row, col)))
        exp = "M %s | %s | %d %d %d %s" % (hx([s["ap"], s["acc"][6], s["prec"][6], s["rec"][6]]), " ".join(map(str, s["tp"])), c["tp"], c["fp"],
                                           c["fn"], hx([c["acc"], c["prec"], c["recall"]]))
        return text, exp

    shapes = [(1, 1), (1, 5), (5, 1), (6, 5), (5, 6), (15, 12), (12, 15), (40, 40), (3, 70)]
    for k in range(300):
        P, G = shapes[k % len(shapes)]
        M = matrix(P, G, ("zero", "zero", "tenths", "linspace", "random", "random", "random")[k % 7])
        row, col = linear_sum_assignment(M, maximize=True)
        out.append(m_record(M, row, col))
    # an assignment that is not scipy's (fewer pairs than min(P, G), any order)
    M = matrix(8, 9, "random")
    out.append(m_record(M, np.array([5, 2, 7]), np.array([1, 8, 0])))
    out.append(m_record(M, np.zeros(0, np.int64), np.zeros(0, np.int64)))
    for k in range(60):
        P, G = shapes[k % len(shapes)]
        a, b = np.minimum(matrix(P, G, "random") * 1.3, 1.0), np.minimum(matrix(P, G, "random") * 1.3, 1.0)
        hp, hr = R.hydra(a, b)
        out.append(("H %d %d\n%s\n%s\n" % (P, G, hx(a), hx(b)), "H " + hx([hp, hr])))
    # floors: 1, 2, 3 (and 5) storeys, predictions off by less / more than half a metre, bounds exactly 0.5 apart
    for k in range(80):
        F = (1, 2, 3, 5)[k % 4]
        cuts = np.sort(rng.uniform(-2, 12, 2 * F))
        lower, upper = cuts[0::2].copy(), cuts[1::2].copy()
        order = rng.permutation(F)
        shift = rng.choice([0.0, 0.2, 0.5, 0.6, 3.0], (F, 2)) * rng.choice([-1, 1], (F, 2))
        verts = np.array([box_vertices(rng, *sorted((lower[f] + shift[f, 0], upper[f] + shift[f, 1]))) for f in order])
        m = R.floors(lower, upper, verts)
        out.append(("F %d %d\n%s\n%s\n%s\n" % (F, F, hx(lower), hx(upper), hx(verts)),
                    "F %d %d %d %s" % (m["tp"], m["fp"], m["fn"], hx([m["acc"], m["prec"], m["recall"]]))))
    for Fg, Fp in ((1, 2), (3, 2), (2, 0), (0, 2)):
        lower, upper = np.arange(Fg) * 3.0, np.arange(Fg) * 3.0 + 2.5
        verts = np.array([box_vertices(rng, 3.0 * f, 3.0 * f + 2.5) for f in range(Fp)]).reshape(Fp, 8, 3)
        with pytest.raises((ValueError, IndexError)):
            R.floors(lower, upper, verts)
        out.append(("F %d %d\n%s\n%s\n%s\n" % (Fg, Fp, hx(lower), hx(upper), hx(verts)), "F invalid"))
    # top-k
    for k in range(60):
        C = (3, 10, 11, 40, 95, 1030, 2000)[k % 7]
        n = (1, 12, 33)[k % 3]
        rank = rng.integers(0, C + 1, n)
        ks = [0, 1, 5, 10, C, C + 1][: 2 + k % 5]
        acc, auc = R.top_k_from_ranks(rank, ks, C)
        out.append(("K %d %d %d\n%s\n%s\n" % (n, C, len(ks), " ".join(map(str, rank)), " ".join(map(str, ks))),
                    "K " + hx([acc[k_] for k_ in ks] + [auc])))
    # np.trapz by itself: every length around the switches of numpy's sum (8, 128 and the halving above)
    for n in list(range(0, 20)) + [127, 128, 129, 130, 137, 255, 257, 300, 1031]:
        y, x = rng.random(n), np.sort(rng.random(n))
        out.append(("T %d\n%s\n%s\n" % (n, hx(y), hx(x)), "T " + hx([R.trapz(y, x) if n else 0.0])))
    return out


@pytest.fixture(scope="module")
def recs():
    return records()


def test_records_hold_what_they_are_meant_to(recs):
    m = [e.split(" | ") for _, e in recs if e.startswith("M ")]
    assert len(m) >= 300
    tp0 = [int(p[1].split()[0]) for p in m]
    assert sum(t == 0 for t in tp0) >= 40 and sum(t > 0 for t in tp0) >= 100
    assert sum(len(set(p[1].split())) > 3 for p in m) >= 50                   # sweeps that actually fall
    f = [e.split() for _, e in recs if e.startswith("F ") and "invalid" not in e]
    assert {int(v[1]) + int(v[3]) for v in f} >= {2, 3, 4} and any(int(v[1]) == 0 for v in f) and any(int(v[2]) == 0 for v in f)
    assert sum(e == "F invalid" for _, e in recs) == 4


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address", "-fsanitize=undefined", "-fno-sanitize-recover=all", "-g", "-O1"]],
                         ids=["plain", "asan_ubsan"])
def test_eval_metrics_header_stand_alone(tmp_path, recs, flags):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ is needed to build tests/host_cpp/eval_metrics_host.cpp")
    exe = str(tmp_path / "eval_metrics_host")
    r = subprocess.run([cxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-I", os.path.join(root, "holoagent_amd", "csrc"),
                        os.path.join(root, "tests", "host_cpp", "eval_metrics_host.cpp"), "-o", exe] + flags, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe], input="".join(t for t, _ in recs), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.strip().split("\n")
    assert len(lines) == len(recs)

    def norm(line):                      # hexadecimal floats as numbers (C's %a and Python's hex() spell them differently)
        return [float.fromhex(w).hex() if ("x" in w or w in ("inf", "nan")) else w for w in line.split()]
    for i, (got, (text, exp)) in enumerate(zip(lines, recs)):
        assert norm(got) == norm(exp), (i, text[:200], got, exp)


def test_c_abi_and_python_wrappers():
    """hmsg_eval_floors / _metrics_from_matrix / _counts_at / _hydra_means / _top_k (host code of the library; here the simulator
    build carries it) through holoagent_amd._lib, the same bits as numpy"""
    from holoagent_amd import _lib as B
    from tests import parity_common as PC
    if not os.path.exists(PC.EMU_PATH):
        pytest.skip("kernel simulator not built")
    L = B.HmsgLib(PC.EMU_PATH)
    rng = np.random.default_rng(3)
    for P, G in ((6, 5), (5, 9), (1, 1)):
        M = np.round(rng.random((P, G)), 1) * (rng.random((P, G)) < 0.7)
        row, col = linear_sum_assignment(M, maximize=True)
        s, c = R.sweep(M, row, col, P, G), R.counts_at(M, row, col, P, G)
        assert B.eval_metrics_from_matrix(M, row, col, 6, lib_=L) == (float(s["ap"]), float(s["acc"][6]), float(s["prec"][6]), float(s["rec"][6]))
        got = B.eval_counts_at(M, row, col, 0.5, lib_=L)
        assert {k: got[k] for k in c} == {k: (float(v) if k in ("acc", "prec", "recall") else v) for k, v in c.items()}
        a, b = rng.random((P, G)), rng.random((P, G))
        assert B.eval_hydra_means(a, b, lib_=L) == tuple(float(v) for v in R.hydra(a, b))
    lower, upper = np.array([0.0, 3.1]), np.array([2.9, 6.0])
    verts = np.array([box_vertices(rng, 0.1, 2.8), box_vertices(rng, 3.9, 6.2)])
    want = R.floors(lower, upper, verts)
    assert B.eval_floors(lower, upper, verts, lib_=L) == {k: (float(v) if k in ("acc", "prec", "recall") else v) for k, v in want.items()}
    with pytest.raises(B.HmsgError):
        B.eval_floors(lower, upper, verts[:1], lib_=L)
    with pytest.raises(B.HmsgError):
        B.eval_metrics_from_matrix(np.zeros((2, 2)), [0, 2], [0, 1], 6, lib_=L)       # a pair outside the matrix
    rank = rng.integers(0, 41, 12)
    acc, auc = R.top_k_from_ranks(rank, [1, 5, 10], 40)
    assert B.eval_top_k(rank, 40, [1, 5, 10], lib_=L) == (acc, float(auc))
