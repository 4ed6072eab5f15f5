"""The host half of the navigation maps (holoagent_amd/csrc/hmsg_nav_host.h: the pose selection of get_poses_region and the disc)
against sklearn's DBSCAN and numpy themselves -- tests/navmap_reference.py -- exactly, and on heights that are not finite.  The header is built into a program of its
own (tests/host_cpp/nav_host.cpp) with the host compiler, plain and under its address and undefined-behaviour sanitizers; nothing
of it is loaded into Python."""
import os
import shutil
import subprocess

import numpy as np
import pytest
from sklearn.cluster import DBSCAN

from tests import navmap_reference as NR


def height_sets():
    """-> list of (kind, heights, eps, min_samples)"""
    rng = np.random.default_rng(77)
    out = []
    for n in list(range(1, 12)) + [31, 64, 129, 300, 1000]:                       # (129, 300, 1000: numpy's pairwise sum recurses)
        out.append(("one level", 0.8 + rng.uniform(-0.02, 0.02, n), 0.1, 5))
        out.append(("uniform", rng.uniform(0, 3, n), 0.1, 5))
    for k in range(60):                                                           # storeys, stairs between them, stray poses
        lv = rng.uniform(0, 6, int(rng.integers(1, 4)))
        h = np.concatenate([l + rng.normal(0, rng.choice([0.005, 0.03, 0.08]), int(rng.integers(3, 80))) for l in lv] +
                           [rng.uniform(0, 6, int(rng.integers(0, 30)))])
        out.append(("storeys", h[rng.permutation(len(h))], 0.1, 5))
    for k in range(20):                                                           # other parameters
        out.append(("params", rng.uniform(0, 2, int(rng.integers(5, 120))), float(rng.choice([0.05, 0.2, 0.5])), int(rng.integers(1, 8))))
    # tied counts: two clusters of equal size, a cluster as large as the noise, three equal clusters in shuffled order
    out.append(("tie", np.r_[np.full(6, 0.8), np.full(6, 1.3)], 0.1, 5))
    out.append(("tie", np.r_[np.full(6, 1.3), np.full(6, 0.8)], 0.1, 5))
    out.append(("tie noise", np.r_[0.8 + 0.01 * np.arange(5), 1.2 + 0.3 * np.arange(5)], 0.1, 5))
    out.append(("tie", rng.permutation(np.r_[np.full(7, 0.5), np.full(7, 1.5), np.full(7, 2.5), 4.0]), 0.1, 5))
    # chains on a lattice (every gap equal, far from eps), border samples between two clusters, duplicates
    out.append(("chain", 0.021 * np.arange(14) + 0.7, 0.1, 5))
    out.append(("chain", rng.permutation(0.03 * np.arange(40)), 0.1, 5))
    out.append(("border", np.r_[np.full(5, 0.0), 0.095, np.full(5, 0.19)], 0.1, 5))
    out.append(("border", np.r_[np.full(5, 0.19), 0.095, np.full(5, 0.0)], 0.1, 5))
    out.append(("border", np.r_[0.095, np.full(5, 0.19), np.full(5, 0.0)], 0.1, 5))
    out.append(("duplicates", np.repeat(rng.uniform(0, 1, 9), 4), 0.1, 5))
    # heights that are not finite (a failed localisation): sklearn refuses them; the header must stay inside its arrays -- the
    # sanitizer build watches -- and answers all noise, nothing kept
    for bad in (np.inf, -np.inf, np.nan):
        out.append(("not finite", np.r_[0.8, 0.8, bad, 0.8, 0.8, 0.8], 0.1, 5))
        out.append(("not finite", np.r_[bad, rng.uniform(0, 2, 40)], 0.1, 5))
        out.append(("not finite", np.full(7, bad), 0.1, 5))
    out.append(("not finite", np.r_[np.nan, 0.8, np.inf, 0.8, -np.inf, 0.8, 0.8, 0.8], 0.1, 5))
    return [(k, np.ascontiguousarray(h, np.float64), float(e), int(m)) for k, h, e, m in out]


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address", "-fsanitize=undefined", "-fno-sanitize-recover=all", "-g", "-O1"]],
                         ids=["plain", "asan_ubsan"])
def test_nav_host_header_stand_alone(tmp_path, flags):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ is needed to build tests/host_cpp/nav_host.cpp")
    exe = str(tmp_path / "nav_host")
    r = subprocess.run([cxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-I", os.path.join(root, "holoagent_amd", "csrc"),
                        os.path.join(root, "tests", "host_cpp", "nav_host.cpp"), "-o", exe] + flags, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    sets = height_sets()
    radii = list(range(0, 40)) + [100, 333]
    values = [0.0, 0.4, -0.4, -0.999, -1.2, 1.999, 16.5, -16.5, 2.0 ** 31, -2.0 ** 33, float("nan"), 1e300]
    text = "".join("P %d %s %d\n%s\n" % (len(h), e.hex(), m, " ".join(v.hex() for v in h.tolist())) for _, h, e, m in sets)
    text += "".join("C %d\n" % r_ for r_ in radii) + "".join("T %s\n" % float(v).hex() for v in values)
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.strip().split("\n")
    assert len(lines) == 2 * len(sets) + len(radii) + len(values)
    tied = noise_major = 0
    for i, (kind, h, eps, ms) in enumerate(sets):
        lab, keep = lines[2 * i].split(), lines[2 * i + 1].split()
        assert (lab[0], keep[0]) == ("L", "K")
        if kind == "not finite":
            assert [int(v) for v in lab[1:]] == [-1] * len(h) and keep[1:] == [], (i, kind)
            continue
        want = DBSCAN(eps=eps, min_samples=ms).fit(h.reshape(-1, 1)).labels_
        assert [int(v) for v in lab[1:]] == want.tolist(), (i, kind)
        want_keep, _ = NR.select_poses(h, eps, ms)
        assert [int(v) for v in keep[1:]] == want_keep.tolist(), (i, kind)
        counts = np.unique(want, return_counts=True)[1]
        tied += int((counts == counts.max()).sum() > 1)
        noise_major += int(want[0] == -1 and (want == -1).sum() == counts.max())
    assert tied >= 4 and noise_major >= 1                                          # the set holds what it is meant to
    for j, rad in enumerate(radii):
        got = [int(v) for v in lines[2 * len(sets) + j].split()[1:]]
        img = np.zeros((2 * rad + 1, 2 * rad + 1), np.uint8)
        NR.circle(img, (rad, rad), rad)
        assert len(got) == rad + 1
        for d in range(-rad, rad + 1):
            row = np.flatnonzero(img[rad + d])
            assert row.tolist() == list(range(rad - got[abs(d)], rad + got[abs(d)] + 1)), (rad, d)
    for j, v in enumerate(values):
        got = int(lines[2 * len(sets) + len(radii) + j].split()[1])
        if np.isfinite(v) and abs(v) < 2.0 ** 30:
            assert got == int(np.int32(v))
        else:
            assert abs(got) == 2 ** 30
