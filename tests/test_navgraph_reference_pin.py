"""tests/golden/navgraph.npz is what the REFERENCE's own NavigationGraph gives (with the OpenCV stand-in of
scripts/gen_navgraph_golden.py): where the reference checkout exists, a child process records the fixture again into a temporary
directory, and every array must equal the committed one.  Skipped where there is no reference tree (the fixture is then taken as
recorded)."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "navgraph.npz")


def _reference_dir():
    from oracle.refdrive.gen_golden import REF
    return REF


def test_fixture_regenerates_identically(tmp_path):
    ref = _reference_dir()
    if not os.path.isfile(os.path.join(ref, "memory", "hmsg", "graph", "navigation_graph.py")):
        pytest.skip("no reference checkout on this machine")
    out = str(tmp_path / "navgraph.npz")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "gen_navgraph_golden.py"), out], capture_output=True, text=True,
                       cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    a, b = np.load(GOLDEN), np.load(out)
    assert sorted(a.files) == sorted(b.files)
    for key in a.files:
        assert a[key].dtype == b[key].dtype and a[key].shape == b[key].shape, key
        assert np.array_equal(a[key], b[key]), key
