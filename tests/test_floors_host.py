"""The host half of hmsg_segment_floors (holoagent_amd/csrc/hmsg_floors_host.h: scipy.ndimage.gaussian_filter1d on int64 counts,
np.percentile, scipy.signal.find_peaks(distance, height), the chaining of the peak heights and the pick / adjust rules of the
reference's graph.py:645-741) against scipy and numpy themselves -- tests/floors_cases.py::reference --, EVERY number exactly: the
smoothed counts, the peaks, the slabs bit for bit.

The header is built into a program of its own (tests/host_cpp/floors_host.cpp) with the host compiler, plain and under its address
and undefined-behaviour sanitizers (nothing of it is loaded into Python), and fed more than 500 height histograms of 1 to 1200 bins:
shorter than the filter's reflect padding, one bin, all zero, constant, single spikes, plateaus, combs of equal peaks (peaks exactly
at the percentile height, chains of more than 16 peaks, ties of the distance rule and of the pick), peaks 19 / 20 / 21 bins apart,
chain gaps of exactly 1.0 and one ulp more, picks exactly 2.5 apart and one ulp less.  What the set is meant to contain is asserted
on the reference's answers, not on the program's.  Equal heights follow the library's rule (hmsg_floors_host.h); histograms
without such a tie must also equal plain find_peaks(distance=20.0) and numpy's default argsort."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import floors_cases as FC


def _spikes(bins, where, amount):
    c = np.zeros(bins, np.int64)
    for w, a in zip(where, amount):
        c[w] += a
    return c


def _gap_pairs(lo, hi, bins, apart, want):
    """bins a, a + apart whose lower edges differ by exactly `want`"""
    e = np.linspace(lo, hi, bins + 1)
    return [int(a) for a in np.flatnonzero(e[apart:-1] - e[:-apart - 1] == want) if 30 < a < bins - apart - 30]


def histograms():
    """-> list of (kind, counts int64, ymin, ymax)"""
    rng = np.random.default_rng(2024)
    out = []

    def span(bins):                          # a range whose int(|hi - lo| / 0.01) is about `bins`, as the library would see it
        lo = float(np.round(rng.uniform(-3, 3), 3))
        return lo, lo + bins * 0.01 + 0.004

    # ---- every length up to 40 (the filter's reflect padding is 8: longer than the array below 9, and more than twice it below 5)
    for n in range(1, 41):
        for k in range(3):
            c = rng.integers(0, (3, 40, 2000)[k], n)
            out.append(("short", c, *span(n)))
    for n in (1, 2, 3, 16, 17, 18, 100, 1200):
        out.append(("zeros", np.zeros(n, np.int64), *span(n)))
        out.append(("constant", np.full(n, 7, np.int64), *span(n)))
        out.append(("spike", _spikes(n, [n // 2], [500]), *span(n)))
        out.append(("spike_first", _spikes(n, [0], [500]), *span(n)))
        out.append(("spike_last", _spikes(n, [n - 1], [500]), *span(n)))
    # ---- random: sparse small counts (plateaus after truncation), storeys with walls, huge counts
    for k in range(120):
        n = int(rng.integers(41, 1201))
        c = rng.poisson(rng.choice([0.2, 1.0, 3.0]), n)
        out.append(("poisson", c, *span(n)))
    for k in range(120):
        n = int(rng.integers(60, 1201))
        x = np.arange(n)
        c = rng.poisson(rng.choice([0.0, 0.5, 4.0]), n).astype(np.float64)
        for lvl in rng.uniform(0, n, int(rng.integers(1, 9))):
            c += rng.choice([30, 200, 200, 5000]) * np.exp(-0.5 * ((x - lvl) / rng.choice([0.3, 1.5, 4.0])) ** 2)
        out.append(("storeys", c.astype(np.int64), *span(n)))
    for k in range(20):
        n = int(rng.integers(30, 400))
        out.append(("huge", rng.integers(0, 2 ** 40, n) * (rng.random(n) < 0.2), *span(n)))
    # ---- combs of EQUAL spikes: every peak at the percentile height when more than a tenth of the bins are peaks, ties of the distance
    # rule below 20 bins, chains of more than 16 peaks, ties of the pick
    for period in (7, 9, 10, 11, 13, 19, 20, 21, 25, 30, 50, 99, 100, 101):
        for n in (240, 601, 1200):
            for amount in (17, 400):
                out.append(("comb", _spikes(n, range(period // 2, n - 2, period), [amount] * n), *span(n)))
        c = _spikes(900, range(period // 2, 898, period), [300] * 900)
        c[rng.integers(0, 900, 40)] += 1                                     # ... and nearly equal ones
        out.append(("comb_jitter", c, *span(900)))
    # ---- two and three peaks 19, 20 and 21 bins apart, equal and unequal, either side the higher
    for d in (19, 20, 21):
        for a, b in ((300, 300), (300, 301), (301, 300), (40, 41)):
            out.append(("apart", _spikes(200, [60, 60 + d, 150], [a, b, 100]), *span(200)))
            out.append(("apart", _spikes(200, [60, 60 + d, 60 + 2 * d], [a, b, a]), *span(200)))
    # ---- plateaus: flat tops of two to five bins, wide enough to survive the filter as equal integers
    for w in (2, 3, 4, 5, 12, 13):
        for amount in (10, 1000):
            c = np.zeros(300, np.int64)
            c[100:100 + w] = amount
            c[200:200 + 2 * w] = amount
            out.append(("plateau", c, *span(300)))
    # ---- chain gaps of exactly 1.0, one ulp more and one ulp less; picks exactly 2.5 apart, one ulp more and less
    lo, hi, bins = -0.37, -0.37 + 700 * 0.01, 700
    assert int(np.abs(hi - lo) / 0.01) in (699, 700)
    for want in (1.0, np.nextafter(1.0, 2.0), np.nextafter(1.0, 0.0)):
        pairs = _gap_pairs(lo, hi, bins, 100, want)
        assert len(pairs) >= 2, want
        for a in pairs[:3]:
            out.append(("gap_1.0", _spikes(bins, [a, a + 100], [300, 200]), lo, hi))
            out.append(("gap_1.0", _spikes(bins, [a, a + 100, min(a + 400, bins - 20)], [300, 200, 250]), lo, hi))
    for want in (2.5, np.nextafter(2.5, 3.0), np.nextafter(2.5, 0.0)):
        pairs = _gap_pairs(lo, hi, bins, 250, want)
        assert len(pairs) >= 2, want
        for a in pairs[:3]:
            out.append(("gap_2.5", _spikes(bins, [a, a + 250], [300, 200]), lo, hi))
            out.append(("gap_2.5", _spikes(bins, [a, a + 250, min(a + 380, bins - 20)], [300, 200, 250]), lo, hi))
    return [(k, np.ascontiguousarray(c, np.int64), float(a), float(b)) for k, c, a, b in out]


@pytest.fixture(scope="module")
def cases():
    hs = histograms()
    return hs, [FC.reference(c, lo, hi) for _, c, lo, hi in hs]


def test_histograms_hold_what_they_are_meant_to(cases):
    hs, refs = cases
    assert len(hs) >= 500
    lens = {len(c) for _, c, _, _ in hs}
    assert set(range(1, 41)) <= lens and max(lens) == 1200
    n_peaks = np.array([len(r.peaks) for r in refs])
    assert (n_peaks == 0).sum() >= 10 and (n_peaks == 1).sum() >= 10                       # the fallback slab
    assert sum(len(r.slabs) == 1 and len(r.picks) < 2 for r in refs) >= 20
    assert max(max((len(c) for c in r.chains), default=0) for r in refs) > 16
    plateau = at_height = 0
    gaps, pick_gaps, apart = set(), set(), set()
    for r in refs:
        s, p = r.smooth, r.peaks
        plateau += int(((s[p - 1] == s[p]) | (s[p + 1] == s[p])).sum()) if len(p) else 0
        at_height += int((s[p] == r.height).sum()) if len(p) else 0
        gaps |= set(np.diff(r.edges[p]).tolist())
        pick_gaps |= set(np.diff(r.picks).tolist())
        apart |= set(np.diff(r.candidates).tolist())
    assert plateau >= 20 and at_height >= 20
    assert {1.0, np.nextafter(1.0, 2.0), np.nextafter(1.0, 0.0)} <= gaps
    assert {2.5, np.nextafter(2.5, 3.0), np.nextafter(2.5, 0.0)} <= pick_gaps
    assert {19, 20, 21} <= apart
    assert sum(r.pick_tie for r in refs) >= 10 and sum(r.dist_tie_decides for r in refs) >= 10


def test_reference_is_plain_scipy_and_numpy_without_ties(cases):
    """the library's rule for equal heights is the ONLY thing the reference adds to scipy and numpy"""
    hs, refs = cases
    n = 0
    for (kind, c, lo, hi), r in zip(hs, refs):
        if r.pick_tie or r.dist_tie:
            continue
        q = FC.reference(c, lo, hi, ties="numpy")
        assert np.array_equal(q.peaks, r.peaks) and np.array_equal(q.slabs, r.slabs), (kind, len(c))
        n += 1
    assert n >= 200


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address", "-fsanitize=undefined", "-fno-sanitize-recover=all", "-g", "-O1"]],
                         ids=["plain", "asan_ubsan"])
def test_floors_host_header_stand_alone(tmp_path, cases, flags):
    hs, refs = cases
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ is needed to build tests/host_cpp/floors_host.cpp")
    exe = str(tmp_path / "floors_host")
    r = subprocess.run([cxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-I", os.path.join(root, "holoagent_amd", "csrc"),
                        os.path.join(root, "tests", "host_cpp", "floors_host.cpp"), "-o", exe] + flags, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    text = "".join("H %d %s %s\n%s\n" % (len(c), lo.hex(), hi.hex(), " ".join(str(int(v)) for v in c)) for _, c, lo, hi in hs)
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.strip().split("\n")
    assert len(lines) == 3 * len(hs)
    for i, ((kind, c, lo, hi), ref) in enumerate(zip(hs, refs)):
        s, p, l = (lines[3 * i + k].split() for k in range(3))
        assert (s[0], p[0], l[0]) == ("S", "P", "L")
        what = (i, kind, len(c))
        assert int(s[1]) == len(c) and [int(v) for v in s[2:]] == ref.smooth.tolist(), what
        assert int(p[1]) == len(p) - 2 and [int(v) for v in p[2:]] == ref.peaks.tolist(), what
        got = np.array([float.fromhex(v) for v in l[2:]]).reshape(-1, 2)
        assert int(l[1]) == len(got) and got.shape == ref.slabs.shape and (got == ref.slabs).all(), (what, got.tolist(), ref.slabs.tolist())
