"""hmsg_cloud_set_overlaps / hmsg_cloud_set_overlaps_kd (include/hmsg.h; holoagent_amd/csrc/hmsg_eval.hip: k_ev_cells, k_ev_gather,
k_ev_probe) pinned on their COUNTS.

The sets are those of tests/overlap_cases.py, whose answer is known exactly (an integer model on the knife-edge lattice, the
reference's float32 arithmetic restated in numpy on realistic clouds, oracle.faiss_blas_nn_sqdist for faiss's BLAS form), at the
radius the sets were built for, 1.5 * case.vs; every set is given three ways: one set against itself (sorted once), the same clouds
as two separate arrays, and as two different sets (the pairs' first clouds | their second clouds).  On top of them: cloud sizes around
the kernel's chunk of 256 query points and around faiss's switch at 20, an empty cloud, one cloud named by many pairs, no pairs, bad
arguments refused with the output untouched, and the float64 comparison of find_intersection_share against scipy's cKDTree with a
point placed exactly at the radius.

Simulator here; tests/test_eval_gpu.py runs the same checks on the library (host arrays and torch device tensors)."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import overlap_cases as OC
from tests import parity_common as PC

HMSG_ERR_INVALID = -1
SIZES = (1, 19, 20, 255, 256, 257, 513)


class Hook:
    """the library + one handle per distance form; `wrap` turns the numpy inputs into what is handed over (torch device tensors in
    the GPU test)"""

    def __init__(self, L, wrap=None):
        self.L, self.scenes, self.wrap = L, {}, wrap or (lambda a: a)

    def scene(self, form):
        from holoagent_amd._lib import Scene
        if form not in self.scenes:
            self.scenes[form] = Scene(lib_=self.L, height=8, width=8, max_frames=1, max_masks=1, feat_dim=16, overlap_distance_form=form)
        return self.scenes[form]

    def close(self):
        for s in self.scenes.values():
            s.close()
        self.scenes = {}

    def counts(self, form, A, B, pairs, radius, kd=False):
        """A, B: lists of float64 [n][3] clouds (B is A: one set against itself) -> int64 [P][2]"""
        pa, oa = csr(A)
        pa, oa = self.wrap(pa), self.wrap(oa)
        pb, ob = (pa, oa) if B is A else tuple(self.wrap(v) for v in csr(B))
        pr = self.wrap(np.ascontiguousarray(pairs, np.int32).reshape(-1, 2))
        return self.scene(form).cloud_set_overlaps(pa, oa, pb, ob, pr, radius, kd=kd).astype(np.int64)


def csr(clouds):
    off = np.zeros(len(clouds) + 1, np.int64)
    off[1:] = np.cumsum([len(c) for c in clouds])
    pts = np.concatenate([np.asarray(c, np.float64).reshape(-1, 3) for c in clouds] + [np.zeros((0, 3))])
    return np.ascontiguousarray(pts), off


def three_ways(case, pairs):
    """-> [(tag, A, B, pairs)]"""
    pairs = np.asarray(pairs, np.int32).reshape(-1, 2)
    ua, ia = np.unique(pairs[:, 0], return_inverse=True)
    ub, ib = np.unique(pairs[:, 1], return_inverse=True)
    split = np.stack([ia.reshape(-1), ib.reshape(-1)], 1).astype(np.int32)
    return [("one set", case.clouds, case.clouds, pairs),
            ("two arrays", case.clouds, [c.copy() for c in case.clouds], pairs),
            ("two sets", [case.clouds[k] for k in ua], [case.clouds[k] for k in ub], split)]


def check_case(hk, case, form, ways=(0, 1, 2)):
    exp = case.expected(form)
    radius = 1.5 * case.vs
    for w, (tag, A, B, pairs) in enumerate(three_ways(case, case.pairs)):
        if w not in ways:
            continue
        got = hk.counts(form, A, B, pairs, radius)
        bad = np.flatnonzero((got != exp).any(1))
        assert len(bad) == 0, "%s (form %d, %s): %d of %d pairs miscounted; pair %d %s: got %s, expected %s of (%d, %d) points" % (
            case.name, form, tag, len(bad), len(pairs), bad[0], case.pairs[bad[0]].tolist(), got[bad[0]].tolist(), exp[bad[0]].tolist(),
            len(case.clouds[case.pairs[bad[0], 0]]), len(case.clouds[case.pairs[bad[0], 1]]))


LATTICE = {
    "knife": lambda: [OC.knife(p) for p in OC.PLACES],
    "piles": lambda: [OC.piles(p) for p in ("origin", "far")],
    "degenerate": lambda: [OC.degenerate(p) for p in ("origin", "far")],
    "neighbours": lambda: [OC.neighbours(p) for p in ("origin", "far")],
}


def lattice(hk, family, form):
    for case in LATTICE[family]():
        check_case(hk, case, form)


def realistic(hk, place, form):
    check_case(hk, OC.realistic(place), form, ways=(0, 2))


def size_case():
    """query clouds of 1 .. 513 points on EITHER side: prefixes of two different delta sets hung on one 7^3 lattice, every size
    against every size, and each against the lattice itself (343 points)"""
    X1, Y, _, _ = OC.knife_clouds("far", ny=7, seed=1)
    X2, Y2, _, _ = OC.knife_clouds("far", ny=7, seed=4)
    assert np.array_equal(Y, Y2) and len(X1) > 513 and len(X2) > 513
    ints = [X1[:n] for n in SIZES] + [X2[100:100 + n] for n in SIZES] + [Y]
    k = len(SIZES)
    pairs = [(a, k + b) for a in range(k) for b in range(k)] + [(a, 2 * k) for a in range(2 * k)] + [(2 * k, a) for a in range(k)]
    return OC.Case("eval_sizes", OC.VS_LATTICE, ints=ints, pairs=pairs)


def sizes(hk, form):
    case = size_case()
    exp = case.expected(form)
    assert (exp > 0).any() and (exp[:, 0] < case.sizes[case.pairs[:, 0]]).any()
    check_case(hk, case, form, ways=(0, 2))


def shapes_of_the_pair_list(hk):
    """an empty cloud, one cloud named by many pairs (and one pair named twice), nA != nB, no pairs at all"""
    X, Y, cls, _ = OC.knife_clouds("origin")
    base = OC.Case("eval_shapes", OC.VS_LATTICE, ints=[X[:300], X[300:700], X[700:], Y], pairs=[(0, 3), (1, 3), (2, 3)])
    exp = base.expected()
    radius = 1.5 * OC.VS_LATTICE
    empty = np.zeros((0, 3))
    A = [base.clouds[0], empty, base.clouds[1], base.clouds[2], empty]            # nA = 5
    B = [empty, base.clouds[3]]                                                   # nB = 2
    pairs = np.array([(0, 1), (2, 1), (3, 1), (1, 1), (0, 0), (4, 0), (2, 1), (0, 1), (3, 1)], np.int32)
    want = np.array([exp[0], exp[1], exp[2], (0, 0), (0, 0), (0, 0), exp[1], exp[0], exp[2]], np.int64)
    got = hk.counts(0, A, B, pairs, radius)
    assert np.array_equal(got, want), (got.tolist(), want.tolist())
    assert hk.counts(0, A, B, np.zeros((0, 2), np.int32), radius).shape == (0, 2)
    only_empty = hk.counts(0, [empty], [empty, empty], np.array([(0, 1)], np.int32), radius)      # sets without a single point
    assert np.array_equal(only_empty, [[0, 0]])
    # a point set without points on one side only
    assert np.array_equal(hk.counts(0, [empty], B, np.array([(0, 1)], np.int32), radius), [[0, 0]])


def wide_span(hk):
    """two groups of clouds a kilometre apart: the lattice over both has more than 2^32 cells, so the cell key is sorted in two passes
    (low half, high half); pairs inside either group and across (no witness)"""
    base = OC.realistic("origin")
    shift = np.array([900.0, -500.0, 700.0])
    near = base.clouds[:5]
    clouds = near + [c + shift for c in near]
    radius = 1.5 * base.vs
    cell = radius * (1.0 + 1e-3) + 2e-3
    assert np.prod(np.floor(np.abs(shift) / cell) + 1.0) > 2.0 ** 33
    pairs = [(a, b) for a in range(5) for b in range(a + 1, 5)]
    pairs = pairs + [(a + 5, b + 5) for a, b in pairs] + [(0, 5), (6, 1), (2, 7)]
    case = OC.Case("eval_wide_span", base.vs, clouds=clouds, pairs=pairs)
    exp = case.expected()
    assert (exp[:10] > 0).any() and (exp[10:20] > 0).any() and (exp[20:] == 0).all()
    check_case(hk, case, OC.FORM_DIRECT, ways=(0, 2))


def raw(hk, form, nA, ptsA, offA, nB, ptsB, offB, pairs, radius, kd=False):
    P = len(pairs)
    counts = np.full((max(P, 1), 2), 0xDEADBEEF, np.uint32)
    fn = hk.L.c.hmsg_cloud_set_overlaps_kd if kd else hk.L.c.hmsg_cloud_set_overlaps
    rc = fn(hk.scene(form).h, nA, ptsA.ctypes.data, offA.ctypes.data, nB, ptsB.ctypes.data, offB.ctypes.data, P, pairs.ctypes.data, float(radius),
            counts.ctypes.data)
    return rc, counts


def bad_arguments(hk):
    pts = np.arange(30, dtype=np.float64).reshape(10, 3)
    off = np.array([0, 4, 10], np.int64)
    ok = np.array([[0, 1]], np.int32)
    rc, counts = raw(hk, 0, 2, pts, off, 2, pts, off, ok, 0.1)
    assert rc == 0 and (counts != 0xDEADBEEF).all()
    refused = [
        (np.array([1, 4, 10], np.int64), off, ok, 0.1),              # offsets that do not start at 0
        (np.array([0, 6, 4], np.int64), off, ok, 0.1),               # ... that decrease
        (off, np.array([0, 11, 10], np.int64), ok, 0.1),
        (off, off, np.array([[0, 2]], np.int32), 0.1),               # no such cloud
        (off, off, np.array([[0, 1], [-1, 0]], np.int32), 0.1),
        (off, off, ok, 0.0), (off, off, ok, -1.0), (off, off, ok, float("nan")),
    ]
    for oa, ob, pr, r in refused:
        for kd in (False, True):
            rc, counts = raw(hk, 0, 2, pts, oa, 2, pts, ob, pr, r, kd)
            assert rc == HMSG_ERR_INVALID, (oa.tolist(), ob.tolist(), pr.tolist(), r)
            assert (counts == 0xDEADBEEF).all(), "a refused call wrote its output"
        assert len(hk.L.c.hmsg_last_error(hk.scene(0).h)) > 0
    assert hk.L.c.hmsg_cloud_set_overlaps(None, 0, None, None, 0, None, None, 0, None, 0.1, None) == HMSG_ERR_INVALID
    bad = pts.copy()
    bad[3, 1] = np.inf
    assert raw(hk, 0, 2, bad, off, 2, bad, off, ok, 0.1)[0] == HMSG_ERR_INVALID


def kd_share(A, B, radius):
    """the counting of find_intersection_share (utils/graph_utils.py:160-189): points of A with a point of B inside the bound"""
    from scipy.spatial import cKDTree
    if len(A) == 0 or len(B) == 0:
        return 0
    _, idx = cKDTree(B).query(A, k=1, distance_upper_bound=radius, p=2)
    return int((idx != len(B)).sum())


def kd_mode(hk):
    rng = np.random.default_rng(21)
    r = 0.05
    room = lambda n, shift: np.stack([rng.uniform(0, 3.0, n), np.full(n, 1.25), rng.uniform(0, 2.0, n)], 1) + np.asarray(shift)
    clouds = [room(1500, (0, 0, 0)), room(900, (0.5, 0, 0.3)), room(400, (2.9, 0.03, 0)), room(20, (1.0, 0.049, 1.0)), room(1, (1.5, 0, 1.0)),
              np.round(room(700, (10.0, -3.0, 20.0)) / 0.05) * 0.05, np.round(room(700, (10.0, -3.0, 20.0)) / 0.05) * 0.05 + [0.05, 0, 0]]
    # a point exactly AT the radius (0.05 * 0.05 is radius * radius to the bit: not closer), one just inside, one just outside
    at, inside, outside = r, np.nextafter(r, 0.0), np.nextafter(r, 1.0)
    clouds += [np.zeros((1, 3))] + [np.array([[d, 0.0, 0.0]]) for d in (at, inside, outside)]
    pairs = [(a, b) for a in range(7) for b in range(7) if a != b] + [(7, 8), (7, 9), (7, 10), (8, 7)]
    want = np.array([[kd_share(clouds[a], clouds[b], r), kd_share(clouds[b], clouds[a], r)] for a, b in pairs], np.int64)
    assert want[-4:].tolist() == [[0, 0], [1, 1], [0, 0], [0, 0]], "cKDTree takes a point at the bound?"
    assert (want[:42] > 0).any() and (want[30:42] > 0).any()
    got = hk.counts(0, clouds, clouds, np.array(pairs, np.int32), r, kd=True)
    bad = np.flatnonzero((got != want).any(1))
    assert len(bad) == 0, (bad.tolist(), got[bad].tolist(), want[bad].tolist())
    # the same clouds (two of them snapped to a 5 cm lattice: neighbouring sites lie AT the radius up to rounding) in the float32
    # comparison of find_overlapping_ratio_faiss
    f32 =hk.counts(0, clouds, clouds, np.array(pairs[:42], np.int32), r)
    ref = np.array([[OC.brute_f32(clouds[a], clouds[b], np.float32(r * r)).sum(), OC.brute_f32(clouds[b], clouds[a], np.float32(r * r)).sum()]
                    for a, b in pairs[:42]], np.int64)
    assert np.array_equal(f32, ref)


# ---- fixtures and tests
needs_emu = pytest.mark.skipif(not os.path.exists(PC.EMU_PATH), reason="kernel simulator not built")


@pytest.fixture(scope="module")
def emu():
    from holoagent_amd._lib import HmsgLib
    hk = Hook(HmsgLib(PC.EMU_PATH))
    yield hk
    hk.close()


@needs_emu
@pytest.mark.parametrize("form", [OC.FORM_DIRECT, OC.FORM_BLAS])
@pytest.mark.parametrize("family", list(LATTICE))
def test_lattice_sets_simulator(emu, family, form):
    lattice(emu, family, form)


@needs_emu
@pytest.mark.parametrize("form", [OC.FORM_DIRECT, OC.FORM_BLAS])
@pytest.mark.parametrize("place", ["origin", "far"])
def test_realistic_sets_simulator(emu, place, form):
    realistic(emu, place, form)


@needs_emu
@pytest.mark.parametrize("form", [OC.FORM_DIRECT, OC.FORM_BLAS])
def test_cloud_sizes_simulator(emu, form):
    sizes(emu, form)


@needs_emu
def test_the_forms_are_told_apart_simulator(emu):
    """the BLAS switch is seen to do something on these sets"""
    cases = [OC.realistic("far"), OC.knife("far"), size_case()]
    assert sum(OC.forms_differ(c) for c in cases) > 0


@needs_emu
def test_shapes_of_the_pair_list_simulator(emu):
    shapes_of_the_pair_list(emu)


@needs_emu
def test_wide_span_simulator(emu):
    wide_span(emu)


@needs_emu
def test_bad_arguments_simulator(emu):
    bad_arguments(emu)


@needs_emu
def test_kd_comparison_simulator(emu):
    kd_mode(emu)
