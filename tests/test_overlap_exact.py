"""The overlap counting of instance merging, pinned on its COUNTS (find_overlapping_ratio_faiss, utils/graph_utils.py:620-662).

The scene-level merge tests only see `ratio > threshold` per pair, far from the threshold; the hierarchical merge caches the ratio
values.  Here the hook hmsg_test_overlap (include/hmsg_test.h) drives Merger::build_indices / push_grids / overlap_ratios
(holoagent_amd/csrc/hmsg_merge.hip) -- the launches, work lists and read-back of a fold step -- on the sets of
tests/overlap_cases.py, whose counts are known exactly: an integer model on the knife-edge lattice, the reference's float32
arithmetic restated in numpy on realistic clouds, oracle.faiss_blas_nn_sqdist for faiss's BLAS form.

  value mode     (decide_th < 0, the hierarchical merge) both counts of every pair are exact, nothing is skipped, the ratio has
                 the bits of max(c1 / n1, c2 / n2)
  decision mode  (the sequential merge) the first count is exact; a pair the first ratio decides is not scanned further; a pair
                 the box bound decides must indeed stay at or below the threshold; every other pair has an exact second count; the
                 decision is the reference's
Simulator here, the same checks marked `gpu` on the library."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import overlap_cases as OC
from tests import parity_common as PC

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
HMSG_ERR_INVALID = -1


class Hook:
    """the library + one handle per (voxel_size, distance form): the hook takes both from the handle's config"""

    def __init__(self, L):
        self.L, self.scenes = L, {}

    def handle(self, vs, form):
        from holoagent_amd._lib import Scene
        if (vs, form) not in self.scenes:
            self.scenes[(vs, form)] = Scene(lib_=self.L, height=8, width=8, max_frames=1, max_masks=1, feat_dim=16, voxel_size=vs,
                                            overlap_distance_form=form)
        return self.scenes[(vs, form)].h

    def close(self):
        for s in self.scenes.values():
            s.close()
        self.scenes = {}

    def raw(self, vs, form, sizes, n_base, pts, pairs, th):
        sizes = np.ascontiguousarray(sizes, np.int64)
        pts = np.ascontiguousarray(pts, np.float64)
        pairs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
        nb = None if n_base is None else np.ascontiguousarray(n_base, np.int64)
        P = len(pairs)
        counts, state = np.full((max(P, 1), 2), 0xDEADBEEF, np.uint32), np.full(max(P, 1), 9, np.uint8)
        ratio = np.full(max(P, 1), np.nan)
        rc = self.L.c.hmsg_test_overlap(self.handle(vs, form), len(sizes), sizes.ctypes.data, None if nb is None else nb.ctypes.data,
                                        pts.ctypes.data, P, pairs.ctypes.data, float(th), counts.ctypes.data, state.ctypes.data,
                                        ratio.ctypes.data)
        return rc, counts[:P].astype(np.int64), state[:P], ratio[:P]

    def run(self, case, form, th, pairs=None):
        pairs = case.pairs if pairs is None else pairs
        rc, counts, state, ratio = self.raw(case.vs, form, case.sizes, case.n_base, np.concatenate(case.clouds), pairs, th)
        assert rc == 0, (case.name, rc)
        return counts, state, ratio


def oriented(case, pairs, exp):
    """expected counts as the hook reports them: the pair's SMALLER cloud first (of equal sizes: the pair's first)"""
    n = case.sizes
    na, nb = n[pairs[:, 0]], n[pairs[:, 1]]
    swap = na > nb
    c1, c2 = np.where(swap, exp[:, 1], exp[:, 0]), np.where(swap, exp[:, 0], exp[:, 1])
    return c1, c2, np.minimum(na, nb), np.maximum(na, nb)


def first_bad(ok):
    return int(np.flatnonzero(~ok)[0]) if not ok.all() else -1


def check_value(hk, case, form=OC.FORM_DIRECT, pairs=None):
    pairs = case.pairs if pairs is None else pairs
    c1, c2, n1, n2 = oriented(case, pairs, case.expected(form, pairs))
    counts, state, ratio = hk.run(case, form, -1.0, pairs)
    ok = (counts[:, 0] == c1) & (counts[:, 1] == c2)
    k = first_bad(ok)
    assert k < 0, "%s (form %d): %d of %d pairs miscounted; pair %d %s: got %s, expected (%d, %d) of (%d, %d) points" % (
        case.name, form, int((~ok).sum()), len(pairs), k, pairs[k].tolist(), counts[k].tolist(), c1[k], c2[k], n1[k], n2[k])
    assert (state == 0).all(), (case.name, "value mode skipped a direction")
    want = np.maximum(c1.astype(np.float64) / n1.astype(np.float64), c2.astype(np.float64) / n2.astype(np.float64))
    assert np.array_equal(ratio.view(np.uint64), want.view(np.uint64)), case.name
    return counts


def check_decision(hk, case, th, form=OC.FORM_DIRECT, pairs=None):
    """-> the states (for the tally)"""
    pairs = case.pairs if pairs is None else pairs
    c1, c2, n1, n2 = oriented(case, pairs, case.expected(form, pairs))
    r1, r2 = c1.astype(np.float64) / n1.astype(np.float64), c2.astype(np.float64) / n2.astype(np.float64)
    counts, state, ratio = hk.run(case, form, th, pairs)
    tag = "%s (th %g, %d pairs)" % (case.name, th, len(pairs))
    k = first_bad(counts[:, 0] == c1)
    assert k < 0, "%s: first count of pair %d %s is %d, expected %d of %d" % (tag, k, pairs[k].tolist(), counts[k, 0], c1[k], n1[k])
    first = r1 > th
    assert (state[first] == 1).all(), tag + ": a pair the first ratio decides was not reported so"
    assert (state[~first] != 1).all(), tag + ": a first ratio AT or below the threshold was taken to decide"
    assert np.isin(state, (0, 1, 2)).all()
    bounded = ~first & (state == 2)
    k = first_bad(~bounded | (r2 <= th))
    assert k < 0, "%s: the box bound dropped pair %d %s whose second ratio %d / %d exceeds the threshold" % (tag, k, pairs[k].tolist(), c2[k], n2[k])
    scanned = ~first & ~bounded
    k = first_bad(~scanned | (counts[:, 1] == c2))
    assert k < 0, "%s: second count of pair %d %s is %d, expected %d of %d" % (tag, k, pairs[k].tolist(), counts[k, 1], c2[k], n2[k])
    assert np.array_equal(ratio > th, np.maximum(r1, r2) > th), tag + ": a decision differs from the reference's"
    return state, scanned, n2, first, r1, r2


# ---- the sets, by family (a failure names the set)
FAMILIES = {
    "knife": lambda: [OC.knife(p) for p in OC.PLACES],
    "sizes": lambda: [OC.knife_sizes()],
    "faces": lambda: [OC.faces(p) for p in ("origin", "far", "binade_edges", "negative")],
    "degenerate": lambda: [OC.degenerate(p) for p in ("origin", "far")],
    "piles": lambda: [OC.piles(p) for p in ("origin", "far")],
    "neighbours": lambda: [OC.neighbours(p) for p in ("origin", "far")],
    "base_delta": lambda: [OC.base_delta(p) for p in ("origin", "far", "across_zero")],
    "small_clouds": lambda: [OC.lattice_small(p) for p in ("origin", "far")],
    "many_pairs": lambda: [OC.decision_pool(), OC.many_small()],
}
WORK_LIMIT = 5 * 10 ** 7                 # sum of n_a * n_b over the pairs of one test, both directions


def value_lattice(hk, family, edges=True):
    cases = FAMILIES[family]()
    assert sum(c.work() for c in cases) <= WORK_LIMIT and max(int(c.sizes.max()) for c in cases) <= 4096
    for c in cases:
        check_value(hk, c)
    if family == "many_pairs" and edges:  # launch shapes of the pair list
        pool = cases[0]
        for P in OC.P_EDGES:
            check_value(hk, pool, pairs=pool.pairs[:P])


def value_realistic(hk, place):
    c = OC.realistic(place)
    assert c.work() <= WORK_LIMIT
    check_value(hk, c)


def blas_cases():
    return [OC.realistic("origin"), OC.realistic("far"), OC.knife("far"), OC.lattice_small("far"), OC.faces("far"), OC.base_delta("far")]


def value_blas(hk):
    cases = blas_cases()
    assert sum(c.work() for c in cases) <= WORK_LIMIT
    # the switch must be seen to do something: the forms differ on point decisions of these sets -- on queries of 20 points and
    # more only, a smaller query cloud takes the direct form in both
    differ = sum(OC.forms_differ(c) for c in cases)
    print("point decisions on which the two distance forms differ: %d" % differ)
    assert differ > 0, "the sets do not separate the two forms"
    small = OC.lattice_small("far")
    assert [len(small.clouds[k]) for k in (1, 2, 3)] == [19, 20, 21]
    assert np.array_equal(small.hits(1, 0, OC.FORM_BLAS), small.hits(1, 0, OC.FORM_DIRECT))
    for c in cases:
        check_value(hk, c, OC.FORM_BLAS)


def decision_sets(edges=True):
    pool = OC.decision_pool()
    sets = [(pool, pool.pairs[:P]) for P in (OC.P_EDGES if edges else OC.P_EDGES[-1:])] + [(OC.many_small(), None)]
    sets += [(OC.knife_sizes(), None), (OC.base_delta("far"), None), (OC.piles("origin"), None)]
    return sets


def decision(hk, th, tally=True, edges=True):
    pool = OC.decision_pool()
    n_state = np.zeros(3, np.int64)
    exact = over = under = 0
    for case, pairs in decision_sets(edges):
        state, scanned, n2, first, r1, r2 = check_decision(hk, case, th, pairs=pairs)
        if case is pool and len(pairs) < len(pool.pairs):
            continue                                        # (a prefix of the full list: counted once, below)
        n_state += np.bincount(state, minlength=3)
        exact += int((r1 == th).sum())
        over += int((scanned & (r2 > th)).sum())
        under += int((scanned & (r2 <= th)).sum())
        if case is pool:
            # the fixed 512-workgroup grid of the planned second launch has to loop: more chunks to scan than that
            assert int(np.ceil(n2[scanned] / 256.0).sum()) > 512, th
        if case.name == "many_small":
            assert len(state) > 2048
    print("th %g: pairs by state (scanned, first ratio decides, bound decides) = %s, first ratio exactly th: %d, scanned second ratio above / not above th: %d / %d"
          % (th, n_state.tolist(), exact, over, under))
    # conditions on the INPUTS: the sets were built so that no branch goes untested
    assert exact >= (20 if th < 0.9 else 0), (th, exact)
    # the second direction is scanned and does / does not exceed the threshold (in the direct form a witness is mutual: nothing
    # exceeds a threshold of 0 that the first ratio has not exceeded already)
    assert under >= 20 and (over >= 4 or th == 0.0), (th, over, under)
    if tally:
        assert (n_state >= 20).all(), (th, n_state.tolist())
    return n_state


def pair_order(hk):
    rng = np.random.default_rng(8)
    for case, th in ((OC.knife_sizes(), -1.0), (OC.decision_pool(), -1.0), (OC.decision_pool(), 0.75), (OC.realistic("origin"), -1.0)):
        P = len(case.pairs)
        c0, s0, r0 = hk.run(case, OC.FORM_DIRECT, th)
        o = rng.permutation(P)
        pairs = case.pairs[o].copy()
        flip = rng.random(P) < 0.5
        pairs[flip] = pairs[flip][:, ::-1]
        n = case.sizes
        assert (n[pairs[:, 0]] != n[pairs[:, 1]]).all()      # (of two equal clouds the pair's first is counted first: not these sets)
        c1, s1, r1 = hk.run(case, OC.FORM_DIRECT, th, pairs)
        assert np.array_equal(c1, c0[o]) and np.array_equal(s1, s0[o]) and np.array_equal(r1.view(np.uint64), r0[o].view(np.uint64)), case.name
        if th < 0:
            check_value(hk, case, pairs=pairs)
        else:
            check_decision(hk, case, th, pairs=pairs)


def bad_arguments(hk):
    sizes = np.array([3, 0, 2], np.int64)
    pts = np.arange(15, dtype=np.float64).reshape(5, 3)
    ok = np.array([[0, 2]], np.int32)
    assert hk.raw(OC.VS_LATTICE, 0, sizes, None, pts, ok, -1.0)[0] == 0
    for bad in ([[0, 1]], [[1, 2]], [[0, 3]], [[-1, 0]], [[0, 2], [2, 7]], [[0, 0]]):      # an empty cloud / no such cloud / one cloud twice
        assert hk.raw(OC.VS_LATTICE, 0, sizes, None, pts, np.array(bad, np.int32), -1.0)[0] == HMSG_ERR_INVALID, bad
    for nb in ([0, 0, 2], [4, 0, 2], [3, 0, -1]):                                           # n_base outside [1, size]
        assert hk.raw(OC.VS_LATTICE, 0, sizes, np.array(nb, np.int64), pts, ok, -1.0)[0] == HMSG_ERR_INVALID, nb
    assert hk.raw(OC.VS_LATTICE, 0, np.array([3, -1, 2], np.int64), None, pts, ok, -1.0)[0] == HMSG_ERR_INVALID
    rc, counts, state, ratio = hk.raw(OC.VS_LATTICE, 0, sizes, None, pts, np.zeros((0, 2), np.int32), 0.75)     # no pairs: nothing to do
    assert rc == 0 and len(counts) == 0
    assert hk.L.c.hmsg_test_overlap(None, 0, None, None, None, 0, None, -1.0, None, None, None) == HMSG_ERR_INVALID


def child():
    """what a child process of test_debug_fallbacks_simulator runs: the lattice sets in value mode and the decision sets, on a
    path chosen by an environment variable the library reads once per process.  A path without the bound reports other states:
    the rules of check_decision hold on every path, equality of states does not.  (Whole pair lists only: the prefixes that walk the
    default path's launch shapes are left to the parent.)"""
    from holoagent_amd._lib import HmsgLib
    hk = Hook(HmsgLib(PC.EMU_PATH))
    for family in FAMILIES:
        value_lattice(hk, family, edges=False)
    for th in OC.THRESHOLDS:
        decision(hk, th, tally=False, edges=False)
    hk.close()
    print("overlap child ok")


# ---- fixtures and tests
@pytest.fixture(scope="module")
def emu():
    from holoagent_amd._lib import HmsgLib
    hk = Hook(HmsgLib(PC.EMU_PATH))
    yield hk
    hk.close()


@pytest.fixture(scope="module")
def gpu():
    from holoagent_amd._lib import HmsgLib
    hk = Hook(HmsgLib())
    yield hk
    hk.close()


needs_emu = pytest.mark.skipif(not os.path.exists(PC.EMU_PATH), reason="kernel simulator not built")


@needs_emu
@pytest.mark.parametrize("family", list(FAMILIES))
def test_value_mode_lattice_simulator(emu, family):
    value_lattice(emu, family)


@needs_emu
@pytest.mark.parametrize("place", ["origin", "far"])
def test_value_mode_realistic_simulator(emu, place):
    value_realistic(emu, place)


@needs_emu
def test_value_mode_blas_form_simulator(emu):
    value_blas(emu)


@needs_emu
@pytest.mark.parametrize("th", OC.THRESHOLDS)
def test_decision_mode_simulator(emu, th):
    decision(emu, th)


@needs_emu
def test_pair_order_does_not_matter_simulator(emu):
    pair_order(emu)


@needs_emu
def test_bad_arguments_simulator(emu):
    bad_arguments(emu)


@needs_emu
@pytest.mark.parametrize("var", ["HMSG_OV_ONE_LAUNCH", "HMSG_OV_LEGACY_SECOND", "HMSG_OV_POOL_ORDER"])
def test_debug_fallbacks_simulator(var):
    """the debug paths of Merger::overlap_ratios (one launch for both directions; a workgroup per chunk in the second launch; X's
    points from the pool instead of its sorted copies), each in a fresh process: the switches are read once per process"""
    env = dict(os.environ)
    for v in ("HMSG_OV_ONE_LAUNCH", "HMSG_OV_LEGACY_SECOND", "HMSG_OV_POOL_ORDER"):
        env.pop(v, None)
    env[var] = "1"
    r = subprocess.run([sys.executable, "-c", "from tests import test_overlap_exact as T; T.child()"], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "overlap child ok" in r.stdout, (var, r.stdout[-2000:], r.stderr[-4000:])


@pytest.mark.gpu
@pytest.mark.parametrize("family", list(FAMILIES))
def test_value_mode_lattice_gpu(gpu, family):
    value_lattice(gpu, family)


@pytest.mark.gpu
@pytest.mark.parametrize("place", ["origin", "far"])
def test_value_mode_realistic_gpu(gpu, place):
    value_realistic(gpu, place)


@pytest.mark.gpu
def test_value_mode_blas_form_gpu(gpu):
    value_blas(gpu)


@pytest.mark.gpu
@pytest.mark.parametrize("th", OC.THRESHOLDS)
def test_decision_mode_gpu(gpu, th):
    decision(gpu, th)


@pytest.mark.gpu
def test_pair_order_does_not_matter_gpu(gpu):
    pair_order(gpu)


@pytest.mark.gpu
def test_bad_arguments_gpu(gpu):
    bad_arguments(gpu)
