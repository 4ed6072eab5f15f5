"""hmsg_segment_floors (include/hmsg.h; the kernels k_fl_yrange / k_fl_hist / k_fl_crop of holoagent_amd/csrc/hmsg_floors.hip and the
host half hmsg_floors_host.h) on hostile height profiles -- tests/floors_cases.py:

  exact family    one point per 5 cm voxel, so the re-sampled cloud is the cloud: the C ABI against np.histogram, scipy's filter and
                  peaks, np.percentile and numpy crops, with NO tolerance -- slabs, zero levels, heights, boxes and counts.  The
                  Python mirror (Graph._segment_floors_host) is held to the same answer.
  general family  many points per voxel: the C ABI against the mirror bit for bit, and both against the reference on the ORACLE's
                  re-sampling of the cloud.
  refusals        a map less than a centimetre high, a capacity of 0 / below n_floors, a map that is not finalised.

Equal peak heights follow the library's rule (stable ascending order read from its end); cases without such a tie also equal
plain scipy.signal.find_peaks(distance=20.0) and numpy's default argsort.  Everything runs on the kernel simulator and, marked gpu,
on the device."""
import ctypes as C
import os

import numpy as np
import pytest

from oracle import hmsg_oracle as O
from tests import floors_cases as FC
from tests import parity_common as PC

needs_emu = pytest.mark.skipif(not os.path.exists(PC.EMU_PATH), reason="kernel simulator not built")

EXACT, GENERAL = FC.EXACT_NAMES, FC.GENERAL_NAMES
D = 8


def case(name):
    return {c.name: c for c in FC.exact_cases() + FC.general_cases()}[name]


@pytest.fixture(scope="module")
def emu():
    from holoagent_amd._lib import HmsgLib
    return HmsgLib(PC.EMU_PATH)


@pytest.fixture(scope="module")
def gpu():
    from holoagent_amd._lib import HmsgLib
    return HmsgLib()


def scene_of(L, pts):
    from holoagent_amd._lib import Scene
    sc = Scene(lib_=L, height=8, width=8, max_frames=1, max_masks=1, feat_dim=D)
    sc.restore_stage(pts, [], np.zeros((0, D), np.float32), np.eye(3))
    return sc


def mirror_floors(L, sc, pts):
    """Graph._segment_floors_host on the cloud -> dicts like Scene.segment_floors'"""
    from holoagent_amd.graph import Graph, _Pcd
    g = Graph(dict(main=dict(), models=dict(clip=dict(feat_dim=D))), lib=L)
    g.scene = sc
    g.full_pcd = _Pcd(pts)
    slabs = g._segment_floors_host(None)
    assert len(slabs) == len(g.floors)
    out = []
    for (lo, hi), fl in zip(slabs, g.floors):
        p = np.asarray(fl.pcd.points)
        out.append(dict(y_lo=float(lo), y_hi=float(hi), n_points=len(p), zero_level=fl.floor_zero_level, height=fl.floor_height,
                        bbox_min=p.min(0) if len(p) else np.zeros(3), bbox_max=p.max(0) if len(p) else np.zeros(3)))
    return out


def same_floors(got, want, what):
    """every number equal.  The SIGN of a zero is not pinned: np.min / np.max of an array that holds both zeros return whichever
    comes first, the kernels order -0.0 below +0.0 (fl_key), and nothing downstream reads the sign."""
    assert len(got) == len(want), (what, [(f["y_lo"], f["y_hi"]) for f in got], [(f["y_lo"], f["y_hi"]) for f in want])
    for i, (g, w) in enumerate(zip(got, want)):
        for k in ("y_lo", "y_hi", "n_points", "zero_level", "height"):
            assert g[k] == w[k], (what, i, k, g[k], w[k])
        for k in ("bbox_min", "bbox_max"):
            assert np.array_equal(g[k], w[k]), (what, i, k, g[k], w[k])


def check_exact(L, name):
    c = case(name)
    keys, _ = O.o3d_voxel_keys(c.points, 0.05)
    assert len(np.unique(keys, axis=0)) == len(c.points)         # the re-sampled cloud is the cloud
    want, _ = FC.reference_floors(c.points)
    sc = scene_of(L, c.points)
    try:
        same_floors(sc.segment_floors(), want, name + ": C ABI")
        same_floors(mirror_floors(L, sc, c.points), want, name + ": mirror")
    finally:
        sc.close()


def check_general(L, name):
    c = case(name)
    ref, _ = FC.general_analysis(name)
    sc = scene_of(L, c.points)
    try:
        got = sc.segment_floors()
        same_floors(got, mirror_floors(L, sc, c.points), name + ": C ABI against the mirror")
        same_floors(got, FC.crops(c.points, ref.slabs), name + ": C ABI against the reference on the oracle's re-sampling")
    finally:
        sc.close()


def check_refusals(L):
    from holoagent_amd._lib import HmsgError, Scene
    # less than a centimetre high
    sc = scene_of(L, FC.columns(np.linspace(1.0, 1.0099, 300), 1))
    try:
        with pytest.raises(HmsgError, match="centimetre"):
            sc.segment_floors()
    finally:
        sc.close()
    # capacity 0 is answered with n_floors; a capacity below it is refused and `out` stays as it was
    c = case("tall_20000")
    want, _ = FC.reference_floors(c.points)
    assert len(want) >= 3
    sc = scene_of(L, c.points)
    try:
        n = C.c_int32(-7)
        assert L.c.hmsg_segment_floors(sc.h, None, 0, C.byref(n)) == 0 and n.value == len(want)
        for cap in (1, len(want) - 1):
            rec = np.full((len(want), 11), 12345.5)
            n = C.c_int32(-7)
            assert L.c.hmsg_segment_floors(sc.h, rec.ctypes.data_as(C.c_void_p), cap, C.byref(n)) == -1      # HMSG_ERR_INVALID
            assert (rec == 12345.5).all() and n.value == len(want)
            assert b"capacity" in L.c.hmsg_last_error(sc.h)
        assert L.c.hmsg_segment_floors(sc.h, None, 2, C.byref(n)) == -1                                      # nowhere to write to
        same_floors(sc.segment_floors(), want, "after the refusals")
    finally:
        sc.close()
    # no map yet
    sc = Scene(lib_=L, height=8, width=8, max_frames=1, max_masks=1, feat_dim=D)
    try:
        with pytest.raises(HmsgError, match="finalize"):
            sc.segment_floors()
    finally:
        sc.close()


# ------------------------------------------------------------------------------------------------ the cases themselves (CPU)
def test_cases_hold_what_they_are_meant_to():
    """conditions on the inputs, computed with numpy, scipy and the oracle alone; nothing is skipped"""
    exact = {c.name: FC.reference_floors(c.points) for c in FC.exact_cases()}
    for c in FC.exact_cases() + FC.general_cases():
        assert 2 <= len(c.points) <= FC.MAX_POINTS
    assert {len(c.points) for c in FC.exact_cases()} >= set(FC.SIZES) and any(19000 <= len(c.points) <= 21000 for c in FC.exact_cases())
    for c in FC.exact_cases():
        assert FC.one_per_voxel(c.points), c.name
    assert all(not FC.one_per_voxel(c.points) for c in FC.general_cases())
    y = case("across_zero").points[:, 1]
    assert (y < 0).any() and (y > 0).any() and (np.signbit(y) & (y == 0)).any() and (~np.signbit(y) & (y == 0)).any()
    assert (case("all_negative").points[:, 1] < 0).all()
    # heights on bin edges as np.linspace computes them, and the doubles either side
    for name in ("tall_20000", "across_zero"):
        y = case(name).points[:, 1]
        e = exact[name][1].edges
        assert len(e) > 400
        for q in (e[1:-1], np.nextafter(e[1:-1], -np.inf), np.nextafter(e[1:-1], np.inf)):
            assert np.isin(q, y).all(), name
        assert (y == y.max()).sum() >= 2
    # a point exactly on an edge that two storeys share: both count it
    floors, _ = exact["tall_20000"]
    y = case("tall_20000").points[:, 1]
    shared = [f["y_hi"] for f in floors[:-1] if (y == f["y_hi"]).any()]
    assert len(shared) >= 1 and all(a["y_hi"] == b["y_lo"] for a, b in zip(floors[:-1], floors[1:]))
    assert sum(f["n_points"] for f in floors) - int(((y >= floors[0]["y_lo"]) & (y <= floors[-1]["y_hi"])).sum()) == \
        sum(int((y == f["y_hi"]).sum()) for f in floors[:-1])
    # an empty slab between two others: zero level = its lower edge, boxes of zeros
    floors, _ = exact["empty_slab"]
    assert [f["n_points"] == 0 for f in floors] == [False, True, False, False]
    assert floors[1]["zero_level"] == floors[1]["y_lo"] and not floors[1]["bbox_min"].any() and not floors[1]["bbox_max"].any()
    # the points at ymax decide the answer of this one
    c = case("ceiling_at_ymax")
    counts, lo, hi = FC.histogram(c.points[:, 1])
    assert counts[-1] == 400 == (c.points[:, 1] == hi).sum()
    less = counts.copy()
    less[-1] = 0
    assert len(FC.reference(less, lo, hi).slabs) != len(FC.reference(counts, lo, hi).slabs)
    # a peak exactly at the percentile height, which decides the lower pick
    r = exact["peak_at_percentile"][1]
    x = np.sort(r.smooth)
    assert len(x) == 311 and r.height == x[279] < x[280] and r.smooth[30] == r.height
    assert r.peaks.tolist() == [30, 140, 200, 260] and [len(ch) for ch in r.chains] == [1, 3] and r.picks.tolist() == r.edges[[30, 200]].tolist()
    # whole levels on bin edges: np.histogram puts the one ON edge 209 into bin 209 and the one a double under edge 330 into bin 329,
    # both are peaks and both are slab edges; one bin off, and a slab edge moves by a centimetre
    c, (floors, r) = case("levels_on_edges"), exact["levels_on_edges"]
    counts, lo, hi = FC.histogram(c.points[:, 1])
    assert (lo, hi) == FC.EDGE_LEVELS_RANGE and (c.points[:, 1] == r.edges[209]).sum() == 300 == (c.points[:, 1] == np.nextafter(r.edges[330], -np.inf)).sum()
    assert counts[[208, 209, 210, 328, 329, 330]].tolist() == [0, 300, 0, 0, 300, 0] and r.peaks.tolist() == [60, 209, 329, 445]
    assert [f["y_hi"] for f in floors[:-1]] == [r.edges[209], r.edges[329]] and [f["n_points"] for f in floors] == [600, 300, 602]
    for a, b in ((209, 208), (329, 330)):
        moved = counts.copy()
        moved[a], moved[b] = 0, 300
        assert not np.array_equal(FC.reference(moved, lo, hi).slabs, r.slabs)
    # fallback slab, one bin
    assert len(exact["size_2"][1].peaks) == 0 and len(exact["one_bin"][1].smooth) == 1
    # ties: which cases have them, and that the library's rule is all the reference adds to scipy and numpy
    refs = {name: r for name, (_, r) in exact.items()}
    plain = {c.name: FC.reference(*FC.histogram(c.points[:, 1]), ties="numpy") for c in FC.exact_cases()}
    for name in GENERAL:
        refs[name], plain[name] = FC.general_analysis(name)
    assert sum(refs[n].pick_tie for n in GENERAL) >= 3 and all(refs["repro_%d" % s].pick_tie for s in FC.REPRO_SEEDS)
    assert refs["five_equals"].pick_tie and refs["twin_levels"].dist_tie_decides
    assert sum(r.dist_tie_decides for r in refs.values()) >= 1
    neither = [n for n, r in refs.items() if not r.pick_tie and not r.dist_tie]
    assert len(neither) >= 10
    for n in neither:
        assert np.array_equal(refs[n].peaks, plain[n].peaks) and np.array_equal(refs[n].slabs, plain[n].slabs), n
    # the general family: two to seven storeys, one long chain, chains of single peaks
    assert len(refs["twenty_levels"].chains) == 1 and len(refs["twenty_levels"].peaks) == 20
    assert all(len(ch) == 1 for ch in refs["levels_1p5_apart"].chains) and len(refs["levels_1p5_apart"].chains) == 6


# ------------------------------------------------------------------------------------------------ simulator
@needs_emu
@pytest.mark.parametrize("name", EXACT)
def test_exact_emu(emu, name):
    check_exact(emu, name)


@needs_emu
@pytest.mark.parametrize("name", GENERAL)
def test_general_emu(emu, name):
    check_general(emu, name)


@needs_emu
def test_refusals_emu(emu):
    check_refusals(emu)


# ------------------------------------------------------------------------------------------------ device
@pytest.mark.gpu
@pytest.mark.parametrize("name", EXACT)
def test_exact_gpu(gpu, name):
    check_exact(gpu, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", GENERAL)
def test_general_gpu(gpu, name):
    check_general(gpu, name)


@pytest.mark.gpu
def test_refusals_gpu(gpu):
    check_refusals(gpu)
