"""The cases of N10 (include/hmsg.h: hmsg_nav_height_map, hmsg_nav_viewpoints_h, hmsg_nav_view_route_h), shared by the simulator
tests (tests/test_navsight.py) and the GPU tests (tests/test_navsight_gpu.py), laid out as tests/navview_cases.py is.  A case takes
`api` (the wrappers of holoagent_amd._lib on one library or the other, arrays handed over as numpy or as device tensors, results as
numpy) and compares every output with tests/navsight_reference.py by array_equal: nothing here has a tolerance.  The first three
functions test the restatement alone (the three properties the rule was checked for, with their exact counts); the cases that take
the library itself (refusals, capacity, the slab forms, NavigationGraph, Graph) are at the end."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import navroute_cases as NC
from tests import navroute_reference as RR
from tests import navsight_reference as SR
from tests import navview_cases as VC
from tests import navview_reference as VR

U = SR.UNREACHED
UNSUPPORTED = -3
frozen = VC.frozen


def check_views_h(api, top, pas, goals, band, eye, gh, gr2=None, field=None, prefer=0, want_visible=True, what="", ref=None):
    got = api.viewpoints_h(top, pas, goals, eye, gh, gr2, field=field, want_visible=want_visible, r_min2=band[0], r_max2=band[1], prefer=prefer)
    ref = ref if ref is not None else SR.viewpoints_h(top, pas, goals, band[0], band[1], eye, gh, gr2, field, prefer, want_visible)
    VC.compare_views(got, ref, what)
    return got


# ------------------------------------------------------------------------------------------ 1. the restatement alone
def binary_top(blk):
    return np.where(np.asarray(blk) != 0, 65535, 0).astype(np.uint16)


HEIGHT_PAIRS = ((1, 65535), (65535, 1), (150, 90), (700, 700))


def property_contains_v2():
    """with top = 65535 where blocking else 0, no footprint, eye and goal_h anywhere in [1, 65535]: S3 == V3 bit for bit"""
    rng = np.random.default_rng(20)
    for _ in range(6):
        blk = (rng.random((23, 29)) < 0.2).astype(np.uint8)
        pas = ((blk == 0) & (rng.random((23, 29)) < 0.9)).astype(np.uint8)
        goals = [(11, 14), (0, 0), (22, 28), tuple(np.argwhere(blk != 0)[3])]
        for g in goals:
            v = VR.visible_set_np(blk, pas, g, 1, 400)
            for eye, gh in HEIGHT_PAIRS:
                assert np.array_equal(SR.visible_set_h_np(binary_top(blk), pas, g, 1, 400, eye, gh), v), (g, eye, gh)
            assert np.array_equal(SR.visible_set_h(binary_top(blk), pas, g, 1, 400, 1, 65535), v), g


@functools.lru_cache(maxsize=None)
def motivating_map():
    """21 x 41: a wall (250) in column 20 with a door at rows 8 to 12, a table (75) over rows 8 to 12, columns 28 to 30"""
    top = np.zeros((21, 41), np.uint16)
    top[:, 20] = 250
    top[8:13, 20] = 0
    top[8:13, 28:31] = 75
    return frozen(top), frozen((top == 0).astype(np.uint8)), (10, 34), (4, 900)


MOTIVATING = ((150, 90, 119, 520), (150, 40, 0, 379), (60, 40, 0, 304))    # eye, goal_h, seen from west of the wall, seen in all


def property_motivating_case(visible_h=None, visible_v=None):
    """visible_h / visible_v: how a visible set is made (default: the restatement; the library's case hands its own in)"""
    top, pas, g, band = motivating_map()
    visible_h = visible_h or (lambda eye, gh: SR.visible_set_h_np(top, pas, g, band[0], band[1], eye, gh))
    v2 = (visible_v or (lambda: VR.visible_set_np((top > 0).astype(np.uint8), pas, g, *band)))()
    assert (int(v2[:, :20].sum()), int(v2.sum())) == (0, 304)
    sets = {}
    for eye, gh, west, total in MOTIVATING:
        sets[eye, gh] = s = visible_h(eye, gh)
        assert (int(s[:, :20].sum()), int(s.sum())) == (west, total), (eye, gh)
    assert np.array_equal(sets[60, 40], v2)                                # the eye below the table top: the flat rule's answer
    assert (sets[150, 90] >= v2).all() and (sets[150, 90] >= sets[150, 40]).all()


@functools.lru_cache(maxsize=None)
def sofa_map():
    top = np.zeros((21, 41), np.uint16)
    top[9:12, 30:39] = 80
    return frozen(top), frozen((top == 0).astype(np.uint8)), (10, 34), (4, 400)


def property_footprint(visible_h=None):
    top, pas, g, band = sofa_map()
    visible_h = visible_h or (lambda r2: SR.visible_set_h_np(top, pas, g, band[0], band[1], 150, 40, r2))
    assert int(visible_h(-1).sum()) == 4 and int(visible_h(25).sum()) == 508


@functools.lru_cache(maxsize=None)
def random_heights(H=31, W=37, seed=21, lo=30, hi=200):
    """heights drawn close to the range of a ray between lo and hi, a fifth of the cells; the rest 0"""
    rng = np.random.default_rng(seed)
    top = np.where(rng.random((H, W)) < 0.2, rng.integers(lo - 20, hi + 20, (H, W)), 0).astype(np.uint16)
    pas = ((top < lo) & (rng.random((H, W)) < 0.9)).astype(np.uint8)
    return frozen(top), frozen(pas)


def loops_against_numpy():
    top, pas = random_heights()
    f, _ = RR.field(pas, [NC.first_free(pas, (15, 18))])
    goals = [(0, 0), (15, 18), (30, 36), (0, 20), (-1, 3), (31, 3)] + [tuple(c) for c in np.argwhere(top > 150)[:3]]
    for fld, prefer, (eye, gh), r2 in ((None, 0, (150, 60), -1), (f, 1, (60, 150), 9), (f, 0, (100, 100), 0), (None, 1, (0, 120), -1)):
        for g in goals:
            a = SR.viewpoint_h(top, pas, g, 2, 150, eye, gh, r2, fld, prefer)
            b = SR.viewpoint_h_np(top, pas, g, 2, 150, eye, gh, r2, fld, prefer)
            assert a[:4] == b[:4] and np.array_equal(a[4], b[4]), (g, prefer, eye, gh, a[:4], b[:4])
    pts, zero = height_cloud()[:2]
    for d in (0, 3, 5):
        a, b = SR.height_map(pts, zero, **dict(HP, dilation=d)), SR.height_map_np(pts, zero, **dict(HP, dilation=d))
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[0].dtype == np.uint16, d


# ------------------------------------------------------------------------------------------ 2. the height map
HP = dict(cell_size=0.05, height_unit=0.01, top_max=2.5)


@functools.lru_cache(maxsize=None)
def height_cloud():
    """about 3300 points on a 60 x 40 grid: random ones, points exactly on cell edges and on multiples of the height unit, y at
    zero + top_max (left out) and one ulp below (taken), points below the floor, duplicates, tall cells in the corners and on the
    border, and a column of cells with no point"""
    rng = np.random.default_rng(22)
    zero, cell, W, H = 0.37, 0.05, 60, 40
    x0, z0 = -1.3, 2.1
    rand = np.c_[x0 + rng.uniform(0, (W - 1) * cell, 2500), zero + rng.uniform(-0.3, 3.0, 2500), z0 + rng.uniform(0, (H - 1) * cell, 2500)]
    k = rng.integers(0, W - 1, 300)
    edges = np.c_[x0 + k * cell, zero + rng.integers(0, 240, 300) * 0.01, z0 + rng.integers(0, H - 1, 300) * cell]
    limit = float(np.float64(zero) + np.float64(2.5))
    special = np.array([[x0 + 0.52, limit, z0 + 0.52], [x0 + 0.77, np.nextafter(limit, -np.inf), z0 + 0.77],
                        [x0 + 1.02, zero - 5.0, z0 + 1.02], [x0 + 1.02, zero - 0.004, z0 + 1.27],
                        [x0, zero + 2.2, z0], [x0 + (W - 1) * cell, zero + 2.3, z0], [x0, zero + 2.4, z0 + (H - 1) * cell],
                        [x0 + (W - 1) * cell, zero + 2.45, z0 + (H - 1) * cell], [x0 + 1.5, zero + 2.1, z0], [x0, zero + 1.9, z0 + 1.0]])
    pts = np.concatenate([rand, edges, special, rand[:200], edges[:50]])
    mn = pts.min(axis=0)
    col = np.floor((pts[:, 0] - mn[0]) / cell)
    pts = pts[col != 17]                                                  # an empty column
    pts = pts[rng.permutation(len(pts))]
    grid = SR.grid_of(pts, cell)[2]                                       # (59 cells of extent: 60 or 61 by the division's rounding)
    assert grid[0] in (W, W + 1) and grid[1] in (H, H + 1) and 2000 <= len(pts) <= 5000
    return frozen(pts), zero, grid


def compare_height(got, ref, grid, what=""):
    assert got["top"].dtype == np.uint16 and got["known"].dtype == np.uint8 and tuple(got["grid"]) == tuple(grid), what
    assert got["top"].shape == ref[0].shape and np.array_equal(got["top"], ref[0]), (what, "top", int((got["top"] != ref[0]).sum()))
    assert np.array_equal(got["known"], ref[1]), (what, "known")


def height_map_cases(api):
    pts, zero, (W, H) = height_cloud()
    mn, mx, grid = api.grid(pts, 0.05)
    for d in (0, 1, 3, 5):
        got = api.height_map(pts, zero, **dict(HP, dilation=d))
        compare_height(got, SR.height_map_np(pts, zero, **dict(HP, dilation=d)), (W, H), "dilation %d" % d)
        assert np.array_equal(got["pcd_min"], mn) and np.array_equal(got["pcd_max"], mx) and tuple(got["grid"]) == tuple(grid)
    raw, top5 = api.height_map(pts, zero, **dict(HP, dilation=1)), got
    assert np.array_equal(raw["top"], api.height_map(pts, zero, **dict(HP, dilation=0))["top"])
    known = raw["known"]
    assert not known[:, 17].any() and not raw["top"][:, 17].any() and top5["top"][:, 17].any()       # the empty column: filled by the dilation only
    cell = lambda x, z: (int(np.floor((z - mn[2]) / 0.05)), int(np.floor((x - mn[0]) / 0.05)))
    x0, z0 = -1.3, 2.1
    far_r, far_c = cell(x0 + 59 * 0.05, z0 + 39 * 0.05)                     # the cell of the cloud's far corner
    assert raw["top"][0, 0] >= 219 and raw["top"][0, far_c] >= 229 and raw["top"][far_r, 0] >= 239 and raw["top"][far_r, far_c] >= 244
    assert top5["top"][2, 2] >= 219 and top5["top"][far_r - 2, far_c - 2] >= 244      # a corner's box is clipped, not wrapped
    assert raw["top"].max() <= 249                                        # nothing at or above top_max: 2.5 / 0.01
    below = cell(x0 + 1.02, z0 + 1.02)
    assert known[below] == 1                                              # a point five metres under the floor takes part, at height 0
    # a point 700 m up: left out by the default top_max, clamped to 65535 with top_max raised
    high = np.concatenate([pts, [[x0 + 2.0, zero + 700.0, z0 + 1.0]]])
    far = api.height_map(high, zero, cell_size=0.05, height_unit=0.01, top_max=1000.0, dilation=0)
    compare_height(far, SR.height_map_np(high, zero, 0.05, 0.01, 1000.0, 0), (W, H), "700 m up")
    assert far["top"].max() == 65535 and far["top"][cell(x0 + 2.0, z0 + 1.0)] == 65535
    compare_height(api.height_map(high, zero, **dict(HP, dilation=3)), SR.height_map_np(high, zero, **dict(HP, dilation=3)), (W, H), "ceiling left out")
    # another unit and cell size; the loops say the same
    got = api.height_map(pts, zero, cell_size=0.07, height_unit=0.125, top_max=1.0, dilation=3)
    ref = SR.height_map(pts, zero, 0.07, 0.125, 1.0, 3)
    compare_height(got, ref, SR.grid_of(pts, 0.07)[2], "unit 0.125")
    # the map lies on hmsg_nav_floor_maps' maps of the same cloud
    from tests import navmap_cases as MC
    rp, rc_, rz, rposes = MC.room(41, 3.0, 2.4, n_floor=2500, n_wall=2000, n_box=500)
    maps = api.floor_maps(rp, rz, rposes)
    hm = api.height_map(rp, rz)
    assert hm["top"].shape == maps["main_free_map"].shape and np.array_equal(hm["pcd_min"], maps["pcd_min"]) and tuple(hm["grid"]) == tuple(maps["grid"])
    compare_height(hm, SR.height_map_np(rp, rz), maps["grid"], "room")


def height_map_refusals(api, L):
    from holoagent_amd._lib import HmsgError, HmsgHeightParams, _ptr
    pts, zero, (W, H) = height_cloud()
    for kw in (dict(dilation=2), dict(dilation=4), dict(dilation=-1), dict(dilation=65), dict(height_unit=0.0), dict(height_unit=-1.0),
               dict(top_max=0.0), dict(cell_size=0.0), dict(cell_size=-0.05), dict(height_unit=float("nan"))):
        with pytest.raises(HmsgError):
            api.height_map(pts, zero, **kw)
    for bad in (np.nan, np.inf):
        p = np.array(pts)
        p[77, 2] = bad
        with pytest.raises(HmsgError):
            api.height_map(p, zero, **HP)
    with pytest.raises(HmsgError):
        api.height_map(np.zeros((0, 3)), zero, **HP)
    c = L.c
    p = np.ascontiguousarray(pts)
    prm = HmsgHeightParams(0.05, 0.01, 2.5, 5, 0)
    top, known, grid = np.zeros((H, W), np.uint16), np.zeros((H, W), np.uint8), np.zeros(2, np.int32)
    ok = (0, C.byref(prm), len(p), _ptr(p), zero, _ptr(top), _ptr(known), None, None, _ptr(grid))
    assert c.hmsg_nav_height_map(*ok) == 0 and tuple(grid) == (W, H)
    for k in (1, 3, 5):                                                   # prm, xyz, top
        assert c.hmsg_nav_height_map(*[None if i == k else a for i, a in enumerate(ok)]) == -1, k
    assert c.hmsg_nav_height_map(*[None if i in (6, 9) else a for i, a in enumerate(ok)]) == 0           # known and grid are optional
    even = HmsgHeightParams(0.05, 0.01, 2.5, 4, 0)
    assert c.hmsg_nav_height_map(0, C.byref(even), *ok[2:]) == UNSUPPORTED
    d = HmsgHeightParams(7, 7, 7, 7, 7)
    c.hmsg_height_default_params(C.byref(d))
    assert (d.cell_size, d.height_unit, d.top_max, d.dilation, d.reserved_) == (0.03, 0.01, 2.5, 5, 0)


def slab_forms(L, tmp_path):
    """hmsg_graph_nav_height_map and hmsg_map_nav_height_map on a small built scene == the cloud form on the slab's points == the
    restatement; they refuse what their _floor_maps siblings refuse"""
    from holoagent_amd._lib import HmsgError, SceneGraph, nav_height_map
    from tests import navmap_cases as MC
    sc, g, poses = MC.built_graph(L)
    xyz, _ = sc.map_points(colors=True)
    fl = sc.segment_floors()[0]
    slab = xyz[(xyz[:, 1] >= fl["y_lo"]) & (xyz[:, 1] <= fl["y_hi"])]
    for kw in (dict(cell_size=0.05), dict(cell_size=0.05, dilation=3, height_unit=0.02, top_max=1.8)):
        ref = SR.height_map_np(slab, fl["zero_level"], **{**dict(height_unit=0.01, top_max=2.5, dilation=5), **kw})
        want = nav_height_map(slab, fl["zero_level"], lib_=L, **kw)
        for got in (g.nav_height_map(0, **kw), sc.nav_height_map(fl["y_lo"], fl["y_hi"], fl["zero_level"], **kw)):
            compare_height(got, ref, want["grid"], "slab")
            assert np.array_equal(got["top"], want["top"]) and np.array_equal(got["pcd_min"], want["pcd_min"]) and ref[0].any()
    with pytest.raises(HmsgError, match="no such floor"):
        g.nav_height_map(7)
    with pytest.raises(HmsgError):
        sc.nav_height_map(fl["y_hi"], fl["y_lo"] - 1.0, 0.0)              # y_lo > y_hi
    g.save(tmp_path / "graph")
    lg = SceneGraph.load(tmp_path / "graph", lib_=L)
    with pytest.raises(HmsgError, match="hmsg_load"):
        lg.nav_height_map(0)
    lg.close()
    g.close()
    sc.close()


# ------------------------------------------------------------------------------------------ 3. the sight call
def contains_v2(api):
    """property 1 on the library: hmsg_nav_viewpoints_h on a 0 / 65535 map == hmsg_nav_viewpoints itself"""
    rng = np.random.default_rng(23)
    blk = (rng.random((23, 29)) < 0.2).astype(np.uint8)
    pas = ((blk == 0) & (rng.random((23, 29)) < 0.9)).astype(np.uint8)
    f, _ = RR.field(pas, [NC.first_free(pas, (11, 14))])
    goals = [(11, 14), (0, 0), (22, 28), (5, 20), (-1, 4), (23, 0)] + [tuple(c) for c in np.argwhere(blk != 0)[:3]]
    for fld in (None, f):
        for prefer in (0, 1):
            old = api.viewpoints(blk, pas, goals, field=fld, want_visible=True, r_min2=1, r_max2=400, prefer=prefer)
            assert (old["n_visible"] > 0).any()
            for eye, gh in HEIGHT_PAIRS:
                got = api.viewpoints_h(binary_top(blk), pas, goals, eye, gh, field=fld, want_visible=True, r_min2=1, r_max2=400, prefer=prefer)
                VC.compare_views(got, old, "contains V2 %d %d" % (eye, gh))


def motivating_and_footprint(api):
    top, pas, g, band = motivating_map()
    one = lambda t, p, b, eye, gh, r2=None: check_views_h(api, t, p, [g], b, eye, gh, r2, what="motivating")["visible"][0]
    property_motivating_case(lambda eye, gh: one(top, pas, band, eye, gh),
                             lambda: api.viewpoints((top > 0).astype(np.uint8), pas, [g], want_visible=True, r_min2=band[0], r_max2=band[1])["visible"][0])
    stop, spas, g, sband = sofa_map()
    property_footprint(lambda r2: one(stop, spas, sband, 150, 40, None if r2 < 0 else r2))
    # one call, one eye, several goals with their own heights and footprints
    got = check_views_h(api, stop, spas, [g, g, g, (3, 3)], sband, 150, [40, 40, 100, 40], [-1, 25, -1, 0], what="per goal")
    assert list(got["n_visible"][:2]) == [4, 508] and got["n_visible"][2] > 4


def heights_and_edges(api):
    """goals outside the image, on the border and inside tall cells; every order of eye and goal_h; 0 and 65535"""
    top, pas = random_heights(40, 50, 24)
    H, W = top.shape
    tall = [tuple(c) for c in np.argwhere(top > 180)[:4]]
    inside = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (0, 25), (H - 1, 25), (20, 0), (20, W - 1)] + tall
    outside = [(-1, 5), (5, -1), (H, 0), (0, W), (10 ** 6, 3), (-2 ** 31, 2 ** 31 - 1)]
    for prefer, (eye, gh) in ((0, (150, 60)), (1, (60, 150)), (0, (110, 110)), (1, (0, 120)), (0, (120, 0)), (0, (0, 0))):
        got = check_views_h(api, top, pas, inside + outside, (1, 30 * 30), eye, gh, prefer=prefer, what="edges %d %d" % (eye, gh))
        assert (got["n_visible"][:8] > 0).all() or eye == gh == 0
        assert (got["n_visible"][len(inside):] == 0).all() and (got["view_rc"][len(inside):] == -1).all() and not got["visible"][len(inside):].any()
        assert (got["view_d2"][len(inside):] == -1).all() and (got["view_dist"][len(inside):] == U).all()
    # goal_h is read clamped: below 0 is 0, above 65535 is 65535
    a = api.viewpoints_h(top, pas, inside, 100, [-5] * len(inside), want_visible=True, r_min2=1, r_max2=900)
    b = api.viewpoints_h(top, pas, inside, 100, [0] * len(inside), want_visible=True, r_min2=1, r_max2=900)
    VC.compare_views(a, b, "goal_h < 0")
    # a map of 65535 everywhere but a corridor, goals at 0 and at 65535, the eye at 65535: only the corridor is looked along
    full = np.full((15, 30), 65535, np.uint16)
    full[7, :] = 0
    cpas = (full == 0).astype(np.uint8)
    for eye, gh in ((65535, 0), (65535, 65535), (0, 65535)):
        got = check_views_h(api, full, cpas, [(7, 15), (3, 15)], (1, 400), eye, gh, what="65535")
        assert got["n_visible"][0] == 29 and got["n_visible"][1] == 0       # along the corridor; nothing looks into the block
    got = api.viewpoints_h(top, pas, np.zeros((0, 2), np.int32), 100, np.zeros(0, np.int32))
    assert all(len(got[k]) == 0 for k in VC.KEYS)


@functools.lru_cache(maxsize=None)
def clutter_h():
    """33 x 47, a fifth of the cells with heights drawn close to the ray's range [60, 150], so that most cells a line meets take
    the path between the two bitmaps; 40 goals with their own heights and footprints"""
    top, pas = random_heights(33, 47, 25, 60, 150)
    rng = np.random.default_rng(26)
    f, _ = RR.field(pas, [NC.first_free(pas, (16, 23))])
    goals = np.concatenate([rng.integers(0, (33, 47), (34, 2)), np.argwhere(top > 100)[:4], [[16, 23], [16, 23]]]).astype(np.int32)
    gh = rng.integers(40, 170, len(goals)).astype(np.int32)
    gr2 = rng.choice([-1, 0, 2, 9], len(goals)).astype(np.int64)
    refs = {prefer: SR.viewpoints_h(top, pas, goals, 4, 400, 150, gh, gr2, f, prefer, want_visible=(prefer == 0)) for prefer in (0, 1)}
    between = ((top >= 60) & (top < 150)).sum()
    assert between > 150 and (refs[0]["n_visible"] > 0).sum() >= 30
    return top, pas, frozen(f), frozen(goals), frozen(gh), frozen(gr2), refs


def clutter_heights(api):
    top, pas, f, goals, gh, gr2, refs = clutter_h()
    for prefer in (0, 1):
        check_views_h(api, top, pas, goals, (4, 400), 150, gh, gr2, field=f, prefer=prefer, want_visible=(prefer == 0), what="clutter", ref=refs[prefer])
    # the eye below the goals: the other end of the line carries the greater height
    check_views_h(api, top, pas, goals[:12], (4, 400), 50, gh[:12], gr2[:12], field=f, what="clutter, low eye")


def both_layouts(api, L):
    """the LDS row stride of the kernel's bitmaps, 17 and the 16 of a device with 64 KB a workgroup: the same answers"""
    top, pas, f, goals, gh, gr2, refs = clutter_h()
    used, limit = C.c_int32(0), C.c_int32(0)
    try:
        for ld in (16, 17):
            assert L.c.hmsg_test_nav_sight_layout(0, ld, C.byref(used), C.byref(limit)) == 0
            assert used.value == ld or (ld == 17 and limit.value < 70000 and used.value == 16)
            check_views_h(api, top, pas, goals, (4, 400), 150, gh, gr2, field=f, what="stride %d" % ld, ref=refs[0])
            mt, mp, g, band = motivating_map()
            assert check_views_h(api, mt, mp, [g], band, 150, 90, what="stride %d" % ld)["n_visible"][0] == 520
        assert L.c.hmsg_test_nav_sight_layout(0, 5, None, None) == -1
    finally:
        assert L.c.hmsg_test_nav_sight_layout(0, 0, C.byref(used), C.byref(limit)) == 0
    assert used.value == (17 if limit.value >= 70000 else 16) or 65536 < limit.value < 70000


# ------------------------------------------------------------------------------------------ 4. the largest window (GPU only)
@functools.lru_cache(maxsize=None)
def large_h():
    """300 x 520 as tests/navview_cases.py's large(): pillars and two walls with a door each, now with random heights round the
    ray's range, the band from 150 to 255 cells"""
    rng = np.random.default_rng(27)
    top = np.where(rng.random((300, 520)) < 0.004, rng.integers(80, 200, (300, 520)), 0).astype(np.uint16)
    top[:260, 180] = top[40:, 400] = 250
    top[120:124, 180] = top[200:204, 400] = 0
    p = (top == 0).astype(np.uint8)
    f, _ = RR.field(p, [NC.first_free(p, (150, 260))])
    goals = np.array([[150, 260], [0, 0], [299, 519], [150, 0], [297, 300]], np.int32)
    gh = np.array([100, 60, 180, 140, 90], np.int32)
    refs = {prefer: SR.viewpoints_h(top, p, goals, *VC.LARGE_BAND, 150, gh, None, f, prefer, want_visible=(prefer == 0)) for prefer in (0, 1)}
    return frozen(top), frozen(p), frozen(f), frozen(goals), frozen(gh), refs


def large_window(api):
    top, p, f, goals, gh, refs = large_h()
    assert (refs[0]["n_visible"] > 1000).all()
    for prefer in (0, 1):
        check_views_h(api, top, p, goals, VC.LARGE_BAND, 150, gh, field=f, prefer=prefer, want_visible=(prefer == 0), what="large", ref=refs[prefer])


# ------------------------------------------------------------------------------------------ 5. the composition
def view_route_h_against_the_calls(api):
    m = NC.rooms_map()
    rng = np.random.default_rng(28)
    top = np.where(m == 0, 250, np.where(rng.random(m.shape) < 0.04, rng.integers(40, 160, m.shape), 0)).astype(np.uint16)
    goals = np.concatenate([rng.integers(-10, 200, (24, 2)), np.argwhere(m == 0)[::400][:8]])
    gh = rng.integers(20, 200, len(goals)).astype(np.int32)
    gr2 = rng.choice([-1, 4], len(goals)).astype(np.int64)
    for start, minc, band, prefer, eye in (((3, 3), 0, (0, 400), 0, 150), ((64, 95), 10, (4, 900), 1, 90)):
        got = api.view_route_h(m, top, start, goals, eye, gh, gr2, min_clearance=minc, r_min2=band[0], r_max2=band[1], prefer=prefer, want_field=True)
        VC.compare_view_route(got, SR.view_route_h(m, top, start, goals, eye, gh, gr2, band[0], band[1], prefer, min_clearance=minc))
        old = api.route(m, start, goals, min_clearance=minc, want_field=True)
        assert got["start_cell"] == old["start_cell"] and np.array_equal(got["passable"], old["passable"]) and np.array_equal(got["field"], old["field"])
        v = api.viewpoints_h(top, old["passable"], goals, eye, gh, gr2, field=old["field"], r_min2=band[0], r_max2=band[1], prefer=prefer)
        off, rc = api.paths(old["passable"], old["field"], v["view_rc"])
        assert np.array_equal(got["goal_cell"], v["view_rc"]) and np.array_equal(got["goal_d2"], v["view_d2"])
        assert np.array_equal(got["goal_dist"], v["view_dist"]) and np.array_equal(got["n_visible"], v["n_visible"])
        assert np.array_equal(got["path_off"], off) and np.array_equal(got["path_rc"], rc)
        assert (got["n_visible"] > 0).any() and (got["n_visible"] == 0).any()
        flat = api.view_route(m, (top > 0).astype(np.uint8), start, goals, min_clearance=minc, r_min2=band[0], r_max2=band[1], prefer=prefer)
        assert (got["n_visible"] >= flat["n_visible"]).all() and (got["n_visible"] > flat["n_visible"]).any()      # over the furniture
    none = api.view_route_h(np.zeros((6, 7), np.uint8), np.zeros((6, 7), np.uint16), (2, 2), [(1, 1), (3, 3)], 100, [50, 50])
    assert none["start_cell"] == (-1, -1) and (none["goal_cell"] == -1).all() and (none["n_visible"] == 0).all() and np.array_equal(none["path_off"], [0, 0, 0])
    empty = api.view_route_h(m, top, (3, 3), np.zeros((0, 2), np.int32), 100, np.zeros(0, np.int32))
    assert len(empty["goal_cell"]) == 0 and np.array_equal(empty["path_off"], [0]) and len(empty["n_visible"]) == 0


def view_route_h_capacity_too_small(L):
    """a list that is too short behaves as hmsg_nav_view_route's"""
    from holoagent_amd._lib import HmsgNavRoutes, HmsgRouteParams, HmsgViewParams, _ptr
    m = np.ascontiguousarray(NC.rooms_map())
    top = np.ascontiguousarray(np.where(m == 0, 250, 0).astype(np.uint16))
    goals = np.ascontiguousarray(np.argwhere(m != 0)[::1499].astype(np.int32))
    gh = np.full(len(goals), 80, np.int32)
    start = np.array(NC.first_free(m, (60, 90)), np.int32)
    ref = SR.view_route_h(m, top, start, goals, 150, gh, None, 4, 400)
    need, n = len(ref["path_rc"]), len(goals)
    assert need > 1
    prm, vp = HmsgRouteParams(5, 7, 0, 0), HmsgViewParams(4, 400, 0, 0)
    for cap in (need - 1, 0, need):
        out = HmsgNavRoutes()
        rc, off, cell, nv = np.full((max(cap, 1), 2), -7, np.int32), np.zeros(n + 1, np.int64), np.zeros((n, 2), np.int32), np.zeros(n, np.int32)
        out.path_rc, out.path_capacity, out.path_off, out.goal_cell = _ptr(rc), cap, _ptr(off), _ptr(cell)
        st = L.c.hmsg_nav_view_route_h(0, m.shape[0], m.shape[1], _ptr(m), _ptr(top), C.byref(prm), C.byref(vp), 150, _ptr(start), n, _ptr(goals),
                                       _ptr(gh), None, C.byref(out), _ptr(nv))
        assert out.n_path_cells == need and np.array_equal(off, ref["path_off"]) and np.array_equal(cell, ref["goal_cell"])
        assert np.array_equal(nv, ref["n_visible"]) and tuple(out.start_cell) == ref["start_cell"]
        assert (st != 0 and (rc == -7).all()) if cap < need else (st == 0 and np.array_equal(rc, ref["path_rc"]))


# ------------------------------------------------------------------------------------------ 6. refusals (S5)
def refusals(api, L):
    from holoagent_amd._lib import HmsgError, HmsgNavRoutes, HmsgRouteParams, HmsgViewParams, _ptr
    t, p = np.zeros((4, 5), np.uint16), np.ones((4, 5), np.uint8)
    for kw in (dict(r_min2=-1), dict(r_min2=10, r_max2=9), dict(prefer=2), dict(r_max2=255 * 255 + 1)):
        with pytest.raises(HmsgError):
            api.viewpoints_h(t, p, [(1, 1)], 100, 50, **kw)
        with pytest.raises(HmsgError):
            api.view_route_h(p, t, (0, 0), [(1, 1)], 100, 50, **kw)
    for eye in (-1, 65536):
        with pytest.raises(HmsgError):
            api.viewpoints_h(t, p, [(1, 1)], eye, 50)
        with pytest.raises(HmsgError):
            api.view_route_h(p, t, (0, 0), [(1, 1)], eye, 50)
    with pytest.raises(HmsgError):
        api.viewpoints_h(t, p, [(1, 1), (2, 2)], 100, 50, [0, -2])
    with pytest.raises(HmsgError):
        api.view_route_h(p, t, (0, 0), [(1, 1)], 100, 50, -2)
    assert api.viewpoints_h(t, p, [(1, 1)], 65535, 0, -1, r_max2=255 * 255)["n_visible"][0] == 20       # the limits themselves are fine
    c = L.c
    vp, prm, out = HmsgViewParams(0, 100, 0, 0), HmsgRouteParams(5, 7, 0, 0), HmsgNavRoutes()
    g, gh, rc, start = np.array([[1, 1]], np.int32), np.array([50], np.int32), np.zeros((1, 2), np.int32), np.zeros(2, np.int32)
    V, R = c.hmsg_nav_viewpoints_h, c.hmsg_nav_view_route_h
    ok = (0, 4, 5, _ptr(t), _ptr(p), None, C.byref(vp), 100, 1, _ptr(g), _ptr(gh), None, _ptr(rc), None, None, None, None)
    assert V(*ok) == 0 and tuple(rc[0]) == (1, 1)
    for k in (3, 4, 6, 9, 10, 12):                                        # top, passable, prm, goal_rc, goal_h, view_rc
        assert V(*[None if i == k else a for i, a in enumerate(ok)]) == -1, k
    assert V(0, 0, 5, *ok[3:]) == -1 and V(0, 4, 0, *ok[3:]) == -1
    assert V(*ok[:8], -1, *ok[9:]) == -1 and V(*ok[:8], 0, None, None, None, None, None, None, None, None) == 0
    assert V(*ok[:7], -1, *ok[8:]) == -1 and V(*ok[:7], 65536, *ok[8:]) == -1
    big = HmsgViewParams(0, 255 * 255 + 1, 0, 0)
    assert V(*[C.byref(big) if i == 6 else a for i, a in enumerate(ok)]) == UNSUPPORTED
    assert V(0, 1 << 14, 1 << 14, *ok[3:]) == UNSUPPORTED
    ok = (0, 4, 5, _ptr(p), _ptr(t), C.byref(prm), C.byref(vp), 100, _ptr(start), 1, _ptr(g), _ptr(gh), None, C.byref(out), None)
    assert R(*ok) == 0 and out.n_path_cells == 1
    for k in (3, 4, 5, 6, 8, 10, 11, 13):                                 # main_free_map, top, both params, start_rc, goal_rc, goal_h, out
        assert R(*[None if i == k else a for i, a in enumerate(ok)]) == -1, k
    assert R(*[C.byref(big) if i == 6 else a for i, a in enumerate(ok)]) == UNSUPPORTED
    assert R(*ok[:7], 65536, *ok[8:]) == -1


# ------------------------------------------------------------------------------------------ 7. the Python layer
def counter_room(seed=42):
    """a 3.6 x 3.0 m room with walls to 2.7 m and a counter 1.1 m high across its middle (x 1.7 to 1.9, z 0.6 to 2.4, open at both
    ends): under the obstacle band, so the flat maps neither see nor feel it"""
    from tests import navmap_cases as MC
    rng = np.random.default_rng(seed)
    sx, sz, zero = 3.6, 3.0, 0.25
    fl = np.c_[rng.uniform(0, sx, 9000), zero + rng.uniform(0.0, 0.02, 9000), rng.uniform(0, sz, 9000)]
    t, side = rng.uniform(0, 1, 7000), rng.integers(0, 4, 7000)
    wx = np.where(side == 0, 0.0, np.where(side == 1, sx, t * sx))
    wz = np.where(side < 2, t * sz, np.where(side == 2, 0.0, sz))
    wall = np.c_[wx, zero + rng.uniform(0.0, 2.7, 7000), wz]
    counter = np.c_[rng.uniform(1.7, 1.9, 2500), zero + rng.uniform(0.0, 1.1, 2500), rng.uniform(0.6, 2.4, 2500)]
    pts = np.concatenate([fl, wall, counter])
    pts = pts[rng.permutation(len(pts))]
    poses = np.array([MC.pose_at(rng.uniform(0.4, 3.2), zero + 0.8 + rng.uniform(-0.01, 0.01), rng.uniform(0.4, 2.6)) for _ in range(14)])
    return pts, rng.uniform(0, 1, pts.shape), zero, poses


def navigation_graph_heights(L, wrap=None):
    """NavigationGraph.height_map, route_to_view(sight="heights") and max_step_m on a storey with a counter between start and goal"""
    from holoagent_amd.nav_graph import NavigationGraph
    pts, cols, zero, poses = counter_room()
    cloud = (pts, cols) if wrap is None else (wrap(pts), wrap(cols))
    nav = NavigationGraph(cloud, 0.03, lib_=L)
    nav.get_main_free_map(None, {"floor_zero_level": zero}, None, list(poses), save=False, region_rule=1)       # (the largest component:
    np_ = lambda v: v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)                                   #  the room is larger than its walls)
    before = {k: np.array(np_(v)) for k, v in nav.maps.items() if hasattr(v, "shape")}
    main, blk = np_(nav.maps["main_free_map"]), np_(nav.sight_blocking_map())
    hm = nav.height_map()
    assert hm is nav.height_map() and hasattr(hm["top_map"], "cpu") == hasattr(nav.maps["main_free_map"], "cpu")      # made once, where the maps are
    top = np_(hm["top_map"])
    ref_top, ref_known = SR.height_map_np(pts, zero, 0.03)
    assert np.array_equal(top, ref_top) and np.array_equal(np_(hm["known_map"]), ref_known) and top.shape == main.shape
    assert nav.eye_units(1.5) == 150 and nav.eye_units(-1) == 0 and nav.eye_units(1e9) == 65535
    start = np.array([0.7, zero + 0.8, 1.5])
    goal_hi, goal_lo = np.array([[2.9, zero + 1.35, 1.5]]), np.array([[2.9, zero + 0.3, 1.5]])
    sc, gc = nav.cells_of(start)[0], nav.cells_of(goal_hi)[0]
    h_hi, h_lo, h_arg = (int(np.floor(v / 0.01)) for v in (goal_hi[0, 1] - zero, goal_lo[0, 1] - zero, 0.3))       # as the object forms them
    assert h_hi in (134, 135) and h_lo in (29, 30)
    ccol = nav.cells_of(np.array([1.8, 0, 1.5]))[0][1]
    assert main[tuple(sc)] and main[gc[0], ccol] and not blk[gc[0], ccol] and 105 <= top[gc[0], ccol] <= 110       # the flat maps do not know the counter
    band = nav.view_band((0.3, 3.0))
    # the flat rule: the least walk is the start's own cell, where the counter hides the low goal
    flat = nav.route_to_view(start, goal_lo, view_range_m=(0.3, 3.0))[0]
    assert flat["reachable"] and flat["cell"] == tuple(sc) and not SR.clear_h(top, flat["cell"], gc, 150, h_lo)
    VC.compare_view_route({k: v for k, v in nav.last_route.items() if k != "field"}, VR.view_route(main, blk, sc, [gc], *band))
    # heights, the goal above the counter: seen over it from where the robot stands
    over = nav.route_to_view(start, goal_hi, view_range_m=(0.3, 3.0), sight="heights", camera_height_m=1.5)[0]
    VC.compare_view_route({k: v for k, v in nav.last_route.items() if k != "field"}, SR.view_route_h(main, top, sc, [gc], 150, [h_hi], None, *band))
    assert over["reachable"] and over["cell"][1] < ccol and SR.clear_h(top, over["cell"], gc, 150, h_hi)
    # heights, the goal below the counter: no view, or the robot walks to where it sees it
    under = nav.route_to_view(start, goal_lo, view_range_m=(0.3, 3.0), sight="heights", camera_height_m=1.5)[0]
    ref = SR.view_route_h(main, top, sc, [gc], 150, [h_lo], None, *band)
    VC.compare_view_route({k: v for k, v in nav.last_route.items() if k != "field"}, ref)
    assert under["cell"] != flat["cell"] and (not under["reachable"] or SR.clear_h(top, under["cell"], gc, 150, h_lo))
    assert under["reachable"] == (ref["n_visible"][0] > 0) and under["n_visible"] < over["n_visible"]
    # goals as cells need their heights; a footprint; viewpoints answers as route_to_view does
    with pytest.raises(ValueError):
        nav.route_to_view(start, gc[None], sight="heights")
    with pytest.raises(ValueError):
        nav.route_to_view(start, goal_hi, sight="depth")
    v = nav.viewpoints(goal_lo, start=start, view_range_m=(0.3, 3.0), sight="heights", goal_heights_m=0.3, goal_radius_m=0.1, want_visible=True)
    ref = SR.viewpoints_h(top, main, [gc], *band, 150, [h_arg], [16], RR.field(main, [sc])[0], 0, True)
    VC.compare_views({k: np_(x) for k, x in v.items()}, ref, "viewpoints, heights")
    # max_step_m: the counter is walked through without it and round with it
    assert nav.passable_map(0.0) is nav.maps["main_free_map"] and np.array_equal(np_(nav.passable_map(0.09)), (main != 0) & (RR.clearance(main) >= 15))
    walk = ((main != 0) & (top <= 20)).astype(np.uint8)
    assert np.array_equal(np_(nav.walkable_map(0.2)), walk) and main[gc[0], ccol] and not walk[gc[0], ccol] and walk.sum() < main.sum()
    assert np.array_equal(np_(nav.passable_map(0.09, 0.2)), (walk != 0) & (RR.clearance(walk) >= 15))
    target = np.array([[2.9, zero, 1.5]])
    straight, round_ = nav.route(start, target, min_clearance_m=0.09)[0], nav.route(start, target, min_clearance_m=0.09, max_step_m=0.2)[0]
    NC.compare_route({k: v for k, v in nav.last_route.items() if k != "field"}, RR.route(walk, sc, nav.cells_of(target), min_clearance=15))
    assert straight["reachable"] and round_["reachable"] and round_["length_m"] > straight["length_m"] + 0.5
    cells = nav.cells_of(round_["polyline"])
    assert walk[cells[:, 0], cells[:, 1]].all() and not walk[tuple(nav.cells_of(straight["polyline"]).T)].all()
    assert np.array_equal(np_(nav.distance_field(start, 0.09, 0.2)), RR.field((walk != 0) & (RR.clearance(walk) >= 15), [sc])[0])
    rv = nav.route_to_view(start, goal_hi, min_clearance_m=0.09, view_range_m=(0.3, 3.0), sight="heights", max_step_m=0.2)[0]
    VC.compare_view_route({k: v for k, v in nav.last_route.items() if k != "field"},
                          SR.view_route_h(walk, top, sc, [gc], 150, [h_hi], None, *band, min_clearance=15))
    assert rv["reachable"]
    for k, a in before.items():                                           # None and "map" change nothing: today's arrays
        assert np.array_equal(np_(nav.maps[k]), a), k


def graph_view_routes_heights(L, tmp_path):
    """Graph.view_routes_to_objects(sight="heights") and the across-floors form on the small built scene of
    tests/navview_cases.py: each object's height above its storey's zero level and its footprint reach the library, the result is
    the restatement's on the storey's own maps; the defaults answer as before"""
    from holoagent_amd.graph import Object, Room, _Pcd
    from tests import navmap_cases as MC
    from tests.test_semseg_evaluate import build_graph
    g = build_graph(L)
    g.segment_floors_manually()
    fl = g.floors[0]
    xyz, _ = g.scene.map_points(colors=True)
    slab = xyz[(xyz[:, 1] >= fl._crop[0]) & (xyz[:, 1] <= fl._crop[1])]
    rng = np.random.default_rng(3)
    lo, hi = slab.min(0), slab.max(0)
    track = [MC.pose_at(rng.uniform(lo[0], hi[0]), fl.floor_zero_level + 0.9, rng.uniform(lo[2], hi[2])) for _ in range(12)]
    g.rooms += [Room("0_0", "0")]
    objs = []
    for k in range(6):
        o = Object("0_0_%d" % k, "0_0")
        c = np.array([rng.uniform(lo[0], hi[0]), fl.floor_zero_level + rng.uniform(0.2, 1.4), rng.uniform(lo[2], hi[2])])
        o.pcd = _Pcd(c + rng.normal(0, 0.05, (40, 3)))
        objs.append(o)
    g.objects = objs
    bare = np.asarray(objs[3].pcd.get_center())
    asked = [0, 1, objs[2], bare, 4, 5]
    start = track[0]
    before = g.view_routes_to_objects(start, asked, min_clearance=0.09, view_range=(0.1, 2.0), prefer="look", poses_list=track)
    res = g.view_routes_to_objects(start, asked, min_clearance=0.09, view_range=(0.1, 2.0), prefer="look", poses_list=track, sight="heights",
                                   camera_height=1.2)
    nav = g.floor_navigation(0)
    np_ = lambda v: v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)
    main, top = np_(nav.maps["main_free_map"]), np_(nav.maps["top_map"])
    assert np.array_equal(top, SR.height_map_np(slab, fl.floor_zero_level, 0.03)[0]) and top.any()
    centres = np.array([np.asarray(o.pcd.get_center()) for o in objs])
    centres[3] = bare
    gh = np.floor((centres[:, 1] - fl.floor_zero_level) / 0.01).astype(np.int32)
    r2 = []
    for k, o in enumerate(objs):
        ext = o.pcd.points[:, [0, 2]].max(0) - o.pcd.points[:, [0, 2]].min(0)
        r2.append(0 if k == 3 else int(np.ceil(0.5 * np.sqrt(ext[0] * ext[0] + ext[1] * ext[1]) / 0.03)) ** 2)
    assert r2[3] == 0 and min(r2[:3]) >= 4
    band = nav.view_band((0.1, 2.0))
    ref = SR.view_route_h(main, top, nav.cells_of(start[:3, 3])[0], nav.cells_of(centres), 120, gh, np.array(r2, np.int64), band[0], band[1], 1,
                          min_clearance=nav.clearance_units(0.09))
    assert sum(r["reachable"] for r in res) >= 1
    for k, r in enumerate(res):
        assert r["reachable"] == (ref["goal_dist"][k] != U) and r["cell"] == tuple(ref["goal_cell"][k]) and r["n_visible"] == ref["n_visible"][k]
        assert r["reason"] == (None if r["reachable"] else "no view")
        assert np.array_equal(nav.cells_of(r["polyline"]), ref["path_rc"][ref["path_off"][k]:ref["path_off"][k + 1]])
    across = g.view_routes_across_floors(start, asked, min_clearance=0.09, view_range=(0.1, 2.0), prefer="look", poses_list=track, links=[],
                                         sight="heights", camera_height=1.2)
    for a, r in zip(across, res):
        assert a["cell"] == r["cell"] and a["reachable"] == r["reachable"] and a["n_visible"] == r["n_visible"] and a["reason"] == r["reason"]
    stepped = g.view_routes_to_objects(start, asked, min_clearance=0.09, view_range=(0.1, 2.0), prefer="look", poses_list=track, sight="heights",
                                       camera_height=1.2, max_step=0.15)
    walk = ((main != 0) & (top <= 15)).astype(np.uint8)
    ref = SR.view_route_h(walk, top, nav.cells_of(start[:3, 3])[0], nav.cells_of(centres), 120, gh, np.array(r2, np.int64), band[0], band[1], 1,
                          min_clearance=nav.clearance_units(0.09))
    assert [r["cell"] for r in stepped] == [tuple(c) for c in ref["goal_cell"]]
    after = g.view_routes_to_objects(start, asked, min_clearance=0.09, view_range=(0.1, 2.0), prefer="look", poses_list=track)
    for a, b in zip(before, after):                                       # the defaults answer as they did
        assert a["cell"] == b["cell"] and a["reason"] == b["reason"] and np.array_equal(a["polyline"], b["polyline"])
    g.scene.close()


SIGHT_CASES = (height_map_cases, contains_v2, motivating_and_footprint, heights_and_edges, clutter_heights, view_route_h_against_the_calls)


# ------------------------------------------------------------------------------------------ how a case reaches the library
class api(VC.api):
    """tests/navview_cases.py's api with the calls of N10"""

    def grid(self, pts, cell_size):
        from holoagent_amd._lib import nav_grid
        return nav_grid(self._in(pts, np.float64), cell_size, lib_=self.L)

    def height_map(self, pts, zero, **params):
        from holoagent_amd._lib import nav_height_map
        r = nav_height_map(self._in(np.asarray(pts, np.float64).reshape(-1, 3), np.float64), zero, lib_=self.L, **params)
        return {k: self._out(v) for k, v in r.items()}

    def floor_maps(self, pts, zero, poses):
        from holoagent_amd._lib import nav_floor_maps
        r = nav_floor_maps(self._in(pts, np.float64), None, zero, poses, lib_=self.L)
        return {k: self._out(v) for k, v in r.items()}

    def _heights(self, gh, gr2, n):
        gh = self._in(np.broadcast_to(np.asarray(gh, np.int64).clip(-2 ** 31, 2 ** 31 - 1), (n,)), np.int32)
        return gh, None if gr2 is None else self._in(np.broadcast_to(np.asarray(gr2, np.int64), (n,)), np.int64)

    def viewpoints_h(self, top, pas, goals, eye, gh, gr2=None, field=None, want_visible=False, **w):
        from holoagent_amd._lib import nav_viewpoints_h
        g = np.asarray(goals, np.int64).clip(-2 ** 31, 2 ** 31 - 1).reshape(-1, 2)
        gh, gr2 = self._heights(gh, gr2, len(g))
        r = nav_viewpoints_h(self._in(top, np.uint16), self._in(pas, np.uint8), self._in(g, np.int32), eye, gh, gr2,
                             field=None if field is None else self._in(field, np.int32), want_visible=want_visible, lib_=self.L, **w)
        return {k: self._out(v) for k, v in r.items()}

    def view_route_h(self, m, top, start, goals, eye, gh, gr2=None, want_field=False, **w):
        from holoagent_amd._lib import nav_view_route_h
        g = np.asarray(goals, np.int64).reshape(-1, 2)
        gh, gr2 = self._heights(gh, gr2, len(g))
        r = nav_view_route_h(self._in(m, np.uint8), self._in(top, np.uint16), start, self._in(g, np.int32), eye, gh, gr2, lib_=self.L,
                             want_field=want_field, **w)
        return {k: self._out(v) for k, v in r.items()}
