"""The cases of the viewpoint calls (include/hmsg.h, N8: hmsg_nav_viewpoints, hmsg_nav_view_route), shared by the simulator tests
(tests/test_navview.py) and the GPU tests (tests/test_navview_gpu.py), laid out as tests/navroute_cases.py is.  A case takes `api`
(the wrappers of holoagent_amd._lib on one library or the other, images handed over as numpy arrays or as device tensors, results
as numpy) and compares every output with tests/navview_reference.py by array_equal: nothing here has a tolerance.  line_rule and
vectorised_against_loops test the reference alone; the cases that take the library itself (the refusals, the capacity,
NavigationGraph.route_to_view, Graph.view_routes_to_objects) are at the end."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import navroute_cases as NC
from tests import navroute_reference as RR
from tests import navview_reference as VR

U = VR.UNREACHED
UNSUPPORTED = -3                                                          # include/hmsg.h: HMSG_ERR_UNSUPPORTED
KEYS = ("view_rc", "view_d2", "view_dist", "n_visible")


def frozen(a):
    a.setflags(write=False)
    return a


def compare_views(got, ref, what=""):
    for k in KEYS + (("visible",) if "visible" in ref else ()):
        assert got[k].dtype == ref[k].dtype and got[k].shape == ref[k].shape, (what, k)
        assert np.array_equal(got[k], ref[k]), (what, k, np.flatnonzero((got[k] != ref[k]).reshape(len(ref[k]), -1).any(axis=1))[:8])


def check_views(api, blk, pas, goals, r_min2, r_max2, field=None, prefer=0, want_visible=True, what="", ref=None):
    got = api.viewpoints(blk, pas, goals, field=field, want_visible=want_visible, r_min2=r_min2, r_max2=r_max2, prefer=prefer)
    ref = ref if ref is not None else VR.viewpoints(blk, pas, goals, r_min2, r_max2, field, prefer, want_visible)
    compare_views(got, ref, what)
    return got


# ------------------------------------------------------------------------------------------ 1. the line rule (the reference alone)
def line_rule():
    rng = np.random.default_rng(0)
    for _ in range(2000):
        a, b = (tuple(int(v) for v in rng.integers(-40, 40, 2)) for _ in range(2))
        line = VR.sight_line(a, b)
        assert line == VR.sight_line(b, a)                                 # chosen by the cells, not by the caller
        assert line[0] == min(a, b) and line[-1] == max(a, b) and len(line) == max(abs(a[0] - b[0]), abs(a[1] - b[1])) + 1
        assert all(max(abs(u[0] - v[0]), abs(u[1] - v[1])) == 1 for u, v in zip(line[:-1], line[1:]))       # 8-connected
    assert VR.sight_line((3, 4), (3, 4)) == [(3, 4)]
    # the half-way cases round towards + in both directions: floor((2 i dm + n) / (2 n)) with dm < 0 is not C's truncation
    assert VR.sight_line((0, 5), (2, 0)) == [(0, 5), (0, 4), (1, 3), (1, 2), (2, 1), (2, 0)]
    assert VR.sight_line((0, 0), (2, 5)) == [(0, 0), (0, 1), (1, 2), (1, 3), (2, 4), (2, 5)]
    assert VR.sight_line((0, 1), (2, 0)) == [(0, 1), (1, 1), (2, 0)] and VR.sight_line((0, 0), (2, 1)) == [(0, 0), (1, 1), (2, 1)]
    assert VR.sight_line((5, 0), (0, 2)) == [(0, 2), (1, 2), (2, 1), (3, 1), (4, 0), (5, 0)]       # (truncation: (2, 2) and (4, 1))
    assert VR.sight_line((0, 0), (4, 4)) == [(k, k) for k in range(5)] and VR.sight_line((4, 0), (0, 4)) == [(k, 4 - k) for k in range(5)]


def vectorised_against_loops():
    """the numpy restatement equals the loops: random clutter, every kind of goal, both orders, with and without a field"""
    rng = np.random.default_rng(1)
    blk = (rng.random((31, 37)) < 0.2).astype(np.uint8)
    pas = ((blk == 0) & (rng.random((31, 37)) < 0.9)).astype(np.uint8)
    f, _ = RR.field(pas, [NC.first_free(pas, (15, 18))])
    goals = [(0, 0), (15, 18), (30, 36), (0, 20), (14, 0), (-1, 3), (31, 3), (3, 37)] + [tuple(c) for c in np.argwhere(blk != 0)[:4]]
    for fld in (None, f):
        for prefer in (0, 1):
            for g in goals:
                a, b = VR.viewpoint(blk, pas, g, 2, 150, fld, prefer), VR.viewpoint_np(blk, pas, g, 2, 150, fld, prefer)
                assert a[:4] == b[:4] and np.array_equal(a[4], b[4]), (g, prefer, a[:4], b[:4])


# ------------------------------------------------------------------------------------------ 2. an open room
def open_room(api):
    H, W, g = 33, 47, (16, 23)
    blk, pas = np.zeros((H, W), np.uint8), np.ones((H, W), np.uint8)
    rr, cc = np.mgrid[:H, :W]
    d2 = (rr - g[0]) ** 2 + (cc - g[1]) ** 2
    ring = ((d2 >= 4) & (d2 <= 100)).astype(np.uint8)
    for prefer in (0, 1):
        got = check_views(api, blk, pas, [g], 4, 100, prefer=prefer, what="open room")
        assert np.array_equal(got["visible"][0], ring) and got["n_visible"][0] == ring.sum()
        assert tuple(got["view_rc"][0]) == (14, 23) and got["view_d2"][0] == 4 and got["view_dist"][0] == 0
    got = check_views(api, blk, pas, [g], 0, 0, what="the goal's own cell")
    assert tuple(got["view_rc"][0]) == g and got["n_visible"][0] == 1 and got["view_d2"][0] == 0
    one = VR.viewpoint(blk, pas, g, 4, 100)                                # ... and the loops say the same
    assert np.array_equal(one[4], ring) and one[0] == (14, 23)


# ------------------------------------------------------------------------------------------ 3. the wall the old snap goes through
MINC, WALL_BAND = 20, (0, 100)


@functools.lru_cache(maxsize=None)
def wall_map(door):
    """40 x 60: a wall three cells thick (rows 20 to 22) right across, behind it a room five cells wide (rows 23 to 27) that a
    clearance of 20 (four cells) empties; the goal at the wall's far face.  door: three columns of the wall opposite the goal open"""
    m = np.ones((40, 60), np.uint8)
    m[20:23, :] = 0
    m[28:, :] = 0
    if door:
        m[20:23, 29:32] = 1
    return frozen(m), frozen((m == 0).astype(np.uint8)), (5, 5), np.array([[23, 30]], np.int32)


def wall_between(api):
    for door in (False, True):
        m, blk, start, goals = wall_map(door)
        old = api.route(m, start, goals, min_clearance=MINC)
        NC.compare_route(old, RR.route(m, start, goals, min_clearance=MINC))
        assert not old["passable"][23:28].any()                            # the clearance empties the room behind the wall
        assert tuple(old["goal_cell"][0]) == (16, 30) and old["goal_dist"][0] != U and np.diff(old["path_off"])[0] > 0
        assert not VR.clear(blk, (16, 30), (23, 30)) if not door else VR.clear(blk, (16, 30), (23, 30))      # the old answer faces the wall
        got = api.view_route(m, blk, start, goals, min_clearance=MINC, r_min2=WALL_BAND[0], r_max2=WALL_BAND[1], want_field=True)
        ref = VR.view_route(m, blk, start, goals, *WALL_BAND, min_clearance=MINC)
        compare_view_route(got, ref)
        assert np.array_equal(got["passable"], old["passable"])
        if not door:
            assert tuple(got["goal_cell"][0]) == (-1, -1) and got["goal_d2"][0] == -1 and got["goal_dist"][0] == U and got["n_visible"][0] == 0
            assert np.array_equal(got["path_off"], [0, 0]) and len(got["path_rc"]) == 0
        else:
            cell = tuple(int(v) for v in got["goal_cell"][0])
            assert cell[0] <= 16 and got["passable"][cell] and got["n_visible"][0] > 0 and np.diff(got["path_off"])[0] > 0
            line = VR.sight_line(cell, (23, 30))
            assert VR.clear(blk, cell, (23, 30)) and any(20 <= r <= 22 and 29 <= c <= 31 for r, c in line)       # it looks through the door
            assert tuple(got["path_rc"][-1]) == cell and tuple(got["path_rc"][0]) == got["start_cell"]


# ------------------------------------------------------------------------------------------ 4. the diagonal wall
def diagonal_wall(api):
    pas = np.array([[0, 1], [1, 0]], np.uint8)
    got = check_views(api, np.array([[1, 0], [0, 1]], np.uint8), pas, [(1, 0)], 1, 8, what="[[1, 0], [0, 1]]")
    assert got["n_visible"][0] == 0 and tuple(got["view_rc"][0]) == (-1, -1)
    got = check_views(api, np.array([[1, 0], [0, 0]], np.uint8), pas, [(1, 0)], 1, 8, what="[[1, 0], [0, 0]]")
    assert got["n_visible"][0] == 1 and tuple(got["view_rc"][0]) == (0, 1)
    # a diagonal wall right across a 24 x 24 image: opaque although no two of its cells share an edge; one cell taken out opens it
    blk = np.eye(24, dtype=np.uint8)
    pas = (1 - blk).astype(np.uint8)
    goals = [(20, 3), (12, 11), (23, 0)]
    got = check_views(api, blk, pas, goals, 0, 40 * 40, what="diagonal wall")
    rr, cc = np.mgrid[:24, :24]
    assert not got["visible"][:, rr < cc].any() and (got["n_visible"] > 0).all()
    gap = blk.copy()
    gap[8, 8] = 0
    through = [(12, 8), (10, 6), (8, 3)]                                   # up the gap's column, along its anti-diagonal, along its row
    got = check_views(api, gap, (1 - gap).astype(np.uint8), through + goals, 0, 40 * 40, what="a one-cell gap")
    assert got["visible"][:3, rr < cc].any(axis=1).all() and got["visible"][0, 5, 8] and got["visible"][1, 6, 10] and got["visible"][2, 8, 11]


# ------------------------------------------------------------------------------------------ 5. corners, edges, outside
def corners_and_edges(api):
    rng = np.random.default_rng(6)                                        # (a seed with which the reference sees every corner)
    H, W = 40, 50
    blk = (rng.random((H, W)) < 0.1).astype(np.uint8)
    pas = (1 - blk).astype(np.uint8)
    inside = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (0, 25), (H - 1, 25), (20, 0), (20, W - 1)]
    outside = [(-1, 5), (5, -1), (H, 0), (0, W), (10 ** 6, 3), (-2 ** 31, 2 ** 31 - 1), (-1, -1)]
    for prefer in (0, 1):
        got = check_views(api, blk, pas, inside + outside, 1, 30 * 30, prefer=prefer, what="corners")
        assert (got["n_visible"][:len(inside)] > 0).all()
        assert (got["n_visible"][len(inside):] == 0).all() and (got["view_rc"][len(inside):] == -1).all() and not got["visible"][len(inside):].any()
        assert (got["view_d2"][len(inside):] == -1).all() and (got["view_dist"][len(inside):] == U).all()
    got = api.viewpoints(blk, pas, np.zeros((0, 2), np.int32))
    assert all(len(got[k]) == 0 for k in KEYS)


# ------------------------------------------------------------------------------------------ 6. ties
def ties(api):
    """a 21 x 21 room with nothing in sight's way, walked from (10, 0) on the axis of symmetry; the cells of the axis between the
    start and the goal are not passable, so the best cells come in mirror pairs with equal field and equal d2"""
    blk, pas = np.zeros((21, 21), np.uint8), np.ones((21, 21), np.uint8)
    pas[10, 3:10] = 0
    f, _ = RR.field(pas, [(10, 0)])
    g = (10, 10)
    cells = {}
    for prefer in (0, 1):
        got = check_views(api, blk, pas, [g], 9, 25, field=f, prefer=prefer, what="ties")
        cells[prefer] = r, c = tuple(int(v) for v in got["view_rc"][0])
        assert r < 10 and got["visible"][0, 20 - r, c] and f[20 - r, c] == f[r, c]       # its mirror image ties; the index decides
        assert got["view_dist"][0] == f[r, c] and got["view_d2"][0] == (r - 10) ** 2 + (c - 10) ** 2
    assert cells[0] != cells[1] and f[cells[0]] < f[cells[1]]              # least walk and closest look stand on different cells
    assert (cells[1][0] - 10) ** 2 + (cells[1][1] - 10) ** 2 < (cells[0][0] - 10) ** 2 + (cells[0][1] - 10) ** 2
    got = check_views(api, blk, pas, [g], 9, 25, prefer=0, what="ties, no field")         # no field: (0, d2, index) under both orders
    assert tuple(got["view_rc"][0]) == (7, 10) and got["view_dist"][0] == 0


# ------------------------------------------------------------------------------------------ 7. an island in sight that is not reached
def unreached_island(api):
    blk, pas = np.zeros((15, 30), np.uint8), np.ones((15, 30), np.uint8)
    pas[6:9, 19:22] = 0
    pas[7, 20] = 1                                                        # passable, in sight of the goal, and walled in
    f, _ = RR.field(pas, [(7, 2)])
    assert f[7, 20] == U and f[7, 23] != U
    g = [(7, 22)]
    with_field = check_views(api, blk, pas, g, 1, 16, field=f, what="island, field")
    without = check_views(api, blk, pas, g, 1, 16, what="island, no field")
    assert without["visible"][0, 7, 20] == 1 and with_field["visible"][0, 7, 20] == 0
    assert without["n_visible"][0] == with_field["n_visible"][0] + 1
    only = check_views(api, blk, pas, g, 4, 4, field=f, prefer=1, what="island, band of one distance")
    assert tuple(only["view_rc"][0]) == (5, 22)                            # (7, 20) has d2 4 too and the smaller field... were it reached
    assert tuple(check_views(api, blk, pas, g, 4, 4, prefer=1)["view_rc"][0]) == (5, 22)       # (without a field the index decides: row 5)
    all_unreached = check_views(api, blk, pas, g, 1, 16, field=np.full(pas.shape, U, np.int32), what="a field that reaches nothing")
    assert all_unreached["n_visible"][0] == 0 and all_unreached["view_dist"][0] == U


# ------------------------------------------------------------------------------------------ 8. clutter
@functools.lru_cache(maxsize=None)
def clutter():
    """130 x 130, 22 % blocked at random plus two walls with one door each; 70 goals: anywhere, duplicates, inside obstacles"""
    rng = np.random.default_rng(8)
    blk = (rng.random((130, 130)) < 0.22).astype(np.uint8)
    blk[43, :] = blk[:, 87] = 1
    blk[43, 20:23] = blk[100:103, 87] = 0
    pas = (1 - blk).astype(np.uint8)
    f, _ = RR.field(pas, [NC.first_free(pas, (10, 10))])
    goals = np.concatenate([rng.integers(0, 130, (54, 2)), np.argwhere(blk != 0)[rng.integers(0, int(blk.sum()), 12)], [[64, 64], [64, 64], [0, 0], [129, 129]]])
    goals[5] = goals[2]
    refs = {prefer: VR.viewpoints(blk, pas, goals, 9, 20 * 20, f, prefer, want_visible=(prefer == 0)) for prefer in (0, 1)}
    for r in refs.values():
        for v in r.values():
            v.setflags(write=False)
    return frozen(blk), frozen(pas), frozen(f), frozen(goals.astype(np.int32)), refs


def clutter_map(api):
    blk, pas, f, goals, refs = clutter()
    found = refs[0]["n_visible"] > 0
    assert len(goals) == 70 and found.sum() >= len(goals) / 4 and (~found).sum() >= 3, (int(found.sum()), int((~found).sum()))
    assert (blk[goals[:, 0], goals[:, 1]] != 0).sum() >= 12 and (refs[0]["view_rc"] != refs[1]["view_rc"]).any()
    for prefer in (0, 1):
        check_views(api, blk, pas, goals, 9, 20 * 20, field=f, prefer=prefer, want_visible=(prefer == 0), what="clutter", ref=refs[prefer])
    got = api.viewpoints(blk, pas, goals, field=f, r_min2=9, r_max2=400)    # nothing but the cells asked for
    assert np.array_equal(got["view_rc"], refs[0]["view_rc"])


# ------------------------------------------------------------------------------------------ 9. the largest window (GPU only)
LARGE_BAND = (150 * 150, 255 * 255)


@functools.lru_cache(maxsize=None)
def large():
    """300 x 520, 0.4 % pillars and two long walls with a door each: sight lines of 150 to 255 cells"""
    rng = np.random.default_rng(9)
    blk = (rng.random((300, 520)) < 0.004).astype(np.uint8)
    blk[:260, 180] = blk[40:, 400] = 1
    blk[120:124, 180] = blk[200:204, 400] = 0
    p = (1 - blk).astype(np.uint8)
    f, _ = RR.field(p, [NC.first_free(p, (150, 260))])
    goals = np.array([[150, 260], [0, 0], [299, 519], [150, 0], [297, 300]], np.int32)
    refs = {prefer: VR.viewpoints(blk, p, goals, *LARGE_BAND, f, prefer, want_visible=(prefer == 0)) for prefer in (0, 1)}
    return frozen(blk), frozen(p), frozen(f), frozen(goals), refs


def large_window(api):
    """r_max2 = 255^2 on 300 x 520: the window of the goal in the middle is taller than the image and 511 wide, the corner's is a
    quarter of one; the band starts at 150 cells, so every line walked is long"""
    blk, p, f, goals, refs = large()
    assert (refs[0]["n_visible"] > 1000).all() and (refs[0]["view_rc"] != refs[1]["view_rc"]).any()
    far = np.argwhere(refs[0]["visible"][0])
    assert (np.abs(far[:, 1] - 260) > 240).any()                           # somebody sees the middle from more than 240 cells away
    for prefer in (0, 1):
        check_views(api, blk, p, goals, *LARGE_BAND, field=f, prefer=prefer, want_visible=(prefer == 0), what="large", ref=refs[prefer])


# ------------------------------------------------------------------------------------------ 10. the composition
def compare_view_route(got, ref):
    NC.compare_route(got, ref)
    assert got["n_visible"].dtype == np.int32 and np.array_equal(got["n_visible"], ref["n_visible"])


def view_route_against_the_calls(api):
    m = NC.rooms_map()
    blk = (m == 0).astype(np.uint8)
    rng = np.random.default_rng(13)
    goals = np.concatenate([rng.integers(-10, 200, (30, 2)), np.argwhere(m == 0)[::400][:10]])
    for start, minc, band, prefer in (((3, 3), 0, (0, 400), 0), ((64, 95), 10, (4, 900), 1), ((-50, 400), 10, (9, 2500), 0)):
        got = api.view_route(m, blk, start, goals, min_clearance=minc, r_min2=band[0], r_max2=band[1], prefer=prefer, want_field=True)
        compare_view_route(got, VR.view_route(m, blk, start, goals, band[0], band[1], prefer, min_clearance=minc))
        # ... against the library's own calls, and everything but the goals' cells against hmsg_nav_route
        old = api.route(m, start, goals, min_clearance=minc, want_field=True)
        assert got["start_cell"] == old["start_cell"] and got["start_d2"] == old["start_d2"]
        assert np.array_equal(got["passable"], old["passable"]) and np.array_equal(got["field"], old["field"])
        v = api.viewpoints(blk, old["passable"], goals, field=old["field"], r_min2=band[0], r_max2=band[1], prefer=prefer)
        off, rc = api.paths(old["passable"], old["field"], v["view_rc"])
        assert np.array_equal(got["goal_cell"], v["view_rc"]) and np.array_equal(got["goal_d2"], v["view_d2"])
        assert np.array_equal(got["goal_dist"], v["view_dist"]) and np.array_equal(got["n_visible"], v["n_visible"])
        assert np.array_equal(got["path_off"], off) and np.array_equal(got["path_rc"], rc)
        assert (got["goal_cell"] != old["goal_cell"]).any() and (got["n_visible"] > 0).any() and (got["n_visible"] == 0).any()
        NC.check_walk(old["passable"], old["field"], rc, 5, 7, off)
        without = api.view_route(m, blk, start, goals, min_clearance=minc, r_min2=band[0], r_max2=band[1], prefer=prefer)
        assert "field" not in without and all(np.array_equal(without[k], got[k]) for k in without if k not in ("start_cell", "start_d2"))
    none = api.view_route(np.zeros((6, 7), np.uint8), np.ones((6, 7), np.uint8), (2, 2), [(1, 1), (3, 3)])
    assert none["start_cell"] == (-1, -1) and (none["goal_cell"] == -1).all() and (none["goal_dist"] == U).all() and (none["n_visible"] == 0).all()
    assert np.array_equal(none["path_off"], [0, 0, 0])
    empty = api.view_route(m, blk, (3, 3), np.zeros((0, 2), np.int32))
    assert len(empty["goal_cell"]) == 0 and np.array_equal(empty["path_off"], [0]) and len(empty["n_visible"]) == 0


def view_route_capacity_too_small(L):
    """a list that is too short behaves as hmsg_nav_route's: an error, the count says what is needed, everything else is written"""
    from holoagent_amd._lib import HmsgNavRoutes, HmsgRouteParams, HmsgViewParams, _ptr
    m = np.ascontiguousarray(NC.rooms_map())
    blk = np.ascontiguousarray((m == 0).astype(np.uint8))
    goals = np.ascontiguousarray(np.argwhere(m != 0)[::1499].astype(np.int32))
    start = np.array(NC.first_free(m, (60, 90)), np.int32)
    ref = VR.view_route(m, blk, start, goals, 4, 400)
    need, n = len(ref["path_rc"]), len(goals)
    assert need > 1
    prm, vp = HmsgRouteParams(5, 7, 0, 0), HmsgViewParams(4, 400, 0, 0)
    for cap in (need - 1, 0, need):
        out = HmsgNavRoutes()
        rc, off, cell, nv = np.full((max(cap, 1), 2), -7, np.int32), np.zeros(n + 1, np.int64), np.zeros((n, 2), np.int32), np.zeros(n, np.int32)
        out.path_rc, out.path_capacity, out.path_off, out.goal_cell = _ptr(rc), cap, _ptr(off), _ptr(cell)
        st = L.c.hmsg_nav_view_route(0, m.shape[0], m.shape[1], _ptr(m), _ptr(blk), C.byref(prm), C.byref(vp), _ptr(start), n, _ptr(goals), C.byref(out),
                                     _ptr(nv))
        assert out.n_path_cells == need and np.array_equal(off, ref["path_off"]) and np.array_equal(cell, ref["goal_cell"])
        assert np.array_equal(nv, ref["n_visible"]) and tuple(out.start_cell) == ref["start_cell"]
        assert (st != 0 and (rc == -7).all()) if cap < need else (st == 0 and np.array_equal(rc, ref["path_rc"]))
    out = HmsgNavRoutes()                                                 # nothing wanted but the count
    assert L.c.hmsg_nav_view_route(0, m.shape[0], m.shape[1], _ptr(m), _ptr(blk), C.byref(prm), C.byref(vp), _ptr(start), n, _ptr(goals), C.byref(out),
                                   None) == 0
    assert out.n_path_cells == need and out.start_d2 == 0


# ------------------------------------------------------------------------------------------ 11. refusals
def refusals(api, L):
    from holoagent_amd._lib import HmsgError, HmsgNavRoutes, HmsgRouteParams, HmsgViewParams, _ptr
    b, p = np.zeros((4, 5), np.uint8), np.ones((4, 5), np.uint8)
    for kw in (dict(r_min2=-1), dict(r_min2=10, r_max2=9), dict(prefer=2), dict(prefer=-1), dict(r_max2=255 * 255 + 1)):
        with pytest.raises(HmsgError):
            api.viewpoints(b, p, [(1, 1)], **kw)
        with pytest.raises(HmsgError):
            api.view_route(p, b, (0, 0), [(1, 1)], **kw)
    with pytest.raises(HmsgError):
        api.view_route(p, b, (0, 0), [(1, 1)], min_clearance=-1)           # hmsg_nav_route's own
    assert api.viewpoints(b, p, [(1, 1)], r_max2=255 * 255)["n_visible"][0] == 20        # the limit itself is fine
    c = L.c
    vp, prm, out = HmsgViewParams(0, 100, 0, 0), HmsgRouteParams(5, 7, 0, 0), HmsgNavRoutes()
    g, rc, start = np.array([[1, 1]], np.int32), np.zeros((1, 2), np.int32), np.zeros(2, np.int32)
    V, R = c.hmsg_nav_viewpoints, c.hmsg_nav_view_route
    ok = (0, 4, 5, _ptr(b), _ptr(p), None, C.byref(vp), 1, _ptr(g), _ptr(rc), None, None, None, None)
    assert V(*ok) == 0 and tuple(rc[0]) == (1, 1)                          # (no field: the goal's own cell, d2 0)
    for k in (3, 4, 6, 8, 9):                                             # blocking, passable, prm, goal_rc, view_rc
        assert V(*[None if i == k else a for i, a in enumerate(ok)]) == -1, k
    assert V(0, 0, 5, *ok[3:]) == -1 and V(0, 4, 0, *ok[3:]) == -1 and V(0, -1, 5, *ok[3:]) == -1
    assert V(*ok[:7], -1, *ok[8:]) == -1 and V(*ok[:7], 0, None, None, None, None, None, None) == 0
    okv, ok = ok, (0, 4, 5, _ptr(p), _ptr(b), C.byref(prm), C.byref(vp), _ptr(start), 1, _ptr(g), C.byref(out), None)
    assert R(*ok) == 0 and out.n_path_cells == 1                           # (least walk: the start's own cell sees the goal)
    for k in (3, 4, 5, 6, 7, 9, 10):                                      # main_free_map, blocking, both params, start_rc, goal_rc, out
        assert R(*[None if i == k else a for i, a in enumerate(ok)]) == -1, k
    assert R(0, 0, 5, *ok[3:]) == -1 and R(0, 4, 0, *ok[3:]) == -1
    # r_max2 above 255^2 and the sizes that could overflow are refused before anything is read (HMSG_ERR_UNSUPPORTED)
    big = HmsgViewParams(0, 255 * 255 + 1, 0, 0)
    assert V(*[C.byref(big) if i == 6 else a for i, a in enumerate(okv)]) == UNSUPPORTED
    assert R(*[C.byref(big) if i == 6 else a for i, a in enumerate(ok)]) == UNSUPPORTED
    assert V(0, 1 << 14, 1 << 14, _ptr(b), _ptr(p), None, C.byref(vp), 1, _ptr(g), _ptr(rc), None, None, None, None) == UNSUPPORTED
    assert R(0, 1 << 14, 1 << 14, *ok[3:]) == UNSUPPORTED
    for bad in (HmsgViewParams(-1, 100, 0, 0), HmsgViewParams(5, 4, 0, 0), HmsgViewParams(0, 100, 2, 0)):
        assert V(0, 4, 5, _ptr(b), _ptr(p), None, C.byref(bad), 1, _ptr(g), _ptr(rc), None, None, None, None) == -1
    d = HmsgViewParams(7, 7, 7, 7)
    c.hmsg_view_default_params(C.byref(d))
    assert (d.r_min2, d.r_max2, d.prefer, d.reserved_) == (0, 100 * 100, 0, 0)


# ------------------------------------------------------------------------------------------ 12. the Python layer
def navigation_graph_route_to_view(L, wrap=None):
    """NavigationGraph.route_to_view / viewpoints / sight_blocking_map on a storey made as tests/navmap_cases.py makes one: metres
    to cells by int(m / cell_size), the result against the restatement on the object's own maps, facing and yaw"""
    from holoagent_amd.nav_graph import NavigationGraph
    from tests import navmap_cases as MC
    pts, cols, zero, poses = MC.room(41, 3.0, 2.4, n_floor=5000, n_wall=4000, n_box=900)
    cloud = (pts, cols) if wrap is None else (wrap(pts), wrap(cols))
    nav = NavigationGraph(cloud, 0.03, lib_=L)
    nav.get_main_free_map(None, {"floor_zero_level": zero}, None, list(poses), save=False)
    np_ = lambda v: v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)
    main, blk = np_(nav.maps["main_free_map"]), np_(nav.sight_blocking_map())
    assert blk.dtype == np.uint8 and np.array_equal(blk, (np_(nav.maps["obstacle_map"]) > 0).astype(np.uint8)) and 0 < blk.sum() < blk.size
    assert hasattr(nav.sight_blocking_map(), "cpu") == hasattr(nav.maps["obstacle_map"], "cpu")       # where the maps are
    rng = np.random.default_rng(2)
    lo, hi = pts.min(0), pts.max(0)
    goals = np.c_[rng.uniform(lo[0] - 0.3, hi[0] + 0.3, 24), rng.uniform(0, 2, 24), rng.uniform(lo[2] - 0.3, hi[2] + 0.3, 24)]
    start = np.array([poses[0][0, 3], 0.8, poses[0][2, 3]])
    cells = nav.cells_of(goals)
    assert nav.view_band((0.5, 3.0)) == (16 * 16, 100 * 100) and nav.view_band((0.0, 0.1)) == (0, 9)
    with pytest.raises(ValueError):
        nav.view_band((0.0, 256 * 0.03 + 0.001))
    with pytest.raises(ValueError):
        nav.route_to_view(start, goals, prefer="near")
    seen = 0
    for metres, units, rng_m, prefer in ((0.0, 0, (0.0, 3.0), "walk"), (0.09, 15, (0.2, 1.0), "look"), (0.09, 15, (0.2, 1.0), "walk")):
        band = nav.view_band(rng_m)
        got = nav.route_to_view(start, goals, min_clearance_m=metres, view_range_m=rng_m, prefer=prefer)
        ref = VR.view_route(main, blk, nav.cells_of(start)[0], cells, band[0], band[1], 0 if prefer == "walk" else 1, min_clearance=units)
        compare_view_route({k: v for k, v in nav.last_route.items() if k != "field"}, ref)
        assert ref["start_cell"] != (-1, -1) and len(got) == len(goals)
        v = nav.viewpoints(goals, start=start, min_clearance_m=metres, view_range_m=rng_m, prefer=prefer, want_visible=True)
        assert np.array_equal(np_(v["view_rc"]), ref["goal_cell"]) and np.array_equal(np_(v["view_dist"]), ref["goal_dist"])
        assert np.array_equal(np_(v["n_visible"]), ref["n_visible"]) and np_(v["visible"]).shape == (len(goals),) + main.shape
        anywhere = nav.viewpoints(goals, min_clearance_m=metres, view_range_m=rng_m, prefer=prefer)          # no start: no field
        assert (np_(anywhere["n_visible"]) >= ref["n_visible"]).all()
        for k, r in enumerate(got):
            a, b = ref["path_off"][k], ref["path_off"][k + 1]
            assert r["reachable"] == (ref["goal_dist"][k] != U) and r["cell"] == tuple(ref["goal_cell"][k]) and len(r["polyline"]) == b - a
            assert r["n_visible"] == ref["n_visible"][k] and r["reachable"] == (r["n_visible"] > 0)
            if not r["reachable"]:
                assert r["point"] is None and r["facing"] is None and r["yaw"] is None
                continue
            seen += 1
            row, col = r["cell"]
            assert np.array_equal(r["point"], [(col + 0.5) * 0.03 + nav.pcd_min[0], nav.pcd_min[1], (row + 0.5) * 0.03 + nav.pcd_min[2]])
            assert r["length_m"] == float(ref["goal_dist"][k]) * 0.03 / 5 and np.array_equal(r["polyline"][-1], r["point"])
            assert VR.clear(blk, r["cell"], tuple(cells[k])) and band[0] <= (row - cells[k][0]) ** 2 + (col - cells[k][1]) ** 2 <= band[1]
            d = np.array([goals[k][0] - r["point"][0], goals[k][2] - r["point"][2]])
            assert r["facing"].dtype == np.float64
            if r["cell"] == tuple(cells[k]):
                assert np.array_equal(r["facing"], [0.0, 0.0]) and r["yaw"] == 0.0
            else:
                assert np.array_equal(r["facing"], d / np.sqrt(d[0] * d[0] + d[1] * d[1])) and r["yaw"] == float(np.arctan2(r["facing"][0], r["facing"][1]))
    assert seen >= 3
    on_cell = nav.route_to_view(start, cells[:6], view_range_m=(0.0, 3.0))     # goals given as cells: the facing aims at the cell's centre
    for k, r in enumerate(on_cell):
        if r["reachable"] and r["cell"] != tuple(cells[k]):
            d = np.array([float(cells[k][1] - r["cell"][1]), float(cells[k][0] - r["cell"][0])])
            assert np.allclose(r["facing"], d / np.linalg.norm(d), rtol=0, atol=1e-9)


def graph_view_routes_to_objects(L, tmp_path):
    """Graph.view_routes_to_objects on a scene built from frames (as tests/navroute_cases.py builds it): every object stood for is
    in sight from its cell, "other floor", "no view" and "unreachable" each appear, route_to_objects answers as before"""
    from holoagent_amd.graph import Floor, Object, Room, _Pcd
    from tests import navmap_cases as MC
    from tests.test_semseg_evaluate import build_graph
    g = build_graph(L)
    g.segment_floors_manually()
    assert len(g.floors) == 1 and g.scene is not None
    fl = g.floors[0]
    xyz, _ = g.scene.map_points(colors=True)
    slab = xyz[(xyz[:, 1] >= fl._crop[0]) & (xyz[:, 1] <= fl._crop[1])]
    rng = np.random.default_rng(3)
    lo, hi = slab.min(0), slab.max(0)
    track = [MC.pose_at(rng.uniform(lo[0], hi[0]), fl.floor_zero_level + 0.9, rng.uniform(lo[2], hi[2])) for _ in range(12)]
    upstairs = Floor("1", name="floor_1")
    upstairs.floor_zero_level, upstairs.floor_height = fl.floor_zero_level + 2.7, 2.7
    g.floors.append(upstairs)
    g.rooms += [Room("0_0", "0"), Room("1_0", "1")]
    objs = []
    for k in range(6):
        o = Object("0_0_%d" % k, "0_0")
        c = np.array([rng.uniform(lo[0], hi[0]), fl.floor_zero_level + 0.5, rng.uniform(lo[2], hi[2])])
        o.pcd = _Pcd(c + rng.normal(0, 0.05, (40, 3)))
        objs.append(o)
    up = Object("1_0_0", "1_0")
    up.pcd = _Pcd(np.array([[lo[0] + 0.5, upstairs.floor_zero_level + 0.5, lo[2] + 0.5]]))
    g.objects = objs + [up]
    far_away = np.array([hi[0] + 10.0, fl.floor_zero_level + 0.5, hi[2] + 10.0])          # this storey, ten metres off the map
    asked = [0, 1, objs[2], np.asarray(objs[3].pcd.get_center()), 6, 4, 5, far_away]
    start = track[0]
    before = g.route_to_objects(start, asked, min_clearance=0.09, poses_list=track)
    res = g.view_routes_to_objects(start, asked, min_clearance=0.09, view_range=(0.1, 2.0), prefer="look", poses_list=track)
    nav = g.floor_navigation(0)
    np_ = lambda v: v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)
    main, blk = np_(nav.maps["main_free_map"]), np_(nav.sight_blocking_map())
    assert len(res) == len(asked) and res[4]["reason"] == "other floor" and not res[4]["reachable"] and res[4]["floor_id"] == 1
    assert res[7]["reason"] == "no view" and not res[7]["reachable"] and res[7]["n_visible"] == 0 and len(res[7]["polyline"]) == 0
    here = [k for k in range(len(asked)) if k != 4]
    centres = np.array([np.asarray(o.pcd.get_center()) for o in objs] + [far_away])
    band = nav.view_band((0.1, 2.0))
    assert band == (9, 66 * 66)
    ref = VR.view_route(main, blk, nav.cells_of(start[:3, 3])[0], nav.cells_of(centres), band[0], band[1], 1, min_clearance=nav.clearance_units(0.09))
    assert sum(res[k]["reachable"] for k in here) >= 1
    for j, k in enumerate(here):
        r = res[k]
        assert r["floor_id"] == 0 and r["reachable"] == (ref["goal_dist"][j] != U) and r["cell"] == tuple(ref["goal_cell"][j])
        assert r["reason"] == (None if r["reachable"] else "no view") and r["n_visible"] == ref["n_visible"][j]
        cells = nav.cells_of(r["polyline"])
        assert np.array_equal(cells, ref["path_rc"][ref["path_off"][j]:ref["path_off"][j + 1]]) and main[cells[:, 0], cells[:, 1]].all()
        if r["reachable"]:
            assert VR.clear(blk, r["cell"], tuple(nav.cells_of(centres[j])[0])) and abs(float(np.hypot(*r["facing"])) - 1.0) < 1e-12
    none = g.view_routes_to_objects(start, asked, min_clearance=50.0, poses_list=track)       # no cell has 50 m round it: nothing is reached
    assert [r["reason"] for r in none] == ["unreachable"] * 4 + ["other floor"] + ["unreachable"] * 3
    after = g.route_to_objects(start, asked, min_clearance=0.09, poses_list=track)             # the old call answers as it did
    for a, b in zip(before, after):
        assert a["cell"] == b["cell"] and a["reason"] == b["reason"] and np.array_equal(a["polyline"], b["polyline"])
    g.floors.pop()
    g.scene.close()


VIEW_CASES = (open_room, wall_between, diagonal_wall, corners_and_edges, ties, unreached_island, clutter_map, view_route_against_the_calls)


# ------------------------------------------------------------------------------------------ how a case reaches the library
class api(NC.api):
    """tests/navroute_cases.py's api with the two calls of N8"""

    def viewpoints(self, blk, pas, goals, field=None, want_visible=False, **w):
        from holoagent_amd._lib import nav_viewpoints
        g = self._in(np.asarray(goals, np.int64).clip(-2 ** 31, 2 ** 31 - 1).reshape(-1, 2), np.int32)
        r = nav_viewpoints(self._in(blk, np.uint8), self._in(pas, np.uint8), g, field=None if field is None else self._in(field, np.int32),
                           want_visible=want_visible, lib_=self.L, **w)
        return {k: self._out(v) for k, v in r.items()}

    def view_route(self, m, blk, start, goals, want_field=False, **w):
        from holoagent_amd._lib import nav_view_route
        g = self._in(np.asarray(goals, np.int64).reshape(-1, 2), np.int32)
        r = nav_view_route(self._in(m, np.uint8), self._in(blk, np.uint8), start, g, lib_=self.L, want_field=want_field, **w)
        return {k: self._out(v) for k, v in r.items()}
