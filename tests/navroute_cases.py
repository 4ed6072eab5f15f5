"""The cases of the routing calls (include/hmsg.h, N7: hmsg_nav_clearance, hmsg_nav_distance_fields, hmsg_nav_snap_cells,
hmsg_nav_paths, hmsg_nav_route), shared by the simulator tests (tests/test_navroute.py) and the GPU tests
(tests/test_navroute_gpu.py).  A case takes `api` (api(): the wrappers of holoagent_amd._lib on one library or the other, images
handed over as numpy arrays or as device tensors, results as numpy) and compares every output with tests/navroute_reference.py by
array_equal: nothing here has a tolerance.  The cases that take the library itself (the capacity, NavigationGraph.route,
Graph.route_to_objects) are at the end."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import navroute_reference as RR

U = RR.UNREACHED
UNSUPPORTED = -3                                                          # include/hmsg.h: HMSG_ERR_UNSUPPORTED


# ------------------------------------------------------------------------------------------ maps (made once, never changed)
@functools.lru_cache(maxsize=None)
def serpentine_map(n=130):
    """every odd row blocked but one end cell, the ends alternating: one corridor a cell wide through the whole image"""
    p = np.ones((n, n), np.uint8)
    for k, r in enumerate(range(1, n, 2)):
        p[r, :] = 0
        p[r, n - 1 if k % 2 == 0 else 0] = 1
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def rooms_map(H=130, W=190, seed=5):
    """walls every 37 cells, one 4-cell door per wall segment of 8 cells or more, 3 % clutter"""
    rng = np.random.default_rng(seed)
    p = np.ones((H, W), np.uint8)
    rows, cols = list(range(37, H, 37)), list(range(37, W, 37))
    for r in rows:
        p[r, :] = 0
    for c in cols:
        p[:, c] = 0
    for r in rows:                                                        # a door in every segment of every wall
        for a, b in zip([0] + [c + 1 for c in cols], cols + [W]):
            if b - a < 8:                                                 # (a sliver at the image's edge stays closed)
                continue
            d = int(rng.integers(a + 1, b - 5))
            p[r, d:d + 4] = 1
    for c in cols:
        for a, b in zip([0] + [r + 1 for r in rows], rows + [H]):
            if b - a < 8:
                continue
            d = int(rng.integers(a + 1, b - 5))
            p[d:d + 4, c] = 1
    p[rng.random((H, W)) < 0.03] = 0
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def random_map(H=97, W=131, seed=8, blocked=0.35):
    p = (np.random.default_rng(seed).random((H, W)) >= blocked).astype(np.uint8)
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def ref_graph(which, w_straight=5, w_diag=7):
    return RR.grid_graph({"rooms": rooms_map, "serpentine": serpentine_map, "random": random_map, "rooms_large": lambda: rooms_map(500, 700, 6)}[which](),
                         w_straight, w_diag)


def first_free(p, near=(0, 0)):
    return tuple(int(v) for v in RR.snap(p, [near])[0][0])


def check_fields(api, p, sets, what="", graph=None, **w):
    got, reached = api.fields(p, sets, **w)
    assert got.dtype == np.int32 and got.shape == (len(sets),) + p.shape and reached.dtype == np.int64, what
    refs = []
    for k, s in enumerate(sets):
        ref, n = RR.field(p, s, graph=graph, **w)
        assert np.array_equal(got[k], ref), (what, k, int((got[k] != ref).sum()))
        assert reached[k] == n, (what, k)
        refs.append(ref)
    return got, refs


# ------------------------------------------------------------------------------------------ fields
def tiny_and_thin(api):
    for v, want in ((1, 0), (0, U)):
        got, _ = check_fields(api, np.array([[v]], np.uint8), [[(0, 0)]], "1 x 1")
        assert got[0, 0, 0] == want
    line = np.ones((1, 200), np.uint8)
    line[0, 100] = 0
    got, _ = check_fields(api, line, [[(0, 0)], [(0, 199)], [(0, 100)]], "1 x 200")
    assert got[0, 0, 99] == 99 * 5 and got[0, 0, 101] == U and got[1, 0, 101] == 98 * 5 and (got[2] == U).all()
    got, _ = check_fields(api, np.ascontiguousarray(line.T), [[(0, 0)], [(199, 0)]], "200 x 1")
    assert got[0, 99, 0] == 99 * 5 and got[0, 101, 0] == U


def corner_rule(api):
    for m, want in (([[1, 0], [0, 1]], U), ([[1, 1], [0, 1]], 10), ([[1, 1], [1, 1]], 7)):
        got, _ = check_fields(api, np.array(m, np.uint8), [[(0, 0)]], "2 x 2 %r" % (m,))
        assert got[0, 1, 1] == want, (m, got[0])


def open_grids(api):
    """no obstacle: tile edges at 63 / 64 / 65, the source in each corner and on both sides of the seam"""
    for H, W in ((63, 129), (64, 64), (65, 65), (128, 128)):
        p = np.ones((H, W), np.uint8)
        srcs = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (min(63, H - 1), min(63, W - 1)), (min(64, H - 1), min(64, W - 1))]
        got, _ = check_fields(api, p, [[s] for s in srcs], "open %d x %d" % (H, W))
        rr, cc = np.mgrid[:H, :W]
        dr, dc = np.abs(rr - srcs[4][0]), np.abs(cc - srcs[4][1])                    # the closed form of an open grid
        assert np.array_equal(got[4], 7 * np.minimum(dr, dc) + 5 * np.abs(dr - dc))


def doors_on_seams(api):
    """a full wall with one door cell on a tile seam; the same wall whose only opening is diagonal, which R1 closes"""
    H = W = 130
    for axis, at in ((0, 63), (0, 64), (1, 63), (1, 64)):
        p = np.ones((H, W), np.uint8)
        if axis == 0:
            p[at, :] = 0
            p[at, 64] = 1
        else:
            p[:, at] = 0
            p[64, at] = 1
        got, _ = check_fields(api, p, [[(0, 0)], [(H - 1, W - 1)]], "door %d %d" % (axis, at))
        assert got[0, H - 1, W - 1] != U
    for at in (63, 64):
        p = np.ones((H, W), np.uint8)
        p[at, :] = 0
        p[at + 1, :] = 0
        p[at, 63] = 1                                                     # two openings that touch by their corners only
        p[at + 1, 64] = 1
        got, _ = check_fields(api, p, [[(0, 0)]], "diagonal opening %d" % at)
        assert got[0, at, 63] != U and got[0, at + 1, 64] == U and (got[0, at + 2:] == U).all()


def serpentine(api):
    """the 130 x 130 serpentine: 8515 passable cells, the farthest 42570 away, the seams crossed more than a hundred times"""
    p = serpentine_map()
    assert int(p.sum()) == 8515
    got, refs = check_fields(api, p, [[(0, 0)]], "serpentine", graph=ref_graph("serpentine"))
    assert got[0][p != 0].max() == 42570 and (got[0][p != 0] != U).all()
    rounds, trips = api.last()
    print("serpentine: relaxation rounds", rounds, "host round trips", trips)
    assert rounds >= 1 and trips >= 1
    far = np.argwhere(got[0] == 42570)[0]
    off, rc = api.paths(p, got[0], [far])
    roff, rrc = RR.paths(p, refs[0], [far])
    assert np.array_equal(off, roff) and np.array_equal(rc, rrc) and len(rc) == 8515
    check_walk(p, got[0], rc, 5, 7)


def source_sets(api):
    p = rooms_map()
    g = ref_graph("rooms")
    a, b = first_free(p, (10, 10)), first_free(p, (10, 30))
    got, refs = check_fields(api, p, [[a, b], [a, a, b, a], [a]], "two sources, duplicates", graph=g)
    assert ((refs[0] != U) & (RR.field(p, [a], graph=g)[0] == RR.field(p, [b], graph=g)[0])).sum() > 0      # cells equidistant from both
    assert np.array_equal(got[0], got[1])
    blocked = tuple(int(v) for v in np.argwhere(p == 0)[7])
    got, _ = check_fields(api, p, [[blocked], [], [blocked, a]], "a source on a blocked cell, an empty set", graph=g)
    assert (got[0] == U).all() and (got[1] == U).all() and np.array_equal(got[2], refs[2])


def batch_against_single_calls(api):
    p = rooms_map()
    g = ref_graph("rooms")
    free = np.argwhere(p != 0)
    sets = [free[:1], free[100:103], free[[5, 5000, 9000, 12000, 20000]], np.zeros((0, 2), np.int64), free[-2:]]
    got, _ = check_fields(api, p, sets, "batch", graph=g)
    for k, s in enumerate(sets):
        one, n = api.fields(p, [s])
        assert np.array_equal(one[0], got[k]), k


def weights(api):
    p = random_map()
    for ws, wd in ((5, 7), (2, 3), (1, 1), (1, 2)):
        check_fields(api, p, [[first_free(p), first_free(p, (96, 130))]], "weights %d %d" % (ws, wd), w_straight=ws, w_diag=wd)


def random_blocked(api):
    """35 % blocked at random, three sources: the reference alone leaves passable cells unreached and reaches more than half"""
    p = random_map()
    srcs = [first_free(p, (48, 65)), first_free(p, (5, 5)), first_free(p, (90, 120))]
    ref, n = RR.field(p, srcs, graph=ref_graph("random"))
    assert int(p.sum()) / 2 < n < int(p.sum())
    check_fields(api, p, [srcs], "random", graph=ref_graph("random"))


def rooms_and_doors(api):
    p = rooms_map()
    ref, n = RR.field(p, [first_free(p)], graph=ref_graph("rooms"))
    assert n > 0.99 * int(p.sum())
    check_fields(api, p, [[first_free(p)], [first_free(p, (129, 189))]], "rooms", graph=ref_graph("rooms"))
    rounds, trips = api.last()
    print("rooms 130 x 190: relaxation rounds", rounds, "host round trips", trips)


def rooms_large(api):
    """the same generator at 500 x 700 (the GPU module only)"""
    p = rooms_map(500, 700, 6)
    check_fields(api, p, [[first_free(p)]], "rooms 500 x 700", graph=ref_graph("rooms_large"))
    rounds, trips = api.last()
    print("rooms 500 x 700: relaxation rounds", rounds, "host round trips", trips)


def refusals(api, L):
    from holoagent_amd._lib import HmsgError, HmsgRouteParams, _ptr
    p = np.ones((4, 5), np.uint8)
    for kw in (dict(w_straight=0), dict(w_straight=5, w_diag=4), dict(w_straight=-1, w_diag=7)):
        with pytest.raises(HmsgError):
            api.fields(p, [[(0, 0)]], **kw)
        with pytest.raises(HmsgError):
            api.clearance(p, **kw)
    for bad in ((4, 0), (0, 5), (-1, 0), (0, -1)):
        with pytest.raises(HmsgError):
            api.fields(p, [[(0, 0), bad]])
    with pytest.raises(HmsgError):                                        # decreasing src_off
        api.fields(p, (np.array([0, 2, 1], np.int64), np.zeros((2, 2), np.int32)))
    with pytest.raises(HmsgError):
        api.route(p, (0, 0), [(1, 1)], min_clearance=-1)
    prm = HmsgRouteParams(5, 7, 0, 0)
    out, one = np.zeros(20, np.int32), np.zeros(2, np.int64)
    c = L.c
    assert c.hmsg_nav_clearance(0, 4, 5, None, C.byref(prm), _ptr(out)) == -1 and c.hmsg_nav_clearance(0, 4, 5, _ptr(p), None, _ptr(out)) == -1
    assert c.hmsg_nav_clearance(0, 4, 5, _ptr(p), C.byref(prm), None) == -1
    assert c.hmsg_nav_clearance(0, 0, 5, _ptr(p), C.byref(prm), _ptr(out)) == -1 and c.hmsg_nav_clearance(0, 4, 0, _ptr(p), C.byref(prm), _ptr(out)) == -1
    assert c.hmsg_nav_distance_fields(0, 4, 5, _ptr(p), C.byref(prm), 1, None, None, _ptr(out), None) == -1
    assert c.hmsg_nav_distance_fields(0, 4, 5, _ptr(p), C.byref(prm), 1, _ptr(one), None, None, None) == -1
    assert c.hmsg_nav_snap_cells(0, 4, 5, None, None, 0, None, None, None) == -1
    assert c.hmsg_nav_paths(0, 4, 5, _ptr(p), C.byref(prm), None, 0, None, None, None, 0, None) == -1
    assert c.hmsg_nav_route(0, 4, 5, _ptr(p), C.byref(prm), None, 0, None, None) == -1
    # the sizes that could overflow are refused before anything is read (HMSG_ERR_UNSUPPORTED)
    assert c.hmsg_nav_clearance(0, 1 << 14, 1 << 14, _ptr(p), C.byref(prm), _ptr(out)) == UNSUPPORTED
    big = HmsgRouteParams(5, 1 << 12, 0, 0)
    assert c.hmsg_nav_clearance(0, 1 << 10, 1 << 9, _ptr(p), C.byref(big), _ptr(out)) == UNSUPPORTED
    assert c.hmsg_nav_distance_fields(0, 1 << 10, 1 << 9, _ptr(p), C.byref(big), 1, _ptr(one), None, _ptr(out), None) == UNSUPPORTED


# ------------------------------------------------------------------------------------------ clearance
def clearance_cases(api):
    for H, W in ((1, 1), (7, 12), (70, 131)):
        full = np.ones((H, W), np.uint8)
        rr, cc = np.mgrid[:H, :W]
        got = api.clearance(full)
        assert got.dtype == np.int32 and np.array_equal(got, 5 * (1 + np.minimum(np.minimum(rr, H - 1 - rr), np.minimum(cc, W - 1 - cc))))
        assert np.array_equal(got, RR.clearance(full))
        assert np.array_equal(api.clearance(np.zeros((H, W), np.uint8)), np.zeros((H, W), np.int32))
    hole = np.ones((131, 140), np.uint8)
    hole[64, 63] = 0
    assert np.array_equal(api.clearance(hole), RR.clearance(hole))
    rr, cc = np.mgrid[:66, :67]
    board = ((rr + cc) % 2).astype(np.uint8)
    assert np.array_equal(api.clearance(board), RR.clearance(board)) and api.clearance(board).max() == 5
    for ws, wd in ((5, 7), (1, 1), (2, 3)):
        got = api.clearance(rooms_map(), w_straight=ws, w_diag=wd)
        assert np.array_equal(got, RR.clearance(rooms_map(), ws, wd)), (ws, wd)
    assert np.array_equal(api.clearance(rooms_map() * 255), RR.clearance(rooms_map()))         # any byte but 0 is in the mask


# ------------------------------------------------------------------------------------------ snap
def snap_cases(api):
    p = np.zeros((9, 11), np.uint8)
    p[2, 3] = p[2, 7] = p[6, 3] = p[6, 7] = 1
    t = [(2, 3), (2, 5), (4, 5), (4, 3), (-5, -5), (100, 100), (10 ** 9, -10 ** 9), (-10 ** 9, 10 ** 9), (4, 10 ** 9), (-10 ** 9, 5)]
    cells, d2 = api.snap(p, t)
    rc, rd = RR.snap(p, t)
    assert cells.dtype == np.int32 and d2.dtype == np.int64 and np.array_equal(cells, rc) and np.array_equal(d2, rd)
    assert tuple(cells[0]) == (2, 3) and d2[0] == 0                        # a target on a candidate
    assert tuple(cells[1]) == (2, 3) and d2[1] == 4                        # two-way tie: the smaller row-major index
    assert tuple(cells[2]) == (2, 3) and d2[2] == 8                        # four-way tie
    assert tuple(cells[6]) == (6, 3) and d2[6] == (6 - (1 << 20)) ** 2 + (3 + (1 << 20)) ** 2        # the clamp, int64
    cells, d2 = api.snap(np.zeros((5, 6), np.uint8), [(1, 1), (9, 9)])
    assert (cells == -1).all() and (d2 == -1).all()                        # no candidate
    rng = np.random.default_rng(3)
    p = random_map()
    t = rng.integers(-30, 160, (64, 2))
    f, _ = RR.field(p, [first_free(p, (48, 65))], graph=ref_graph("random"))
    for fld in (None, f):
        cells, d2 = api.snap(p, t, fld)
        rc, rd = RR.snap(p, t, fld)
        assert np.array_equal(cells, rc) and np.array_equal(d2, rd)
    cells, d2 = api.snap(p, t, np.full(p.shape, U, np.int32))              # a field that reaches nothing
    assert (cells == -1).all() and (d2 == -1).all()


def snap_that_only_the_field_catches(api):
    """with min_clearance 10 the rooms map falls into components; a goal whose nearest clear cell lies in another component than
    the start's must snap to a farther, reached one"""
    from scipy.ndimage import label
    m = rooms_map()
    clr = RR.clearance(m)
    pas = ((m != 0) & (clr >= 10)).astype(np.uint8)
    lab, n = label(pas, structure=np.ones((3, 3)))
    assert n > 1
    start = first_free(pas, (20, 20))
    f, reached = RR.field(pas, [start])
    assert 0 < reached < int(pas.sum())
    unreached = np.argwhere((pas != 0) & (f == U))
    goals = unreached[:: max(1, len(unreached) // 16)][:16]               # goals ON clear cells of other components
    plain, _ = RR.snap(pas, goals)
    with_field, _ = RR.snap(pas, goals, f)
    assert np.array_equal(plain, goals) and not (with_field == goals).all(axis=1).any()
    got = api.route(m, (20, 20), goals, min_clearance=10, want_field=True)
    compare_route(got, RR.route(m, (20, 20), goals, min_clearance=10))
    assert np.array_equal(got["goal_cell"], with_field) and (got["goal_d2"] > 0).all() and (got["goal_dist"] != U).all()
    assert np.array_equal(got["passable"], pas) and np.array_equal(got["field"], f)
    assert np.array_equal(api.clearance(m), clr)


# ------------------------------------------------------------------------------------------ paths
def check_walk(p, f, rc, ws, wd, off=None):
    """consecutive cells are legal moves and the weights sum to field[goal]"""
    off = np.array([0, len(rc)]) if off is None else off
    for a, b in zip(off[:-1], off[1:]):
        cells = [tuple(int(v) for v in c) for c in rc[a:b]]
        if not cells:
            continue
        assert f[cells[0]] == 0
        total = 0
        for u, v in zip(cells[:-1], cells[1:]):
            assert RR.legal(p, u, v), (u, v)
            total += wd if (u[0] != v[0] and u[1] != v[1]) else ws
        assert total == f[cells[-1]]


def path_cases(api):
    p = rooms_map()
    src = first_free(p, (60, 90))
    f, _ = RR.field(p, [src], graph=ref_graph("rooms"))
    blocked = tuple(int(v) for v in np.argwhere(p == 0)[50])
    island = np.argwhere((p != 0) & (f == U))
    rng = np.random.default_rng(4)
    reach = np.argwhere(f != U)
    goals = [src, blocked, (-1, 5), (5, -1), (130, 0), (0, 190), (10 ** 9, 0)] + [tuple(c) for c in reach[rng.integers(0, len(reach), 24)]]
    if len(island):
        goals.append(tuple(island[0]))
    off, rc = api.paths(p, f, goals)
    roff, rrc = RR.paths(p, f, goals)
    assert off.dtype == np.int64 and rc.dtype == np.int32 and np.array_equal(off, roff) and np.array_equal(rc, rrc)
    assert off[1] == 1 and tuple(rc[0]) == src and (np.diff(off)[1:7] == 0).all()
    check_walk(p, f, rc, 5, 7, off)
    # (1, 1) weights on the open 65 x 65: every shortest walk costs the same and only R5's order decides
    q = np.ones((65, 65), np.uint8)
    fq, _ = RR.field(q, [(32, 32)], 1, 1)
    goals = [(0, 0), (64, 64), (0, 64), (64, 0), (0, 32), (64, 31), (10, 50), (50, 10), (33, 33)]
    off, rc = api.paths(q, fq, goals, w_straight=1, w_diag=1)
    roff, rrc = RR.paths(q, fq, goals, 1, 1)
    assert np.array_equal(off, roff) and np.array_equal(rc, rrc)
    check_walk(q, fq, rc, 1, 1, off)
    off, rc = api.paths(q, fq, np.zeros((0, 2), np.int32), w_straight=1, w_diag=1)
    assert np.array_equal(off, [0]) and len(rc) == 0


def path_capacity_too_small(L):
    """a list that is too short: an error, the count says what is needed, the offsets are written, the list is not"""
    from holoagent_amd._lib import HmsgNavRoutes, HmsgRouteParams, _ptr
    p = np.ascontiguousarray(rooms_map())
    src = first_free(p, (60, 90))
    f, _ = RR.field(p, [src], graph=ref_graph("rooms"))
    goals = np.ascontiguousarray(np.argwhere(f != U)[::997].astype(np.int32))
    roff, rrc = RR.paths(p, f, goals)
    need, n = len(rrc), len(goals)
    prm = HmsgRouteParams(5, 7, 0, 0)
    for cap in (need - 1, 0, need):
        rc, off, cnt = np.full((max(cap, 1), 2), -7, np.int32), np.zeros(n + 1, np.int64), C.c_int64(-1)
        st = L.c.hmsg_nav_paths(0, p.shape[0], p.shape[1], _ptr(p), C.byref(prm), _ptr(f), n, _ptr(goals), _ptr(off), _ptr(rc), cap, C.byref(cnt))
        assert cnt.value == need and np.array_equal(off, roff)
        assert (st != 0 and (rc == -7).all()) if cap < need else (st == 0 and np.array_equal(rc, rrc))
        out = HmsgNavRoutes()
        rc, off, cell = np.full((max(cap, 1), 2), -7, np.int32), np.zeros(n + 1, np.int64), np.zeros((n, 2), np.int32)
        out.path_rc, out.path_capacity, out.path_off, out.goal_cell = _ptr(rc), cap, _ptr(off), _ptr(cell)
        start = np.array(src, np.int32)
        st = L.c.hmsg_nav_route(0, p.shape[0], p.shape[1], _ptr(p), C.byref(prm), _ptr(start), n, _ptr(goals), C.byref(out))
        assert out.n_path_cells == need and np.array_equal(off, roff) and np.array_equal(cell, goals) and tuple(out.start_cell) == src
        assert (st != 0 and (rc == -7).all()) if cap < need else (st == 0 and np.array_equal(rc, rrc))
    out = HmsgNavRoutes()                                                 # nothing wanted but the count
    assert L.c.hmsg_nav_route(0, p.shape[0], p.shape[1], _ptr(p), C.byref(prm), _ptr(start), n, _ptr(goals), C.byref(out)) == 0
    assert out.n_path_cells == need and out.start_d2 == 0


# ------------------------------------------------------------------------------------------ the composition
def compare_route(got, ref):
    assert got["start_cell"] == ref["start_cell"] and got["start_d2"] == ref["start_d2"]
    for k in ("goal_cell", "goal_d2", "goal_dist", "path_off", "path_rc", "passable") + (("field",) if "field" in got else ()):
        assert got[k].dtype == ref[k].dtype and np.array_equal(got[k], ref[k]), k


def route_against_the_four_calls(api):
    m = rooms_map()
    rng = np.random.default_rng(12)
    goals = np.concatenate([rng.integers(-10, 200, (40, 2)), np.argwhere(m == 0)[:5]])
    for start, minc in (((3, 3), 0), ((64, 95), 5), ((-50, 400), 10), ((64, 95), 10)):
        got = api.route(m, start, goals, min_clearance=minc, want_field=True)
        compare_route(got, RR.route(m, start, goals, min_clearance=minc))
        # ... and against the four calls of the library itself
        pas = ((m != 0) & (api.clearance(m) >= minc)).astype(np.uint8) if minc else (m != 0).astype(np.uint8)
        s, sd = api.snap(pas, [start])
        f, _ = api.fields(pas, [s])
        cell, d2 = api.snap(pas, goals, f[0])
        off, rc = api.paths(pas, f[0], cell)
        assert np.array_equal(got["passable"], pas) and got["start_cell"] == tuple(s[0]) and got["start_d2"] == sd[0]
        assert np.array_equal(got["field"], f[0]) and np.array_equal(got["goal_cell"], cell) and np.array_equal(got["goal_d2"], d2)
        assert np.array_equal(got["path_off"], off) and np.array_equal(got["path_rc"], rc)
        check_walk(pas, f[0], rc, 5, 7, off)
        assert (got["path_rc"][got["path_off"][:-1][np.diff(got["path_off"]) > 0]] == s[0]).all()       # every path starts at the start
    none = api.route(np.zeros((6, 7), np.uint8), (2, 2), [(1, 1), (3, 3)])
    assert none["start_cell"] == (-1, -1) and none["start_d2"] == -1 and (none["goal_cell"] == -1).all() and (none["goal_dist"] == U).all()
    assert np.array_equal(none["path_off"], [0, 0, 0])
    empty = api.route(m, (3, 3), np.zeros((0, 2), np.int32))
    assert len(empty["goal_cell"]) == 0 and np.array_equal(empty["path_off"], [0])


def navigation_graph_route(L, wrap=None):
    """NavigationGraph.route on a storey made as tests/navmap_cases.py makes one: cells by R6, metres to field units by ceil,
    the result against the restatement on the object's own main_free_map; the maps call gives the same bytes afterwards"""
    from holoagent_amd._lib import nav_floor_maps
    from holoagent_amd.nav_graph import NavigationGraph
    from tests import navmap_cases as NC
    pts, cols, zero, poses = NC.room(41, 3.0, 2.4, n_floor=5000, n_wall=4000, n_box=900)
    cloud = (pts, cols) if wrap is None else (wrap(pts), wrap(cols))
    before = nav_floor_maps(cloud[0], cloud[1], zero, poses, lib_=L)
    nav = NavigationGraph(cloud, 0.03, lib_=L)
    nav.get_main_free_map(None, {"floor_zero_level": zero}, None, list(poses), save=False)
    np_ = lambda v: v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)
    main = np_(nav.maps["main_free_map"])
    rng = np.random.default_rng(2)
    lo, hi = pts.min(0), pts.max(0)
    goals = np.c_[rng.uniform(lo[0] - 0.5, hi[0] + 0.5, 30), rng.uniform(0, 2, 30), rng.uniform(lo[2] - 0.5, hi[2] + 0.5, 30)]
    goals[0] = (lo[0], 0.3, lo[2])                                        # exactly on the grid's origin: cell (0, 0)
    goals[1] = (lo[0] - 1e-9, 0.3, lo[2] + 0.03 * 7)                      # a hair outside: floor gives column -1, truncation would give 0
    start = np.array([poses[0][0, 3], 0.8, poses[0][2, 3]])
    cells = nav.cells_of(goals)
    assert tuple(cells[0]) == (0, 0) and cells[1, 1] == -1
    assert np.array_equal(cells, np.floor((goals[:, [2, 0]] - nav.pcd_min[[2, 0]]) / 0.03).astype(np.int32))
    assert np.array_equal(np_(nav.clearance_map()), RR.clearance(main))
    for metres, units in ((0.0, 0), (0.25, 42), (0.06, 10), (0.061, 11)):
        assert nav.clearance_units(metres) == units
        got = nav.route(start, goals, min_clearance_m=metres)
        ref = RR.route(main, nav.cells_of(start)[0], cells, min_clearance=units)
        compare_route({k: v for k, v in nav.last_route.items() if k != "field"}, ref)
        assert np.array_equal(np_(nav.passable_map(metres)), ref["passable"])
        assert ref["start_cell"] != (-1, -1)
        assert np.array_equal(np_(nav.distance_field(np.array([ref["start_cell"]]), metres)), ref["field"])
        inside = np.array([lo[0] + 1.0, 0.0, lo[2] + 1.0])                  # a world point: its cell by R6, a source as it is (no snap)
        assert np.array_equal(np_(nav.distance_field(inside, metres)), RR.field(ref["passable"], [nav.cells_of(inside)[0]])[0])
        assert len(got) == 30 and any(r["reachable"] for r in got)
        for k, r in enumerate(got):
            a, b = ref["path_off"][k], ref["path_off"][k + 1]
            assert r["reachable"] == (ref["goal_dist"][k] != U) and r["cell"] == tuple(ref["goal_cell"][k]) and len(r["polyline"]) == b - a
            if r["reachable"]:
                row, col = r["cell"]
                assert np.array_equal(r["point"], [(col + 0.5) * 0.03 + nav.pcd_min[0], nav.pcd_min[1], (row + 0.5) * 0.03 + nav.pcd_min[2]])
                assert r["length_m"] == float(ref["goal_dist"][k]) * 0.03 / 5 and np.array_equal(r["polyline"][-1], r["point"])
                assert main[row, col] and RR.clearance(main)[row, col] >= units
    after = nav_floor_maps(cloud[0], cloud[1], zero, poses, lib_=L)
    for k in NC.MAPS + ("top_down_bgr", "boundary_rc"):
        assert np.array_equal(np_(before[k]), np_(after[k])) and np.array_equal(np_(before[k]), np_(nav.maps[k])), k


def graph_route_to_objects(L, tmp_path):
    """Graph.route_to_objects on a scene built from frames: every path cell lies in main_free_map, every stand-on cell has the
    clearance asked for, a second storey's object comes back as "other floor", and create_nav_graph writes the same bytes before
    and after"""
    from holoagent_amd.graph import Floor, Object, Room, _Pcd
    from tests import navmap_cases as NC
    from tests.test_semseg_evaluate import build_graph
    g = build_graph(L)
    g.segment_floors_manually()
    assert len(g.floors) == 1 and g.scene is not None
    fl = g.floors[0]
    xyz, _ = g.scene.map_points(colors=True)
    slab = xyz[(xyz[:, 1] >= fl._crop[0]) & (xyz[:, 1] <= fl._crop[1])]
    rng = np.random.default_rng(3)
    lo, hi = slab.min(0), slab.max(0)
    track = [NC.pose_at(rng.uniform(lo[0], hi[0]), fl.floor_zero_level + 0.9, rng.uniform(lo[2], hi[2])) for _ in range(12)]
    g.create_nav_graph(nav_dir=str(tmp_path / "a"), poses_list=track)
    # objects: nodes of a room of this storey, a bare centre, and a node of a room one storey up
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
    asked = [0, 1, objs[2], np.asarray(objs[3].pcd.get_center()), 6, 4, 5]
    start = track[0]
    res = g.route_to_objects(start, asked, min_clearance=0.09, poses_list=track)
    assert g.floor_of_pose(start) == 0 and len(res) == len(asked)
    nav = g.floor_navigation(0)
    assert nav is g.floor_navigation(0, track) and nav.points is None            # made once; the storey stayed in HBM
    np_ = lambda v: v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)
    main = np_(nav.maps["main_free_map"])
    clr = RR.clearance(main)
    units = nav.clearance_units(0.09)
    assert units == 15
    assert res[4]["reason"] == "other floor" and not res[4]["reachable"] and res[4]["floor_id"] == 1 and len(res[4]["polyline"]) == 0
    here = [r for k, r in enumerate(res) if k != 4]
    centres = np.array([np.asarray(o.pcd.get_center()) for o in (objs[0], objs[1], objs[2], objs[3], objs[4], objs[5])])
    ref = RR.route(main, nav.cells_of(start[:3, 3])[0], nav.cells_of(centres), min_clearance=units)
    assert sum(r["reachable"] for r in here) >= 1
    for k, r in enumerate(here):
        assert r["floor_id"] == 0 and r["reachable"] == (ref["goal_dist"][k] != U) and r["cell"] == tuple(ref["goal_cell"][k])
        assert r["reason"] == (None if r["reachable"] else "unreachable")
        cells = nav.cells_of(r["polyline"])
        assert np.array_equal(cells, ref["path_rc"][ref["path_off"][k]:ref["path_off"][k + 1]])
        assert main[cells[:, 0], cells[:, 1]].all()
        if r["reachable"]:
            assert clr[r["cell"]] >= units and r["length_m"] == float(ref["goal_dist"][k]) * 0.03 / 5
    g.floors.pop()
    g.create_nav_graph(nav_dir=str(tmp_path / "b"), poses_list=track)
    for name in ("sparse_voronoi_graph.json", "global_nav_graph_graph.json"):
        assert open(tmp_path / "a" / name, "rb").read() == open(tmp_path / "b" / name, "rb").read(), name
    g.scene.close()


FIELD_CASES = (tiny_and_thin, corner_rule, open_grids, doors_on_seams, serpentine, source_sets, batch_against_single_calls, weights,
               random_blocked, rooms_and_doors)
OTHER_CASES = (clearance_cases, snap_cases, snap_that_only_the_field_catches, path_cases, route_against_the_four_calls)
ALL = FIELD_CASES + OTHER_CASES


# ------------------------------------------------------------------------------------------ how a case reaches the library
class api:
    """the wrappers of holoagent_amd._lib on library L; wrap: how an image is handed over (a device tensor), results as numpy"""

    def __init__(self, L, wrap=None):
        self.L, self.wrap = L, wrap

    def _in(self, a, dtype):
        a = np.ascontiguousarray(np.asarray(a, dtype))
        return a if self.wrap is None else self.wrap(a)

    @staticmethod
    def _out(v):
        return v.cpu().numpy() if hasattr(v, "cpu") else v

    def clearance(self, mask, **w):
        from holoagent_amd._lib import nav_clearance
        return self._out(nav_clearance(self._in(mask, np.uint8), lib_=self.L, **w))

    def fields(self, p, sets, **w):
        from holoagent_amd._lib import nav_distance_fields
        f, n = nav_distance_fields(self._in(p, np.uint8), sets, lib_=self.L, **w)
        return self._out(f), self._out(n)

    def snap(self, p, targets, field=None):
        from holoagent_amd._lib import nav_snap_cells
        t = self._in(np.asarray(targets, np.int64).clip(-2 ** 31, 2 ** 31 - 1).reshape(-1, 2), np.int32)
        c, d = nav_snap_cells(self._in(p, np.uint8), t, None if field is None else self._in(field, np.int32), lib_=self.L)
        return self._out(c), self._out(d)

    def paths(self, p, field, goals, **w):
        from holoagent_amd._lib import nav_paths
        g = self._in(np.asarray(goals, np.int64).clip(-2 ** 31, 2 ** 31 - 1).reshape(-1, 2), np.int32)
        off, rc = nav_paths(self._in(p, np.uint8), self._in(field, np.int32), g, lib_=self.L, **w)
        return self._out(off), self._out(rc)

    def route(self, m, start, goals, want_field=False, **w):
        from holoagent_amd._lib import nav_route
        g = self._in(np.asarray(goals, np.int64).reshape(-1, 2), np.int32)
        r = nav_route(self._in(m, np.uint8), start, g, lib_=self.L, want_field=want_field, **w)
        return {k: self._out(v) for k, v in r.items()}

    def last(self):
        a, b = C.c_int32(0), C.c_int32(0)
        self.L.c.hmsg_test_nav_route_last(C.byref(a), C.byref(b))
        return a.value, b.value
