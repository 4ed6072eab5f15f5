"""The cases of the calls that route across storeys (include/hmsg.h, N9: hmsg_nav_seeded_fields, hmsg_nav_building_fields,
hmsg_nav_building_paths, hmsg_nav_building_route), shared by the simulator tests (tests/test_navbuilding.py) and the GPU tests
(tests/test_navbuilding_gpu.py).  A case takes `api` (the wrappers of holoagent_amd._lib on one library or the other, images handed
over as numpy arrays or as device tensors, results as numpy) and compares every output with tests/navbuilding_reference.py by
array_equal: nothing here has a tolerance.  Every case also checks its own reference: along each reference path every consecutive
pair is a legal R1 move or a link and the costs add up to the field at the goal.  The cases that take the library itself (the
refusals, the capacity, BuildingNavigation, Graph.route_across_floors) are at the end."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import navbuilding_reference as RB
from tests import navroute_cases as NC
from tests import navroute_reference as RR

U = RR.UNREACHED
UNSUPPORTED = -3                                                          # include/hmsg.h: HMSG_ERR_UNSUPPORTED


# ------------------------------------------------------------------------------------------ maps (made once, never changed)
@functools.lru_cache(maxsize=None)
def cluttered(H, W, seed, blocked=0.12):
    p = (np.random.default_rng(seed).random((H, W)) >= blocked).astype(np.uint8)
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def two_rooms(door=False, H=70, W=90):
    """two rooms with a solid wall between them at column 45; door: one opening in the wall's last row, a long way round"""
    p = np.ones((H, W), np.uint8)
    p[:, 45] = 0
    if door:
        p[H - 1, 45] = 1
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def open_map(H=130, W=67):
    p = np.ones((H, W), np.uint8)
    p.setflags(write=False)
    return p


def check_building(api, passables, links, starts, goals=None, what="", **w):
    """fields and n_reached of every start against the reference; the paths of the first start to `goals` too -> (got, refs, B)"""
    B = RB.Building(passables, links, w.get("w_straight", 5), w.get("w_diag", 7))
    got, reached = api.fields(passables, links, starts, **w)
    assert len(got) == len(passables) and reached.dtype == np.int64 and reached.shape == (len(starts), len(passables)), what
    refs = []
    for k, s in enumerate(starts):
        ref, n = B.fields(s)
        for l in range(len(passables)):
            assert got[l].dtype == np.int32 and got[l].shape == (len(starts),) + passables[l].shape, what
            assert np.array_equal(got[l][k], ref[l]), (what, k, l, int((got[l][k] != ref[l]).sum()))
        assert np.array_equal(reached[k], n), (what, k, reached[k], n)
        refs.append(ref)
    if goals is not None:
        roff, rsrc = B.paths(refs[0], goals)
        B.check_walk(refs[0], roff, rsrc)
        off, src = api.paths(passables, links, [f[0] for f in got], goals, **w)
        assert off.dtype == np.int64 and src.dtype == np.int32 and np.array_equal(off, roff) and np.array_equal(src, rsrc), what
    return got, refs, B


def storeys_of(B, fields, goal):
    return [c[0] for c in B.path(fields, goal)]


# ------------------------------------------------------------------------------------------ building fields and paths
def one_link(api):
    """two storeys of different, odd shapes and one link; a start on each storey"""
    p0, p1 = cluttered(70, 90, 1), cluttered(130, 67, 2)
    a, b = NC.first_free(p0, (30, 40)), NC.first_free(p1, (100, 20))
    links = [(0,) + a + (1,) + b + (23,)]
    goals = [(0, 3, 3), (1, 5, 60), (1, 129, 66), (0, 69, 89), (1,) + b, (0,) + a, (1, -1, 4), (0, 70, 0)]
    s0, s1 = (0,) + NC.first_free(p0, (2, 2)), (1,) + NC.first_free(p1, (120, 60))
    got, refs, B = check_building(api, [p0, p1], links, [s0], goals, "one link, from below")
    assert refs[0][1][b] == refs[0][0][a] + 23 and (refs[0][1] != U).sum() > 0.8 * p1.sum()
    check_building(api, [p0, p1], links, [s1], goals, "one link, from above")


def up_across_and_down(api):
    """storey 0 is two rooms with a solid wall between them, storey 1 is open, one link in each room: the far room's field exists
    only through two links.  With the storeys listed in both index orders: no sweep that visits the storeys once in order gets both"""
    rooms, top = two_rooms(), open_map()
    for order in (0, 1):
        r_, t_ = (0, 1) if order == 0 else (1, 0)
        passables = [rooms, top] if order == 0 else [top, rooms]
        links = [(r_, 10, 10, t_, 5, 5, 13), (t_, 120, 60, r_, 60, 80, 17)]
        start = (r_, 35, 20)
        goals = [(r_, 5, 85), (r_, 69, 46), (t_, 64, 33), (r_, 35, 44)]
        got, refs, B = check_building(api, passables, links, [start], goals, "up, across and down %d" % order)
        far = refs[0][r_][:, 46:]
        assert (far != U).all() and (refs[0][r_][:, 45] == U).all()
        assert set(storeys_of(B, refs[0], goals[0])) == {0, 1}
        ways = storeys_of(B, refs[0], goals[0])
        assert sum(a != b for a, b in zip(ways[:-1], ways[1:])) == 2         # up once and down once


def over_the_top(api):
    """the same scene with a door at the far end of the wall: with cheap links the way over the top is shorter, with dear ones
    the door is -- and the reference takes different ways in the two variants"""
    rooms, top = two_rooms(door=True), open_map()
    start, goal = (0, 2, 20), (0, 2, 70)
    seen = []
    for cost in (13, 400):
        links = [(0, 10, 10, 1, 5, 5, cost), (1, 5, 50, 0, 10, 80, cost)]
        got, refs, B = check_building(api, [rooms, top], links, [start], [goal, (1, 100, 30), (0, 69, 45)], "over the top, cost %d" % cost)
        seen.append(set(storeys_of(B, refs[0], goal)))
    assert seen == [{0, 1}, {0}]


def three_storeys_in_a_chain(api):
    p = [cluttered(67, 70, 3), cluttered(70, 90, 4), cluttered(90, 65, 5)]
    a0, a1 = NC.first_free(p[0], (60, 60)), NC.first_free(p[1], (5, 5))
    b1, b2 = NC.first_free(p[1], (65, 85)), NC.first_free(p[2], (40, 30))
    links = [(1,) + b1 + (2,) + b2 + (31,), (0,) + a0 + (1,) + a1 + (29,)]
    start = (2,) + NC.first_free(p[2], (88, 2))
    goals = [(0, 1, 1), (0, 66, 69), (1, 35, 45), (2, 0, 64)]
    got, refs, B = check_building(api, p, links, [start], goals, "three storeys")
    assert storeys_of(B, refs[0], (0,) + NC.first_free(p[0], (1, 1)))[0] == 2 and (refs[0][0] != U).sum() > 0.8 * p[0].sum()
    ways = storeys_of(B, refs[0], (0,) + NC.first_free(p[0], (1, 1)))
    assert [l for k, l in enumerate(ways) if k == 0 or ways[k - 1] != l] == [2, 1, 0]


def parallel_links(api):
    """two links between the storeys at different total cost: the cheaper one makes the field.  An exact tie at an isolated cell
    upstairs: B5 takes the first link in index order, whichever way round the link is written"""
    low = open_map(20, 30)
    up = np.zeros((9, 11), np.uint8)
    up[4, 5] = 1                                                          # X: no neighbour to step to, only links
    up[0, :3] = 1
    S, A, Bc, X = (0, 10, 10), (0, 10, 12), (0, 10, 14), (1, 4, 5)         # field[A] = 10, field[B] = 20
    for links, via in (([A + X + (30,), Bc + X + (20,)], A), ([Bc + X + (20,), A + X + (30,)], Bc), ([X + Bc + (20,), A + X + (30,)], Bc),
                       ([A + X + (31,), Bc + X + (20,)], Bc), ([A + X + (30,), Bc + X + (21,)], A)):
        got, refs, B = check_building(api, [low, up], links, [S], [X, (1, 0, 0)], "parallel links %r" % (links,))
        assert refs[0][1][4, 5] == 40 and B.path(refs[0], X)[-2] == via and (refs[0][1][0] == U).all()
    # two links into one open storey, the dearer one nearer to the goal
    top = open_map(70, 67)
    links = [(0, 2, 2, 1, 2, 2, 50), (0, 2, 27, 1, 2, 60, 11)]
    check_building(api, [low, top], links, [(0, 2, 3)], [(1, 2, 2), (1, 2, 30), (1, 69, 66)], "two ways up")


def links_that_do_not_exist_or_do_not_win(api):
    rooms, top, lone = two_rooms(), open_map(), cluttered(40, 45, 6)
    wall = (0, 20, 45)                                                    # not passable
    base = [(0, 10, 10, 1, 5, 5, 13)]
    start = (0, 35, 20)
    got, refs, B = check_building(api, [rooms, top, lone], base, [start], [(2, 5, 5), (1, 5, 5)], "a storey with no link")
    assert (refs[0][2] == U).all() and (refs[0][0][:, 46:] == U).all()
    reached = api.fields([rooms, top, lone], base, [start])[1]
    assert reached[0, 2] == 0 and reached[0, 1] == top.size
    # a link with an endpoint that is not passable: the same as without it, at either end
    for dead in (wall + (1, 100, 60, 1), (1, 100, 60) + wall + (1,), (0, 60, 80) + wall + (1,)):
        g2, _, _ = check_building(api, [rooms, top, lone], base + [dead], [start], [(0, 60, 80)], "a link on a wall")
        for l in range(3):
            assert np.array_equal(g2[l], got[l])
    # a same-storey link (a door the map does not show) opens the far room; a link from a cell to itself changes nothing
    door = (0, 30, 44, 0, 30, 46, 9)
    g3, r3, B3 = check_building(api, [rooms, top, lone], base + [door], [start], [(0, 60, 80), (0, 30, 46)], "a same-storey link")
    assert (r3[0][0][:, 46:] != U).all() and r3[0][0][30, 46] == r3[0][0][30, 44] + 9
    g4, _, _ = check_building(api, [rooms, top, lone], base + [(0, 12, 12, 0, 12, 12, 1), (1, 7, 7, 1, 7, 7, 3)], [start], [(1, 7, 7)], "a -> a")
    for l in range(3):
        assert np.array_equal(g4[l], got[l])
    # a start on a cell that is not passable: nothing anywhere
    g5, r5, _ = check_building(api, [rooms, top, lone], base + [door], [wall], [(0, 1, 1)], "a start on a wall")
    assert all((f == U).all() for f in g5)


def links_at_tile_seams(api):
    """link endpoints on both sides of the 64-cell seams and in the last row and column.  Upstairs the tile (0, 0) holds ONE passable
    cell, (63, 63), where a link arrives: nothing changes in that tile, so only the link's own stamps wake the three tiles round
    the corner"""
    low = open_map(130, 130)
    up = np.ones((130, 131), np.uint8)
    up[:64, :64] = 0
    up[63, 63] = 1
    for a, b in (((63, 63), (63, 63)), ((64, 64), (63, 63)), ((63, 64), (64, 64)), ((129, 129), (129, 130)), ((0, 129), (63, 64)),
                 ((129, 0), (64, 63)), ((64, 63), (0, 130))):
        links = [(0,) + a + (1,) + b + (7,)]
        goals = [(1, 129, 130), (1, 64, 64), (1, 0, 64), (1, 63, 63), (0, 129, 129)]
        got, refs, B = check_building(api, [low, up], links, [(0, 70, 3)], goals, "seam %r %r" % (a, b))
        assert (refs[0][1][up != 0] != U).all()
    # ... and the other way round: the start upstairs on the lone cell, the links' far ends on the seams downstairs
    links = [(1, 63, 63, 0, 63, 64, 3), (1, 129, 130, 0, 129, 129, 3)]
    check_building(api, [low, up], links, [(1, 63, 63), (1, 129, 0)], [(0, 0, 0), (0, 64, 64)], "seams, from above")


def serpentine_upstairs(api):
    """the 130 x 130 serpentine is the upper storey, entered by a link: hundreds of rounds after the link fires, no cap may show"""
    low, up = open_map(20, 30), NC.serpentine_map()
    links = [(0, 19, 29, 1, 0, 0, 40)]
    got, refs, B = check_building(api, [low, up], links, [(0, 0, 0)], [(1, 129, 0), (1, 128, 129)], "serpentine upstairs")
    f = refs[0][1]
    assert f[0, 0] == 19 * 7 + 10 * 5 + 40 and f[up != 0].max() == f[0, 0] + 42570 and (f[up != 0] != U).all()
    rounds, trips = api.last()
    print("serpentine upstairs: rounds", rounds, "host round trips", trips)
    # 65 corridor rows, every other one walked against the order in which a launch runs its tiles: a round carries the front at
    # most one corridor row further, so more rounds than the largest batch (32) holds and more than the first three batches
    assert rounds > 32 and 4 <= trips <= rounds


def batches_and_weights(api):
    """three starts in one call equal three calls of one start; weights (1, 1) and (5, 7)"""
    p = [cluttered(70, 90, 1), cluttered(130, 67, 2), two_rooms()]
    links = [(0,) + NC.first_free(p[0], (30, 40)) + (1,) + NC.first_free(p[1], (100, 20)) + (23,),
             (1,) + NC.first_free(p[1], (3, 3)) + (2, 60, 80, 5), (2, 10, 10, 0) + NC.first_free(p[0], (60, 5)) + (2,)]
    starts = [(0,) + NC.first_free(p[0], (2, 2)), (2, 35, 20), (1,) + NC.first_free(p[1], (64, 33))]
    for ws, wd in ((5, 7), (1, 1)):
        got, refs, B = check_building(api, p, links, starts, [(2, 5, 85), (0, 69, 89), (1, 129, 0)], "batch %d %d" % (ws, wd), w_straight=ws,
                                      w_diag=wd)
        for k, s in enumerate(starts):
            one, n1 = api.fields(p, links, [s], w_straight=ws, w_diag=wd)
            for l in range(3):
                assert np.array_equal(one[l][0], got[l][k]), (k, l)
    none, n0 = api.fields(p, links, np.zeros((0, 3), np.int32))
    assert [f.shape for f in none] == [(0,) + m.shape for m in p] and n0.shape == (0, 3)


# ------------------------------------------------------------------------------------------ B1
def check_seeded(api, p, sets, what="", graph=None, **w):
    got, reached = api.seeded(p, sets, **w)
    assert got.dtype == np.int32 and got.shape == (len(sets),) + p.shape and reached.dtype == np.int64, what
    for k, (cells, costs) in enumerate(sets):
        ref, n = RB.seeded_field(p, cells, costs, graph=graph, **w)
        assert np.array_equal(got[k], ref), (what, k, int((got[k] != ref).sum()))
        assert reached[k] == n, (what, k)
    return got


def seeded_fields(api):
    p = NC.rooms_map()
    g = NC.ref_graph("rooms")
    a, b, c = NC.first_free(p, (10, 10)), NC.first_free(p, (10, 30)), NC.first_free(p, (120, 180))
    blocked = tuple(int(v) for v in np.argwhere(p == 0)[7])
    fa = RR.field(p, [a], graph=g)[0]
    # duplicates with different costs on one cell; a seed dominated by another seed's walk; a seed on a blocked cell; an empty set
    sets = [([a, a, a], [9, 4, 6]), ([a, b], [0, int(fa[b]) + 50]), ([a, b, c], [100, 3, 0]), ([blocked, a], [0, 12]), ([blocked], [0]),
            (np.zeros((0, 2), np.int64), np.zeros(0, np.int64))]
    got = check_seeded(api, p, sets, "seeds", graph=g)
    assert got[0][a] == 4 and np.array_equal(got[1], fa) and got[1][b] == fa[b] and (got[4] == U).all() and (got[5] == U).all()
    # every cost 0: hmsg_nav_distance_fields
    zero = check_seeded(api, p, [([a, b], [0, 0]), ([c], [0])], "cost 0", graph=g)
    plain, _ = NC.api(api.L, api.wrap).fields(p, [[a, b], [c]])
    assert np.array_equal(zero, plain)
    # a batch of three equals three single calls
    for k, s in enumerate(sets[:3]):
        one, _ = api.seeded(p, [s])
        assert np.array_equal(one[0], got[k]), k
    # seeds on the seams, in the last row and the last column, weights (1, 1)
    q = np.ones((130, 131), np.uint8)
    q[:64, :64] = 0
    q[63, 63] = 1
    check_seeded(api, q, [([(63, 63)], [5]), ([(64, 64), (63, 64)], [2, 9]), ([(129, 130), (129, 0), (0, 130)], [7, 0, 3])], "seams",
                 w_straight=1, w_diag=1)
    check_seeded(api, q, [([(63, 63), (129, 130)], [0, 1000])], "seams 5 7")


# ------------------------------------------------------------------------------------------ the composition
def compare_route(got, ref):
    assert got["start_cell"] == ref["start_cell"] and got["start_d2"] == ref["start_d2"]
    for k in ("goal_cell", "goal_d2", "goal_dist", "path_off", "path_src"):
        assert got[k].dtype == ref[k].dtype and np.array_equal(got[k], ref[k]), k
    for k in ("passable",) + (("fields",) if "fields" in got else ()):
        assert len(got[k]) == len(ref[k])
        for a, b in zip(got[k], ref[k]):
            assert a.dtype == b.dtype and np.array_equal(a, b), k


def route_against_its_parts(api):
    maps = [NC.rooms_map(), cluttered(70, 90, 1), two_rooms()]
    links = [(0,) + NC.first_free(maps[0], (60, 90)) + (1,) + NC.first_free(maps[1], (35, 45)) + (27,),
             (1,) + NC.first_free(maps[1], (5, 5)) + (2, 35, 20, 19), (1,) + NC.first_free(maps[1], (65, 85)) + (2, 35, 70, 19)]
    rng = np.random.default_rng(12)
    goals = np.concatenate([np.c_[rng.integers(0, 3, 30), rng.integers(-10, 200, (30, 2))], [(0,) + tuple(np.argwhere(maps[0] == 0)[3]), (2, 20, 45)]])
    plain = NC.api(api.L, api.wrap)
    for start, minc in (((0, 3, 3), 0), ((2, 35, 20), 10), ((1, -50, 400), 5)):
        got = api.route(maps, links, start, goals, min_clearance=minc, want_fields=True)
        ref, B = RB.route(maps, links, start, goals, min_clearance=minc)
        compare_route(got, ref)
        B.check_walk(ref["fields"], ref["path_off"], ref["path_src"])
        # ... and against the parts of the library itself, called one by one
        pas = [((m != 0) & (plain.clearance(m) >= minc)).astype(np.uint8) if minc else (m != 0).astype(np.uint8) for m in maps]
        s, sd = plain.snap(pas[start[0]], [start[1:]])
        f, _ = api.fields(pas, links, [(start[0],) + tuple(s[0])])
        f = [x[0] for x in f]
        cell = np.zeros((len(goals), 3), np.int32)
        d2 = np.zeros(len(goals), np.int64)
        for k, (l, r, c) in enumerate(goals):
            c2, dd = plain.snap(pas[l], [(r, c)], f[l])
            cell[k], d2[k] = (l,) + tuple(c2[0]), dd[0]
        off, src = api.paths(pas, links, f, cell)
        assert got["start_cell"] == (start[0],) + tuple(int(v) for v in s[0]) and got["start_d2"] == sd[0]
        for l in range(3):
            assert np.array_equal(got["passable"][l], pas[l]) and np.array_equal(got["fields"][l], f[l])
        assert np.array_equal(got["goal_cell"], cell) and np.array_equal(got["goal_d2"], d2)
        assert np.array_equal(got["path_off"], off) and np.array_equal(got["path_src"], src)
        assert minc or ((np.diff(off) > 0).sum() > 10 and len({int(t[0]) for t in src}) == 3)
    none = api.route([np.zeros((6, 7), np.uint8), open_map(5, 5)], [], (0, 2, 2), [(0, 1, 1), (1, 3, 3)])
    assert none["start_cell"] == (0, -1, -1) and none["start_d2"] == -1 and (none["goal_cell"][:, 1:] == -1).all() and (none["goal_dist"] == U).all()
    assert np.array_equal(none["path_off"], [0, 0, 0]) and np.array_equal(none["goal_cell"][:, 0], [0, 1])
    empty = api.route(maps, links, (0, 3, 3), np.zeros((0, 3), np.int32))
    assert len(empty["goal_cell"]) == 0 and np.array_equal(empty["path_off"], [0])


def one_storey_is_nav_route(api):
    """one storey and no links: every output equals hmsg_nav_route's, the triples carrying storey 0"""
    m = NC.rooms_map()
    rng = np.random.default_rng(12)
    goals = np.concatenate([rng.integers(-10, 200, (40, 2)), np.argwhere(m == 0)[:5]])
    plain = NC.api(api.L, api.wrap)
    for start, minc in (((3, 3), 0), ((64, 95), 10), ((-50, 400), 5)):
        one = plain.route(m, start, goals, min_clearance=minc, want_field=True)
        got = api.route([m], [], (0,) + start, np.c_[np.zeros(len(goals), np.int64), goals], min_clearance=minc, want_fields=True)
        assert got["start_cell"] == (0,) + one["start_cell"] and got["start_d2"] == one["start_d2"]
        assert np.array_equal(got["passable"][0], one["passable"]) and np.array_equal(got["fields"][0], one["field"])
        assert (got["goal_cell"][:, 0] == 0).all() and np.array_equal(got["goal_cell"][:, 1:], one["goal_cell"])
        assert np.array_equal(got["goal_d2"], one["goal_d2"]) and np.array_equal(got["goal_dist"], one["goal_dist"])
        assert np.array_equal(got["path_off"], one["path_off"]) and (got["path_src"][:, 0] == 0).all()
        assert np.array_equal(got["path_src"][:, 1:], one["path_rc"]) and len(one["path_rc"]) > 0


ALL = (one_link, up_across_and_down, over_the_top, three_storeys_in_a_chain, parallel_links, links_that_do_not_exist_or_do_not_win,
       links_at_tile_seams, serpentine_upstairs, batches_and_weights, seeded_fields, route_against_its_parts, one_storey_is_nav_route)


# ------------------------------------------------------------------------------------------ the library itself
def _building_args(maps, links, dtype=np.uint8):
    from holoagent_amd._lib import _NavBuilding
    return _NavBuilding([np.ascontiguousarray(m) for m in maps], links, dtype)


def path_capacity_too_small(L):
    """a list that is too short: an error, the count says what is needed, everything else is written, the list is not"""
    from holoagent_amd._lib import HmsgNavBuildingRoutes, HmsgRouteParams, _ptr
    maps = [two_rooms(), open_map()]
    links = [(0, 10, 10, 1, 5, 5, 13), (1, 120, 60, 0, 60, 80, 17)]
    start = (0, 35, 20)
    B = RB.Building(maps, links)
    f, _ = B.fields(start)
    goals = np.ascontiguousarray(np.array([(0, 5, 85), (1, 64, 33), (0, 35, 21), (0, 20, 45)], np.int32))
    roff, rsrc = B.paths(f, goals)
    need, n = len(rsrc), len(goals)
    b = _building_args(maps, links)
    fb = _building_args(f, None, np.int32)
    gc, _, _ = B.snap(f, goals)
    goff, gsrc = B.paths(f, gc)
    prm = HmsgRouteParams(5, 7, 0, 0)
    st = np.array(start, np.int32)
    for cap in (need - 1, 0, need):
        src, off, cnt = np.full((max(cap, 1), 3), -7, np.int32), np.zeros(n + 1, np.int64), C.c_int64(-1)
        rc = L.c.hmsg_nav_building_paths(*b.head(0), C.byref(prm), fb.ptrs, n, _ptr(goals), _ptr(off), _ptr(src), cap, C.byref(cnt))
        assert cnt.value == need and np.array_equal(off, roff)
        assert (rc != 0 and (src == -7).all()) if cap < need else (rc == 0 and np.array_equal(src, rsrc))
    assert len(gsrc) > need                                                 # (the goal on the wall is snapped off it)
    for cap in (len(gsrc) - 1, 0, len(gsrc)):
        out = HmsgNavBuildingRoutes()
        src, off, cell = np.full((max(cap, 1), 3), -7, np.int32), np.zeros(n + 1, np.int64), np.zeros((n, 3), np.int32)
        out.path_src, out.path_capacity, out.path_off, out.goal_cell = _ptr(src), cap, _ptr(off), _ptr(cell)
        rc = L.c.hmsg_nav_building_route(*b.head(0), C.byref(prm), _ptr(st), n, _ptr(goals), C.byref(out))
        assert out.n_path_cells == len(gsrc) and np.array_equal(off, goff) and np.array_equal(cell, gc) and tuple(out.start_cell) == start
        assert (rc != 0 and (src == -7).all()) if cap < len(gsrc) else (rc == 0 and np.array_equal(src[:len(gsrc)], gsrc))
    out = HmsgNavBuildingRoutes()                                          # nothing wanted but the count
    assert L.c.hmsg_nav_building_route(*b.head(0), C.byref(prm), _ptr(st), n, _ptr(goals), C.byref(out)) == 0
    assert out.n_path_cells == len(gsrc) and out.start_d2 == 0


def refusals(api, L):
    """every line of B6"""
    from holoagent_amd._lib import HmsgError, HmsgNavBuildingRoutes, HmsgRouteParams, _ptr
    p = [np.ones((4, 5), np.uint8), np.ones((3, 6), np.uint8)]
    ok = [(0, 1, 1, 1, 2, 5, 4)]
    f, _ = api.fields(p, ok, [(0, 0, 0)])
    assert f[1][0, 2, 5] == 7 + 4
    f1 = [x[0] for x in f]
    for bad in ((2, 1, 1, 1, 2, 5, 4), (0, 1, 1, -1, 2, 5, 4),             # a storey out of range
                (0, 4, 1, 1, 2, 5, 4), (0, 1, 5, 1, 2, 5, 4), (0, 1, 1, 1, 3, 5, 4), (0, 1, 1, 1, 2, 6, 4), (0, -1, 1, 1, 2, 5, 4),      # a cell outside
                (0, 1, 1, 1, 2, 5, 0), (0, 1, 1, 1, 2, 5, -3)):            # a cost < 1
        with pytest.raises(HmsgError):
            api.fields(p, [bad], [(0, 0, 0)])
        with pytest.raises(HmsgError):
            api.paths(p, ok + [bad], f1, [(0, 0, 0)])
        with pytest.raises(HmsgError):
            api.route(p, [bad], (0, 0, 0), [(1, 1, 1)])
    for bad in ((2, 0, 0), (-1, 0, 0), (0, 4, 0), (0, 0, 5), (1, 3, 0), (1, 0, -1)):           # a start: its storey, its cell
        with pytest.raises(HmsgError):
            api.fields(p, ok, [(0, 0, 0), bad])
    for bad in ((2, 0, 0), (-1, 0, 0)):                                   # a goal's storey (its cell may lie anywhere: R5, B4)
        with pytest.raises(HmsgError):
            api.paths(p, ok, f1, [bad])
        with pytest.raises(HmsgError):
            api.route(p, ok, (0, 0, 0), [bad])
        with pytest.raises(HmsgError):
            api.route(p, ok, bad, [(0, 0, 0)])
    for kw in (dict(w_straight=0), dict(w_straight=5, w_diag=4)):
        with pytest.raises(HmsgError):
            api.fields(p, ok, [(0, 0, 0)], **kw)
        with pytest.raises(HmsgError):
            api.seeded(p[0], [([(0, 0)], [0])], **kw)
    with pytest.raises(HmsgError):
        api.route(p, ok, (0, 0, 0), [(1, 1, 1)], min_clearance=-1)
    for cells, costs in (([(4, 0)], [0]), ([(0, 5)], [0]), ([(-1, 0)], [0]), ([(0, 0)], [-1])):        # a seed outside, a cost < 0
        with pytest.raises(HmsgError):
            api.seeded(p[0], [([(0, 0)] + cells, [0] + costs)])
    with pytest.raises(HmsgError):                                        # decreasing seed_off
        api.seeded(p[0], (np.array([0, 2, 1], np.int64), np.zeros((2, 2), np.int32), np.zeros(2, np.int32)))
    # the limits on the counts, and null pointers
    b = _building_args(p, ok)
    prm = HmsgRouteParams(5, 7, 0, 0)
    st, out, cnt = np.zeros(3, np.int32), [np.zeros((1, 4, 5), np.int32), np.zeros((1, 3, 6), np.int32)], C.c_int64(0)
    outp = b.pointers(out)
    head = b.head(0)
    assert L.c.hmsg_nav_building_fields(*head, C.byref(prm), 1, _ptr(st), outp, None) == 0
    assert L.c.hmsg_nav_building_fields(head[0], 0, *head[2:], C.byref(prm), 1, _ptr(st), outp, None) == -1
    assert L.c.hmsg_nav_building_fields(head[0], 257, *head[2:], C.byref(prm), 1, _ptr(st), outp, None) == -1
    assert L.c.hmsg_nav_building_fields(*head[:5], 1 << 20, head[6], C.byref(prm), 1, _ptr(st), outp, None) == -1
    assert L.c.hmsg_nav_building_fields(*head[:5], -1, head[6], C.byref(prm), 1, _ptr(st), outp, None) == -1
    assert L.c.hmsg_nav_building_fields(*head[:5], 1, None, C.byref(prm), 1, _ptr(st), outp, None) == -1
    assert L.c.hmsg_nav_building_fields(*head, None, 1, _ptr(st), outp, None) == -1
    assert L.c.hmsg_nav_building_fields(*head, C.byref(prm), 1, None, outp, None) == -1
    assert L.c.hmsg_nav_building_fields(*head, C.byref(prm), 1, _ptr(st), None, None) == -1
    assert L.c.hmsg_nav_building_fields(*head[:4], None, *head[5:], C.byref(prm), 1, _ptr(st), outp, None) == -1
    assert L.c.hmsg_nav_building_paths(*head, C.byref(prm), outp, 0, None, None, None, 0, None) == -1
    assert L.c.hmsg_nav_building_route(*head, C.byref(prm), _ptr(st), 0, None, None) == -1
    assert L.c.hmsg_nav_building_route(*head, C.byref(prm), None, 0, None, C.byref(HmsgNavBuildingRoutes())) == -1
    assert L.c.hmsg_nav_seeded_fields(0, 4, 5, None, C.byref(prm), 1, _ptr(np.zeros(2, np.int64)), None, None, _ptr(out[0]), None) == -1
    # the overflow bound, by costs alone on a tiny map: 7 * (20 + 18) + the costs must stay below 2^31
    room = (1 << 31) - 7 * 38
    for costs, want in (((room - 1,), 0), ((room,), UNSUPPORTED), ((room - 5, 4), 0), ((room - 5, 5), UNSUPPORTED), ((1 << 30, 1 << 30), UNSUPPORTED)):
        lk = np.ascontiguousarray(np.array([(0, 1, 1, 1, 2, 5, c) for c in costs], np.int32))
        rc = L.c.hmsg_nav_building_fields(*head[:5], len(lk), _ptr(lk), C.byref(prm), 1, _ptr(st), outp, None)
        assert rc == want, (costs, rc)
        if rc == 0 and len(costs) == 1:
            assert out[1][0, 2, 5] == 7 + costs[0]
    # ... and for B1: max seed cost + rows * cols * w_diag
    q = np.ones((4, 5), np.uint8)
    top = (1 << 31) - 20 * 7
    got, _ = api.seeded(q, [([(0, 0)], [top - 1])])
    assert got[0, 3, 4] == top - 1 + 3 * 7 + 5
    off, rc_, fld = np.array([0, 1], np.int64), np.zeros((1, 2), np.int32), np.zeros((1, 4, 5), np.int32)
    assert L.c.hmsg_nav_seeded_fields(0, 4, 5, _ptr(q), C.byref(prm), 1, _ptr(off), _ptr(rc_), _ptr(np.array([top], np.int32)), _ptr(fld), None) == UNSUPPORTED


# ------------------------------------------------------------------------------------------ the Python layer
def _np(v):
    return v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)


RAW_MAPS = dict(dilation=0, blur=0, region_rule=1)                        # main_free_map: the floor cells that hold no obstacle


def two_storeys(L, wrap=None):
    """two storeys made as tests/navmap_cases.from_cells makes one, at zero levels 0 and 3.25, of different shapes: downstairs 37 x
    50 with a wall (column 25, rows 0 .. 29), upstairs 41 x 33 with a wall (row 20, columns 5 ..)"""
    from holoagent_amd.nav_graph import NavigationGraph
    from tests import navmap_cases as MC
    navs = []
    for shape, wall, zero in (((37, 50), (slice(0, 30), 25), 0.0), ((41, 33), (20, slice(5, 33)), 3.25)):
        ob = np.zeros(shape, bool)
        ob[wall] = True
        pts = MC.from_cells(np.ones(shape, bool), ob, zero=zero)
        nav = NavigationGraph((pts if wrap is None else wrap(pts), None), 0.25, lib_=L)
        nav.get_main_free_map(None, {"floor_zero_level": zero}, None, list(MC.FAR), save=False, **RAW_MAPS)
        assert np.array_equal(_np(nav.maps["main_free_map"]) != 0, ~ob)
        navs.append(nav)
    return navs


def climbing_track(n=9):
    """poses that climb from over cell (33, 3) downstairs to over cell (2, 30) upstairs, 0.25 m cells"""
    from tests import navmap_cases as MC
    a, b = np.array([3.1 * 0.25, 1.5, 33.1 * 0.25]), np.array([30.1 * 0.25, 3.25 + 1.5, 2.1 * 0.25])
    return [MC.pose_at(*(a + (b - a) * t)) for t in np.linspace(0.0, 1.0, n)]


def building_navigation(L, wrap=None):
    """stair_link lands on passable cells at the formula's cost; BuildingNavigation.route reaches a goal upstairs through it, every
    path cell passable on its storey, `floors` changing exactly where the link is crossed; route_to_view upstairs stands where the
    sight line is clear by the numpy form of V1 / V2"""
    from holoagent_amd.nav_graph import BuildingNavigation, stair_link
    from tests import navview_reference as VR
    low, up = two_storeys(L, wrap)
    track = climbing_track()
    pos = np.array([p[:3, 3] for p in track])
    length = float(np.sqrt(((pos[1:] - pos[:-1]) ** 2).sum(axis=1)).sum())
    for metres in (0.0, 0.5):
        link, d2 = stair_link(low, up, track, 0, 1, metres)
        pas = [_np(n.passable_map(metres)) for n in (low, up)]
        assert link[0] == 0 and link[3] == 1 and pas[0][link[1], link[2]] and pas[1][link[4], link[5]]
        assert link[6] == max(1, int(np.ceil(length * 5 / 0.25))) and link[6] > 100
        (ra, rd), (rb, rdb) = RR.snap(pas[0], [(33, 3)]), RR.snap(pas[1], [(2, 30)])
        assert link[1:3] == tuple(ra[0]) and link[4:6] == tuple(rb[0]) and d2 == (int(rd[0]), int(rdb[0]))
        nav = BuildingNavigation([low, up], [link], lib_=L)
        start = np.array([40 * 0.25 + 0.1, 0.9, 5 * 0.25 + 0.1])           # downstairs, beyond the wall
        goals = np.array([[3 * 0.25, 3.3, 38 * 0.25], [20.4 * 0.25, 3.3, 20.2 * 0.25], [10 * 0.25, 0.2, 10 * 0.25]])       # upstairs (one in the wall), downstairs
        floors = [1, 1, 0]
        got = nav.route(0, start, goals, floors, min_clearance_m=metres)
        ref, B = RB.route([_np(n.maps["main_free_map"]) for n in (low, up)], [link], (0, 5, 40),
                          [(1, 38, 3), (1, 20, 20), (0, 10, 10)], min_clearance=low.clearance_units(metres))
        compare_route({k: v for k, v in nav.last_route.items() if k != "fields"}, ref)
        for k, r in enumerate(got):
            a, b = ref["path_off"][k], ref["path_off"][k + 1]
            assert r["reachable"] and r["floor"] == floors[k] and r["cell"] == tuple(ref["goal_cell"][k][1:])
            assert np.array_equal(r["floors"], ref["path_src"][a:b, 0]) and np.array_equal(r["cells"], ref["path_src"][a:b, 1:])
            assert all(pas[l][rr, cc] for l, (rr, cc) in zip(r["floors"], r["cells"]))
            assert r["length_m"] == float(ref["goal_dist"][k]) * 0.25 / 5 and len(r["polyline"]) == b - a
            assert np.array_equal(r["polyline"][:, 1], np.where(r["floors"] == 0, 0.0, 3.25))         # each storey's zero level
            change = np.flatnonzero(np.diff(r["floors"]))
            if floors[k] == 1:                                            # the storey changes once, from one end of the link to the other
                assert len(change) == 1 and tuple(r["cells"][change[0]]) == link[1:3] and tuple(r["cells"][change[0] + 1]) == link[4:6]
            else:
                assert len(change) == 0
        f = nav.fields(0, np.array([5, 40]), metres)
        assert all(np.array_equal(_np(x), y) for x, y in zip(f, ref["fields"]))
        # a viewpoint upstairs: the goal behind the upstairs wall is seen from a reached cell with a clear sight line
        views = nav.route_to_view(0, start, goals[:2], [1, 1], min_clearance_m=metres, view_range_m=(0.5, 4.0))
        blocking = _np(up.sight_blocking_map())
        for k, v in enumerate(views):
            assert v["reachable"] and v["floor"] == 1 and v["n_visible"] > 0 and v["floors"][0] == 0 and v["floors"][-1] == 1
            goal_cell = tuple(int(x) for x in up.cells_of(goals[k])[0])
            assert VR.clear(blocking, v["cell"], goal_cell) and pas[1][v["cell"]] and ref["fields"][1][v["cell"]] != U
            assert tuple(v["cells"][-1]) == v["cell"] and abs(float(np.hypot(*v["facing"])) - 1.0) < 1e-12
            assert v["length_m"] == float(ref["fields"][1][v["cell"]]) * 0.25 / 5
    none = BuildingNavigation([low, up], [], lib_=L).route(0, start, goals, floors)
    assert [r["reachable"] for r in none] == [False, False, True] and len(none[0]["polyline"]) == 0


def stairs_track_helper(L):
    """get_stairs_graph_with_poses_v2 returns the same graph as before its pose track was factored out: the comparison graph is made
    here from a copy of the body as it stood; Graph.stair_links' track is the helper's"""
    import networkx as nx
    from scipy.signal import find_peaks
    from holoagent_amd.nav_graph import NavigationGraph
    from tests import navmap_cases as MC
    low, up = two_storeys(L)
    rng = np.random.default_rng(9)
    lower = [MC.pose_at(rng.uniform(1, 9), 1.5 + rng.uniform(-0.01, 0.01), rng.uniform(1, 8)) for _ in range(60)]
    upper = [MC.pose_at(rng.uniform(1, 7), 4.75 + rng.uniform(-0.01, 0.01), rng.uniform(1, 9)) for _ in range(60)]
    poses = lower + climbing_track(30) + upper

    def before(self, floor, floor_id, poses_list):
        zero = floor.floor_zero_level
        heights = np.array([p[1, 3] - 1.5 for p in poses_list])
        counts, edges = np.histogram(heights, bins=100)
        padded = np.concatenate([[np.min(counts)], counts, [np.min(counts)]])
        peaks = find_peaks(padded, height=0.3 * np.max(counts))[0] - 1
        if floor_id >= len(peaks) - 1:
            return nx.Graph(), False, None
        h_lo, h_hi = edges[peaks[int(floor_id)] + 1], edges[peaks[int(floor_id) + 1]]
        if heights[0] > heights[-1]:
            heights, poses_list = heights[::-1], poses_list[::-1]
        first_low = 0
        if heights[0] > h_lo:
            first_low = next((i for i, h in enumerate(heights) if h <= h_lo), 0)
        st = next((i for i, h in enumerate(heights) if h > h_lo and i > first_low), None)
        ed = next((i for i, h in enumerate(heights) if h > h_hi), None)
        for i in range(st, ed):
            if heights[i] < h_lo:
                st = i
        st, ed = np.max([st - 5, 0]), ed + 20
        track = [p[:3, 3] for p in poses_list[st:ed]]
        if not track:
            return nx.Graph(), False, None
        lowest = np.min([p[1] for p in track])
        chain = nx.Graph()
        last = None
        for p in track:
            cell = (p - self.pcd_min) / self.cell_size
            chain.add_node((cell[2], cell[0], floor_id), pos=(p[0], p[1] - lowest + zero, p[2]), floor_id=floor_id)
            if last is not None:
                chain.add_edge((cell[2], cell[0], floor_id), (last[2], last[0], floor_id), dist=np.linalg.norm(cell - last))
            last = cell
        return self.sparsify_graph(chain, resampling_dist=0.4), True, poses_list[st:ed]

    class _Floor:
        floor_zero_level = 0.0

    for order in (poses, poses[::-1]):
        for floor_id in (0, 1):
            want, has, seg = before(low, _Floor, floor_id, order)
            got = low.get_stairs_graph_with_poses_v2(_Floor, floor_id, order)
            assert low.has_stairs == has and list(got.nodes(data=True)) == list(want.nodes(data=True))
            assert list(got.edges(data=True)) == list(want.edges(data=True))
            track = NavigationGraph.stairs_pose_track(floor_id, order)
            assert (track is None) == (seg is None) and (seg is None or (len(track) == len(seg) and all(a is b for a, b in zip(track, seg))))
    assert low.get_stairs_graph_with_poses_v2(_Floor, 0, poses).number_of_nodes() > 3


def graph_route_across_floors(L, tmp_path):
    """Graph.route_across_floors on a scene built from frames with a second storey above it: a way where route_to_objects says
    "other floor", "no stairs" with links=[]; create_nav_graph writes the same bytes before and after"""
    from holoagent_amd.graph import Floor, Object, Room, _Pcd
    from holoagent_amd.nav_graph import stair_link
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
    g.create_nav_graph(nav_dir=str(tmp_path / "a"), poses_list=track)
    zero1 = fl.floor_zero_level + 2.7
    pts, cols, _, poses_up = MC.room(41, 3.0, 2.4, n_floor=5000, n_wall=4000, n_box=900, zero=zero1)
    upstairs = Floor("1", name="floor_1")
    upstairs.floor_zero_level, upstairs.floor_height, upstairs.pcd = zero1, 2.7, (pts, cols)
    g.floors.append(upstairs)
    g.rooms += [Room("0_0", "0"), Room("1_0", "1")]
    down = Object("0_0_0", "0_0")
    down.pcd = _Pcd(np.array([rng.uniform(lo[0], hi[0]), fl.floor_zero_level + 0.5, rng.uniform(lo[2], hi[2])]) + rng.normal(0, 0.05, (40, 3)))
    up = Object("1_0_0", "1_0")
    up.pcd = _Pcd(np.array([[2.2, zero1 + 0.5, 0.9]]))
    g.objects = [down, up]
    poses = track + list(poses_up)
    start = track[0]
    same = g.route_to_objects(start, [0, 1], min_clearance=0.09, poses_list=poses)
    assert same[1]["reason"] == "other floor" and not same[1]["reachable"]
    climb = [MC.pose_at(*(start[:3, 3] + (np.array([1.5, zero1 + 0.9, 1.2]) - start[:3, 3]) * t)) for t in np.linspace(0, 1, 8)]
    navs = [g.floor_navigation(0, poses), g.floor_navigation(1, poses)]
    link, _ = stair_link(navs[0], navs[1], climb, 0, 1, 0.09)
    assert link is not None
    res = g.route_across_floors(start, [0, 1], min_clearance=0.09, poses_list=poses, links=[link])
    assert [r["floor_id"] for r in res] == [0, 1]
    assert res[0]["reachable"] == same[0]["reachable"] and res[0]["cell"] == same[0]["cell"] and res[0]["length_m"] == same[0]["length_m"]
    assert np.array_equal(navs[0].cells_of(res[0]["polyline"]), navs[0].cells_of(same[0]["polyline"])) and (res[0]["floors"] == 0).all()
    r = res[1]
    assert r["reachable"] and r["reason"] is None and r["floors"][0] == 0 and r["floors"][-1] == 1 and len(r["polyline"]) == len(r["floors"])
    change = np.flatnonzero(np.diff(r["floors"]))
    assert len(change) == 1 and tuple(r["cells"][change[0]]) == link[1:3] and tuple(r["cells"][change[0] + 1]) == link[4:6]
    pas = [_np(n.passable_map(0.09)) for n in navs]
    assert all(pas[l][rr, cc] for l, (rr, cc) in zip(r["floors"], r["cells"]))
    ref, _ = RB.route([_np(n.maps["main_free_map"]) for n in navs], [link], (0,) + tuple(navs[0].cells_of(start[:3, 3])[0]),
                      [(1,) + tuple(navs[1].cells_of(np.asarray(up.pcd.get_center()))[0])], min_clearance=navs[0].clearance_units(0.09))
    assert np.array_equal(np.c_[r["floors"], r["cells"]], ref["path_src"]) and r["length_m"] == float(ref["goal_dist"][0]) * 0.03 / 5
    assert g.building_navigation(poses) is g.building_navigation(poses)              # made once and kept
    none = g.route_across_floors(start, [0, 1], min_clearance=0.09, poses_list=poses, links=[])
    assert none[1]["reason"] == "no stairs" and not none[1]["reachable"] and len(none[1]["polyline"]) == 0 and none[0]["reason"] == res[0]["reason"]
    views = g.view_routes_across_floors(start, [0, 1], min_clearance=0.09, poses_list=poses, links=[link])
    assert views[1]["reason"] in (None, "no view") and views[1]["reachable"] == (views[1]["reason"] is None)
    if views[1]["reachable"]:
        assert views[1]["floors"][-1] == 1 and views[1]["n_visible"] > 0
    assert g.view_routes_across_floors(start, [1], min_clearance=0.09, poses_list=poses, links=[])[0]["reason"] == "no stairs"
    g.floors.pop()
    g.create_nav_graph(nav_dir=str(tmp_path / "b"), poses_list=track)
    for name in ("sparse_voronoi_graph.json", "global_nav_graph_graph.json"):
        assert open(tmp_path / "a" / name, "rb").read() == open(tmp_path / "b" / name, "rb").read(), name
    g.scene.close()


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

    def seeded(self, p, sets, **w):
        from holoagent_amd._lib import nav_seeded_fields
        f, n = nav_seeded_fields(self._in(p, np.uint8), sets, lib_=self.L, **w)
        return self._out(f), self._out(n)

    def fields(self, passables, links, starts, **w):
        from holoagent_amd._lib import nav_building_fields
        f, n = nav_building_fields([self._in(p, np.uint8) for p in passables], links, starts, lib_=self.L, **w)
        return [self._out(x) for x in f], self._out(n)

    def paths(self, passables, links, fields, goals, **w):
        from holoagent_amd._lib import nav_building_paths
        off, src = nav_building_paths([self._in(p, np.uint8) for p in passables], links, [self._in(f, np.int32) for f in fields], goals,
                                      lib_=self.L, **w)
        return self._out(off), self._out(src)

    def route(self, maps, links, start, goals, want_fields=False, **w):
        from holoagent_amd._lib import nav_building_route
        r = nav_building_route([self._in(m, np.uint8) for m in maps], links, start, goals, lib_=self.L, want_fields=want_fields, **w)
        return {k: ([self._out(x) for x in v] if isinstance(v, list) else self._out(v)) for k, v in r.items()}

    def last(self):
        a, b = C.c_int32(0), C.c_int32(0)
        self.L.c.hmsg_test_nav_building_last(C.byref(a), C.byref(b))
        return a.value, b.value
