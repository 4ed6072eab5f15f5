"""The cases of the room calls (include/hmsg.h, N11: hmsg_nav_room_labels, hmsg_nav_doors, hmsg_nav_path_rooms,
hmsg_nav_room_doors), shared by the simulator tests (tests/test_navrooms.py) and the GPU tests (tests/test_navrooms_gpu.py).  A
case takes `api` (the wrappers of holoagent_amd._lib on one library or the other, images handed over as numpy arrays or as device
tensors, results as numpy) and compares every output with tests/navrooms_reference.py by array_equal: nothing here has a
tolerance.  The maps are those of tests/navroute_cases.py.  The cases that take the library itself (the capacities, the refusals,
NavigationGraph, Graph) are at the end."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import navroute_cases as NC
from tests import navroute_reference as RR
from tests import navrooms_reference as GR

U = RR.UNREACHED
UNSUPPORTED = -3                                                          # include/hmsg.h: HMSG_ERR_UNSUPPORTED


# ------------------------------------------------------------------------------------------ what every case checks
def check_properties(p, lab, n_rooms, got, n_cells):
    """the issue's properties, on the library's own outputs"""
    adj, pair, off, rc, oth = got["adjacency"], got["door_pair"], got["door_off"], got["door_rc"], got["other"]
    assert np.array_equal(adj, adj.T) and (np.diag(adj) == 0).all()
    want = np.zeros_like(adj)
    for a, b in pair:
        want[a, b] += 1
        want[b, a] += 1
    assert np.array_equal(adj, want)
    seen = np.zeros(lab.shape, np.int32)
    for k, (a, b) in enumerate(pair):
        cells = rc[off[k]:off[k + 1]]
        assert len(cells) and np.isin(lab[cells[:, 0], cells[:, 1]], (a, b)).all()
        seen[cells[:, 0], cells[:, 1]] += 1
    assert np.array_equal(seen, (oth >= 0).astype(np.int32))              # every threshold cell in exactly one door
    assert int(n_cells.sum()) == int((lab >= 0).sum()) and len(n_cells) == n_rooms


def check_rooms(api, p, seeds, what="", graph=None, reference=GR.labels, **w):
    """labels, dist, n_cells and the door table of one map and one seed list against the restatement -> (label, door table)"""
    p = np.asarray(p)
    n = len(seeds)
    lab, cells, dist = api.labels(p, seeds, **w)
    rl, rd, rn = reference(p, seeds, graph=graph, **w)
    assert lab.dtype == np.int32 and dist.dtype == np.int32 and cells.dtype == np.int64 and lab.shape == p.shape, what
    assert np.array_equal(dist, rd), (what, int((dist != rd).sum()))
    assert np.array_equal(lab, rl), (what, int((lab != rl).sum()))
    assert np.array_equal(cells, rn), what
    union = np.concatenate([np.asarray(s, np.int64).reshape(-1, 2) for s in seeds]) if n else np.zeros((0, 2), np.int64)
    assert np.array_equal(dist, api.fields(p, [union], **w)[0][0]), what  # hmsg_nav_distance_fields of the union of the seeds
    got = api.doors(p, lab, n)
    ref = GR.doors(p, rl, n)
    for k in ("other", "door_pair", "door_off", "door_rc", "adjacency"):
        assert got[k].dtype == ref[k].dtype and np.array_equal(got[k], ref[k]), (what, k)
    assert got["n_doors"] == len(ref["door_pair"]) and got["n_door_cells"] == len(ref["door_rc"])
    check_properties(p, lab, n, got, cells)
    return lab, got


def block(r0, r1, c0, c1, step=1):
    rr, cc = np.mgrid[r0:r1:step, c0:c1:step]
    return np.c_[rr.ravel(), cc.ravel()]


# ------------------------------------------------------------------------------------------ small shapes
def tiny_and_degenerate(api):
    for v in (1, 0):
        lab, got = check_rooms(api, np.array([[v]], np.uint8), [[(0, 0)]], "1 x 1")
        assert lab[0, 0] == (0 if v else -1) and got["n_doors"] == 0
    line = np.ones((1, 90), np.uint8)
    lab, got = check_rooms(api, line, [[(0, 0)], [(0, 89)]], "1 x 90")
    assert lab[0, 44] == 0 and lab[0, 45] == 1 and got["n_doors"] == 1 and np.array_equal(got["door_rc"], [(0, 44), (0, 45)])
    p = np.ones((9, 11), np.uint8)
    p[4, :] = 0
    lab, got = check_rooms(api, p, [], "no room")
    assert (lab == -1).all() and got["n_doors"] == 0 and got["adjacency"].shape == (0, 0)
    # room 1 has no seed, room 2's seeds are all blocked, rooms 0 and 3 share a seed: the smaller index has it
    lab, got = check_rooms(api, p, [[(0, 0), (1, 1)], [], [(4, 3), (4, 4)], [(0, 0), (8, 10)], [(8, 0), (8, 0)]], "empty, blocked, shared")
    assert lab[0, 0] == 0 and set(np.unique(lab)) == {-1, 0, 3, 4} and got["n_doors"] == 1 and tuple(got["door_pair"][0]) == (3, 4)


def unreached_island(api):
    p = np.ones((20, 30), np.uint8)
    p[:, 14] = 0                                                          # a wall: the right part is reached by no seed
    p[10, :14] = 0
    lab, got = check_rooms(api, p, [[(2, 2)], [(17, 2)], [(5, 5), (3, 14)]], "island")
    assert (lab[:, 15:] == -1).all() and (lab[:10, :14] >= 0).all() and got["n_doors"] == 1 and tuple(got["door_pair"][0]) == (0, 2)


def exact_ties(api):
    """two seeds at equal walk from the middle column: it goes to the smaller index, whichever seed carries it"""
    p = np.ones((7, 9), np.uint8)
    a, b = [(3, 0)], [(3, 8)]
    lab, _ = check_rooms(api, p, [a, b], "tie")
    swapped, _ = check_rooms(api, p, [b, a], "tie, swapped")
    assert (lab[:, 4] == 0).all() and (swapped[:, 4] == 0).all() and (lab[:, :4] == 0).all() and (swapped[:, :4] == 1).all()
    q = NC.random_map()
    s0, s1 = [NC.first_free(q, (40, 40))], [NC.first_free(q, (60, 90))]
    l0, _ = check_rooms(api, q, [s0, s1], "random tie", graph=NC.ref_graph("random"))
    l1, _ = check_rooms(api, q, [s1, s0], "random tie, swapped", graph=NC.ref_graph("random"))
    f0, f1 = RR.field(q, s0, graph=NC.ref_graph("random"))[0], RR.field(q, s1, graph=NC.ref_graph("random"))[0]
    tie = (f0 == f1) & (f0 != U)
    assert tie.sum() > 0 and (l0[tie] == 0).all() and (l1[tie] == 0).all()


def corner_contact(api):
    lab, got = check_rooms(api, np.array([[1, 0], [0, 1]], np.uint8), [[(0, 0)], [(1, 1)]], "corner contact")
    assert np.array_equal(lab, [[0, -1], [-1, 1]]) and got["n_doors"] == 0 and (got["other"] == -1).all()
    p = np.ones((12, 12), np.uint8)                                       # two rooms that touch by one diagonal only
    p[6, :] = 0
    p[:, 6] = 0
    p[6, 6] = 0
    lab, got = check_rooms(api, p, [[(2, 2)], [(9, 9)]], "diagonal rooms")
    assert got["n_doors"] == 0


def three_rooms_at_a_point(api):
    p = np.ones((21, 21), np.uint8)
    lab, got = check_rooms(api, p, [[(0, 10)], [(20, 0)], [(20, 20)]], "three rooms")
    assert got["n_doors"] == 3 and [tuple(d) for d in got["door_pair"]] == [(0, 1), (0, 2), (1, 2)]
    oth = got["other"]
    three = [(r, c) for r, c in np.argwhere(oth >= 0)
             if len({int(lab[r + dr, c + dc]) for dr, dc in RR.MOVES if 0 <= r + dr < 21 and 0 <= c + dc < 21} - {int(lab[r, c])}) == 2]
    assert three and all(oth[r, c] == min({0, 1, 2} - {int(lab[r, c])}) for r, c in three)    # the least of the two neighbours' labels
    lab, got = check_rooms(api, p, [[(0, 0)], [(0, 20)], [(20, 0)], [(20, 20)]], "four rooms")
    assert got["n_doors"] >= 4


def two_doors_one_pair(api):
    p = np.ones((30, 41), np.uint8)
    p[:, 20] = 0
    p[4:7, 20] = 1
    p[22:25, 20] = 1
    lab, got = check_rooms(api, p, [[(15, 3)], [(15, 37)]], "two doors")
    assert got["n_doors"] == 2 and got["adjacency"][0, 1] == 2 and (got["door_pair"] == (0, 1)).all()
    assert got["door_rc"][got["door_off"][1]][0] > 20 > got["door_rc"][got["door_off"][1] - 1][0]      # ordered by the least cell


def door_on_a_seam(api):
    """a 70 x 130 map: a wall along column 63 | 64 with a door over the tile seam of the rows, and the same turned"""
    for wall_c in (63, 64):
        p = np.ones((70, 130), np.uint8)
        p[:, wall_c] = 0
        p[61:67, wall_c] = 1                                              # the opening spans rows 63 | 64
        lab, got = check_rooms(api, p, [[(35, 13)], [(35, 114)]], "seam, wall at column %d" % wall_c)     # (13 + 114 = 63 + 64)
        assert got["n_doors"] == 1 and got["n_door_cells"] >= 6 and set(got["door_rc"][:, 1]) == {63, 64}
        assert {63, 64} <= set(got["door_rc"][:, 0])
    p = np.ones((130, 70), np.uint8)
    p[63, :] = 0
    p[64, :] = 0
    p[63:65, 30:34] = 1
    lab, got = check_rooms(api, p, [[(13, 35)], [(114, 35)]], "seam of the rows")
    assert got["n_doors"] == 1 and set(got["door_rc"][:, 0]) == {63, 64}


# ------------------------------------------------------------------------------------------ the rooms map of the routing cases
def room_blocks(H=130, W=190):
    """the rooms of NC.rooms_map as (r0, r1, c0, c1), row-major: the cells between the walls at every 37th row and column"""
    rows = [(a, b) for a, b in zip([0] + [r + 1 for r in range(37, H, 37)], list(range(37, H, 37)) + [H])]
    cols = [(a, b) for a, b in zip([0] + [c + 1 for c in range(37, W, 37)], list(range(37, W, 37)) + [W])]
    return [(r0, r1, c0, c1) for r0, r1 in rows for c0, c1 in cols]


@functools.lru_cache(maxsize=None)
def room_seeds(which, H=130, W=190):
    if which == "all":
        return tuple(block(*b) for b in room_blocks(H, W))
    if which == "third":
        return tuple(block(*b, step=3) for b in room_blocks(H, W))
    return tuple(np.array([((r0 + r1) // 2, (c0 + c1) // 2)]) for r0, r1, c0, c1 in room_blocks(H, W))      # (a centre on clutter: no source)


def rooms_every_cell(api):
    """every cell of each room a seed: a door per wall opening, split where clutter splits the opening; no door is one-sided"""
    p = NC.rooms_map()
    lab, got = check_rooms(api, p, list(room_seeds("all")), "rooms, every cell", graph=NC.ref_graph("rooms"))
    sizes = np.diff(got["door_off"])
    print("rooms, every cell: labels", len(np.unique(lab[lab >= 0])), "pairs", int((got["adjacency"] > 0).sum()) // 2, "doors", got["n_doors"],
          "cells per door", int(sizes.min()), "to", int(sizes.max()))
    assert len(np.unique(lab[lab >= 0])) == 24 and int((got["adjacency"] > 0).sum()) // 2 == 35 and got["n_doors"] == 41
    assert sizes.min() >= 2 and sizes.max() <= 8
    for k, (a, b) in enumerate(got["door_pair"]):                         # both rooms have cells in every door
        cells = got["door_rc"][got["door_off"][k]:got["door_off"][k + 1]]
        assert set(lab[cells[:, 0], cells[:, 1]]) == {a, b}


def rooms_every_third_cell(api):
    check_rooms(api, NC.rooms_map(), list(room_seeds("third")), "rooms, every third cell", graph=NC.ref_graph("rooms"))


def rooms_centre_seeds(api):
    """one centre cell per room; two of the 24 centres lie on clutter, so their rooms fall to the neighbours.  The figures are the
    restatement's (50 doors, the longest 94 cells, 22 labels in use)."""
    p = NC.rooms_map()
    lab, got = check_rooms(api, p, list(room_seeds("centre")), "rooms, centres", graph=NC.ref_graph("rooms"))
    sizes = np.diff(got["door_off"])
    print("rooms, centres: doors", got["n_doors"], "longest", int(sizes.max()))
    assert got["n_doors"] == 50 and sizes.max() == 94 and len(np.unique(lab[lab >= 0])) == 22
    rounds, trips = api.last()
    print("rooms, centres: rounds", rounds, "host round trips", trips)


def open_plan(api):
    """no wall at all: the doors are bisectors hundreds of cells long that cross the tiles -- the case for the union-find"""
    p = np.ones((130, 130), np.uint8)
    lab, got = check_rooms(api, p, [[(20, 15)], [(100, 110)]], "open plan, two seeds")
    assert got["n_doors"] == 1 and got["n_door_cells"] > 250
    lab, got = check_rooms(api, p, [[(20, 15)], [(100, 110)], [(64, 64)], [(10, 120)], [(125, 5)]], "open plan, five seeds")
    assert np.diff(got["door_off"]).max() > 100 and got["n_doors"] >= 6


def serpentine(api):
    """a seed at each end of the 8515-cell corridor: one door deep inside.  Each half of the corridor crosses a tile seam some 97
    times; the GPU carries a value over one seam a round, the simulator, which runs a round's tiles in order, over several, so the
    count of rounds (the field's and the labels' together) differs between the two and only its order is asserted: well past one
    batch of 32, with the round trips far behind."""
    p = NC.serpentine_map()
    end = tuple(int(v) for v in np.argwhere(RR.field(p, [(0, 0)], graph=NC.ref_graph("serpentine"))[0] == 42570)[0])
    lab, got = check_rooms(api, p, [[(0, 0)], [end]], "serpentine", graph=NC.ref_graph("serpentine"))
    assert got["n_doors"] == 1 and got["n_door_cells"] == 2 and 60 < got["door_rc"][0][0] < 70
    rounds, trips = api.last()
    print("serpentine: rounds", rounds, "host round trips", trips)
    assert rounds > 60 and trips * 4 < rounds


def random_rooms(api):
    p = NC.random_map()
    rng = np.random.default_rng(17)
    free = np.argwhere(p != 0)
    seeds = [free[rng.integers(0, len(free), int(k))] for k in rng.integers(1, 6, 9)]
    lab, got = check_rooms(api, p, seeds, "random, 9 rooms", graph=NC.ref_graph("random"))
    assert got["n_doors"] > 9
    check_rooms(api, p, seeds, "random, 9 rooms, weights 2 3", w_straight=2, w_diag=3)


def rooms_large(api):
    """the generator at 500 x 700 (the GPU module only); its labels by G2's second form"""
    p = NC.rooms_map(500, 700, 6)
    lab, got = check_rooms(api, p, list(room_seeds("centre", 500, 700)), "rooms 500 x 700", graph=NC.ref_graph("rooms_large"),
                           reference=GR.labels_by_order)
    rounds, trips = api.last()
    print("rooms 500 x 700: labels", len(np.unique(lab[lab >= 0])), "doors", got["n_doors"], "rounds", rounds, "host round trips", trips)


# ------------------------------------------------------------------------------------------ legs
def legs_cases(api):
    p = NC.rooms_map()
    lab, _, _ = api.labels(p, list(room_seeds("all")))
    src = NC.first_free(p, (60, 90))
    f, _ = RR.field(p, [src], graph=NC.ref_graph("rooms"))
    rng = np.random.default_rng(6)
    reach = np.argwhere(f != U)
    blocked = tuple(int(v) for v in np.argwhere(p == 0)[50])
    goals = [tuple(c) for c in reach[rng.integers(0, len(reach), 17)]] + [src, blocked, (-1, 5)]       # a one-cell path, two empty ones
    off, rc = api.paths(p, f, goals)
    assert len(goals) == 20 and off[18] - off[17] == 1 and off[20] == off[18]
    # ... and a hand-made path that leaves the image and comes back
    extra = np.array([(0, 1), (0, 0), (-1, 0), (0, -1), (0, 0), (130, 5), (129, 190), (129, 189)], np.int32)
    off = np.concatenate([off, [off[-1] + len(extra)]]).astype(np.int64)
    rc = np.concatenate([rc, extra]).astype(np.int32)
    got = api.legs(lab, off, rc)
    ref = GR.legs(lab, off, rc)
    for g, r in zip(got, ref):
        assert g.dtype == r.dtype and np.array_equal(g, r)
    leg_off, room, first = got
    assert leg_off[19] == leg_off[18] and leg_off[18] - leg_off[17] == 1 and (room[leg_off[20]:] == [lab[0, 1], -1, lab[0, 0], -1, lab[129, 189]]).all()
    assert (np.diff(leg_off) > 1).sum() >= 10                                # most ways cross a door
    for a, b in zip(leg_off[:-1], leg_off[1:]):
        if b > a:
            assert first[a] == 0 and (np.diff(first[a:b]) > 0).all() and (np.diff(room[a:b]) != 0).all()
    none = api.legs(lab, np.zeros(1, np.int64), np.zeros((0, 2), np.int32))
    assert np.array_equal(none[0], [0]) and len(none[1]) == 0 and len(none[2]) == 0


# ------------------------------------------------------------------------------------------ the composition
def composition(api):
    m = NC.rooms_map()
    seeds = list(room_seeds("third"))
    for minc in (0, 10):
        got = api.room_doors(m, seeds, min_clearance=minc)
        pas = ((m != 0) & (api.clearance(m) >= minc)).astype(np.uint8) if minc else (m != 0).astype(np.uint8)
        lab, cells, _ = api.labels(pas, seeds)
        three = api.doors(pas, lab, len(seeds))
        assert np.array_equal(got["passable"], pas) and np.array_equal(got["label"], lab)
        for k in ("other", "door_pair", "door_off", "door_rc", "adjacency"):
            assert got[k].dtype == three[k].dtype and np.array_equal(got[k], three[k]), (minc, k)
        ref = GR.doors(pas, GR.labels(pas, seeds)[0], len(seeds))
        for k in ("other", "door_pair", "door_off", "door_rc", "adjacency"):
            assert np.array_equal(got[k], ref[k]), (minc, k)
        assert got["n_doors"] > 20


ALL = (tiny_and_degenerate, unreached_island, exact_ties, corner_contact, three_rooms_at_a_point, two_doors_one_pair, door_on_a_seam,
       rooms_every_cell, rooms_every_third_cell, rooms_centre_seeds, open_plan, serpentine, random_rooms, legs_cases, composition)


# ------------------------------------------------------------------------------------------ capacities and refusals (the library itself)
def capacities_too_small(L):
    """lists that are too short: an error, the counts say what is needed, everything else is written, the list is not"""
    from holoagent_amd._lib import HmsgNavDoorTable, HmsgRouteParams, _ptr
    p = np.ascontiguousarray(NC.rooms_map())
    H, W = p.shape
    seeds = list(room_seeds("all"))
    lab, _, _ = GR.labels(p, seeds, graph=NC.ref_graph("rooms"))
    ref = GR.doors(p, lab, 24)
    nd, nc = len(ref["door_pair"]), len(ref["door_rc"])
    off = np.concatenate([[0], np.cumsum([len(s) for s in seeds])]).astype(np.int64)
    rc = np.ascontiguousarray(np.concatenate(seeds).astype(np.int32))
    prm = HmsgRouteParams(5, 7, 0, 0)
    for dcap, ccap in ((nd - 1, nc), (nd, nc - 1), (0, 0), (nd, nc)):
        for composed in (False, True):
            out = HmsgNavDoorTable()
            pair, doff, drc = np.full((max(dcap, 1), 2), -7, np.int32), np.full(dcap + 1, -7, np.int64), np.full((max(ccap, 1), 2), -7, np.int32)
            oth, adj, lab_out = np.zeros((H, W), np.int32), np.zeros((24, 24), np.int32), np.zeros((H, W), np.int32)
            out.door_pair, out.door_off, out.door_rc, out.other, out.adjacency = _ptr(pair), _ptr(doff), _ptr(drc), _ptr(oth), _ptr(adj)
            out.door_capacity, out.cell_capacity = dcap, ccap
            if composed:
                st = L.c.hmsg_nav_room_doors(0, H, W, _ptr(p), C.byref(prm), 24, _ptr(off), _ptr(rc), _ptr(lab_out), None, C.byref(out))
                assert np.array_equal(lab_out, lab)
            else:
                st = L.c.hmsg_nav_doors(0, H, W, _ptr(p), _ptr(lab), 24, C.byref(out))
            assert out.n_doors == nd and out.n_door_cells == nc and np.array_equal(oth, ref["other"]) and np.array_equal(adj, ref["adjacency"])
            assert (st == 0) == (dcap >= nd and ccap >= nc)
            if dcap >= nd:
                assert np.array_equal(pair, ref["door_pair"]) and np.array_equal(doff, ref["door_off"])
            else:
                assert (pair == -7).all() and (doff == -7).all()
            assert np.array_equal(drc, ref["door_rc"]) if ccap >= nc else (drc == -7).all()
    out = HmsgNavDoorTable()                                              # nothing wanted but the counts
    assert L.c.hmsg_nav_doors(0, H, W, _ptr(p), _ptr(lab), 24, C.byref(out)) == 0 and out.n_doors == nd and out.n_door_cells == nc
    # the legs
    src = NC.first_free(p, (60, 90))
    f, _ = RR.field(p, [src], graph=NC.ref_graph("rooms"))
    goals = np.argwhere(f != U)[::1201]
    poff, prc = RR.paths(p, f, goals)
    prc = np.ascontiguousarray(prc)
    roff, rroom, rfirst = GR.legs(lab, poff, prc)
    need, n = len(rroom), len(goals)
    assert need > n
    for cap in (need - 1, 0, need):
        loff, room, first, cnt = np.zeros(n + 1, np.int64), np.full(max(cap, 1), -7, np.int32), np.full(max(cap, 1), -7, np.int64), C.c_int64(-1)
        st = L.c.hmsg_nav_path_rooms(0, H, W, _ptr(lab), n, _ptr(poff), _ptr(prc), _ptr(loff), _ptr(room), _ptr(first), cap, C.byref(cnt))
        assert cnt.value == need and np.array_equal(loff, roff)
        if cap < need:
            assert st != 0 and (room == -7).all() and (first == -7).all()
        else:
            assert st == 0 and np.array_equal(room, rroom) and np.array_equal(first, rfirst)
    cnt = C.c_int64(-1)
    assert L.c.hmsg_nav_path_rooms(0, H, W, _ptr(lab), n, _ptr(poff), _ptr(prc), None, None, None, 0, C.byref(cnt)) == 0 and cnt.value == need


def refusals(api, L):
    from holoagent_amd._lib import HmsgError, HmsgNavDoorTable, HmsgRouteParams, _ptr
    p = np.ones((4, 5), np.uint8)
    lab = np.zeros((4, 5), np.int32)
    for kw in (dict(w_straight=0), dict(w_straight=5, w_diag=4), dict(w_straight=-1, w_diag=7), dict(min_clearance=-1)):
        with pytest.raises(HmsgError):
            api.labels(p, [[(0, 0)]], **kw)
        with pytest.raises(HmsgError):
            api.room_doors(p, [[(0, 0)]], **kw)
    for bad in ((4, 0), (0, 5), (-1, 0), (0, -1)):                         # a seed outside the image
        with pytest.raises(HmsgError):
            api.labels(p, [[(0, 0)], [bad]])
        with pytest.raises(HmsgError):
            api.room_doors(p, [[(0, 0)], [bad]])
    with pytest.raises(HmsgError):                                        # decreasing seed_off
        api.labels(p, (np.array([0, 2, 1], np.int64), np.zeros((2, 2), np.int32)))
    with pytest.raises(HmsgError):                                        # decreasing path_off
        api.legs(lab, np.array([0, 2, 1], np.int64), np.zeros((2, 2), np.int32))
    for v in (1, -2, 7):                                                  # a label outside [-1, n_rooms)
        bad = lab.copy()
        bad[2, 3] = v
        with pytest.raises(HmsgError):
            api.doors(p, bad, 1)
    api.doors(p, np.full((4, 5), -1, np.int32), 0)
    with pytest.raises(HmsgError):
        api.doors(p, lab, -1)
    prm, out = HmsgRouteParams(5, 7, 0, 0), HmsgNavDoorTable()
    one, rc, o32, cnt = np.zeros(2, np.int64), np.zeros((1, 2), np.int32), np.zeros(20, np.int32), C.c_int64(0)
    c, P, T = L.c, C.byref(prm), C.byref(out)
    assert c.hmsg_nav_room_labels(0, 4, 5, None, P, 1, _ptr(one), _ptr(rc), _ptr(o32), None, None) == -1
    assert c.hmsg_nav_room_labels(0, 4, 5, _ptr(p), None, 1, _ptr(one), _ptr(rc), _ptr(o32), None, None) == -1
    assert c.hmsg_nav_room_labels(0, 4, 5, _ptr(p), P, 1, None, _ptr(rc), _ptr(o32), None, None) == -1
    assert c.hmsg_nav_room_labels(0, 4, 5, _ptr(p), P, 1, _ptr(one), _ptr(rc), None, None, None) == -1
    assert c.hmsg_nav_room_labels(0, 4, 5, _ptr(p), P, 1, _ptr(np.array([0, 1], np.int64)), None, _ptr(o32), None, None) == -1      # seeds without seed_rc
    assert c.hmsg_nav_room_labels(0, 4, 5, _ptr(p), P, -1, _ptr(one), _ptr(rc), _ptr(o32), None, None) == -1
    assert c.hmsg_nav_room_labels(0, 0, 5, _ptr(p), P, 1, _ptr(one), _ptr(rc), _ptr(o32), None, None) == -1
    assert c.hmsg_nav_room_labels(0, 4, 0, _ptr(p), P, 1, _ptr(one), _ptr(rc), _ptr(o32), None, None) == -1
    assert c.hmsg_nav_doors(0, 4, 5, None, _ptr(lab), 1, T) == -1 and c.hmsg_nav_doors(0, 4, 5, _ptr(p), None, 1, T) == -1
    assert c.hmsg_nav_doors(0, 4, 5, _ptr(p), _ptr(lab), 1, None) == -1 and c.hmsg_nav_doors(0, 0, 5, _ptr(p), _ptr(lab), 1, T) == -1
    assert c.hmsg_nav_path_rooms(0, 4, 5, None, 0, _ptr(one), None, None, None, None, 0, C.byref(cnt)) == -1
    assert c.hmsg_nav_path_rooms(0, 4, 5, _ptr(lab), 0, None, None, None, None, None, 0, C.byref(cnt)) == -1
    assert c.hmsg_nav_path_rooms(0, 4, 5, _ptr(lab), 0, _ptr(one), None, None, None, None, 0, None) == -1
    assert c.hmsg_nav_path_rooms(0, 4, 5, _ptr(lab), -1, _ptr(one), None, None, None, None, 0, C.byref(cnt)) == -1
    assert c.hmsg_nav_path_rooms(0, 4, 5, _ptr(lab), 0, _ptr(one), None, None, None, None, 0, C.byref(cnt)) == 0 and cnt.value == 0
    assert c.hmsg_nav_room_doors(0, 4, 5, None, P, 1, _ptr(one), _ptr(rc), _ptr(o32), None, T) == -1
    assert c.hmsg_nav_room_doors(0, 4, 5, _ptr(p), P, 1, _ptr(one), _ptr(rc), None, None, T) == -1
    assert c.hmsg_nav_room_doors(0, 4, 5, _ptr(p), P, 1, _ptr(one), _ptr(rc), _ptr(o32), None, None) == -1
    # N7's size limits, before anything is read; adjacency with more than 4096 rooms
    assert c.hmsg_nav_room_labels(0, 1 << 14, 1 << 14, _ptr(p), P, 1, _ptr(one), _ptr(rc), _ptr(o32), None, None) == UNSUPPORTED
    big = HmsgRouteParams(5, 1 << 12, 0, 0)
    assert c.hmsg_nav_room_labels(0, 1 << 10, 1 << 9, _ptr(p), C.byref(big), 1, _ptr(one), _ptr(rc), _ptr(o32), None, None) == UNSUPPORTED
    assert c.hmsg_nav_doors(0, 1 << 14, 1 << 14, _ptr(p), _ptr(lab), 1, T) == UNSUPPORTED
    assert c.hmsg_nav_path_rooms(0, 1 << 14, 1 << 14, _ptr(lab), 0, _ptr(one), None, None, None, None, 0, C.byref(cnt)) == UNSUPPORTED
    out.adjacency = _ptr(o32)
    assert c.hmsg_nav_doors(0, 4, 5, _ptr(p), _ptr(lab), 4097, T) == UNSUPPORTED
    out.adjacency = None
    assert c.hmsg_nav_doors(0, 4, 5, _ptr(p), _ptr(lab), 4097, T) == 0


# ------------------------------------------------------------------------------------------ the Python layer
class _Room:
    """what NavigationGraph.room_seeds reads of a room: its (x, z) vertices"""

    def __init__(self, vertices, room_id="", name=None):
        self.vertices, self.room_id, self.name = np.asarray(vertices, np.float64), room_id, name


def navigation_graph_rooms(L, wrap=None):
    """NavigationGraph.room_seeds / room_map / doors / rooms_along on a storey made as tests/navmap_cases.py makes one: seeds by
    R6, the results against the restatement on the object's own main_free_map"""
    from holoagent_amd.nav_graph import NavigationGraph
    from tests import navmap_cases as MC
    pts, cols, zero, poses = MC.room(41, 3.0, 2.4, n_floor=5000, n_wall=4000, n_box=900)
    cloud = (pts, cols) if wrap is None else (wrap(pts), wrap(cols))
    nav = NavigationGraph(cloud, 0.03, lib_=L)
    nav.get_main_free_map(None, {"floor_zero_level": zero}, None, list(poses), save=False)
    np_ = lambda v: v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)
    main = np_(nav.maps["main_free_map"])
    lo, hi = pts.min(0), pts.max(0)
    rng = np.random.default_rng(9)
    mid = (lo[0] + hi[0]) / 2
    rooms = [_Room(np.c_[rng.uniform(lo[0], mid, 40), rng.uniform(lo[2], hi[2], 40)]), _Room(np.c_[rng.uniform(mid, hi[0], 40), rng.uniform(lo[2], hi[2], 40)]),
             _Room(np.zeros((0, 2))), _Room([(lo[0] - 5.0, lo[2]), (mid, hi[2] + 5.0)])]         # no vertex; vertices outside the grid only
    seeds = nav.room_seeds(rooms)
    assert len(seeds) == 4 and len(seeds[2]) == 0 and len(seeds[3]) == 0 and seeds[0].dtype == np.int32
    want = np.floor((rooms[0].vertices[:, [1, 0]] - nav.pcd_min[[2, 0]]) / 0.03).astype(np.int32)
    inside = (want[:, 0] >= 0) & (want[:, 0] < main.shape[0]) & (want[:, 1] >= 0) & (want[:, 1] < main.shape[1])
    assert np.array_equal(seeds[0], want[inside])
    for metres in (0.0, 0.09):
        pas = np_(nav.passable_map(metres))
        rl, _, _ = GR.labels(pas, seeds)
        ref = GR.doors(pas, rl, 4)
        lab = np_(nav.room_map(rooms, min_clearance_m=metres))
        assert np.array_equal(lab, rl) and (metres > 0 or set(np.unique(rl)) >= {0, 1})
        ds = nav.doors(rooms, min_clearance_m=metres)
        assert len(ds) == len(ref["door_pair"]) >= (0 if metres else 1)
        for k, d in enumerate(ds):
            cells = ref["door_rc"][ref["door_off"][k]:ref["door_off"][k + 1]]
            assert d["rooms"] == tuple(ref["door_pair"][k]) and np.array_equal(d["cells"], cells) and d["n_cells"] == len(cells)
            row, col = d["middle_cell"]
            assert (row, col) == tuple(cells[(len(cells) - 1) // 2])
            assert np.array_equal(d["middle"], [(col + 0.5) * 0.03 + nav.pcd_min[0], nav.pcd_min[1], (row + 0.5) * 0.03 + nav.pcd_min[2]])
    start = np.array([poses[0][0, 3], 0.8, poses[0][2, 3]])
    goals = np.c_[rng.uniform(lo[0], hi[0], 12), rng.uniform(0, 2, 12), rng.uniform(lo[2], hi[2], 12)]
    res = nav.route(start, goals)
    lab = np_(nav.room_map(rooms))
    for r in res:
        cells = nav.cells_of(r["polyline"]) if len(r["polyline"]) else np.zeros((0, 2), np.int32)
        legs = nav.rooms_along(cells)
        _, room, first = GR.legs(lab, np.array([0, len(cells)]), cells)
        assert [l["room"] for l in legs] == list(room) and [l["first"] for l in legs] == list(first)
        assert [l["n_cells"] for l in legs] == list(np.diff(np.concatenate([first, [len(cells)]])))


def graph_rooms(L, tmp_path):
    """Graph.room_map / room_doors / room_graph / rooms_on_route on a scene built from frames, with two rooms laid over the storey"""
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
    nav = g.floor_navigation(0, track)
    np_ = lambda v: v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)
    main = np_(nav.maps["main_free_map"])
    # two rooms: the halves of the storey's main free area along x, their vertices the free cells' centres at every 4th cell
    free = np.argwhere(main != 0)[::4]
    xs = (free[:, 1] + 0.5) * 0.03 + nav.pcd_min[0]
    zs = (free[:, 0] + 0.5) * 0.03 + nav.pcd_min[2]
    cut = np.median(xs)
    rooms = []
    for k, sel in enumerate((xs < cut, xs >= cut)):
        r = Room("0_%d" % k, "0", name=("hall", "study")[k])
        r.vertices = np.c_[xs[sel], zs[sel]]
        rooms.append(r)
    g.rooms = rooms
    seeds = nav.room_seeds(rooms)
    minc = 0.09
    pas = np_(nav.passable_map(minc))
    rl, _, _ = GR.labels(pas, seeds)
    ref = GR.doors(pas, rl, 2)
    assert len(ref["door_pair"]) >= 1
    assert np.array_equal(np_(g.room_map(0, min_clearance=minc)), rl)
    ds = g.room_doors(0, min_clearance=minc)
    assert len(ds) == len(ref["door_pair"])
    for k, d in enumerate(ds):
        assert d["rooms"] == ("0_0", "0_1") and np.array_equal(d["cells"], ref["door_rc"][ref["door_off"][k]:ref["door_off"][k + 1]])
    big = g.room_doors(0, min_clearance=minc, min_cells=3)
    assert [d["n_cells"] for d in big] == [d["n_cells"] for d in ds if d["n_cells"] >= 3]
    G = g.room_graph(0, min_clearance=minc, walks=True)
    assert set(G.nodes) == {"0_0", "0_1"} and list(G.edges) == [("0_0", "0_1")]
    e = G.edges["0_0", "0_1"]
    assert len(e["doors"]) == len(ds) and e["n_doors"] == len(ds) and G.nodes["0_1"]["name"] == "study"
    mids = np.array([d["middle_cell"] for d in ds])
    f = RR.field(pas, [mids[0]])[0]
    assert e["walk_m"][0][0] == 0.0 and all(e["walk_m"][0][k] == (float(f[tuple(m)]) * 0.03 / 5 if f[tuple(m)] != U else None) for k, m in enumerate(mids))
    # a route from the first room into the second: the two cells farthest from the first door, one in each room
    lab = rl
    far = lambda room: np.argwhere((lab == room) & (f != U))[np.argmax(f[(lab == room) & (f != U)])]
    a_cell, b_cell = far(0), far(1)
    world = lambda c: np.array([(c[1] + 0.5) * 0.03 + nav.pcd_min[0], fl.floor_zero_level + 0.5, (c[0] + 0.5) * 0.03 + nav.pcd_min[2]])
    o = Object("0_1_0", "0_1")
    o.pcd = _Pcd(world(b_cell) + rng.normal(0, 0.01, (20, 3)))
    g.objects = [o]
    start = MC.pose_at(world(a_cell)[0], fl.floor_zero_level + 0.9, world(a_cell)[2])
    res = g.route_to_objects(start, [0], min_clearance=minc, poses_list=track)
    assert res[0]["reachable"]
    legs = g.rooms_on_route(res[0], min_clearance=minc)
    assert legs[0]["room_id"] == "0_0" and legs[-1]["room_id"] == "0_1" and legs[0]["name"] == "hall" and legs[0]["first"] == 0
    assert all(G.has_edge(u["room_id"], v["room_id"]) for u, v in zip(legs[:-1], legs[1:]))
    assert abs(sum(l["length_m"] for l in legs) - res[0]["length_m"]) < 1e-9 and [l["first"] for l in legs] == sorted({l["first"] for l in legs})
    g.scene.close()


# ------------------------------------------------------------------------------------------ how a case reaches the library
class api(NC.api):
    """NC.api plus the wrappers of the room calls"""

    def labels(self, p, seeds, **w):
        from holoagent_amd._lib import nav_room_labels
        lab, cells, dist = nav_room_labels(self._in(p, np.uint8), seeds, want_dist=True, lib_=self.L, **w)
        return self._out(lab), self._out(cells), self._out(dist)

    def doors(self, p, label, n_rooms):
        from holoagent_amd._lib import nav_doors
        return {k: self._out(v) for k, v in nav_doors(self._in(p, np.uint8), self._in(label, np.int32), n_rooms, lib_=self.L).items()}

    def legs(self, label, path_off, path_rc):
        from holoagent_amd._lib import nav_path_rooms
        off = self._in(path_off, np.int64)
        got = nav_path_rooms(self._in(label, np.int32), off, self._in(np.asarray(path_rc, np.int32).reshape(-1, 2), np.int32), lib_=self.L)
        return tuple(self._out(v) for v in got)

    def room_doors(self, m, seeds, **w):
        from holoagent_amd._lib import nav_room_doors
        return {k: self._out(v) for k, v in nav_room_doors(self._in(m, np.uint8), seeds, lib_=self.L, **w).items()}

    def last(self):
        a, b = C.c_int32(0), C.c_int32(0)
        self.L.c.hmsg_test_nav_rooms_last(C.byref(a), C.byref(b))
        return a.value, b.value
