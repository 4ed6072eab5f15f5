"""The cases of the navigation maps (include/hmsg.h: hmsg_nav_floor_maps), shared by the simulator tests (tests/test_navmap.py)
and the GPU tests (tests/test_navmap_gpu.py).  A map case builds a small storey, runs it through `run(points, colors, zero, poses,
**params) -> dict` (runner(): holoagent_amd._lib.nav_floor_maps on one library or the other) and compares EVERY output with
tests/navmap_reference.py by array_equal: nothing here has a tolerance.  The cases that take the library itself (the boundary
capacity, the graph and scene calls, Graph.create_nav_graph, the Voronoi graph) are at the end."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from tests import navmap_reference as NR
from tests import parity_common as PC

MAPS = ("obstacle_map", "region_map", "poses_map", "free_map", "main_free_map")


def pose_at(x, y, z):
    p = np.eye(4)
    p[:3, 3] = (x, y, z)
    return p


def compare(got, ref, what=""):
    assert tuple(got["grid"]) == tuple(ref["grid"]), (what, got["grid"], ref["grid"])
    assert np.array_equal(got["pcd_min"], ref["pcd_min"]) and np.array_equal(got["pcd_max"], ref["pcd_max"]), what
    for k in MAPS:
        g = np.asarray(got[k])
        assert g.dtype == ref[k].dtype and g.shape == ref[k].shape, (what, k, g.dtype, g.shape, ref[k].shape)
        assert np.array_equal(g, ref[k]), (what, k, int((g != ref[k]).sum()))
    m16 = np.asarray(got["obstacle_map"]) * 16
    assert np.array_equal(m16, np.round(m16)), what
    assert (got["n_regions"], got["main_label"], got["main_area"]) == (ref["n_regions"], ref["main_label"], ref["main_area"]), what
    rc = np.asarray(got["boundary_rc"])
    assert rc.dtype == np.int32 and np.array_equal(rc, ref["boundary_rc"]), (what, rc.shape, ref["boundary_rc"].shape)
    assert np.array_equal(rc, np.argwhere(ref["boundary"]).astype(np.int32)), what            # row-major order
    if "top_down_bgr" in ref:
        assert np.array_equal(np.asarray(got["top_down_bgr"]), ref["top_down_bgr"]), (what, "top_down_bgr")
    else:
        assert "top_down_bgr" not in got, what


def check(run, points, colors, zero, poses, what="", ties="project", **params):
    ref = NR.floor_maps(points, colors, zero, poses, ties=ties, **params)
    got = run(points, colors, zero, poses, **params)
    compare(got, ref, what)
    return got, ref


# ------------------------------------------------------------------------------------------ scenes
def room(seed, size_x=6.0, size_z=4.0, n_floor=9000, n_wall=6000, n_box=1500, zero=0.0, door=True):
    """a walled room with a cupboard (an obstacle inside) and a door gap in one wall; heights relative to `zero`"""
    rng = np.random.default_rng(seed)
    fl = np.c_[rng.uniform(0, size_x, n_floor), zero + rng.uniform(0.0, 0.02, n_floor), rng.uniform(0, size_z, n_floor)]
    t = rng.uniform(0, 1, n_wall)
    side = rng.integers(0, 4, n_wall)
    wx = np.where(side == 0, 0.0, np.where(side == 1, size_x, t * size_x))
    wz = np.where(side < 2, t * size_z, np.where(side == 2, 0.0, size_z))
    wall = np.c_[wx, zero + rng.uniform(0.0, 2.7, n_wall), wz]
    if door:
        wall = wall[~((side == 2) & (np.abs(wx - size_x * 0.6) < 0.45) & (wall[:, 1] < zero + 2.0))]
    box = np.c_[rng.uniform(1.0, 1.6, n_box), zero + rng.uniform(0.0, 2.2, n_box), rng.uniform(1.2, 2.4, n_box)]
    pts = np.concatenate([fl, wall, box])
    pts = pts[rng.permutation(len(pts))]
    cols = rng.uniform(0, 1, pts.shape)
    poses = [pose_at(rng.uniform(2.5, 5.0), zero + 0.8 + rng.uniform(-0.01, 0.01), rng.uniform(0.8, 3.2)) for _ in range(12)]
    return pts, cols, float(zero), np.array(poses)


def from_cells(floor_cells, obstacle_cells, cell=0.25, zero=0.0):
    """points on the lower edges of cells (cell = 0.25: exact in binary): floor cells at height zero, obstacle cells at zero + 2.0,
    and two anchors above every band that fix the bounds, so that the grid is exactly the masks' shape"""
    H, W = floor_cells.shape
    pts = []
    for mask, y in ((floor_cells, zero), (obstacle_cells, zero + 2.0)):
        r, c = np.nonzero(mask)
        pts.append(np.c_[c * cell, np.full(len(r), y), r * cell])
    pts.append(np.array([[0.0, zero + 3.0, 0.0], [(W - 1) * cell, zero + 3.0, (H - 1) * cell]]))
    pts = np.concatenate(pts)
    assert tuple(NR.grid_of(pts, cell)[2]) == (W, H)
    return pts


FAR = np.array([pose_at(-1000.0, 0.8, -1000.0)] * 5)          # poses whose discs are wholly outside any grid
RAW = dict(cell_size=0.25, dilation=0, blur=0)                # the maps are the cells themselves


# ------------------------------------------------------------------------------------------ cases
def rooms(run):
    """whole rooms at the reference's parameters: widths that are no multiple of 64, a door, a cupboard"""
    for seed, sx, sz, z0 in ((1, 6.0, 4.0, 0.0), (2, 3.31, 5.77, -1.37), (3, 2.0, 2.0, 10.25)):
        pts, cols, zero, poses = room(seed, sx, sz, zero=z0)
        got, ref = check(run, pts, cols, zero, poses, what="room %d" % seed)
        assert got["grid"][0] % 64 and ref["boundary_rc"].shape[0] > 50
    pts, cols, zero, poses = room(4, 2.5, 2.2)
    check(run, pts, cols, zero, poses, what="rule 1", region_rule=1)


def one_column_and_one_row(run):
    rng = np.random.default_rng(5)
    n = 3000
    for axis in (0, 2):
        pts = np.c_[rng.uniform(0, 3, n), rng.uniform(0, 2.7, n), rng.uniform(0, 3, n)]
        pts[:, axis] = 1.25
        pts[pts[:, 2 - axis] > 0.8, 1] *= 0.45                               # obstacles at one end only
        cols = rng.uniform(0, 1, pts.shape)
        poses = np.array([pose_at(1.25, 0.8, 1.25)] * 6)
        got, ref = check(run, pts, cols, 0.0, poses, what="flat axis %d" % axis)
        assert got["grid"][0 if axis == 0 else 1] == 1


def cell_edges_and_band_limits(run):
    """coordinates exactly on cell edges and on the cloud's maximum (cell 0.25 is exact in binary); heights exactly on each band
    limit, the limit formed as zero + c in float64"""
    rng = np.random.default_rng(6)
    for zero in (0.0, 0.1, -2.3):
        xs, zs = np.meshgrid(np.arange(0, 41) * 0.25, np.arange(0, 23) * 0.25)
        base = np.c_[xs.ravel(), np.full(xs.size, zero), zs.ravel()]
        limits = [zero + 1.4, zero + 2.5, zero + 1.5, np.nextafter(zero + 1.4, 9), np.nextafter(zero + 2.5, -9), np.nextafter(zero + 1.5, -9)]
        extra = np.c_[rng.integers(0, 12, 600) * 0.25, rng.choice(limits, 600), rng.integers(0, 23, 600) * 0.25]
        base[rng.random(len(base)) < 0.5, 1] = zero + 2.6                # holes in the floor
        pts = np.concatenate([base, extra])
        cols = rng.uniform(0, 1, pts.shape)
        poses = np.array([pose_at(5.0, zero + 0.8, 2.5)] * 5)
        got, ref = check(run, pts, cols, zero, poses, what="limits %r" % zero, cell_size=0.25)
        assert got["grid"] == (41, 23)
        check(run, pts, cols, zero, poses, what="limits raw %r" % zero, **RAW)


def obstacles_at_the_border(run):
    """obstacle cells in a corner and along an edge: the clipped dilation and the reflected blur"""
    H, W = 37, 70
    fl = np.ones((H, W), bool)
    for k, cells in enumerate(([(0, 0)], [(H - 1, W - 1)], [(0, c) for c in range(10, 30)], [(r, W - 1) for r in range(5, 20)],
                               [(1, 1), (H - 2, 0), (17, 33)], [(r, 0) for r in range(H)])):
        ob = np.zeros((H, W), bool)
        for r, c in cells:
            ob[r, c] = True
        pts = from_cells(fl, ob)
        got, ref = check(run, pts, None, 0.0, FAR, what="border %d" % k, cell_size=0.25)
        assert 0 < (ref["obstacle_map"] > 0).sum() < H * W and len(np.unique(ref["obstacle_map"])) > 3


def poses_and_discs(run):
    rng = np.random.default_rng(7)
    pts, cols, zero, _ = room(8, 4.0, 3.0, n_floor=500)                  # a sparse floor: the discs decide what is free
    cell = 0.03
    mn = pts.min(axis=0)

    def at(cx, cz, h=0.8):                                               # a pose `cx`, `cz` cells from the cloud's minimum
        return pose_at(mn[0] + cx * cell, h, mn[2] + cz * cell)
    sets = {
        "inside": [at(60, 50)] * 5,
        "partly outside": [at(3, 4), at(130, 2), at(50.5, 99)] + [at(60, 50)] * 2,
        "fully outside": [at(-40, -40)] * 3 + [at(70, 50)] * 3,
        "minus 0.4 and 1.2 cells": [at(-0.4, 30), at(30, -1.2), at(-1.2, -0.4), at(60, 50), at(61, 50)],
        "fewer than 5: all noise": [at(40, 40, 0.8), at(80, 60, 0.83), at(20, 70, 0.86)],
        "two clusters of equal count": [at(30 + 3 * i, 40, 0.8) for i in range(6)] + [at(30 + 3 * i, 70, 1.3) for i in range(6)],
        "noise wins a tie": [at(30 + 3 * i, 40, 0.8) for i in range(5)] + [at(90, 20 + 9 * i, 1.2 + 0.3 * i) for i in range(5)],
        "spread heights": [at(20 + 5 * i, 30 + 2 * i, 0.7 + 0.021 * i) for i in range(14)],
    }
    for name, poses in sets.items():
        got, ref = check(run, pts, None, zero, np.array(poses), what=name)
        assert ref["poses_map"].any(), name
    assert not NR.floor_maps(pts, None, zero, np.array([at(-40, -40)] * 5))["poses_map"].any()
    check(run, pts, None, zero, np.array([at(-40, -40)] * 5), what="every disc outside")
    _, labels = NR.select_poses([p[1, 3] for p in sets["fewer than 5: all noise"]])
    assert (labels == -1).all()
    _, labels = NR.select_poses([p[1, 3] for p in sets["two clusters of equal count"]])
    assert sorted(np.bincount(labels)) == [6, 6]


def top_down_cases(run):
    rng = np.random.default_rng(9)
    cell = 0.03
    # fifty points in one cell, equal and unequal height cells, in shuffled order
    for trial in range(4):
        ys = np.concatenate([np.full(20, 0.3001 + 0.0001 * trial), rng.uniform(0.0, 0.31, 30)])      # several in the top height cell
        one = np.c_[rng.uniform(0.30, 0.3299, 50), ys, rng.uniform(0.60, 0.6299, 50)]
        rest = np.c_[rng.uniform(0, 1.5, 400), rng.uniform(0, 1.7, 400), rng.uniform(0, 1.1, 400)]
        pts = np.concatenate([one, rest[:399], np.zeros((1, 3))])[rng.permutation(450)]
        cols = rng.uniform(0, 1, pts.shape)
        cols[rng.random(450) < 0.1] = (1.0, 0.0, 1.0)
        check(run, pts, cols, 0.0, np.array([pose_at(0.7, 0.8, 0.5)] * 5), what="one cell %d" % trial)
    # an image 2 cells wide, and 2 cells high: the median's borders meet
    for axis in (0, 2):
        pts = np.c_[rng.uniform(0, 2, 1500), rng.uniform(0, 1.0, 1500), rng.uniform(0, 2, 1500)]
        pts[:, axis] = rng.uniform(0, 0.02, 1500)
        pts[0, axis], pts[1, axis] = 0.0, 0.02
        cols = rng.uniform(0, 1, pts.shape)
        got, ref = check(run, pts, cols, 0.0, np.array([pose_at(0.01, 0.8, 0.01)] * 5), what="two wide %d" % axis)
        assert got["grid"][0 if axis == 0 else 1] == 2
    got, ref = check(run, pts, None, 0.0, np.array([pose_at(0.01, 0.8, 0.01)] * 5), what="no colours")
    assert "top_down_bgr" not in got


def serpentine(run):
    """a corridor one cell wide through a 96 x 96 grid, its turns joined by corners only: one label has to travel 4000 cells"""
    H = W = 96
    fl = np.zeros((H, W), bool)
    for k, r in enumerate(range(1, H - 1, 2)):
        fl[r, 1:W - 1] = True
        if r + 2 < H - 1:                                                 # the turns touch the corridor by their corners only
            fl[r + 1, W - 1 if k % 2 == 0 else 0] = True
    fl[H - 1, 3:9] = True                                                 # a second, small component on the border
    got, ref = check(run, from_cells(fl, np.zeros((H, W), bool)), None, 0.0, FAR, what="serpentine", region_rule=1, **RAW)
    assert ref["n_regions"] == 3 and ref["main_area"] > 4000
    # how many rounds (of four scans) the labelling took depends on the order the cells are run in -- the simulator runs a scan's
    # cells in raster order and carries a label down a whole row at once, the GPU does not -- so it is printed, not asserted
    print("serpentine: labelling rounds", run.label_rounds())
    assert run.label_rounds() >= 1
    check(run, from_cells(fl, np.zeros((H, W), bool)), None, 0.0, FAR, what="serpentine rule 0", **RAW)


def free_larger_than_background(run):
    """the reference's own rule returns the BACKGROUND when the free region is the larger of the two; rule 1 does not"""
    H, W = 40, 90
    fl = np.ones((H, W), bool)
    ob = np.zeros((H, W), bool)
    ob[10:14, 20:60] = True
    ob[30, 5] = True
    fl[0:3, 70:75] = False
    pts = from_cells(fl, ob)
    got, ref = check(run, pts, None, 0.0, FAR, what="background wins", ties="numpy", **RAW)
    assert ref["main_label"] == 0 and np.array_equal(ref["main_free_map"], 1 - ref["free_map"]) and ref["areas"][1] > ref["areas"][0]
    got, ref = check(run, pts, None, 0.0, FAR, what="rule 1", region_rule=1, **RAW)
    assert ref["main_label"] == 1 and np.array_equal(ref["main_free_map"], ref["free_map"])
    # ... and touches the image edge on all four sides: boundary cells on the border
    assert ref["boundary"][0].any() and ref["boundary"][-1].any() and ref["boundary"][:, 0].any() and ref["boundary"][:, -1].any()


def equal_areas(run):
    """components of equal area: this project's rule (the larger label first), not numpy's"""
    H, W = 30, 70
    for layout in range(3):
        fl = np.zeros((H, W), bool)
        if layout == 0:                                                   # two equal components, both larger than nothing else
            fl[2:8, 3:13], fl[15:25, 40:46] = True, True                 # 60 and 60
        elif layout == 1:                                                 # three equal ones
            fl[1:4, 1:21], fl[10:20, 5:11], fl[22:28, 50:60] = True, True, True
        else:                                                             # a component as large as the background
            fl[:, :35] = True
        pts = from_cells(fl, np.zeros((H, W), bool))
        for rule in (0, 1):
            got, ref = check(run, pts, None, 0.0, FAR, what="equal %d rule %d" % (layout, rule), region_rule=rule, **RAW)
        areas = NR.floor_maps(pts, None, 0.0, FAR, **RAW)["areas"]
        assert len(set(areas.tolist())) < len(areas)


def larger(run):
    """3 * 10^5 points on a 700 x 500 grid (the GPU module only)"""
    rng = np.random.default_rng(11)
    pts, cols, zero, poses = room(12, 699 * 0.03 - 0.01, 499 * 0.03 - 0.01, n_floor=200000, n_wall=80000, n_box=20000)
    got, ref = check(run, pts, cols, zero, poses, what="larger")
    assert got["grid"] == (700, 500) and len(pts) >= 290000


def refusals(run, raises):
    """no poses, none left, no free cell, a boundary list that is too short"""
    pts, cols, zero, poses = room(13, 2.0, 2.0, n_floor=2000, n_wall=1500, n_box=300)
    with raises():
        run(pts, cols, zero, np.zeros((0, 4, 4)))
    with raises():                                                        # all noise, and no height within eps of the mean
        run(pts, cols, zero, np.array([pose_at(1, 0.2, 1), pose_at(1, 0.5, 1), pose_at(1, 2.0, 1)]))
    H, W = 12, 20
    fl = np.ones((H, W), bool)
    with raises():                                                        # obstacles everywhere: no free cell
        run(from_cells(fl, fl), None, 0.0, FAR, **RAW)
    with raises():
        run(pts, cols, zero, poses, blur=5)
    for bad in (np.nan, np.inf, -np.inf):                                 # a pose height that is not finite (a failed localisation)
        track = poses.copy()
        track[3, 1, 3] = bad
        with raises():
            run(pts, cols, zero, track)
        cloud = pts.copy()                                                # ... and a coordinate of the cloud
        cloud[17, int(np.isnan(bad)) * 2] = bad
        with raises():
            run(cloud, cols, zero, poses)
        cloud = pts.copy()
        cloud[5, 1] = bad
        with raises():
            run(cloud, cols, zero, poses)
    track = poses.copy()
    track[:, 0, 3], track[:, 2, 3] = np.nan, np.inf                       # x and z may be anything: the discs fall outside
    with np.errstate(invalid="ignore"):                                   # (numpy's own cast of NaN to int32 warns)
        check(run, pts, None, zero, track, what="poses nowhere")


ALL = (rooms, one_column_and_one_row, cell_edges_and_band_limits, obstacles_at_the_border, poses_and_discs, top_down_cases, serpentine,
       free_larger_than_background, equal_areas)


# ------------------------------------------------------------------------------------------ cases that take the library
def runner(L, wrap=None):
    """run(points, colors, zero, poses, **params) -> dict of numpy arrays; wrap: how the cloud is handed over (a device tensor)"""
    from holoagent_amd._lib import nav_floor_maps

    def run(points, colors, zero, poses, **params):
        if wrap is not None:
            points, colors = wrap(points), None if colors is None else wrap(colors)
        out = nav_floor_maps(points, colors, zero, poses, lib_=L, **params)
        return {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in out.items()}

    def label_rounds():
        n = C.c_int32(0)
        L.c.hmsg_test_nav_last(C.byref(n))
        return n.value
    run.label_rounds = label_rounds                     # the labelling rounds (four scans each) of the last call
    return run


def raises():
    from holoagent_amd._lib import HmsgError
    return pytest.raises(HmsgError)


def capacity_too_small(L):
    """a boundary list that is too short: an error, n_boundary says what is needed, the maps are written"""
    from holoagent_amd._lib import HmsgNavMaps, _ptr, nav_grid, nav_params
    pts, cols, zero, poses = room(21, 2.0, 2.0, n_floor=2000, n_wall=1500, n_box=300)
    ref = NR.floor_maps(pts, None, zero, poses)
    need = len(ref["boundary_rc"])
    _, _, (W, H) = nav_grid(pts, 0.03, lib_=L)
    prm = nav_params(L)
    P_ = np.ascontiguousarray(poses.reshape(-1, 16))
    for cap in (need - 1, 0, need):
        rc, main = np.full((max(cap, 1), 2), -7, np.int32), np.zeros((H, W), np.uint8)
        out = HmsgNavMaps()
        out.main_free_map, out.boundary_rc, out.boundary_capacity = _ptr(main), _ptr(rc), cap
        status = L.c.hmsg_nav_floor_maps(0, C.byref(prm), len(pts), _ptr(pts), None, zero, len(P_), _ptr(P_), C.byref(out))
        assert out.n_boundary == need and np.array_equal(main, ref["main_free_map"])
        if cap < need:
            assert status != 0 and (rc == -7).all()
        else:
            assert status == 0 and np.array_equal(rc, ref["boundary_rc"])
    # without a list the count alone comes back
    out = HmsgNavMaps()
    assert L.c.hmsg_nav_floor_maps(0, C.byref(prm), len(pts), _ptr(pts), None, zero, len(P_), _ptr(P_), C.byref(out)) == 0
    assert out.n_boundary == need and (out.grid[0], out.grid[1]) == (W, H)


def built_graph(L):
    from holoagent_amd._lib import SceneGraph
    from holoagent_amd.synth import SceneSpec, SynthScene
    D = 16
    spec = SceneSpec(seed=31, rooms_x=1, rooms_z=1, room_size=(3.6, 2.5, 3.2), objects_per_room=4, width=64, height=48, n_frames=6, n_masks=8,
                     feat_dim=D, yaw_step_deg=25.0)
    scn = SynthScene(spec)
    frames = [scn.frame(i) for i in range(spec.n_frames)]
    S = PC.stack_frames(frames)
    sc = PC.make_scene(L, frames, dict(feat_dim=D, outlier_nb_points=20, outlier_radius=0.3, feat_dbscan_min=8))
    sc.add_frames(S["rgb"], S["depth"], S["pose"], S["K"])
    sc.finalize_map()
    sc.add_frame_features(0, S["masks"], S["f_g"], S["f_masked"], S["f_crop"], S["n_masks"])
    sc.fuse_frames()
    sc.merge_instances()
    sc.pool_instances()
    return sc, SceneGraph.build(sc, S["pose"], S["f_g"], num_views=3, host_threads=1), S["pose"]


def graph_call_equals_generic_call(L, tmp_path):
    """hmsg_graph_nav_floor_maps on a built graph == hmsg_nav_floor_maps on the slab taken through hmsg_get_map_points, and both
    == the restatement; a loaded graph is refused"""
    from holoagent_amd._lib import HmsgError, SceneGraph, nav_floor_maps
    sc, g, poses = built_graph(L)
    xyz, rgb = sc.map_points(colors=True)
    fl = sc.segment_floors()[0]
    slab = (xyz[:, 1] >= fl["y_lo"]) & (xyz[:, 1] <= fl["y_hi"])
    assert 0 < slab.sum()
    # the cameras of the synthetic scene stand still: give every pose the same height above the floor, spread over the room
    track = np.array(poses, np.float64).reshape(-1, 4, 4).copy()
    track[:, 1, 3] = fl["zero_level"] + 0.8
    got = g.nav_floor_maps(0, track, cell_size=0.05)
    want = nav_floor_maps(xyz[slab], rgb[slab], fl["zero_level"], track, lib_=L, cell_size=0.05)
    ref = NR.floor_maps(xyz[slab], rgb[slab], fl["zero_level"], track, cell_size=0.05)
    for k in MAPS + ("top_down_bgr", "boundary_rc", "pcd_min", "pcd_max"):
        assert np.array_equal(got[k], want[k]), k
    assert (got["n_regions"], got["main_label"], got["main_area"], got["grid"]) == (want["n_regions"], want["main_label"], want["main_area"], want["grid"])
    compare(got, ref, "graph")
    mn, mx, grid = g.nav_grid(0, 0.05)
    assert np.array_equal(mn, ref["pcd_min"]) and np.array_equal(mx, ref["pcd_max"]) and grid == ref["grid"]
    with pytest.raises(HmsgError, match="no such floor"):
        g.nav_floor_maps(7, track)
    g.save(tmp_path / "graph")
    lg = SceneGraph.load(tmp_path / "graph", lib_=L)
    with pytest.raises(HmsgError, match="hmsg_load"):
        lg.nav_floor_maps(0, track)
    with pytest.raises(HmsgError, match="hmsg_load"):
        lg.nav_grid(0)
    lg.close()
    g.close()
    sc.close()


class _Floor:
    def __init__(self, zero, floor_id):
        self.floor_zero_level, self.floor_height, self.floor_id = zero, 2.7, floor_id


def voronoi_graph(L, tmp_path, wrap=None):
    """get_voronoi_graph on the library's maps == the same function on the restatement's maps: nodes, pos, edges, dist, in order;
    and the JSON bytes of save_voronoi_graph"""
    from holoagent_amd.nav_graph import NavigationGraph
    pts, cols, zero, poses = room(41, 3.0, 2.4, n_floor=5000, n_wall=4000, n_box=900)
    ref = NR.floor_maps(pts, cols, zero, poses)
    cloud = (pts, cols) if wrap is None else (wrap(pts), wrap(cols))
    nav = NavigationGraph(cloud, 0.03, lib_=L)
    assert np.array_equal(nav.pcd_min, ref["pcd_min"]) and tuple(nav.grid_size) == ref["grid"]
    g = nav.get_floor_graph(_Floor(zero, "2"), list(poses), str(tmp_path / "maps"))
    assert g is nav.sparse_floor_voronoi and np.array_equal(np.asarray(nav.top_down.cpu() if hasattr(nav.top_down, "cpu") else nav.top_down),
                                                             ref["top_down_bgr"])
    assert sorted(os.listdir(tmp_path / "maps")) == ["floor_free.png", "floor_free_main.png", "floor_obstacles.png", "floor_region.png",
                                                     "poses_region_map.png", "top_down_rgb.png"]
    from PIL import Image
    assert np.array_equal(np.asarray(Image.open(tmp_path / "maps" / "floor_free_main.png")), ref["main_free_map"] * 255)
    assert np.array_equal(np.asarray(Image.open(tmp_path / "maps" / "top_down_rgb.png")), ref["top_down_bgr"][:, :, ::-1])
    other = NavigationGraph((pts, cols), 0.03, lib_=L)              # the same function, the restatement's maps, the cells found on the host
    want = other.get_voronoi_graph(ref["main_free_map"], None, None, 2)
    assert len(g.nodes) > 50 and len(g.edges) > 50
    assert list(g.nodes) == list(want.nodes) and list(g.edges) == list(want.edges)
    for n in g.nodes:
        assert g.nodes[n] == want.nodes[n]
    for e in g.edges:
        assert g.edges[e] == want.edges[e]
    for n, d in list(g.nodes(data=True))[:20]:                       # the pos formula: (col, height, row) of the vertex in metres
        assert d["pos"] == (n[1] * 0.03 + ref["pcd_min"][0], ref["pcd_min"][1], n[0] * 0.03 + ref["pcd_min"][2]) and d["floor_id"] == 2
        assert ref["main_free_map"][int(n[0]), int(n[1])] == 1
    NavigationGraph.save_voronoi_graph(g, str(tmp_path), "a")
    NavigationGraph.save_voronoi_graph(want, str(tmp_path), "b")
    a, b = open(tmp_path / "a_graph.json", "rb").read(), open(tmp_path / "b_graph.json", "rb").read()
    assert a == b
    doc = json.loads(a)
    assert set(doc) >= {"nodes", "links"} and len(doc["links"]) == len(g.edges) and doc["nodes"][0]["id"][2] == 2
    # a second floor's graph hung on the first by the closest pair
    up = nav.get_voronoi_graph(nav.maps["main_free_map"], None, None, 3)
    nav.has_stairs = True
    both = nav.connect_stairs_and_floor_graphs(up, g)
    assert len(both.nodes) == len(g.nodes) + len(up.nodes) and len(both.edges) == len(g.edges) + len(up.edges) + 1


def create_nav_graph_on_a_built_scene(L, tmp_path):
    """Graph.create_nav_graph on a Graph built from frames -- its floors are slabs of the resident map, so NavigationGraph works on a
    SceneSlab and nothing of the storey goes to the host -- writes the files that the same loop writes on the slab read back
    through hmsg_get_map_points; Scene.nav_floor_maps equals the generic call on that slab."""
    from holoagent_amd._lib import nav_floor_maps
    from holoagent_amd.nav_graph import NavigationGraph, SceneSlab
    from tests.test_semseg_evaluate import build_graph
    g = build_graph(L)
    g.segment_floors_manually()
    assert g.floors and all(getattr(fl, "_crop", None) is not None for fl in g.floors) and g.scene is not None
    sc, fl = g.scene, g.floors[0]
    xyz, rgb = sc.map_points(colors=True)
    slab = (xyz[:, 1] >= fl._crop[0]) & (xyz[:, 1] <= fl._crop[1])
    rng = np.random.default_rng(3)
    lo, hi = xyz[slab].min(0), xyz[slab].max(0)
    track = [pose_at(rng.uniform(lo[0], hi[0]), fl.floor_zero_level + 0.9, rng.uniform(lo[2], hi[2])) for _ in range(12)]
    got = sc.nav_floor_maps(fl._crop[0], fl._crop[1], fl.floor_zero_level, np.array(track), cell_size=0.05)
    want = nav_floor_maps(xyz[slab], rgb[slab], fl.floor_zero_level, np.array(track), lib_=L, cell_size=0.05)
    for k in MAPS + ("top_down_bgr", "boundary_rc", "pcd_min", "pcd_max"):
        assert np.array_equal(got[k], want[k]), k
    compare(got, NR.floor_maps(xyz[slab], rgb[slab], fl.floor_zero_level, np.array(track), cell_size=0.05), "scene slab")
    nav = NavigationGraph(SceneSlab(sc, *fl._crop), 0.03, lib_=L)
    assert nav.points is None and len(nav.get_floor_poses(fl, track)) == 12
    # the whole loop: the scene's floors against the same floors as host clouds
    g.create_nav_graph(nav_dir=str(tmp_path / "a"), poses_list=track)
    host = type(g)({}, lib=L)
    for f in g.floors:
        keep = (xyz[:, 1] >= f._crop[0]) & (xyz[:, 1] <= f._crop[1])
        h = type(f)(f.floor_id, f.name)
        h.pcd = type("Cloud", (), dict(points=xyz[keep], colors=rgb[keep]))()
        h.floor_zero_level, h.floor_height = f.floor_zero_level, f.floor_height
        host.floors.append(h)
    host.create_nav_graph(nav_dir=str(tmp_path / "b"), poses_list=track)
    for name in ("sparse_voronoi_graph.json", "global_nav_graph_graph.json"):
        a, b = open(tmp_path / "a" / name, "rb").read(), open(tmp_path / "b" / name, "rb").read()
        assert a == b and len(json.loads(a)["nodes"]) > 3, name
    sc.close()
