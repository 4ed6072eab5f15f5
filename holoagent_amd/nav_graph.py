"""A floor's navigation graph (the reference's graph/navigation_graph.py NavigationGraph): the image half on the device
(include/hmsg.h: hmsg_nav_floor_maps, or hmsg_map_nav_floor_maps for a SceneSlab of a resident map -- obstacle map, free map, its main region, the boundary cells in row-major order, the
top-down image), the graph half on the host with the same scipy.spatial.Voronoi call the reference makes.  Given an identical,
identically ordered boundary list Qhull numbers vertices and ridges identically, so nodes, `pos`, edges and `dist` come out in the
reference's order.

What is here: the grid (to_grid / to_world), get_floor_poses, the maps (get_main_free_map, get_poses_region, get_top_down_rgb_map,
create_occupancy_grid's result as `map`), get_voronoi_graph, sparsify_graph, trim_graph, get_stairs_graph_with_poses_v2,
get_floor_graph, connect_voronoi_graphs, connect_stairs_and_floor_graphs and save_voronoi_graph: what Graph.create_nav_graph
calls.  The stairs graph and sparsify_graph are host code on a few hundred poses (numpy, scipy.signal, networkx).  The debug
drawings and histogram plots are not reproduced; the map PNGs are written with Pillow when a directory is given.  Out of scope
(DESIGN.md): get_height_map, compute_sdf and the older get_stairs_graph* variants.  tests/golden/navgraph.npz holds what the
reference's own class gives on two scenes; tests/test_navgraph_golden.py compares everything exactly.

Beyond the reference (include/hmsg.h, N7): clearance_map, distance_field and route work on the maps this object already holds --
exact integer distance fields on main_free_map, the nearest reachable free cell of a goal and the cells of the way, on the device.
N8: sight_blocking_map, viewpoints and route_to_view stand the robot on a reached cell from which the goal is in sight on the
obstacle map, not on the nearest one whatever lies between.  N10: height_map is the storey's exact integer height map;
viewpoints and route_to_view with sight="heights" judge sight on it from the camera's height, and max_step_m keeps routes off
cells that the flat maps leave free under furniture (walkable_map).  N11: room_seeds, room_map, doors and rooms_along lay a list
of rooms over the free map -- the room of every reached cell, the doors between rooms with their cells, the rooms along a way."""
import json
import os

import numpy as np

from . import _lib


def _cloud(floor_pcd):
    """(points [n, 3], colors [n, 3] or None) of an Open3D-like cloud, a (points, colors) pair or a bare array"""
    if hasattr(floor_pcd, "points"):
        pts, cols = floor_pcd.points, getattr(floor_pcd, "colors", None)
    elif isinstance(floor_pcd, (tuple, list)) and len(floor_pcd) == 2:
        pts, cols = floor_pcd
    else:
        pts, cols = floor_pcd, None
    on_dev = hasattr(pts, "data_ptr") and getattr(pts, "is_cuda", False)
    if not on_dev:
        pts = np.ascontiguousarray(np.asarray(pts, np.float64).reshape(-1, 3))
        cols = None if cols is None or len(cols) == 0 else np.ascontiguousarray(np.asarray(cols, np.float64).reshape(-1, 3))
    return pts, cols


class SceneSlab:
    """a storey as it lies in HBM: the points of a resident scene's map with y_lo <= y <= y_hi and their colours (what
    Scene.segment_floors returns for it).  NavigationGraph takes it in place of a cloud; nothing of it goes to the host."""

    def __init__(self, scene, y_lo, y_hi):
        self.scene, self.y_lo, self.y_hi = scene, float(y_lo), float(y_hi)


class NavigationGraph:
    def __init__(self, floor_pcd, cell_size, lib_=None, device_id=0):
        self.L = lib_ or _lib.lib()
        self.device_id = int(device_id)
        self.cell_size = cell_size
        self.slab = floor_pcd if isinstance(floor_pcd, SceneSlab) else None
        if self.slab is not None:
            self.points = self.colors = None
            self.pcd_min, self.pcd_max, (gx, gz) = self.slab.scene.nav_grid(self.slab.y_lo, self.slab.y_hi, cell_size)
        else:
            self.points, self.colors = _cloud(floor_pcd)
            self.pcd_min, self.pcd_max, (gx, gz) = _lib.nav_grid(self.points, cell_size, self.device_id, self.L)
        self.grid_size = np.array([gx, gz], np.int32)
        self.has_stairs = False
        self.maps = None
        self.map = None
        self.top_down = None
        self.sparse_floor_voronoi = None
        self.zero_level = None

    # ---- the grid
    def to_grid(self, world_coords):
        return np.int32((world_coords - self.pcd_min) / self.cell_size)

    def to_world(self, grid_coords):
        return grid_coords * self.cell_size + self.pcd_min

    def get_floor_poses(self, floor, poses_list, upper_floor_min_height=None, camera_height=0.8):
        """the poses whose camera, lowered by camera_height, lies inside the floor's height range (or below the next floor's start).
        The floor's cloud is this object's: its lowest and highest y are the bounds the device call returned."""
        lo = self.pcd_min[1]
        hi = upper_floor_min_height if upper_floor_min_height is not None else self.pcd_max[1]
        return [p for p in poses_list if lo <= p[1, 3] - camera_height < hi]

    # ---- the image half: one device call, kept for all the map getters
    def floor_maps(self, floor_info, floor_poses_list, **params):
        poses = np.asarray(floor_poses_list, np.float64).reshape(-1, 4, 4)
        self.zero_level = float(floor_info["floor_zero_level"])
        if self.slab is not None:
            self.maps = self.slab.scene.nav_floor_maps(self.slab.y_lo, self.slab.y_hi, float(floor_info["floor_zero_level"]), poses,
                                                       cell_size=self.cell_size, **params)
            self.map = self.maps["obstacle_map"]
            return self.maps
        self.maps = _lib.nav_floor_maps(self.points, self.colors, float(floor_info["floor_zero_level"]), poses, lib_=self.L,
                                        device_id=self.device_id, cell_size=self.cell_size, **params)
        self.map = self.maps["obstacle_map"]
        return self.maps

    @staticmethod
    def _png(floor_dir, name, img):
        if floor_dir is None:
            return
        from PIL import Image
        os.makedirs(floor_dir, exist_ok=True)
        a = img.cpu().numpy() if hasattr(img, "cpu") else np.asarray(img)
        Image.fromarray(a if a.ndim == 2 else np.ascontiguousarray(a[:, :, ::-1])).save(os.path.join(floor_dir, name))

    def get_main_free_map(self, floor_pcd=None, floor_info=None, floor_dir=None, floor_poses_list=None, save=True, **params):
        m = self.floor_maps(floor_info, floor_poses_list, **params)
        if save and floor_dir is not None:
            for name, key in (("poses_region_map.png", "poses_map"), ("floor_region.png", "region_map"), ("floor_free.png", "free_map"),
                              ("floor_free_main.png", "main_free_map")):
                self._png(floor_dir, name, m[key] * 255)
            obst = m["obstacle_map"].cpu().numpy() if hasattr(m["obstacle_map"], "cpu") else m["obstacle_map"]
            self._png(floor_dir, "floor_obstacles.png", obst.astype(np.uint8) * 255)
        return m["main_free_map"]

    def get_poses_region(self, poses_list=None, floor_dir=None, radius=0.5, save=True, cluster=True):
        assert self.maps is not None, "get_main_free_map makes the maps"
        return self.maps["poses_map"]

    def get_top_down_rgb_map(self, floor_pcd=None, floor_info=None, floor_dir=None):
        assert self.maps is not None and "top_down_bgr" in self.maps, "get_main_free_map makes the maps; the cloud needs colours"
        self._png(floor_dir, "top_down_rgb.png", self.maps["top_down_bgr"])
        return self.maps["top_down_bgr"]

    # ---- routes on the main free map (include/hmsg.h, N7: the rules R1 to R6; no counterpart in the reference)
    def cells_of(self, xyz_or_rc):
        """(row, col) int32 [n, 2]: of world points [n, 3] by R6, floor((v - pcd_min) / cell_size) in float64 for z (row) and x
        (col) -- not to_grid's truncation; [n, 2] arrays are cells already"""
        a = np.asarray(xyz_or_rc.cpu() if hasattr(xyz_or_rc, "cpu") else xyz_or_rc)
        a = a.reshape(-1, a.shape[-1]) if a.ndim > 1 else a.reshape(1, -1)
        if a.shape[1] == 2:
            return np.ascontiguousarray(a.astype(np.int32))
        assert a.shape[1] == 3, "world points [n, 3] or cells [n, 2]"
        a = a.astype(np.float64)
        rc = np.stack([np.floor((a[:, 2] - self.pcd_min[2]) / self.cell_size), np.floor((a[:, 0] - self.pcd_min[0]) / self.cell_size)], axis=1)
        return np.ascontiguousarray(np.clip(rc, -2.0 ** 31, 2.0 ** 31 - 1).astype(np.int32))

    def clearance_units(self, min_clearance_m, w_straight=5):
        return int(np.ceil(float(min_clearance_m) / self.cell_size * w_straight))

    def clearance_map(self, **weights):
        """R3 of main_free_map: int32 [rows, cols] in field units (metres = value * cell_size / w_straight), where the maps are"""
        assert self.maps is not None, "get_main_free_map makes the maps"
        return _lib.nav_clearance(self.maps["main_free_map"], lib_=self.L, device_id=self.device_id, **weights)

    def walkable_map(self, max_step_m=None):
        """main_free_map (max_step_m None), or its cells whose height-map top is at most max_step_m above the zero level: what the
        robot can roll over.  main_free_map alone only loses what the obstacle band (1.4 to 2.5 m by default) holds, so a low box
        in a room stays in it."""
        assert self.maps is not None, "get_main_free_map makes the maps"
        main = self.maps["main_free_map"]
        if max_step_m is None:
            return main
        top = self.height_map()["top_map"]
        step = int(np.floor(float(max_step_m) / self.height_unit))
        if hasattr(top, "to"):
            import torch
            return ((main != 0) & (top.to(torch.int32) <= step)).to(main.dtype)
        return ((main != 0) & (top <= step)).astype(np.uint8)

    def passable_map(self, min_clearance_m=0.0, max_step_m=None, **weights):
        """main_free_map where the clearance is at least min_clearance_m (0: the map itself).  max_step_m: walkable_map(max_step_m)
        in main_free_map's place, the clearance being that mask's own."""
        assert self.maps is not None, "get_main_free_map makes the maps"
        main = self.walkable_map(max_step_m)
        units = self.clearance_units(min_clearance_m, weights.get("w_straight", 5))
        if units <= 0:
            return main
        clearance = self.clearance_map(**weights) if max_step_m is None else _lib.nav_clearance(main, lib_=self.L, device_id=self.device_id, **weights)
        ok = (main != 0) & (clearance >= units)
        return ok.to(main.dtype) if hasattr(ok, "to") else ok.astype(np.uint8)

    def distance_field(self, sources_xyz_or_rc, min_clearance_m=0.0, max_step_m=None, **weights):
        """R2 from the given sources (world points [n, 3] or cells [n, 2]) on passable_map(min_clearance_m, max_step_m): int32 [rows, cols]"""
        fields, _ = _lib.nav_distance_fields(self.passable_map(min_clearance_m, max_step_m, **weights), [self.cells_of(sources_xyz_or_rc)],
                                             lib_=self.L, device_id=self.device_id, **weights)
        return fields[0]

    def route(self, start_xyz, goals_xyz, min_clearance_m=0.0, max_step_m=None, **weights):
        """hmsg_nav_route from start_xyz to every goal (world points, or cells): per goal a dict with the stand-on `point` in world
        coordinates (the centre of the snapped cell, y = pcd_min[1]), its `cell`, `reachable`, `length_m` (None when not
        reachable), `snap_m` (how far the goal's cell is from the cell stood on) and the `polyline` [k, 3] from the start.
        max_step_m: routed on walkable_map(max_step_m)."""
        assert self.maps is not None, "get_main_free_map makes the maps"
        ws = int(weights.get("w_straight", 5))
        r = _lib.nav_route(self.walkable_map(max_step_m), self.cells_of(start_xyz)[0], self.cells_of(goals_xyz), lib_=self.L, device_id=self.device_id,
                           min_clearance=self.clearance_units(min_clearance_m, ws), **weights)
        r = {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in r.items()}
        self.last_route = r

        def world(rc):
            rc = np.asarray(rc, np.float64).reshape(-1, 2)
            return np.stack([(rc[:, 1] + 0.5) * self.cell_size + self.pcd_min[0], np.full(len(rc), self.pcd_min[1]),
                             (rc[:, 0] + 0.5) * self.cell_size + self.pcd_min[2]], axis=1)
        out = []
        for k, cell in enumerate(r["goal_cell"]):
            ok = bool(cell[0] >= 0 and r["goal_dist"][k] != _lib.NAV_UNREACHED)
            out.append(dict(point=world(cell)[0] if ok else None, cell=(int(cell[0]), int(cell[1])), reachable=ok,
                            length_m=float(r["goal_dist"][k]) * self.cell_size / ws if ok else None,
                            snap_m=float(np.sqrt(float(r["goal_d2"][k]))) * self.cell_size if ok else None,
                            polyline=world(r["path_rc"][r["path_off"][k]:r["path_off"][k + 1]])))
        return out

    # ---- rooms on the main free map (include/hmsg.h, N11: the rules G1, G2, D1 to D4, L1; no counterpart in the reference)
    def room_seeds(self, rooms):
        """per room (anything with `vertices`, the (x, z) pairs of Room.vertices) the cells of its vertices by R6, int32 [k, 2];
        vertices outside the grid are left out, a room without vertices has no seed"""
        rows, cols = int(self.grid_size[1]), int(self.grid_size[0])
        out = []
        for room in rooms:
            v = np.asarray(getattr(room, "vertices", room), np.float64).reshape(-1, 2)
            rc = self.cells_of(np.stack([v[:, 0], np.zeros(len(v)), v[:, 1]], axis=1)) if len(v) else np.zeros((0, 2), np.int32)
            ok = (rc[:, 0] >= 0) & (rc[:, 0] < rows) & (rc[:, 1] >= 0) & (rc[:, 1] < cols)
            out.append(np.ascontiguousarray(rc[ok]))
        return out

    def _room_doors(self, rooms, min_clearance_m, max_step_m, weights):
        """hmsg_nav_room_doors on walkable_map(max_step_m), kept until the rooms or the parameters change"""
        assert self.maps is not None, "get_main_free_map makes the maps"
        seeds = self.room_seeds(rooms)
        key = (float(min_clearance_m), max_step_m, tuple(sorted(weights.items())), tuple(s.tobytes() for s in seeds))
        if getattr(self, "_rooms_key", None) != key:
            ws = int(weights.get("w_straight", 5))
            self._rooms = _lib.nav_room_doors(self.walkable_map(max_step_m), seeds, lib_=self.L, device_id=self.device_id,
                                              min_clearance=self.clearance_units(min_clearance_m, ws), **weights)
            self._rooms_key = key
        return self._rooms

    def room_map(self, rooms, min_clearance_m=0.0, max_step_m=None, **weights):
        """G2: int32 [rows, cols], for every cell of passable_map(min_clearance_m, max_step_m) the index in `rooms` of the room whose
        seeds are nearest by the walk (of equal walks the smaller index), -1 where no seed reaches; where the maps are"""
        return self._room_doors(rooms, min_clearance_m, max_step_m, weights)["label"]

    def doors(self, rooms, min_clearance_m=0.0, max_step_m=None, **weights):
        """D1 to D4: the doors between the rooms in the table's order, each a dict with `rooms` (p, q) as indices in `rooms`, its
        `cells` int32 [n, 2] in row-major order, `n_cells`, the `middle_cell` (row, col) at position (n - 1) // 2 and `middle`, that
        cell's centre in world coordinates (y = pcd_min[1])"""
        t = self._room_doors(rooms, min_clearance_m, max_step_m, weights)
        np_ = lambda v: v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)
        pair, off, rc = np_(t["door_pair"]), np_(t["door_off"]), np_(t["door_rc"])
        out = []
        for k in range(len(pair)):
            cells = rc[off[k]:off[k + 1]]
            row, col = (int(v) for v in cells[(len(cells) - 1) // 2])
            out.append(dict(rooms=(int(pair[k, 0]), int(pair[k, 1])), cells=cells, n_cells=len(cells), middle_cell=(row, col),
                            middle=np.array([(col + 0.5) * self.cell_size + self.pcd_min[0], self.pcd_min[1],
                                             (row + 0.5) * self.cell_size + self.pcd_min[2]])))
        return out

    def rooms_along(self, path_cells, rooms=None, min_clearance_m=0.0, max_step_m=None, **weights):
        """L1: the legs of one way (cells int32 [k, 2]) on the room map made last, or on room_map(rooms, ...): a list of dicts with
        `room` (the index, -1 off every room), `first` (the index of the leg's first cell) and `n_cells`"""
        t = self._room_doors(rooms, min_clearance_m, max_step_m, weights) if rooms is not None else getattr(self, "_rooms", None)
        assert t is not None, "room_map or doors makes the room map"
        cells = self.cells_of(path_cells) if len(path_cells) else np.zeros((0, 2), np.int32)
        _, room, first = (v.cpu().numpy() if hasattr(v, "cpu") else v for v in
                          _lib.nav_path_rooms(t["label"], np.array([0, len(cells)], np.int64), cells, lib_=self.L, device_id=self.device_id))
        ends = list(first[1:]) + [len(cells)]
        return [dict(room=int(r), first=int(a), n_cells=int(b - a)) for r, a, b in zip(room, first, ends)]

    # ---- viewpoints (include/hmsg.h, N8: the rules V1 to V5; no counterpart in the reference)
    def sight_blocking_map(self):
        """what blocks a sight line: obstacle_map > 0 as u8 [rows, cols], where the maps are"""
        assert self.maps is not None, "get_main_free_map makes the maps"
        ob = self.maps["obstacle_map"] > 0
        if hasattr(ob, "to"):
            import torch
            return ob.to(torch.uint8)
        return ob.astype(np.uint8)

    def view_band(self, view_range_m):
        """(r_min2, r_max2) in cells of a (near, far) range in metres: int(m / cell_size), squared; V5 bounds the far end"""
        near, far = (int(float(m) / self.cell_size) for m in view_range_m)
        if far > 255:
            raise ValueError("view_range_m: the far bound is %d cells, hmsg_nav_viewpoints takes 255 at the most" % far)
        return near * near, far * far

    @staticmethod
    def _prefer(prefer):
        if prefer not in ("walk", "look"):
            raise ValueError('prefer: "walk" (least walk) or "look" (closest look)')
        return 0 if prefer == "walk" else 1

    # ---- the height map and sight with heights (include/hmsg.h, N10: the rules H1 to H3 and S1 to S5)
    height_unit = 0.01                        # metres per height unit of the kept height map (height_map sets it)

    def height_map(self, floor_pcd=None, **params):
        """hmsg_nav_height_map of the storey (this object's cloud or SceneSlab; floor_pcd: another cloud or slab of the same grid),
        zero_level the one the maps were made with: made once and kept as self.maps["top_map"] (u16 [rows, cols], height units
        above the zero level) and self.maps["known_map"] (u8), where the other maps are.  params: height_unit, top_max, dilation;
        asked again with other values it is made again."""
        assert self.maps is not None and self.zero_level is not None, "get_main_free_map makes the maps and sets the zero level"
        key = tuple(sorted(params.items()))
        if "top_map" in self.maps and getattr(self, "_height_key", None) == key and floor_pcd is None:
            return self.maps
        src = floor_pcd if floor_pcd is not None else (self.slab if self.slab is not None else self.points)
        if isinstance(src, SceneSlab):
            m = src.scene.nav_height_map(src.y_lo, src.y_hi, self.zero_level, cell_size=self.cell_size, **params)
        else:
            m = _lib.nav_height_map(_cloud(src)[0], self.zero_level, lib_=self.L, device_id=self.device_id, cell_size=self.cell_size, **params)
        assert tuple(m["grid"]) == (int(self.grid_size[0]), int(self.grid_size[1])), "the height map's cloud has another grid"
        self.maps.update(top_map=m["top"], known_map=m["known"])
        self._height_key = key
        self.height_unit = float(params.get("height_unit", 0.01))
        return self.maps

    def eye_units(self, camera_height_m):
        """a camera height above the zero level in the height map's units, as S1 takes it"""
        return int(min(max(np.floor(float(camera_height_m) / self.height_unit), 0), 65535))

    def _sight(self, sight, goals_xyz, n, camera_height_m, goal_heights_m, goal_radius_m):
        """None for sight "map"; for "heights" (top_map, eye, goal_h int32 [n], goal_r2 int64 [n] or None).  goal_heights_m:
        metres above the zero level, one or [n]; default: the goals' own y (world points only).  goal_radius_m: the goals'
        footprints in metres, one or [n]: ceil(radius / cell_size), squared."""
        if sight == "map":
            return None
        if sight != "heights":
            raise ValueError('sight: "map" (the obstacle map) or "heights" (the height map)')
        top = self.height_map()["top_map"]
        if goal_heights_m is None:
            g = np.asarray(goals_xyz.cpu() if hasattr(goals_xyz, "cpu") else goals_xyz, np.float64)
            g = g.reshape(-1, g.shape[-1]) if g.ndim > 1 else g.reshape(1, -1)
            if g.shape[1] != 3:
                raise ValueError('sight "heights": goals given as cells need goal_heights_m')
            goal_heights_m = g[:, 1] - self.zero_level
        gh = np.floor(np.broadcast_to(np.asarray(goal_heights_m, np.float64), (n,)) / self.height_unit).clip(0, 65535).astype(np.int32)
        gr2 = None
        if goal_radius_m is not None:
            cells = np.ceil(np.broadcast_to(np.asarray(goal_radius_m, np.float64), (n,)) / self.cell_size).clip(0, 2 ** 20).astype(np.int64)
            gr2 = cells * cells
        return top, self.eye_units(camera_height_m), gh, gr2

    def viewpoints(self, goals, start=None, min_clearance_m=0.0, view_range_m=(0.0, 3.0), prefer="walk", want_visible=False, sight="map",
                   camera_height_m=1.5, goal_heights_m=None, goal_radius_m=None, max_step_m=None, **weights):
        """hmsg_nav_viewpoints for every goal (world points [n, 3] or cells [n, 2]) on passable_map(min_clearance_m) and
        sight_blocking_map(): _lib.nav_viewpoints' dict, where the maps are.  start (a world point or a cell): only cells reached
        from it, snapped by R4 as route snaps it, are candidates, and view_dist is the walk to them.  sight "heights":
        hmsg_nav_viewpoints_h on height_map() from camera_height_m above the zero level (_sight says how the goals' heights and
        footprints are given)."""
        r_min2, r_max2 = self.view_band(view_range_m)
        pas = self.passable_map(min_clearance_m, max_step_m, **weights)
        goal_cells = self.cells_of(goals)
        hs = self._sight(sight, goals, len(goal_cells), camera_height_m, goal_heights_m, goal_radius_m)
        field = None
        if start is not None:
            cell, _ = _lib.nav_snap_cells(pas, self.cells_of(start), lib_=self.L, device_id=self.device_id)
            cell = cell.cpu().numpy() if hasattr(cell, "cpu") else cell
            field = self.distance_field(cell if cell[0, 0] >= 0 else np.zeros((0, 2), np.int32), min_clearance_m, max_step_m, **weights)
        if hs is not None:
            return _lib.nav_viewpoints_h(hs[0], pas, goal_cells, hs[1], hs[2], hs[3], field=field, want_visible=want_visible, lib_=self.L,
                                         device_id=self.device_id, r_min2=r_min2, r_max2=r_max2, prefer=self._prefer(prefer))
        return _lib.nav_viewpoints(self.sight_blocking_map(), pas, goal_cells, field=field, want_visible=want_visible, lib_=self.L,
                                   device_id=self.device_id, r_min2=r_min2, r_max2=r_max2, prefer=self._prefer(prefer))

    def route_to_view(self, start_xyz, goals_xyz, min_clearance_m=0.0, view_range_m=(0.0, 3.0), prefer="walk", sight="map", camera_height_m=1.5,
                      goal_heights_m=None, goal_radius_m=None, max_step_m=None, **weights):
        """hmsg_nav_view_route: route's dict per goal, the cell stood on being the goal's viewpoint (V4: in sight of the goal within
        view_range_m, the least walk or the closest look) in place of R4's nearest cell.  Added: `n_visible` (the cells the goal
        is seen from), `facing` (a float64 unit (x, z) vector from the stand-on point to the goal's world point -- a cell's centre
        for a goal given as a cell -- or (0, 0) when both lie in one cell; None when not reachable) and `yaw` = atan2(facing_x,
        facing_z).  A goal that no reached cell sees is not reachable.  sight "heights": hmsg_nav_view_route_h, as viewpoints
        has it; max_step_m: routed on walkable_map(max_step_m)."""
        assert self.maps is not None, "get_main_free_map makes the maps"
        ws = int(weights.get("w_straight", 5))
        r_min2, r_max2 = self.view_band(view_range_m)
        goal_cells = self.cells_of(goals_xyz)
        hs = self._sight(sight, goals_xyz, len(goal_cells), camera_height_m, goal_heights_m, goal_radius_m)
        common = dict(lib_=self.L, device_id=self.device_id, min_clearance=self.clearance_units(min_clearance_m, ws), r_min2=r_min2, r_max2=r_max2,
                      prefer=self._prefer(prefer), **weights)
        if hs is not None:
            r = _lib.nav_view_route_h(self.walkable_map(max_step_m), hs[0], self.cells_of(start_xyz)[0], goal_cells, hs[1], hs[2], hs[3], **common)
        else:
            r = _lib.nav_view_route(self.walkable_map(max_step_m), self.sight_blocking_map(), self.cells_of(start_xyz)[0], goal_cells, **common)
        r = {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in r.items()}
        self.last_route = r

        def world(rc):
            rc = np.asarray(rc, np.float64).reshape(-1, 2)
            return np.stack([(rc[:, 1] + 0.5) * self.cell_size + self.pcd_min[0], np.full(len(rc), self.pcd_min[1]),
                             (rc[:, 0] + 0.5) * self.cell_size + self.pcd_min[2]], axis=1)
        g = np.asarray(goals_xyz.cpu() if hasattr(goals_xyz, "cpu") else goals_xyz, np.float64)
        g = g.reshape(-1, g.shape[-1]) if g.ndim > 1 else g.reshape(1, -1)
        goal_points = g if g.shape[1] == 3 else world(goal_cells)
        out = []
        for k, cell in enumerate(r["goal_cell"]):
            ok = bool(cell[0] >= 0 and r["goal_dist"][k] != _lib.NAV_UNREACHED)
            point = world(cell)[0] if ok else None
            facing = yaw = None
            if ok:
                d = np.array([goal_points[k, 0] - point[0], goal_points[k, 2] - point[2]], np.float64)
                same = tuple(int(v) for v in cell) == tuple(int(v) for v in goal_cells[k])
                facing = np.zeros(2) if same or not d.any() else d / np.sqrt(d[0] * d[0] + d[1] * d[1])
                yaw = float(np.arctan2(facing[0], facing[1]))
            out.append(dict(point=point, cell=(int(cell[0]), int(cell[1])), reachable=ok,
                            length_m=float(r["goal_dist"][k]) * self.cell_size / ws if ok else None,
                            snap_m=float(np.sqrt(float(r["goal_d2"][k]))) * self.cell_size if ok else None,
                            polyline=world(r["path_rc"][r["path_off"][k]:r["path_off"][k + 1]]), n_visible=int(r["n_visible"][k]),
                            facing=facing, yaw=yaw))
        return out

    # ---- the graph half
    def get_voronoi_graph(self, main_free_map, map_rgb=None, floor_dir=None, floor_id=0, name="", height_map=None, boundary_rc=None):
        """The Voronoi graph of the boundary cells, filtered as the reference filters it: a ridge is kept when both its vertices are
        finite, inside the image and on a cell of main_free_map.  boundary_rc: the device's list (default: this object's, when
        main_free_map is the map it came with; otherwise the cells are found on the host)."""
        import networkx as nx
        from scipy.spatial import Voronoi
        main = main_free_map.cpu().numpy() if hasattr(main_free_map, "cpu") else np.asarray(main_free_map)
        if boundary_rc is None and self.maps is not None and main_free_map is self.maps["main_free_map"]:
            boundary_rc = self.maps["boundary_rc"]
        if boundary_rc is None:
            from scipy.ndimage import binary_erosion
            boundary_rc = np.argwhere(main.astype(bool) & ~binary_erosion(main.astype(bool)))
        elif hasattr(boundary_rc, "cpu"):
            boundary_rc = boundary_rc.cpu().numpy()
        vor = Voronoi(np.asarray(boundary_rc).astype(np.int64))
        H, W = main.shape[:2]
        if height_map is None:
            height_map = np.ones((H, W), np.uint8) * self.pcd_min[1]
        g = nx.Graph()

        def node(v):
            key = (v[0], v[1], floor_id)
            if key not in g.nodes:
                g.add_node(key, pos=(v[1] * self.cell_size + self.pcd_min[0], height_map[int(v[0]), int(v[1])],
                                     v[0] * self.cell_size + self.pcd_min[2]), floor_id=floor_id)
            return key
        for ridge in vor.ridge_vertices:
            ridge = np.asarray(ridge)
            if np.any(ridge < 0):
                continue
            src, tar = vor.vertices[ridge]
            if not (0 <= src[0] < H and 0 <= src[1] < W and 0 <= tar[0] < H and 0 <= tar[1] < W):
                continue
            if main[int(src[0]), int(src[1])] == 0 or main[int(tar[0]), int(tar[1])] == 0:
                continue
            a, b = node(src), node(tar)
            if a not in g[b]:
                g.add_edge(a, b, dist=np.linalg.norm(src - tar))
        return g

    def sparsify_graph(self, floor_graph, resampling_dist=0.4):
        """The nodes of degree other than 2 stay; every pair of them whose shortest path runs over degree-2 nodes only is joined
        directly, and the path between them is re-sampled every resampling_dist metres (its dist, in cells, times cell_size).
        Edges are added in the order the reference adds them.  A graph of fewer than 10 nodes comes back as a copy."""
        import copy
        import networkx as nx
        graph = copy.deepcopy(floor_graph)
        if len(graph.nodes) < 10:
            return graph
        out = nx.Graph()
        for n in graph.nodes:
            if graph.degree(n) != 2:
                out.add_node(n, pos=graph.nodes[n]["pos"], floor_id=graph.nodes[n]["floor_id"])
        kept, kept_set = list(out.nodes), set(out.nodes)
        paths = dict(nx.all_pairs_dijkstra_path(graph, weight="dist"))
        todo = []
        for i, a in enumerate(kept):
            for b in kept[i + 1:]:
                try:
                    path = paths[a][b]
                    if any(graph.degree(n) > 2 for n in path[1:-1]):
                        continue
                    todo.append((path[0], path[-1], np.linalg.norm(np.array(path[0]) - np.array(path[-1]))))
                    steps = [graph.edges[path[k], path[k + 1]]["dist"] for k in range(len(path) - 1)]
                    if len(path) and not set(path[1:-1]) & kept_set:
                        run, prev = 0, path[0]
                        for k, n in enumerate(path[1:-1]):
                            run += steps[k]
                            if run * self.cell_size > resampling_dist:
                                todo.append((prev, n, np.linalg.norm(np.array(prev) - np.array(n))))
                                prev, run = n, 0
                        todo.append((prev, path[-1], np.linalg.norm(np.array(prev) - np.array(path[-1]))))
                except BaseException:                         # (no path between the two, or ids that do not subtract: the pair is skipped)
                    continue
        for a, b, d in todo:
            for n in (a, b):
                if n not in out.nodes:
                    out.add_node(n, pos=graph.nodes[n]["pos"], floor_id=graph.nodes[n]["floor_id"])
            out.add_edge(a, b, dist=d)
        self.floor_graph = out
        return out

    def trim_graph(self, graph, trim_deg=1):
        """nodes of degree trim_deg removed, round after round, until none is left"""
        import copy
        graph = copy.deepcopy(graph)
        while True:
            ends = [n for n in list(graph.nodes) if graph.degree(n) == trim_deg]
            if not ends:
                return graph
            graph.remove_nodes_from(ends)

    def get_stairs_graph_with_poses_v2(self, floor, floor_id, poses_list, floor_dir=None):
        """The stairs above floor `floor_id` as the chain of camera positions between two storeys: the storeys are the peaks of the
        histogram (100 bins) of the pose heights less 1.5 m that reach 0.3 of the highest bin; the track (reversed when it comes
        down) is cut from where it last leaves the lower peak's bin to where it first passes the upper peak, 5 poses added in
        front and 20 behind; the chain is sparsified.  No upper peak: an empty graph and has_stairs False."""
        import networkx as nx
        zero = floor.floor_zero_level
        poses = self.stairs_pose_track(floor_id, poses_list)
        if poses is None:
            self.has_stairs = False
            return nx.Graph()
        track = [p[:3, 3] for p in poses]
        if not track:
            self.has_stairs = False
            return nx.Graph()
        lowest = np.min([p[1] for p in track])
        chain = nx.Graph()
        last = None
        for p in track:
            cell = (p - self.pcd_min) / self.cell_size
            chain.add_node((cell[2], cell[0], floor_id), pos=(p[0], p[1] - lowest + zero, p[2]), floor_id=floor_id)
            if last is not None:
                chain.add_edge((cell[2], cell[0], floor_id), (last[2], last[0], floor_id), dist=np.linalg.norm(cell - last))
            last = cell
        sparse = self.sparsify_graph(chain, resampling_dist=0.4)
        self.has_stairs = True
        return sparse

    @staticmethod
    def stairs_pose_track(floor_id, poses_list):
        """The poses of the stairs above floor `floor_id`, as get_stairs_graph_with_poses_v2 cuts them from the camera track (see
        there): poses_list[st:ed] of the track in climbing order, or None when the pose heights show no storey above."""
        from scipy.signal import find_peaks
        heights = np.array([p[1, 3] - 1.5 for p in poses_list])
        counts, edges = np.histogram(heights, bins=100)
        padded = np.concatenate([[np.min(counts)], counts, [np.min(counts)]])
        peaks = find_peaks(padded, height=0.3 * np.max(counts))[0] - 1
        if floor_id >= len(peaks) - 1:
            return None
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
        return poses_list[st:ed]

    def get_floor_graph(self, floor, floor_poses_list, floor_dir=None, **params):
        info = {"floor_zero_level": floor.floor_zero_level, "floor_height": getattr(floor, "floor_height", None)}
        main = self.get_main_free_map(None, info, floor_dir, floor_poses_list, **params)
        self.top_down = self.get_top_down_rgb_map(None, info, floor_dir) if "top_down_bgr" in self.maps else None
        self.sparse_floor_voronoi = self.get_voronoi_graph(main, self.top_down, floor_dir, int(floor.floor_id))
        return self.sparse_floor_voronoi

    def connect_voronoi_graphs(self, src_graph, tar_graph, floor_dir=None):
        """src_graph joined to tar_graph by one edge between the closest pair (any node of src, a node of tar of degree > 1)"""
        import networkx as nx
        from scipy.spatial.distance import cdist
        tar_nodes, src_nodes = list(tar_graph.nodes), list(src_graph.nodes)
        ids = [i for i, n in enumerate(tar_nodes) if tar_graph.degree(n) > 1]
        d = cdist(np.array([src_graph.nodes[n]["pos"] for n in src_nodes]), np.array([tar_graph.nodes[tar_nodes[i]]["pos"] for i in ids]))
        row, col = np.unravel_index(np.argmin(d), d.shape)
        s, t = src_nodes[row], tar_nodes[ids[col]]
        out = nx.compose(tar_graph, src_graph)
        out.add_edge(s, t, dist=np.linalg.norm(np.array(s[:2]) - np.array(t[:2])))
        return out

    def connect_stairs_and_floor_graphs(self, sparse_stairs_voronoi, sparse_floor_voronoi, floor_dir=None):
        if not self.has_stairs:
            return sparse_floor_voronoi
        self.sparse_floor_voronoi = self.connect_voronoi_graphs(sparse_stairs_voronoi, sparse_floor_voronoi, floor_dir)
        return self.sparse_floor_voronoi

    @staticmethod
    def save_voronoi_graph(graph, floor_dir, name):
        """<floor_dir>/<name>_graph.json: networkx's node-link layout with the edges under "links", indent 4"""
        import networkx as nx
        with open(os.path.join(floor_dir, f"{name}_graph.json"), "w") as f:
            json.dump(nx.node_link_data(graph, edges="links"), f, indent=4)


# ---- routes across storeys (include/hmsg.h, N9: the rules B1 to B6; no counterpart in the reference)
def _host(v):
    return v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)


def stair_link(lower_nav, upper_nav, track, lower_id=0, upper_id=1, min_clearance_m=0.0, w_straight=5):
    """The link (B2) that a stairs' pose track (NavigationGraph.stairs_pose_track: camera-to-world poses in climbing order, or
    positions [n, 3]) makes between two storeys: the first position's cell by R6 on the lower storey's grid and the last one's on
    the upper storey's, each snapped by R4 to its storey's passable_map(min_clearance_m); cost = max(1, ceil(track length in metres
    * w_straight / cell_size)).  -> (link (sa, ra, ca, sb, rb, cb, cost) or None when a storey has no passable cell, (d2 of the
    lower snap, d2 of the upper snap))"""
    pos = np.array([np.asarray(p, np.float64)[:3, 3] if np.ndim(p) == 2 else np.asarray(p, np.float64).reshape(3) for p in track], np.float64)
    assert len(pos) >= 1, "an empty track makes no link"
    length = float(np.sqrt(((pos[1:] - pos[:-1]) ** 2).sum(axis=1)).sum())
    cost = max(1, int(np.ceil(length * w_straight / lower_nav.cell_size)))
    ends = []
    for nav, p in ((lower_nav, pos[0]), (upper_nav, pos[-1])):
        cell, d2 = _lib.nav_snap_cells(nav.passable_map(min_clearance_m, w_straight=w_straight), nav.cells_of(p), lib_=nav.L,
                                       device_id=nav.device_id)
        ends.append((tuple(int(v) for v in _host(cell)[0]), int(_host(d2)[0])))
    (a, da), (b, db) = ends
    if a[0] < 0 or b[0] < 0:
        return None, (da, db)
    return (int(lower_id),) + a + (int(upper_id),) + b + (cost,), (da, db)


class BuildingNavigation:
    """Several storeys' NavigationGraph objects (their maps made) and the links between them (B2: (storey_a, row_a, col_a,
    storey_b, row_b, col_b, cost) in field units, stair_link makes one): fields, routes and routes to a viewpoint over the whole
    building, on the device (hmsg_nav_building_fields / _route / _paths).  The storeys share one cell size; their grids are their
    own.  A link's endpoints are meant for the clearance the routes are asked with: a link whose endpoint is not passable at a
    larger clearance does not exist there."""

    def __init__(self, storeys, links, lib_=None):
        assert len(storeys) >= 1 and all(n.maps is not None for n in storeys), "get_main_free_map makes a storey's maps"
        assert all(n.cell_size == storeys[0].cell_size for n in storeys), "one cell size for the building"
        self.storeys = list(storeys)
        self.links = [tuple(int(v) for v in l) for l in links]
        self.L = lib_ or storeys[0].L
        self.device_id = storeys[0].device_id
        self.cell_size = storeys[0].cell_size
        self.last_route = None

    def _level(self, l):
        nav = self.storeys[l]
        return nav.zero_level if nav.zero_level is not None else float(nav.pcd_min[1])

    def world(self, triples):
        """cell centres of (storey, row, col) triples in world coordinates, y = the storey's zero level -> float64 [n, 3]"""
        t = np.asarray(triples, np.int64).reshape(-1, 3)
        out = np.zeros((len(t), 3), np.float64)
        for k, (l, r, c) in enumerate(t):
            nav = self.storeys[l]
            out[k] = ((c + 0.5) * nav.cell_size + nav.pcd_min[0], self._level(l), (r + 0.5) * nav.cell_size + nav.pcd_min[2])
        return out

    def triples_of(self, floors, xyz_or_rc):
        """(storey, row, col) int32 [n, 3] of world points (or cells) on the given storeys, by R6 on each storey's own grid"""
        a = _host(xyz_or_rc)
        a = a.reshape(-1, a.shape[-1]) if a.ndim > 1 else a.reshape(1, -1)
        floors = np.broadcast_to(np.asarray(floors, np.int64).reshape(-1), (len(a),))
        out = np.zeros((len(a), 3), np.int32)
        for k, l in enumerate(floors):
            out[k] = (l,) + tuple(self.storeys[int(l)].cells_of(a[k])[0])
        return out

    def passables(self, min_clearance_m=0.0, **weights):
        return [n.passable_map(min_clearance_m, **weights) for n in self.storeys]

    def fields(self, start_floor, start_xyz_or_rc, min_clearance_m=0.0, **weights):
        """B3 from the start as it is (a world point or a cell of storey start_floor; no snap): one int32 [rows_l, cols_l] per
        storey, where the maps are"""
        f, _ = _lib.nav_building_fields(self.passables(min_clearance_m, **weights), self.links, self.triples_of(start_floor, start_xyz_or_rc),
                                        lib_=self.L, device_id=self.device_id, **weights)
        return [x[0] for x in f]

    def _dicts(self, r, ws):
        out = []
        for k, cell in enumerate(r["goal_cell"]):
            ok = bool(cell[1] >= 0 and r["goal_dist"][k] != _lib.NAV_UNREACHED)
            src = r["path_src"][r["path_off"][k]:r["path_off"][k + 1]]
            out.append(dict(point=self.world(cell)[0] if ok else None, cell=(int(cell[1]), int(cell[2])), floor=int(cell[0]), reachable=ok,
                            length_m=float(r["goal_dist"][k]) * self.cell_size / ws if ok else None,
                            snap_m=float(np.sqrt(float(r["goal_d2"][k]))) * self.cell_size if ok else None,
                            polyline=self.world(src), floors=np.ascontiguousarray(src[:, 0].astype(np.int32)),
                            cells=np.ascontiguousarray(src[:, 1:].astype(np.int32))))
        return out

    def route(self, start_floor, start_xyz, goals_xyz, goal_floors, min_clearance_m=0.0, **weights):
        """hmsg_nav_building_route from start_xyz on storey start_floor to every goal (world points or cells, goal_floors: their
        storeys): NavigationGraph.route's dict per goal -- point, cell, reachable, length_m, snap_m, polyline [k, 3] (world
        coordinates at each storey's zero level) -- plus `floor` (the cell's storey), and `floors` int32 [k] and `cells` int32
        [k, 2] beside the polyline"""
        ws = int(weights.get("w_straight", 5))
        maps = [n.maps["main_free_map"] for n in self.storeys]
        r = _lib.nav_building_route(maps, self.links, self.triples_of(start_floor, start_xyz)[0], self.triples_of(goal_floors, goals_xyz),
                                    lib_=self.L, device_id=self.device_id, min_clearance=self.storeys[0].clearance_units(min_clearance_m, ws),
                                    **weights)
        r = {k: ([_host(x) for x in v] if isinstance(v, list) else (_host(v) if hasattr(v, "cpu") else v)) for k, v in r.items()}
        self.last_route = r
        return self._dicts(r, ws)

    def route_to_view(self, start_floor, start_xyz, goals_xyz, goal_floors, min_clearance_m=0.0, view_range_m=(0.0, 3.0), prefer="walk",
                      sight="map", camera_height_m=1.5, goal_heights_m=None, goal_radius_m=None, max_step_m=None, **weights):
        """route with the cell stood on chosen so that the goal is in sight on its own storey (composed, no device code of its own):
        the start is snapped by R4, its building field made (B3), and each storey's part of it handed to hmsg_nav_viewpoints as
        the `field` with that storey's sight_blocking_map (V4: least walk from the START, or closest look); then B5 to the
        viewpoints.  route's dict plus n_visible, facing and yaw as NavigationGraph.route_to_view gives them.  sight "heights":
        hmsg_nav_viewpoints_h per storey on its height_map(), the goals' heights above their own storey's zero level (goal_heights_m
        and goal_radius_m: one value or one per goal); max_step_m: every storey's walkable_map(max_step_m) in main_free_map's place."""
        ws = int(weights.get("w_straight", 5))
        pas = [n_.passable_map(min_clearance_m, max_step_m, **weights) for n_ in self.storeys]
        st = self.triples_of(start_floor, start_xyz)[0]
        goals = self.triples_of(goal_floors, goals_xyz)
        cell, d2 = _lib.nav_snap_cells(pas[int(st[0])], st[1:], lib_=self.L, device_id=self.device_id)
        cell, d2 = _host(cell), _host(d2)
        n = len(goals)
        r = dict(start_cell=(int(st[0]), int(cell[0, 0]), int(cell[0, 1])), start_d2=int(d2[0]), goal_cell=np.full((n, 3), -1, np.int32),
                 goal_d2=np.full(n, -1, np.int64), goal_dist=np.full(n, _lib.NAV_UNREACHED, np.int32), n_visible=np.zeros(n, np.int32))
        r["goal_cell"][:, 0] = goals[:, 0]
        if cell[0, 0] >= 0:
            f, _ = _lib.nav_building_fields(pas, self.links, self.triples_of(int(st[0]), cell[0]), lib_=self.L, device_id=self.device_id, **weights)
            fields = [x[0] for x in f]
        else:
            fields = None
        if fields is not None:
            for l in sorted(set(int(v) for v in goals[:, 0])):
                nav = self.storeys[l]
                sel = np.flatnonzero(goals[:, 0] == l)
                r_min2, r_max2 = nav.view_band(view_range_m)
                per = lambda a: None if a is None else (np.asarray(a, np.float64)[sel] if np.ndim(a) else a)
                hs = nav._sight(sight, _host(goals_xyz)[sel] if np.ndim(_host(goals_xyz)) > 1 else goals_xyz, len(sel), camera_height_m,
                                per(goal_heights_m), per(goal_radius_m))
                common = dict(field=fields[l], lib_=self.L, device_id=self.device_id, r_min2=r_min2, r_max2=r_max2, prefer=nav._prefer(prefer))
                if hs is not None:
                    v = _lib.nav_viewpoints_h(hs[0], pas[l], goals[sel, 1:], hs[1], hs[2], hs[3], **common)
                else:
                    v = _lib.nav_viewpoints(nav.sight_blocking_map(), pas[l], goals[sel, 1:], **common)
                r["goal_cell"][sel, 1:] = _host(v["view_rc"])
                r["goal_d2"][sel], r["goal_dist"][sel], r["n_visible"][sel] = _host(v["view_d2"]), _host(v["view_dist"]), _host(v["n_visible"])
            off, src = _lib.nav_building_paths(pas, self.links, fields, r["goal_cell"], lib_=self.L, device_id=self.device_id, **weights)
            r["path_off"], r["path_src"] = _host(off), _host(src)
            r["fields"] = fields
        else:
            r["path_off"], r["path_src"] = np.zeros(n + 1, np.int64), np.zeros((0, 3), np.int32)
        r["passable"] = pas
        self.last_route = r
        out = self._dicts(r, ws)
        g = _host(goals_xyz).astype(np.float64)
        g = g.reshape(-1, g.shape[-1]) if g.ndim > 1 else g.reshape(1, -1)
        goal_points = g if g.shape[1] == 3 else self.world(goals)
        for k, d in enumerate(out):
            d["n_visible"] = int(r["n_visible"][k])
            d["facing"] = d["yaw"] = None
            if d["reachable"]:
                v = np.array([goal_points[k, 0] - d["point"][0], goal_points[k, 2] - d["point"][2]], np.float64)
                same = d["cell"] == (int(goals[k, 1]), int(goals[k, 2]))
                d["facing"] = np.zeros(2) if same or not v.any() else v / np.sqrt(v[0] * v[0] + v[1] * v[1])
                d["yaw"] = float(np.arctan2(d["facing"][0], d["facing"][1]))
        return out
