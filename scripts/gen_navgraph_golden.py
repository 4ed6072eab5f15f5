"""Golden generator for the navigation graph: runs the REFERENCE's own NavigationGraph (graph/navigation_graph.py) and the loop of
Graph.create_nav_graph (graph.py:2081-2127) on two seeded scenes and stores inputs + answers as tests/golden/navgraph.npz.  Nothing
of the reference travels: only data.

    python scripts/gen_navgraph_golden.py [output.npz]        # from the repo root, where the reference checkout exists

The reference is imported with the recipe of oracle/refdrive/gen_golden.py.  OpenCV is not installed; the module's `cv2` is replaced
by the stand-in below, which supplies the calls the path makes: dilate (a zero-bordered maximum filter), GaussianBlur 3 x 3 ((1, 2,
1) x (1, 2, 1) / 16 in float32 on a border reflected without the edge), circle (the midpoint walk of tests/navmap_reference.py),
connectedComponentsWithStats (scipy.ndimage.label, full structure), cvtColor (channel reversal / grey to three channels), and
no-op line / imwrite / applyColorMap.  What the fixture pins is therefore the reference's own arithmetic AROUND those calls: bands,
cells, the pose selection with sklearn, the free-map algebra, argsort's pick, the top-down loop, the median filter, erosion,
scipy's Voronoi and the ridge filter, the stairs track and sparsify_graph, the connections, node_link_data.

Scenes: `one`: a storey of about 2.5 * 10^4 points with a door and a cupboard, 40 poses (no second storey: has_stairs False);
`two`: two storeys of about 6 * 10^3 points each and a pose track that walks floor 0, climbs and walks floor 1 (has_stairs True).
"""
from __future__ import annotations

import json
import os
import sys
import tempfile
import types

import numpy as np

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, REPO)


def standin_cv2():
    from scipy import ndimage
    from tests import navmap_reference as NR
    cv2 = types.ModuleType("cv2")
    cv2.COLOR_RGB2BGR, cv2.COLOR_GRAY2BGR, cv2.CV_8UC1, cv2.COLORMAP_JET = 4, 8, 0, 2

    def dilate(img, kernel, iterations=1):
        assert iterations == 1
        return ndimage.maximum_filter(img, size=kernel.shape, mode="constant", cval=0)

    def gaussian_blur(img, ksize, sigma):
        assert tuple(ksize) == (3, 3) and sigma == 0 and img.dtype == np.float32
        pad = np.pad(img, 1, mode="reflect")
        k = (np.outer([1, 2, 1], [1, 2, 1]) / 16).astype(np.float32)
        out = np.zeros(img.shape, np.float32)
        for dr in range(3):
            for dc in range(3):
                out += k[dr, dc] * pad[dr:dr + img.shape[0], dc:dc + img.shape[1]]
        return out

    def circle(img, center, radius, color, thickness):
        if img.ndim == 2 and thickness == -1:
            assert color == 1
            NR.circle(img, center, radius)                  # (drawings on colour images are debug output: not reproduced)
        return img

    def connected(img, connectivity, ltype):
        assert connectivity == 8
        labels, n = ndimage.label(img, structure=np.ones((3, 3), int))
        areas = np.bincount(labels.ravel(), minlength=n + 1)
        stats = np.zeros((n + 1, 5), np.int32)
        stats[:, -1] = areas
        return n + 1, labels.astype(np.int32), stats, None

    def cvt_color(img, code):
        if code == cv2.COLOR_GRAY2BGR:
            return np.repeat(img[:, :, None], 3, axis=2)
        return np.ascontiguousarray(img[:, :, ::-1])
    cv2.dilate, cv2.GaussianBlur, cv2.circle, cv2.connectedComponentsWithStats, cv2.cvtColor = dilate, gaussian_blur, circle, connected, cvt_color
    cv2.line = lambda img, *a, **k: img
    cv2.imwrite = lambda *a, **k: True
    cv2.applyColorMap = lambda img, cm: img
    return cv2


class Cloud:
    def __init__(self, points, colors):
        self.points, self.colors = points, colors


class FloorStub:
    def __init__(self, floor_id, points, colors, zero, height):
        self.floor_id, self.pcd, self.floor_zero_level, self.floor_height = str(floor_id), Cloud(points, colors), zero, height


def pose_at(x, y, z):
    p = np.eye(4)
    p[:3, 3] = (x, y, z)
    return p


def compact(floor):
    """the cloud as the fixture stores it: coordinates that float32 holds exactly, colours that are whole 255ths (tests/test_navgraph_golden.py
    reads them back with the same two expressions)"""
    floor["points32"] = floor["points"].astype(np.float32)
    floor["colors8"] = np.round(floor["colors"] * 255).astype(np.uint8)
    floor["points"] = floor["points32"].astype(np.float64)
    floor["colors"] = floor["colors8"].astype(np.float64) / 255.0
    return floor


def scene_one(rng):
    from tests.navmap_cases import room
    pts, cols, zero, _ = room(20261021, 5.0, 3.6, n_floor=14000, n_wall=9000, n_box=2000)
    poses = [pose_at(rng.uniform(2.2, 4.5), 0.85, rng.uniform(0.6, 3.0)) for _ in range(40)]      # one height: one peak, no stairs
    return [compact(dict(points=pts, colors=cols, zero=zero, height=2.7))], poses


def scene_two(rng):
    from tests.navmap_cases import room
    floors = []
    for k, z0 in enumerate((0.0, 3.0)):
        pts, cols, zero, _ = room(77 + k, 3.0, 2.4, n_floor=3500, n_wall=2200, n_box=500, zero=z0)
        floors.append(compact(dict(points=pts, colors=cols, zero=zero, height=2.7)))
    poses = []
    for i in range(60):                                    # floor 0: camera 0.8 m above it
        poses.append(pose_at(1.8 + 0.9 * np.cos(i / 9.0), 0.8 + rng.uniform(-0.004, 0.004), 1.2 + 0.7 * np.sin(i / 9.0)))
    for i in range(30):                                    # the stairs
        poses.append(pose_at(2.7 - 0.02 * i, 0.8 + 3.0 * (i + 1) / 31.0, 1.9 - 0.04 * i))
    for i in range(60):                                    # floor 1
        poses.append(pose_at(1.8 + 0.9 * np.cos(i / 9.0), 3.8 + rng.uniform(-0.004, 0.004), 1.2 + 0.7 * np.sin(i / 9.0)))
    return floors, poses


def graph_arrays(prefix, g):
    """a graph as arrays: node ids (row, col, floor), pos, edges as index pairs, dist -- all in the graph's own order"""
    nodes = list(g.nodes)
    index = {n: i for i, n in enumerate(nodes)}
    return {prefix + "_nodes": np.array([[n[0], n[1], float(n[2])] for n in nodes], np.float64).reshape(-1, 3),
            prefix + "_pos": np.array([g.nodes[n]["pos"] for n in nodes], np.float64).reshape(-1, 3),
            prefix + "_edges": np.array([[index[a], index[b]] for a, b in g.edges], np.int64).reshape(-1, 2),
            prefix + "_dist": np.array([g.edges[e]["dist"] for e in g.edges], np.float64)}


def run_reference(NG, floors, poses_list, out, name):
    """the loop of Graph.create_nav_graph (graph.py:2081-2127) with the reference's own NavigationGraph"""
    nav_dir = tempfile.mkdtemp()
    stubs = [FloorStub(i, f["points"], f["colors"], f["zero"], f["height"]) for i, f in enumerate(floors)]
    last, global_voronoi = None, None
    for floor_id, floor in enumerate(stubs):
        nav = NG.NavigationGraph(floor.pcd, cell_size=0.03)
        upper = stubs[floor_id + 1].floor_zero_level if floor_id + 1 < len(stubs) else None
        floor_poses = nav.get_floor_poses(floor, poses_list, upper)
        stairs = nav.get_stairs_graph_with_poses_v2(floor, floor_id, poses_list, nav_dir)
        has_stairs = bool(nav.has_stairs)
        main_free = nav.get_main_free_map(floor.pcd, {"floor_zero_level": floor.floor_zero_level, "floor_height": floor.floor_height}, nav_dir,
                                          floor_poses)
        graph = nav.get_floor_graph(floor, floor_poses, nav_dir)
        key = "%s_f%d" % (name, floor_id)
        out.update({key + "_points": floors[floor_id]["points32"], key + "_colors": floors[floor_id]["colors8"], key + "_zero": np.float64(floor.floor_zero_level),
                    key + "_height": np.float64(floor.floor_height), key + "_n_floor_poses": np.int64(len(floor_poses)),
                    key + "_main_free_map": np.asarray(main_free, np.uint8), key + "_map": np.asarray(nav.map, np.float32),
                    key + "_top_down": np.asarray(nav.top_down, np.uint8), key + "_has_stairs": np.bool_(has_stairs)})
        out.update(graph_arrays(key + "_floor", graph))
        out.update(graph_arrays(key + "_stairs", stairs))
        if stairs is not None:
            graph = nav.connect_stairs_and_floor_graphs(stairs, graph, nav_dir)
        out.update(graph_arrays(key + "_connected", graph))
        NG.NavigationGraph.save_voronoi_graph(graph, nav_dir, "sparse_voronoi")
        out[key + "_json"] = np.frombuffer(open(os.path.join(nav_dir, "sparse_voronoi_graph.json"), "rb").read(), np.uint8)
        if last is not None and last.has_stairs:
            global_voronoi = nav.connect_voronoi_graphs(last.sparse_floor_voronoi, nav.sparse_floor_voronoi)
        last = nav
    if global_voronoi is None:
        global_voronoi = last.sparse_floor_voronoi
    NG.NavigationGraph.save_voronoi_graph(global_voronoi, nav_dir, "global_nav_graph")
    out.update(graph_arrays(name + "_global", global_voronoi))
    out[name + "_global_json"] = np.frombuffer(open(os.path.join(nav_dir, "global_nav_graph_graph.json"), "rb").read(), np.uint8)
    out[name + "_poses"] = np.array(poses_list, np.float64)
    out[name + "_n_floors"] = np.int64(len(floors))


def main(path):
    from oracle.refdrive.gen_golden import import_reference
    import_reference()
    import memory.hmsg.graph.navigation_graph as NG
    import networkx as nx
    NG.cv2 = standin_cv2()
    NG.tqdm = lambda it, **k: it
    data = nx.node_link_data
    nx.node_link_data = lambda g, **k: data(g, edges="links", **k)          # (networkx 3.4 warns about the default: the layout is the same)
    rng = np.random.Generator(np.random.PCG64(20261021))
    out = {}
    devnull = open(os.devnull, "w")
    old, sys.stdout = sys.stdout, devnull                                   # (the reference prints)
    try:
        for name, make in (("one", scene_one), ("two", scene_two)):
            floors, poses = make(rng)
            run_reference(NG, floors, poses, out, name)
    finally:
        sys.stdout = old
        devnull.close()
    np.savez_compressed(path, **out)
    print("navgraph ok:", {k: (int(out[k + "_n_floors"]), bool(out[k + "_f0_has_stairs"]), len(out[k + "_global_nodes"])) for k in ("one", "two")},
          os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(REPO, "tests", "golden", "navgraph.npz"))
