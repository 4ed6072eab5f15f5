"""The image half of the reference's NavigationGraph (graph/navigation_graph.py) restated with numpy, scipy and sklearn, line for
line where a line exists: the yardstick of tests/navmap_cases.py.  OpenCV's three calls are restated as the issue of the feature
pins them: cv2.dilate = a maximum filter with a zero border, cv2.GaussianBlur(3, 3) = the (1, 2, 1) x (1, 2, 1) / 16 kernel in
float32 on a reflect-padded image (edge not repeated), cv2.connectedComponentsWithStats(8) = scipy.ndimage.label with a full 3 x 3
structure, cv2.circle = the midpoint walk of circle() below."""
import numpy as np
from scipy import ndimage
from sklearn.cluster import DBSCAN


def grid_of(points, cell):
    pcd_min, pcd_max = np.min(points, axis=0), np.max(points, axis=0)
    grid = np.ceil((pcd_max - pcd_min) / cell + 1).astype(np.int32)[[0, 2]]
    return pcd_min, pcd_max, grid


def create_occupancy_grid(xz, pcd_min, grid, cell, dilation=5, blur=3):
    occ = np.zeros(grid[::-1], dtype=int)
    pc = xz - pcd_min[[0, 2]]
    x_cells = np.floor(pc[:, 0] / cell).astype(int)
    y_cells = np.floor(pc[:, 1] / cell).astype(int)
    occ[y_cells, x_cells] = 1
    if dilation > 0:
        assert dilation % 2 == 1
        occ = ndimage.maximum_filter(occ.astype(np.uint8), size=(dilation, dilation), mode="constant", cval=0)
    if blur > 0:
        assert blur == 3
        img = np.pad(occ.astype(np.float32), 1, mode="reflect")
        k = (np.outer([1, 2, 1], [1, 2, 1]) / 16).astype(np.float32)
        out = np.zeros(occ.shape, np.float32)
        for dr in range(3):
            for dc in range(3):
                out += k[dr, dc] * img[dr:dr + occ.shape[0], dc:dc + occ.shape[1]]
        occ = out
    return occ


def circle(img, center, radius):
    """cv2.circle(img, center, radius, 1, -1) as the feature's issue states OpenCV's walk"""
    cx, cy = int(center[0]), int(center[1])
    H, W = img.shape

    def fill(y, x0, x1):
        if 0 <= y < H:
            img[y, max(x0, 0):max(min(x1, W - 1) + 1, 0)] = 1
    err, dx, dy, plus, minus = 0, radius, 0, 1, 2 * radius - 1
    while dx >= dy:
        fill(cy - dy, cx - dx, cx + dx)
        fill(cy + dy, cx - dx, cx + dx)
        fill(cy - dx, cx - dy, cx + dy)
        fill(cy + dx, cx - dy, cx + dy)
        dy += 1
        err += plus
        plus += 2
        if err > 0:
            err -= minus
            dx -= 1
            minus -= 2


def select_poses(heights, eps=0.1, min_samples=5):
    """indices of the poses get_poses_region draws (:348-360)"""
    heights = np.asarray(heights, np.float64)
    clusters = DBSCAN(eps=eps, min_samples=min_samples).fit(heights.reshape(-1, 1))
    labels, counts = np.unique(clusters.labels_, return_counts=True)
    mask = clusters.labels_ == labels[np.argmax(counts)]
    major = np.mean(heights[mask])
    idx = [i for i in range(len(heights)) if np.abs(heights[i] - major) < eps]
    if not idx:
        return np.zeros(0, np.int64), clusters.labels_
    mn = np.min(heights[idx])
    return np.array([i for i in idx if heights[i] < mn + eps], np.int64), clusters.labels_


def poses_region(poses, pcd_min, grid, cell, radius=0.5, eps=0.1, min_samples=5):
    poses = np.asarray(poses, np.float64).reshape(-1, 4, 4)
    keep, _ = select_poses(poses[:, 1, 3], eps, min_samples)
    xz = poses[keep][:, [0, 2], 3]
    cells = np.int32((xz - pcd_min[[0, 2]]) / cell)
    poses_map = np.zeros(grid[::-1], dtype=np.uint8)
    for c in cells:
        circle(poses_map, tuple(c), int(radius / cell))
    return poses_map


def largest_region(free, rule=0, ties="project"):
    """get_largest_region (:316-322) -> (main bool, labels, areas, label).  ties="numpy": np.argsort's own order among equal areas."""
    labels, n = ndimage.label(free > 0, structure=np.ones((3, 3), int))
    areas = np.bincount(labels.ravel(), minlength=n + 1)
    if ties == "numpy":
        assert rule == 0
        order = np.argsort(areas)[::-1]
    else:
        order = sorted(range(1 if rule == 1 else 0, n + 1), key=lambda l: (areas[l], l), reverse=True)
    label = int(order[0 if rule == 1 else 1])
    return labels == label, labels, areas, label


def top_down(points, colors, zero, pcd_min, grid, cell, region_max=1.5):
    mask = points[:, 1] < zero + region_max
    pts, col = points[mask], colors[mask]
    verts = np.int32((pts - pcd_min) / cell)
    img = np.zeros([grid[1], grid[0], 3], dtype=np.uint8)
    height = -1000 * np.ones([grid[1], grid[0]], dtype=np.float32)
    for p_i, (c, h, r) in enumerate(verts):
        if h > height[r, c]:
            img[r, c] = (col[p_i] * 255).astype(np.uint8)
            height[r, c] = h
    img = ndimage.median_filter(img, size=3)
    return np.ascontiguousarray(img[:, :, ::-1])


def floor_maps(points, colors, zero, poses, cell_size=0.03, obstacle_lo=1.4, obstacle_hi=2.5, region_max=1.5, dilation=5, blur=3,
               pose_radius=0.5, pose_eps=0.1, pose_min_samples=5, region_rule=0, ties="project"):
    points = np.asarray(points, np.float64)
    pcd_min, pcd_max, grid = grid_of(points, cell_size)
    obst = points[points[:, 1] < zero + obstacle_hi]
    obst = obst[obst[:, 1] > zero + obstacle_lo][:, [0, 2]]
    reg = points[points[:, 1] < zero + region_max][:, [0, 2]]
    region = create_occupancy_grid(reg, pcd_min, grid, cell_size, dilation, blur)
    region_map = (region > 0).astype(np.uint8)
    poses_map = poses_region(poses, pcd_min, grid, cell_size, pose_radius, pose_eps, pose_min_samples)
    occupancy = region.astype(np.float32)
    np.logical_or(occupancy, poses_map, out=occupancy)
    obstacle_map = create_occupancy_grid(obst, pcd_min, grid, cell_size, dilation, blur).astype(np.float32)
    free = occupancy - obstacle_map
    free = np.where(free < 0, 0, free).astype(np.uint8)
    main, labels, areas, label = largest_region(free, region_rule, ties)
    boundary = main.astype(np.uint8) - ndimage.binary_erosion(main, iterations=1).astype(np.uint8)
    rows, cols = np.where(boundary == 1)
    out = dict(obstacle_map=obstacle_map, region_map=region_map, poses_map=poses_map, free_map=free, main_free_map=main.astype(np.uint8),
               boundary_rc=np.array(list(zip(rows, cols)), np.int32).reshape(-1, 2), boundary=boundary, n_regions=len(areas),
               main_label=label, main_area=int(areas[label]), grid=(int(grid[0]), int(grid[1])), pcd_min=pcd_min, pcd_max=pcd_max,
               labels=labels, areas=areas)
    if colors is not None:
        out["top_down_bgr"] = top_down(points, np.asarray(colors, np.float64), zero, pcd_min, grid, cell_size, region_max)
    return out
