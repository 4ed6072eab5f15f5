"""The rules of include/hmsg.h, N10 (a storey's height map H1 to H3, sight with heights S1 to S4) restated twice, as
tests/navview_reference.py restates N8: in plain Python loops, one point, one cell and one line at a time (height_map, clear_h,
visible_set_h), and with numpy (height_map_np: np.maximum.at and scipy.ndimage.maximum_filter with mode="constant", exact for
values that are not negative; visible_set_h_np: one array step per line index), so that a 511 x 511 window takes seconds.
tests/navsight_cases.py pins the second to the first and compares the library with them by array_equal.  view_route_h composes
them with the pieces of tests/navroute_reference.py as hmsg_nav_view_route_h composes the calls."""
import math

import numpy as np

from tests import navroute_reference as RR
from tests import navview_reference as VR

UNREACHED = RR.UNREACHED


# ------------------------------------------------------------------------------------------ the height map
def grid_of(points, cell_size):
    """N6's rule 1 -> (pcd_min [3], pcd_max [3], (columns, rows))"""
    p = np.asarray(points, np.float64).reshape(-1, 3)
    mn, mx = p.min(axis=0), p.max(axis=0)
    g = np.ceil((mx - mn) / cell_size + 1.0).astype(np.int32)
    return mn, mx, (int(g[0]), int(g[2]))


def height_map(points, zero_level, cell_size=0.03, height_unit=0.01, top_max=2.5, dilation=5):
    """H1 to H3 in loops -> (top u16 [rows, cols], known u8 [rows, cols])"""
    p = np.asarray(points, np.float64).reshape(-1, 3)
    mn, _, (W, H) = grid_of(p, cell_size)
    raw, known = np.zeros((H, W), np.int64), np.zeros((H, W), np.uint8)
    limit = float(np.float64(zero_level) + np.float64(top_max))
    for x, y, z in p:
        if not y < limit:
            continue
        r, c = int(math.floor((z - mn[2]) / cell_size)), int(math.floor((x - mn[0]) / cell_size))
        q = min(max(math.floor((y - zero_level) / height_unit), 0), 65535)
        raw[r, c] = max(raw[r, c], q)
        known[r, c] = 1
    k = dilation // 2 if dilation > 1 else 0
    top = np.zeros((H, W), np.uint16)
    for r in range(H):
        for c in range(W):
            top[r, c] = raw[max(r - k, 0):r + k + 1, max(c - k, 0):c + k + 1].max()
    return top, known


def height_map_np(points, zero_level, cell_size=0.03, height_unit=0.01, top_max=2.5, dilation=5):
    from scipy.ndimage import maximum_filter
    p = np.asarray(points, np.float64).reshape(-1, 3)
    mn, _, (W, H) = grid_of(p, cell_size)
    p = p[p[:, 1] < np.float64(zero_level) + np.float64(top_max)]
    r, c = np.floor((p[:, 2] - mn[2]) / cell_size).astype(np.int64), np.floor((p[:, 0] - mn[0]) / cell_size).astype(np.int64)
    q = np.clip(np.floor((p[:, 1] - zero_level) / height_unit), 0, 65535).astype(np.int64)
    raw, known = np.zeros((H, W), np.int64), np.zeros((H, W), np.uint8)
    np.maximum.at(raw, (r, c), q)
    known[r, c] = 1
    top = maximum_filter(raw, size=dilation, mode="constant", cval=0) if dilation > 1 else raw
    return top.astype(np.uint16), known


# ------------------------------------------------------------------------------------------ sight with heights: plain loops
def _T(top, cell, goal, goal_r2):
    d2 = (cell[0] - int(goal[0])) ** 2 + (cell[1] - int(goal[1])) ** 2
    return 0 if d2 <= goal_r2 else int(top[cell[0], cell[1]])


def clear_h(top, view, goal, eye, goal_h, goal_r2=-1):
    """S1 / S2 for the viewpoint cell `view` and the goal cell `goal`, both inside the image"""
    view, goal = (int(view[0]), int(view[1])), (int(goal[0]), int(goal[1]))
    cells = VR.sight_line(view, goal)
    n = len(cells) - 1
    gh = min(max(int(goal_h), 0), 65535)
    h0, hn = (int(eye), gh) if cells[0] == view else (gh, int(eye))        # (view == goal: n == 0 and nothing is tested)
    for i, (r, c) in enumerate(cells):
        if 0 < i < n and _T(top, (r, c), goal, goal_r2) * n >= h0 * (n - i) + hn * i:
            return False
        if i:
            pr, pc = cells[i - 1]
            if pr != r and pc != c:
                w = h0 * (2 * n - 2 * i + 1) + hn * (2 * i - 1)
                if _T(top, (pr, c), goal, goal_r2) * 2 * n >= w and _T(top, (r, pc), goal, goal_r2) * 2 * n >= w:
                    return False
    return True


def visible_set_h(top, passable, goal, r_min2, r_max2, eye, goal_h, goal_r2=-1, field=None):
    """S3 -> u8 [rows, cols]"""
    top, pas = np.asarray(top), np.asarray(passable)
    H, W = pas.shape
    out = np.zeros((H, W), np.uint8)
    gr, gc = int(goal[0]), int(goal[1])
    if not (0 <= gr < H and 0 <= gc < W):
        return out
    for r in range(H):
        for c in range(W):
            d2 = (r - gr) ** 2 + (c - gc) ** 2
            if not pas[r, c] or not r_min2 <= d2 <= r_max2 or (field is not None and field[r, c] == UNREACHED):
                continue
            out[r, c] = 1 if clear_h(top, (r, c), (gr, gc), eye, goal_h, goal_r2) else 0
    return out


def viewpoint_h(top, passable, goal, r_min2, r_max2, eye, goal_h, goal_r2=-1, field=None, prefer=0):
    """S4 -> ((row, col), d2, dist, n_visible, mask)"""
    mask = visible_set_h(top, passable, goal, r_min2, r_max2, eye, goal_h, goal_r2, field)
    return VR._pick(mask, goal, field, prefer) + (mask,)


# ------------------------------------------------------------------------------------------ numpy over the candidates
def visible_set_h_np(top, passable, goal, r_min2, r_max2, eye, goal_h, goal_r2=-1, field=None):
    pas = np.asarray(passable) != 0
    H, W = pas.shape
    out = np.zeros((H, W), np.uint8)
    gr, gc = int(goal[0]), int(goal[1])
    if not (0 <= gr < H and 0 <= gc < W):
        return out
    rr, cc = np.meshgrid(np.arange(H, dtype=np.int64), np.arange(W, dtype=np.int64), indexing="ij")
    d2 = (rr - gr) ** 2 + (cc - gc) ** 2
    T = np.where(d2 <= goal_r2, 0, np.asarray(top).astype(np.int64))
    gh, eye = min(max(int(goal_h), 0), 65535), int(eye)
    cand = pas & (d2 >= r_min2) & (d2 <= r_max2)
    if field is not None:
        cand &= np.asarray(field) != UNREACHED
    r, c = np.nonzero(cand)
    r, c = r.astype(np.int64), c.astype(np.int64)
    if len(r) == 0:
        return out
    first = (r < gr) | ((r == gr) & (c <= gc))                            # the candidate is the smaller cell: the line starts there
    ar, ac = np.where(first, r, gr), np.where(first, c, gc)
    br, bc = np.where(first, gr, r), np.where(first, gc, c)
    h0, hn = np.where(first, eye, gh), np.where(first, gh, eye)
    dr, dc = br - ar, bc - ac
    n = np.maximum(dr, np.abs(dc))
    by_row = dr >= np.abs(dc)
    dm = np.where(by_row, dc, dr)
    step = np.where(dc < 0, -1, 1)
    seen = n == 0
    k = np.flatnonzero(n > 0)
    pr, pc = ar[k], ac[k]
    i = 0
    while len(k):
        i += 1
        nk = n[k]
        q = (2 * i * dm[k] + nk) // (2 * nk)
        lr = np.where(by_row[k], ar[k] + i, ar[k] + q)
        lc = np.where(by_row[k], ac[k] + q, ac[k] + step[k] * i)
        w = h0[k] * (2 * nk - 2 * i + 1) + hn[k] * (2 * i - 1)
        bad = (lr != pr) & (lc != pc) & (T[pr, lc] * 2 * nk >= w) & (T[lr, pc] * 2 * nk >= w)
        bad |= (i < nk) & (T[lr, lc] * nk >= h0[k] * (nk - i) + hn[k] * i)
        done = ~bad & (i == nk)
        seen[k[done]] = True
        go = ~bad & ~done
        k, pr, pc = k[go], lr[go], lc[go]
    out[r[seen], c[seen]] = 1
    return out


def viewpoint_h_np(top, passable, goal, r_min2, r_max2, eye, goal_h, goal_r2=-1, field=None, prefer=0):
    mask = visible_set_h_np(top, passable, goal, r_min2, r_max2, eye, goal_h, goal_r2, field)
    H, W = mask.shape
    r, c = np.nonzero(mask)
    if len(r) == 0:
        return (-1, -1), -1, UNREACHED, 0, mask
    d2 = (r.astype(np.int64) - int(goal[0])) ** 2 + (c.astype(np.int64) - int(goal[1])) ** 2
    fv = np.zeros(len(r), np.int64) if field is None else np.asarray(field)[r, c].astype(np.int64)
    idx = r.astype(np.int64) * W + c
    k = np.lexsort((idx, d2, fv) if prefer == 0 else (idx, fv, d2))[0]
    return (int(r[k]), int(c[k])), int(d2[k]), int(fv[k]), len(r), mask


def viewpoints_h(top, passable, goals, r_min2, r_max2, eye, goal_h, goal_r2=None, field=None, prefer=0, want_visible=False, one=viewpoint_h_np):
    """hmsg_nav_viewpoints_h -> the dict holoagent_amd._lib.nav_viewpoints_h returns"""
    goals = np.asarray(goals, np.int64).reshape(-1, 2)
    H, W = np.asarray(passable).shape
    n = len(goals)
    gh = np.broadcast_to(np.asarray(goal_h, np.int64), (n,))
    gr2 = np.broadcast_to(np.asarray(-1 if goal_r2 is None else goal_r2, np.int64), (n,))
    res = dict(view_rc=np.zeros((n, 2), np.int32), view_d2=np.zeros(n, np.int64), view_dist=np.zeros(n, np.int32), n_visible=np.zeros(n, np.int32))
    if want_visible:
        res["visible"] = np.zeros((n, H, W), np.uint8)
    for k, g in enumerate(goals):
        res["view_rc"][k], res["view_d2"][k], res["view_dist"][k], res["n_visible"][k], mask = one(top, passable, g, r_min2, r_max2, eye, int(gh[k]),
                                                                                                  int(gr2[k]), field, prefer)
        if want_visible:
            res["visible"][k] = mask
    return res


def view_route_h(main_free_map, top, start_rc, goals_rc, eye, goal_h, goal_r2=None, r_min2=0, r_max2=100 * 100, prefer=0, w_straight=5, w_diag=7,
                 min_clearance=0):
    """hmsg_nav_view_route_h's composition: VR.view_route with S3 in V3's place"""
    m = np.asarray(main_free_map).astype(bool)
    pas = m & (RR.clearance(m, w_straight, w_diag) >= min_clearance) if min_clearance > 0 else m
    start, start_d2 = RR.snap(pas, [start_rc])
    f, _ = RR.field(pas, start if start[0, 0] >= 0 else np.zeros((0, 2)), w_straight, w_diag)
    v = viewpoints_h(top, pas, goals_rc, r_min2, r_max2, eye, goal_h, goal_r2, f, prefer)
    off, rc = RR.paths(pas, f, v["view_rc"], w_straight, w_diag)
    return dict(passable=pas.astype(np.uint8), start_cell=(int(start[0, 0]), int(start[0, 1])), start_d2=int(start_d2[0]), field=f,
                goal_cell=v["view_rc"], goal_d2=v["view_d2"], goal_dist=v["view_dist"], path_off=off, path_rc=rc, n_visible=v["n_visible"])
