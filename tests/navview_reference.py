"""The rules V1 to V4 of include/hmsg.h (N8: viewpoints on a floor's free map) restated twice: in plain Python loops, one cell and
one line at a time (sight_line, clear, visible_set, viewpoint), and with numpy vectorised over the candidates, one array step per
line index (visible_set_np, viewpoint_np), so that a 511 x 511 window takes seconds.  tests/navview_cases.py pins the second to the
first on its small cases and compares the library with them by array_equal.  view_route composes them with the pieces of
tests/navroute_reference.py as hmsg_nav_view_route composes the calls."""
import numpy as np

from tests import navroute_reference as RR

UNREACHED = RR.UNREACHED


# ------------------------------------------------------------------------------------------ plain loops
def sight_line(a, b):
    """V1 -> the list of (row, col) from the smaller of the two cells to the other, both included"""
    a, b = (int(a[0]), int(a[1])), (int(b[0]), int(b[1]))
    if b < a:
        a, b = b, a
    dr, dc = b[0] - a[0], b[1] - a[1]
    n = max(abs(dr), abs(dc))
    if n == 0:
        return [a]
    cells = []
    for i in range(n + 1):
        if abs(dr) >= abs(dc):                                            # the row is the major axis (dr >= 0)
            cells.append((a[0] + i, a[1] + (2 * i * dc + n) // (2 * n)))  # (Python's // is the mathematical floor)
        else:
            cells.append((a[0] + (2 * i * dr + n) // (2 * n), a[1] + (i if dc > 0 else -i)))
    return cells


def clear(blocking, a, b):
    """V2: every cell of the line lies inside the image when a and b do"""
    blk = np.asarray(blocking)
    cells = sight_line(a, b)
    for k, (r, c) in enumerate(cells):
        if 0 < k < len(cells) - 1 and blk[r, c]:
            return False
        if k:
            pr, pc = cells[k - 1]
            if pr != r and pc != c and blk[pr, c] and blk[r, pc]:
                return False
    return True


def visible_set(blocking, passable, goal, r_min2, r_max2, field=None):
    """V3 -> u8 [rows, cols]"""
    blk, pas = np.asarray(blocking), np.asarray(passable)
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
            out[r, c] = 1 if clear(blk, (r, c), (gr, gc)) else 0
    return out


def _pick(mask, goal, field, prefer):
    """V4 on a visible set -> ((row, col), d2, dist, n_visible)"""
    H, W = mask.shape
    best = None
    for r, c in np.argwhere(mask != 0):
        d2 = (int(r) - int(goal[0])) ** 2 + (int(c) - int(goal[1])) ** 2
        fv = 0 if field is None else int(field[r, c])
        key = (fv, d2, int(r) * W + int(c)) if prefer == 0 else (d2, fv, int(r) * W + int(c))
        if best is None or key < best[0]:
            best = (key, (int(r), int(c)), d2, fv)
    if best is None:
        return (-1, -1), -1, UNREACHED, 0
    return best[1], best[2], best[3], int((mask != 0).sum())


def viewpoint(blocking, passable, goal, r_min2, r_max2, field=None, prefer=0):
    """-> ((row, col), d2, dist, n_visible, mask)"""
    mask = visible_set(blocking, passable, goal, r_min2, r_max2, field)
    return _pick(mask, goal, field, prefer) + (mask,)


# ------------------------------------------------------------------------------------------ numpy over the candidates
def visible_set_np(blocking, passable, goal, r_min2, r_max2, field=None):
    blk, pas = np.asarray(blocking) != 0, np.asarray(passable) != 0
    H, W = pas.shape
    out = np.zeros((H, W), np.uint8)
    gr, gc = int(goal[0]), int(goal[1])
    if not (0 <= gr < H and 0 <= gc < W):
        return out
    rr, cc = np.meshgrid(np.arange(H, dtype=np.int64), np.arange(W, dtype=np.int64), indexing="ij")
    d2 = (rr - gr) ** 2 + (cc - gc) ** 2
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
    dr, dc = br - ar, bc - ac
    n = np.maximum(dr, np.abs(dc))
    by_row = dr >= np.abs(dc)
    dm = np.where(by_row, dc, dr)
    step = np.where(dc < 0, -1, 1)
    seen = n == 0                                                         # (the goal's own cell: a line of one cell)
    k = np.flatnonzero(n > 0)                                             # the candidates whose line is still being walked
    pr, pc = ar[k], ac[k]
    i = 0
    while len(k):
        i += 1
        q = (2 * i * dm[k] + n[k]) // (2 * n[k])                          # (numpy's // on integers is the mathematical floor)
        lr = np.where(by_row[k], ar[k] + i, ar[k] + q)
        lc = np.where(by_row[k], ac[k] + q, ac[k] + step[k] * i)
        bad = ((lr != pr) & (lc != pc) & blk[pr, lc] & blk[lr, pc]) | ((i < n[k]) & blk[lr, lc])
        done = ~bad & (i == n[k])
        seen[k[done]] = True
        go = ~bad & ~done
        k, pr, pc = k[go], lr[go], lc[go]
    out[r[seen], c[seen]] = 1
    return out


def viewpoint_np(blocking, passable, goal, r_min2, r_max2, field=None, prefer=0):
    mask = visible_set_np(blocking, passable, goal, r_min2, r_max2, field)
    H, W = mask.shape
    r, c = np.nonzero(mask)
    if len(r) == 0:
        return (-1, -1), -1, UNREACHED, 0, mask
    d2 = (r.astype(np.int64) - int(goal[0])) ** 2 + (c.astype(np.int64) - int(goal[1])) ** 2
    fv = np.zeros(len(r), np.int64) if field is None else np.asarray(field)[r, c].astype(np.int64)
    idx = r.astype(np.int64) * W + c
    k = np.lexsort((idx, d2, fv) if prefer == 0 else (idx, fv, d2))[0]     # (lexsort: the LAST key is the primary one)
    return (int(r[k]), int(c[k])), int(d2[k]), int(fv[k]), len(r), mask


def viewpoints(blocking, passable, goals, r_min2, r_max2, field=None, prefer=0, want_visible=False, one=viewpoint_np):
    """hmsg_nav_viewpoints -> the dict holoagent_amd._lib.nav_viewpoints returns"""
    goals = np.asarray(goals, np.int64).reshape(-1, 2)
    H, W = np.asarray(passable).shape
    n = len(goals)
    res = dict(view_rc=np.zeros((n, 2), np.int32), view_d2=np.zeros(n, np.int64), view_dist=np.zeros(n, np.int32), n_visible=np.zeros(n, np.int32))
    if want_visible:
        res["visible"] = np.zeros((n, H, W), np.uint8)
    for k, g in enumerate(goals):
        res["view_rc"][k], res["view_d2"][k], res["view_dist"][k], res["n_visible"][k], mask = one(blocking, passable, g, r_min2, r_max2, field, prefer)
        if want_visible:
            res["visible"][k] = mask
    return res


def view_route(main_free_map, blocking, start_rc, goals_rc, r_min2=0, r_max2=100 * 100, prefer=0, w_straight=5, w_diag=7, min_clearance=0):
    """hmsg_nav_view_route's composition: RR.route with its goal snap replaced by V4 on the start's field"""
    m = np.asarray(main_free_map).astype(bool)
    pas = m & (RR.clearance(m, w_straight, w_diag) >= min_clearance) if min_clearance > 0 else m
    start, start_d2 = RR.snap(pas, [start_rc])
    f, _ = RR.field(pas, start if start[0, 0] >= 0 else np.zeros((0, 2)), w_straight, w_diag)
    v = viewpoints(blocking, pas, goals_rc, r_min2, r_max2, f, prefer)
    off, rc = RR.paths(pas, f, v["view_rc"], w_straight, w_diag)
    return dict(passable=pas.astype(np.uint8), start_cell=(int(start[0, 0]), int(start[0, 1])), start_d2=int(start_d2[0]), field=f,
                goal_cell=v["view_rc"], goal_d2=v["view_d2"], goal_dist=v["view_dist"], path_off=off, path_rc=rc, n_visible=v["n_visible"])
