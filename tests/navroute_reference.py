"""The rules R1 to R5 of include/hmsg.h (N7: routes on a floor's free map) restated with numpy, scipy's Dijkstra on the grid graph
and plain Python: what tests/navroute_cases.py compares the library with, by array_equal.  Costs are small integers, so scipy's
float64 distances are exact."""
import numpy as np
from scipy.sparse import csr_matrix
from scipy.sparse.csgraph import dijkstra

UNREACHED = 2147483647
MOVES = ((-1, 0), (1, 0), (0, -1), (0, 1), (-1, -1), (-1, 1), (1, -1), (1, 1))          # R1's order
CLAMP = 1 << 20


def _shifted(a, dr, dc):
    """b[r, c] = a[r + dr, c + dc], False outside"""
    H, W = a.shape
    b = np.zeros_like(a)
    rs, cs = slice(max(0, -dr), min(H, H - dr)), slice(max(0, -dc), min(W, W - dc))
    rt, ct = slice(max(0, dr), min(H, H + dr)), slice(max(0, dc), min(W, W + dc))
    b[rs, cs] = a[rt, ct]
    return b


def grid_graph(passable, w_straight=5, w_diag=7, corner_rule=True):
    """the directed graph of R1 on the cells of `passable` (bool [rows, cols]) as a csr matrix over row-major cell indices"""
    p = np.asarray(passable).astype(bool)
    H, W = p.shape
    idx = np.arange(H * W).reshape(H, W)
    src, dst, cost = [], [], []
    for dr, dc in MOVES:
        ok = p & _shifted(p, dr, dc)
        if dr and dc and corner_rule:
            ok &= _shifted(p, dr, 0) & _shifted(p, 0, dc)
        r, c = np.nonzero(ok)
        src.append(idx[r, c])
        dst.append(idx[r + dr, c + dc])
        cost.append(np.full(len(r), w_diag if dr and dc else w_straight, np.float64))
    return csr_matrix((np.concatenate(cost), (np.concatenate(src), np.concatenate(dst))), shape=(H * W, H * W))


def field(passable, sources_rc, w_straight=5, w_diag=7, graph=None):
    """R2 -> (int32 [rows, cols], cells reached)"""
    p = np.asarray(passable).astype(bool)
    H, W = p.shape
    out = np.full(H * W, UNREACHED, np.int32)
    s = np.asarray(sources_rc, np.int64).reshape(-1, 2)
    s = np.unique(np.array([r * W + c for r, c in s if p[r, c]], np.int64))
    if len(s):
        g = graph if graph is not None else grid_graph(p, w_straight, w_diag)
        d = dijkstra(g, directed=True, indices=s, min_only=True)
        ok = np.isfinite(d)
        out[ok] = d[ok].astype(np.int32)
    return out.reshape(H, W), int((out != UNREACHED).sum())


def clearance(mask, w_straight=5, w_diag=7):
    """R3: every move allowed, a ring of cells outside the image counting as not in the mask"""
    m = np.asarray(mask).astype(bool)
    H, W = m.shape
    big = np.zeros((H + 2, W + 2), bool)
    big[1:-1, 1:-1] = m
    g = grid_graph(np.ones_like(big), w_straight, w_diag, corner_rule=False)
    d = dijkstra(g, directed=True, indices=np.flatnonzero(~big.ravel()), min_only=True)
    return d.reshape(H + 2, W + 2)[1:-1, 1:-1].astype(np.int32)


def snap(passable, targets_rc, field_=None):
    """R4 -> (int32 [n, 2], int64 [n])"""
    cand = np.asarray(passable).astype(bool)
    if field_ is not None:
        cand = cand & (np.asarray(field_) != UNREACHED)
    H, W = cand.shape
    rr, cc = np.meshgrid(np.arange(H, dtype=np.int64), np.arange(W, dtype=np.int64), indexing="ij")
    t = np.asarray(targets_rc, np.int64).reshape(-1, 2)
    cells, d2 = np.full((len(t), 2), -1, np.int32), np.full(len(t), -1, np.int64)
    if not cand.any():
        return cells, d2
    for k, (tr, tc) in enumerate(np.clip(t, -CLAMP, CLAMP)):
        d = np.where(cand, (rr - tr) ** 2 + (cc - tc) ** 2, np.iinfo(np.int64).max)
        i = int(np.argmin(d))                                             # (the first minimum: the smaller row-major index)
        cells[k], d2[k] = (i // W, i % W), d.ravel()[i]
    return cells, d2


def legal(passable, a, b):
    p = np.asarray(passable)
    H, W = p.shape
    (r, c), (nr, nc) = a, b
    if not (0 <= nr < H and 0 <= nc < W and p[r, c] and p[nr, nc]) or max(abs(nr - r), abs(nc - c)) != 1:
        return False
    return not (nr != r and nc != c) or bool(p[nr, c] and p[r, nc])


def path(passable, field_, goal_rc, w_straight=5, w_diag=7):
    """R5 -> a list of (row, col), source first; [] for a goal without a path"""
    p, f = np.asarray(passable), np.asarray(field_)
    H, W = p.shape
    r, c = int(goal_rc[0]), int(goal_rc[1])
    if not (0 <= r < H and 0 <= c < W) or not p[r, c] or f[r, c] == UNREACHED:
        return []
    cells = [(r, c)]
    while f[r, c] != 0:
        for dr, dc in MOVES:
            n = (r + dr, c + dc)
            if legal(p, (r, c), n) and f[n] != UNREACHED and int(f[n]) + (w_diag if dr and dc else w_straight) == int(f[r, c]):
                r, c = n
                break
        else:
            return []
        cells.append((r, c))
    return cells[::-1]


def paths(passable, field_, goals_rc, w_straight=5, w_diag=7):
    """-> (path_off int64 [n + 1], path_rc int32 [k, 2])"""
    lists = [path(passable, field_, g, w_straight, w_diag) for g in np.asarray(goals_rc).reshape(-1, 2)]
    off = np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.int64)
    flat = [c for l in lists for c in l]
    return off, np.array(flat, np.int32).reshape(-1, 2)


def route(main_free_map, start_rc, goals_rc, w_straight=5, w_diag=7, min_clearance=0):
    """hmsg_nav_route's composition"""
    m = np.asarray(main_free_map).astype(bool)
    pas = m & (clearance(m, w_straight, w_diag) >= min_clearance) if min_clearance > 0 else m
    start, start_d2 = snap(pas, [start_rc])
    f, _ = field(pas, start if start[0, 0] >= 0 else np.zeros((0, 2)), w_straight, w_diag)
    cell, d2 = snap(pas, goals_rc, f)
    dist = np.array([f[r, c] if r >= 0 else UNREACHED for r, c in cell], np.int32)
    off, rc = paths(pas, f, cell, w_straight, w_diag)
    return dict(passable=pas.astype(np.uint8), start_cell=(int(start[0, 0]), int(start[0, 1])), start_d2=int(start_d2[0]), field=f, goal_cell=cell,
                goal_d2=d2, goal_dist=dist, path_off=off, path_rc=rc)
