"""The rules G1, G2, D1 to D4 and L1 of include/hmsg.h (N11: rooms on a floor's free map) restated with scipy and plain loops:
what tests/navrooms_cases.py compares the library with, by array_equal.  Nothing here works as the kernels do: the labels come
from one Dijkstra per room and an argmin over the rooms (G2's first form), `other` from a loop over the cells, the doors from
scipy.ndimage.label per pair, the legs from a loop over the path."""
import numpy as np
from scipy.ndimage import label as nd_label

from tests import navroute_reference as RR

U = RR.UNREACHED


def labels(passable, seed_sets, w_straight=5, w_diag=7, graph=None):
    """G1, G2 -> (label int32 [rows, cols], dist int32 [rows, cols], n_cells int64 [n_rooms])"""
    p = np.asarray(passable)
    n = len(seed_sets)
    if n == 0:
        return np.full(p.shape, -1, np.int32), np.full(p.shape, U, np.int32), np.zeros(0, np.int64)
    g = graph if graph is not None else RR.grid_graph(p, w_straight, w_diag)
    per_room = np.stack([RR.field(p, s, w_straight, w_diag, graph=g)[0] for s in seed_sets])
    dist = per_room.min(0)
    lab = np.where(dist == U, -1, per_room.argmin(0)).astype(np.int32)      # (argmin: the first, smallest room)
    return lab, dist.astype(np.int32), np.bincount(lab[lab >= 0], minlength=n).astype(np.int64)


def labels_by_order(passable, seed_sets, w_straight=5, w_diag=7, graph=None):
    """G2's second form, for maps where a Dijkstra per room takes too long: one field from the union of the seeds, then the cells in
    ascending dist, each taking the least label over its tight predecessors -> (label, dist, n_cells)"""
    p = np.asarray(passable).astype(bool)
    H, W = p.shape
    n = len(seed_sets)
    union = np.concatenate([np.asarray(s, np.int64).reshape(-1, 2) for s in seed_sets]) if n else np.zeros((0, 2), np.int64)
    dist, _ = RR.field(p, union, w_straight, w_diag, graph=graph)
    lab = np.full((H, W), np.iinfo(np.int32).max, np.int64)
    for r_, s in enumerate(seed_sets):
        for r, c in np.asarray(s, np.int64).reshape(-1, 2):
            if p[r, c]:
                lab[r, c] = min(lab[r, c], r_)
    d = dist.astype(np.int64)
    order = np.argsort(d.ravel(), kind="stable")
    order = order[d.ravel()[order] != U]
    pad = np.zeros((H + 2, W + 2), bool)
    pad[1:-1, 1:-1] = p
    for i in order:
        r, c = divmod(int(i), W)
        if d[r, c] == 0:
            continue
        best = lab[r, c]
        for dr, dc in RR.MOVES:
            nr, nc = r + dr, c + dc
            if not pad[nr + 1, nc + 1] or (dr and dc and not (pad[nr + 1, c + 1] and pad[r + 1, nc + 1])):
                continue
            if d[nr, nc] != U and d[nr, nc] + (w_diag if dr and dc else w_straight) == d[r, c]:
                best = min(best, lab[nr, nc])
        lab[r, c] = best
    lab = np.where(dist == U, -1, lab).astype(np.int32)
    return lab, dist, np.bincount(lab[lab >= 0], minlength=n).astype(np.int64)


def other(passable, label):
    """D1, D2 -> int32 [rows, cols]"""
    p, lab = np.asarray(passable), np.asarray(label)
    H, W = p.shape
    out = np.full((H, W), -1, np.int32)
    for r, c in np.argwhere((lab >= 0) & (p != 0)):
        best = -1
        for dr, dc in RR.MOVES:
            b = (r + dr, c + dc)
            if RR.legal(p, (r, c), b) and lab[b] >= 0 and lab[b] != lab[r, c] and (best < 0 or lab[b] < best):
                best = int(lab[b])
        out[r, c] = best
    return out


def doors(passable, label, n_rooms):
    """D3, D4 -> dict(other, door_pair int32 [n, 2], door_off int64 [n + 1], door_rc int32 [k, 2], adjacency int32 [n_rooms, n_rooms])"""
    lab = np.asarray(label)
    oth = other(passable, lab)
    thr = oth >= 0
    lo, hi = np.minimum(lab, oth), np.maximum(lab, oth)
    W = lab.shape[1]
    found = []                                                            # (p, q, least index, cells)
    for p_, q_ in sorted({(int(a), int(b)) for a, b in zip(lo[thr], hi[thr])}):
        comp, n = nd_label(thr & (lo == p_) & (hi == q_), structure=np.ones((3, 3), int))
        for k in range(1, n + 1):
            cells = np.argwhere(comp == k)                                # (argwhere: ascending row-major order)
            found.append((p_, q_, int(cells[0, 0]) * W + int(cells[0, 1]), cells))
    found.sort(key=lambda d: d[:3])
    adj = np.zeros((n_rooms, n_rooms), np.int32)
    for p_, q_, _, _ in found:
        adj[p_, q_] += 1
        adj[q_, p_] += 1
    return dict(other=oth, door_pair=np.array([d[:2] for d in found], np.int32).reshape(-1, 2),
                door_off=np.concatenate([[0], np.cumsum([len(d[3]) for d in found])]).astype(np.int64),
                door_rc=(np.concatenate([d[3] for d in found]) if found else np.zeros((0, 2))).astype(np.int32), adjacency=adj)


def legs(label, path_off, path_rc):
    """L1 -> (leg_off int64 [n + 1], leg_room int32 [k], leg_first int64 [k])"""
    lab = np.asarray(label)
    H, W = lab.shape
    off, room, first = [0], [], []
    for a, b in zip(path_off[:-1], path_off[1:]):
        last = None
        for k in range(int(a), int(b)):
            r, c = int(path_rc[k][0]), int(path_rc[k][1])
            l = int(lab[r, c]) if 0 <= r < H and 0 <= c < W else -1
            if k == a or l != last:
                room.append(l)
                first.append(k - int(a))
            last = l
        off.append(len(room))
    return np.array(off, np.int64), np.array(room, np.int32), np.array(first, np.int64)
