"""The rules B1 to B5 of include/hmsg.h (N9: routes across storeys) restated with scipy's Dijkstra on the layered graph -- the
block-diagonal union of tests/navroute_reference.grid_graph per storey plus the link edges -- and plain Python loops: what
tests/navbuilding_cases.py compares the library with, by array_equal.  Costs are small integers, so scipy's float64 distances are
exact.  No zero-weight edge is used anywhere (B1 takes the minimum over seeds of cost + the single-source field)."""
import numpy as np
from scipy.sparse import block_diag, csr_matrix
from scipy.sparse.csgraph import dijkstra

from tests import navroute_reference as RR

UNREACHED = RR.UNREACHED
MOVES = RR.MOVES


def seeded_field(passable, cells, costs, w_straight=5, w_diag=7, graph=None):
    """B1 -> (int32 [rows, cols], cells reached)"""
    p = np.asarray(passable).astype(bool)
    H, W = p.shape
    best = {}
    for (r, c), v in zip(np.asarray(cells, np.int64).reshape(-1, 2), np.asarray(costs, np.int64).reshape(-1)):
        if p[r, c]:
            i = int(r) * W + int(c)
            best[i] = min(best.get(i, int(v)), int(v))
    out = np.full(H * W, np.inf)
    if best:
        g = graph if graph is not None else RR.grid_graph(p, w_straight, w_diag)
        idx = sorted(best)
        d = dijkstra(g, directed=True, indices=idx).reshape(len(idx), H * W)
        out = (d + np.array([best[i] for i in idx], np.float64)[:, None]).min(axis=0)
    f = np.where(np.isfinite(out), out, UNREACHED).astype(np.int64).astype(np.int32)
    return f.reshape(H, W), int((f != UNREACHED).sum())


class Building:
    """B2: the storeys' passable maps and the links (sa, ra, ca, sb, rb, cb, cost); the layered graph, made once"""

    def __init__(self, passables, links, w_straight=5, w_diag=7):
        self.p = [np.asarray(m).astype(bool) for m in passables]
        self.links = [tuple(int(v) for v in l) for l in np.asarray(links if len(links) else np.zeros((0, 7)), np.int64).reshape(-1, 7)]
        self.ws, self.wd = w_straight, w_diag
        self.base = np.concatenate([[0], np.cumsum([m.size for m in self.p])]).astype(np.int64)
        g = block_diag([RR.grid_graph(m, w_straight, w_diag) for m in self.p], format="coo")
        src, dst, cost = [], [], []
        for sa, ra, ca, sb, rb, cb, w in self.links:
            if not self.exists((sa, ra, ca, sb, rb, cb, w)) or (sa, ra, ca) == (sb, rb, cb):
                continue                                                  # (a link from a cell to itself changes no distance)
            a, b = self.index(sa, ra, ca), self.index(sb, rb, cb)
            src += [a, b]
            dst += [b, a]
            cost += [float(w), float(w)]
        # parallel edges (two links between one pair of cells, a link beside a grid move): the cheapest -- a sparse matrix would
        # ADD duplicates
        n = int(self.base[-1])
        src = np.concatenate([g.row.astype(np.int64), np.array(src, np.int64)])
        dst = np.concatenate([g.col.astype(np.int64), np.array(dst, np.int64)])
        cost = np.concatenate([g.data.astype(np.float64), np.array(cost, np.float64)])
        key = src * n + dst
        order = np.lexsort((cost, key))
        first = np.concatenate([[True], key[order][1:] != key[order][:-1]])
        sel = order[first]
        self.graph = csr_matrix((cost[sel], (src[sel], dst[sel])), shape=(n, n))

    def index(self, l, r, c):
        return int(self.base[l]) + int(r) * self.p[l].shape[1] + int(c)

    def exists(self, link):
        sa, ra, ca, sb, rb, cb, w = link
        return bool(self.p[sa][ra, ca] and self.p[sb][rb, cb])

    def fields(self, start):
        """B3 -> (a list of int32 [rows_l, cols_l], n_reached int64 [storeys])"""
        l, r, c = (int(v) for v in start)
        n = int(self.base[-1])
        d = np.full(n, np.inf)
        if self.p[l][r, c]:
            d = dijkstra(self.graph, directed=True, indices=self.index(l, r, c))
        f = np.where(np.isfinite(d), d, UNREACHED).astype(np.int64).astype(np.int32)
        out = [f[self.base[k]:self.base[k + 1]].reshape(self.p[k].shape) for k in range(len(self.p))]
        return out, np.array([(m != UNREACHED).sum() for m in out], np.int64)

    def snap(self, fields, goals):
        """B4 -> (cells int32 [n, 3], d2 int64 [n], dist int32 [n])"""
        g = np.asarray(goals, np.int64).reshape(-1, 3)
        cells, d2, dist = np.full((len(g), 3), -1, np.int32), np.full(len(g), -1, np.int64), np.full(len(g), UNREACHED, np.int32)
        for k, (l, r, c) in enumerate(g):
            cell, d = RR.snap(self.p[l], [(r, c)], fields[l])
            cells[k] = (l, cell[0, 0], cell[0, 1])
            d2[k] = d[0]
            if cell[0, 0] >= 0:
                dist[k] = fields[l][cell[0, 0], cell[0, 1]]
        return cells, d2, dist

    def path(self, fields, goal):
        """B5 -> a list of (storey, row, col), the start first; [] for a goal without a path"""
        l, r, c = (int(v) for v in goal)
        if not (0 <= l < len(self.p)):
            return []
        H, W = self.p[l].shape
        if not (0 <= r < H and 0 <= c < W) or not self.p[l][r, c] or fields[l][r, c] == UNREACHED:
            return []
        cells = [(l, r, c)]
        while fields[l][r, c] != 0:
            v = int(fields[l][r, c])
            nxt = None
            for dr, dc in MOVES:
                n = (r + dr, c + dc)
                if RR.legal(self.p[l], (r, c), n) and fields[l][n] != UNREACHED and int(fields[l][n]) + (self.wd if dr and dc else self.ws) == v:
                    nxt = (l,) + n
                    break
            if nxt is None:
                for link in self.links:
                    if not self.exists(link):
                        continue
                    a, b, w = link[0:3], link[3:6], link[6]
                    for here, other in ((b, a), (a, b)):                  # the walk a -> b first: here is b
                        if here == (l, r, c) and fields[other[0]][other[1], other[2]] != UNREACHED and \
                                int(fields[other[0]][other[1], other[2]]) + w == v:
                            nxt = other
                            break
                    if nxt is not None:
                        break
            if nxt is None:
                return []
            l, r, c = nxt
            cells.append(nxt)
        return cells[::-1]

    def paths(self, fields, goals):
        lists = [self.path(fields, g) for g in np.asarray(goals, np.int64).reshape(-1, 3)]
        off = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64)
        return off, np.array([c for x in lists for c in x], np.int32).reshape(-1, 3)

    def check_walk(self, fields, off, src):
        """along each path every consecutive pair is a legal R1 move or an existing link, and the costs add up to the field at the goal"""
        for a, b in zip(off[:-1], off[1:]):
            cells = [tuple(int(v) for v in t) for t in src[a:b]]
            if not cells:
                continue
            assert fields[cells[0][0]][cells[0][1:]] == 0
            total = 0
            for u, v in zip(cells[:-1], cells[1:]):
                cands = [k[6] for k in self.links if self.exists(k) and ((k[0:3], k[3:6]) == (u, v) or (k[0:3], k[3:6]) == (v, u))]
                if u[0] == v[0] and RR.legal(self.p[u[0]], u[1:], v[1:]):
                    cands.append(self.wd if (u[1] != v[1] and u[2] != v[2]) else self.ws)
                step = int(fields[v[0]][v[1:]]) - int(fields[u[0]][u[1:]])
                assert step in cands, (u, v, step, cands)                 # a legal R1 move or a link, at its cost
                total += step
            assert total == fields[cells[-1][0]][cells[-1][1:]]


def route(main_free_maps, links, start, goals, w_straight=5, w_diag=7, min_clearance=0):
    """hmsg_nav_building_route's composition"""
    pas = []
    for m in main_free_maps:
        m = np.asarray(m).astype(bool)
        pas.append(m & (RR.clearance(m, w_straight, w_diag) >= min_clearance) if min_clearance > 0 else m)
    B = Building(pas, links, w_straight, w_diag)
    l = int(start[0])
    cell, d2 = RR.snap(pas[l], [start[1:]])
    if cell[0, 0] >= 0:
        fields, _ = B.fields((l, cell[0, 0], cell[0, 1]))
    else:
        fields = [np.full(m.shape, UNREACHED, np.int32) for m in pas]
    gc, gd2, dist = B.snap(fields, goals)
    off, src = B.paths(fields, gc)
    return dict(passable=[m.astype(np.uint8) for m in pas], start_cell=(l, int(cell[0, 0]), int(cell[0, 1])), start_d2=int(d2[0]), fields=fields,
                goal_cell=gc, goal_d2=gd2, goal_dist=dist, path_off=off, path_src=src), B
