"""Inputs for the overlap counting of instance merging (find_overlapping_ratio_faiss, utils/graph_utils.py:620-662; the kernels
k_ov_count / k_ov_fill / k_ov_query / k_ov_query_second of holoagent_amd/csrc/hmsg_merge.hip behind the hook hmsg_test_overlap)
whose answer is known EXACTLY.

  lattice sets   voxel_size = 2^-4, so radius = 1.5 * voxel_size = 96 u and radius^2 = 9216 u^2 with u = 2^-10, both exact in
                 float32; every coordinate is an integer number of u below 64 m.  A difference is then an integer below 2^17 u, and
                 whenever all three are below 4096 u their squares and the sum (dx*dx + dy*dy) + dz*dz are integers below 2^26
                 that float32 holds exactly when below 2^24 (9216 is far below), while a larger difference squares to 2^24 u^2 or
                 more and rounding is monotone: "x has a point of Y closer than the radius" is `min_y |x - y|^2 < 9216` ON
                 INTEGERS (`model_hits`).  Query points are y + D for D among the integer triples with |D|^2 - 9216 in
                 {-2, 0, +1, +2} (`delta_classes`; -1 has no solution), every sign and axis order: only the -2 class is closer than
                 the radius, (0, 0, 96) and (32, 64, 64) lie ON the sphere and miss because the compare is strict.
  realistic sets voxel_size = 0.05 (radius 0.075, not dyadic): seeded surface patches with re-observed duplicates.  No model
                 here: the expectation is the reference's arithmetic restated in numpy float32 (`brute_f32`).
  BLAS form      overlap_distance_form = HMSG_OVERLAP_FAISS_BLAS: oracle.faiss_blas_nn_sqdist for a query cloud of 20 points or
                 more, the direct form below (faiss's own switch).

A `Case` holds clouds, optional base/delta splits and pairs; `Case.expected(form)` gives the counts of both directions of every pair.
For a lattice set in the direct form that is the integer model, and the float32 brute force is asserted to agree with it.  Builders
assert what a set is meant to contain (piles sit in one grid cell, a query's only witness is the intended point, ...): conditions on
the inputs, computed without the code under test."""
import functools
import itertools

import numpy as np

from oracle import hmsg_oracle as O

U = 2.0 ** -10
VS_LATTICE = 2.0 ** -4
VS_REAL = 0.05
R_U, R2_U = 96, 9216
FORM_DIRECT, FORM_BLAS = 0, 1

PLACES = {                                   # lower corner of a set, in u
    "origin": (0, 0, 0),
    "across_zero": (-300, -290, -310),
    "far": (31 * 1024, -6 * 1024, 27 * 1024),
    "binade_edges": (8 * 1024 - 300, 16 * 1024 - 300, 32 * 1024 - 300),
    "negative": (-40 * 1024, -17 * 1024, -3 * 1024),
}


def radius2_f32(vs):
    r = 1.5 * vs
    return np.float32(r * r)                 # (float)(radius * radius), as the merge passes it


def cell_index(p, mn, vs):
    """the grid cell of points p (float64 [n][3]) in the direct form's grid of a cloud whose lower corner is mn: the expression of
    ov_cell / Merger::grid_at / merger_set_reach in float64"""
    cell = (1.5 * vs) * (1.0 + 1e-3) + 2e-3
    o = np.asarray(mn, np.float64).astype(np.float32).astype(np.float64) - 1e-3
    return np.floor((np.asarray(p, np.float64).astype(np.float32).astype(np.float64) - o) / cell).astype(np.int64)


@functools.lru_cache(None)
def delta_classes():
    """{-2, 0, 1, 2} -> int64 [m][3]: every signed axis permutation of the triples with |D|^2 - 9216 = the key; and the triples up
    to order"""
    base = {c: [] for c in (-2, -1, 0, 1, 2)}
    for a in range(98):
        for b in range(a, 98):
            for c in range(b, 98):
                e = a * a + b * b + c * c - R2_U
                if e in base:
                    base[e].append((a, b, c))
    assert [len(base[c]) for c in (-2, -1, 0, 1, 2)] == [16, 0, 2, 15, 27], [len(base[c]) for c in (-2, -1, 0, 1, 2)]
    assert base[0] == [(0, 0, 96), (32, 64, 64)]
    out = {}
    for c in (-2, 0, 1, 2):
        s = set()
        for t in base[c]:
            for p in itertools.permutations(t):
                for sg in itertools.product((-1, 1), repeat=3):
                    s.add(tuple(x * y for x, y in zip(p, sg)))
        out[c] = np.array(sorted(s), np.int64)
    return out, base


def all_deltas():
    """-> (D int64 [m][3], cls int64 [m]) over the four classes"""
    cl, _ = delta_classes()
    return np.concatenate([cl[c] for c in (-2, 0, 1, 2)]), np.concatenate([np.full(len(cl[c]), c) for c in (-2, 0, 1, 2)])


def model_hits(X, Y):
    """integer model: which points of X (int64 [n][3], in u) have a point of Y with |x - y|^2 < 9216"""
    X, Y = np.asarray(X, np.int64), np.asarray(Y, np.int64)
    out = np.zeros(len(X), bool)
    step = max(1, (1 << 21) // max(len(Y), 1))
    for s in range(0, len(X), step):
        d = X[s:s + step, None, :] - Y[None, :, :]
        out[s:s + step] = (d * d).sum(-1).min(1) < R2_U
    return out


def brute_f32(X, Y, r2):
    """the reference's arithmetic, plainly: float32 points, (dx*dx + dy*dy) + dz*dz < r2 for SOME y (the exact float32 nearest
    neighbour is closer than the radius iff some point is)"""
    x, y = np.asarray(X).astype(np.float32), np.asarray(Y).astype(np.float32)
    out = np.zeros(len(x), bool)
    step = max(1, (1 << 21) // max(len(y), 1))
    for s in range(0, len(x), step):
        dx = x[s:s + step, None, 0] - y[None, :, 0]
        dy = x[s:s + step, None, 1] - y[None, :, 1]
        dz = x[s:s + step, None, 2] - y[None, :, 2]
        d = (dx * dx + dy * dy) + dz * dz
        assert d.dtype == np.float32
        out[s:s + step] = d.min(1) < r2
    return out


class Case:
    """clouds: float64 [n][3] each; ints: the same in u for a lattice set (None otherwise); n_base: per cloud, points in its base grid
    (None: one grid everywhere); pairs int32 [P][2]"""

    def __init__(self, name, vs, clouds=None, pairs=(), n_base=None, ints=None):
        self.name, self.vs = name, vs
        self.ints = None if ints is None else [np.asarray(c, np.int64).reshape(-1, 3) for c in ints]
        if self.ints is not None:
            assert all(np.abs(c).max(initial=0) < 64 * 1024 for c in self.ints), name
            clouds = [c * U for c in self.ints]
        self.clouds = [np.ascontiguousarray(c, np.float64).reshape(-1, 3) for c in clouds]
        self.pairs = np.ascontiguousarray(np.asarray(pairs, np.int32).reshape(-1, 2))
        self.n_base = None if n_base is None else np.array([len(c) if b is None else b for b, c in zip(n_base, self.clouds)], np.int64)
        self._hits = {}

    @property
    def sizes(self):
        return np.array([len(c) for c in self.clouds], np.int64)

    def work(self):
        n = self.sizes
        return int(2 * (n[self.pairs[:, 0]] * n[self.pairs[:, 1]]).sum())

    def hits(self, a, b, form):
        """which points of cloud a count against cloud b"""
        key = (int(a), int(b), int(form))
        if key not in self._hits:
            r2 = radius2_f32(self.vs)
            if form == FORM_BLAS and len(self.clouds[a]) >= 20:
                h = O.faiss_blas_nn_sqdist(self.clouds[a], self.clouds[b]) < r2
            else:
                h = brute_f32(self.clouds[a], self.clouds[b], r2)
                if self.ints is not None:
                    assert np.array_equal(h, model_hits(self.ints[a], self.ints[b])), \
                        "%s: the float32 brute force is not the integer model (%d, %d)" % (self.name, a, b)
            self._hits[key] = h
        return self._hits[key]

    def expected(self, form=FORM_DIRECT, pairs=None):
        """int64 [P][2]: points of the pair's first cloud that count, points of its second"""
        pairs = self.pairs if pairs is None else pairs
        return np.array([[int(self.hits(a, b, form).sum()), int(self.hits(b, a, form).sum())] for a, b in pairs], np.int64).reshape(-1, 2)


def _place(name):
    return np.array(PLACES[name], np.int64)


def grid_points(n, spacing):
    g = np.arange(n) * spacing
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).astype(np.int64)


def knife_clouds(place, ny=3, seed=0):
    """Y: ny^3 points 256 u apart (no two of them can serve one query); X: every delta of every class once, each hung on some y.
    -> X, Y, cls (of X's points), owner (which y)"""
    rng = np.random.default_rng(1000 + seed)
    Y = grid_points(ny, 256) + _place(place)
    D, cls = all_deltas()
    o = rng.permutation(len(D))
    D, cls = D[o], cls[o]
    owner = np.arange(len(D)) % len(Y)
    X = Y[owner] + D
    assert np.array_equal(model_hits(X, Y), cls == -2)
    return X, Y, cls, owner


@functools.lru_cache(None)
def knife(place):
    """every delta class around a 3 x 3 x 3 cloud, both directions, pair given both ways round"""
    X, Y, cls, _ = knife_clouds(place)
    c = Case("knife_" + place, VS_LATTICE, ints=[X, Y], pairs=[(0, 1), (1, 0)])
    c.cls = cls
    return c


SIZE_EDGES = (1, 255, 256, 257, 511, 512, 513)


@functools.lru_cache(None)
def knife_sizes():
    """query clouds of 1 .. 513 points and the full set (about 3000) against a 7^3 = 343-point cloud: the work lists' edges in either
    direction, and one pair with both clouds past a workgroup's 256 points"""
    X, Y, cls, _ = knife_clouds("far", ny=7, seed=1)
    assert len(X) > 2500 and len(Y) > 256
    ints = [Y] + [X[:n] for n in SIZE_EDGES] + [X]
    return Case("knife_sizes", VS_LATTICE, ints=ints, pairs=[(k, 0) for k in range(1, len(ints))])


@functools.lru_cache(None)
def faces(place):
    """the box filter: Y = the corners of a cube; beyond each of its six faces query points exactly r outside (|d|^2 = r^2: a miss
    the filter lets through), r + 1 u outside (the filter drops them), and -2 class deltas turned so that their longest side points
    outwards: beyond the face, yet with a witness"""
    cl, base = delta_classes()
    Y = grid_points(2, 256) + _place(place)
    t = max(base[-2], key=lambda q: q[2])                    # sorted ascending: q[2] is its longest side
    assert t[2] >= 90
    X, want, beyond = [], [], []
    for a in range(3):
        for s in (-1, 1):
            face = Y[:, a].min() if s < 0 else Y[:, a].max()
            rest = [q for q in range(3) if q != a]
            for y in Y[Y[:, a] == face]:
                for length, hit in ((96, False), (97, False)):
                    d = np.zeros(3, np.int64)
                    d[a] = s * length
                    X.append(y + d), want.append(hit), beyond.append(length)
                for (p, q) in ((t[0], t[1]), (t[1], t[0])):
                    for sp, sq in itertools.product((-1, 1), repeat=2):
                        d = np.zeros(3, np.int64)
                        d[a], d[rest[0]], d[rest[1]] = s * t[2], sp * p, sq * q
                        X.append(y + d), want.append(True), beyond.append(t[2])
                d = np.zeros(3, np.int64)                    # (32, 64, 64): on the sphere, 64 u beyond the face
                d[a], d[rest[0]], d[rest[1]] = s * 64, 32, -64
                X.append(y + d), want.append(False), beyond.append(64)
    X, want = np.array(X, np.int64), np.array(want)
    assert np.array_equal(model_hits(X, Y), want) and want.sum() >= 6 * 4 * 8
    lo, hi = Y.min(0), Y.max(0)
    assert (((X < lo) | (X > hi)).any(1)).all()              # every query lies outside Y's box
    return Case("faces_" + place, VS_LATTICE, ints=[X, Y], pairs=[(0, 1)])


@functools.lru_cache(None)
def degenerate(place):
    """a one-point cloud (a grid of one cell), a collinear one, a planar one (one layer of cells), two clouds with the same points"""
    D, cls = all_deltas()
    p0 = _place(place)
    ints, pairs = [], []
    one = p0[None, :]
    line = p0 + np.stack([np.arange(5) * 256, np.zeros(5, np.int64), np.zeros(5, np.int64)], -1)
    g = np.arange(3) * 256
    plane = p0 + np.stack(np.meshgrid(g, g, [0], indexing="ij"), -1).reshape(-1, 3)
    for Y in (one, line, plane):
        X = Y[np.arange(len(D)) % len(Y)] + D
        assert np.array_equal(model_hits(X, Y), cls == -2)
        pairs.append((len(ints), len(ints) + 1))
        ints += [X, Y]
    X = plane[np.arange(len(D)) % len(plane)] + D
    pairs.append((len(ints), len(ints) + 1))
    ints += [X, X.copy()]
    pairs.append((len(ints), len(ints) + 1))                 # one point against one point, a miss on the sphere and a hit
    ints += [one + np.array([0, 0, 96]), one]
    pairs.append((len(ints), len(ints) + 1))
    ints += [one + np.array([1, 95, 13]), one]
    assert 1 + 95 * 95 + 13 * 13 < R2_U
    return Case("degenerate_" + place, VS_LATTICE, ints=ints, pairs=pairs)


def _unique_witness(X, Y):
    """for every x: the number of y closer than r, and the first of them"""
    d = X[:, None, :] - Y[None, :, :]
    w = (d * d).sum(-1) < R2_U
    return w.sum(1), w.argmax(1)


PILE_SIZES = (1, 2, 3, 4, 5, 8, 9)


@functools.lru_cache(None)
def piles(place):
    """cells that hold 1, 2, 3, 4, 5, 8 and 9 points (the tail of the 4-wide scan): the corners of one grid cell (98.1 u wide) and a
    point on an edge, and for every one of them a query whose ONLY witness it is -- whichever ends up last in the cell's sorted run
    is somebody's only witness.  Then one cell with 400 copies of each of two points and a query for either."""
    cl, base = delta_classes()
    t = max((q for q in base[-2] if q[0] > 0), key=lambda q: q[0])       # a -2 class delta with three non-zero sides
    p0 = _place(place)
    corners = np.array([(x, y, z) for x in (0, 97) for y in (0, 97) for z in (0, 97)], np.int64)
    pts = np.concatenate([corners, [[48, 0, 0]]])
    qry = np.concatenate([corners + np.where(corners == 0, -1, 1) * np.array(t), [[48, -60, -60]]])
    ints, pairs = [], []
    for k in PILE_SIZES:
        Y, X = pts[:k] + p0, qry[:k] + p0
        n_w, who = _unique_witness(X, Y)
        assert (n_w == 1).all() and np.array_equal(who, np.arange(k)), (k, n_w, who)
        assert (cell_index(Y * U, Y.min(0) * U, VS_LATTICE) == 0).all()   # one cell
        pairs.append((len(ints), len(ints) + 1))
        ints += [X, Y]
    two = np.array([(0, 0, 0), (97, 97, 97)], np.int64) + p0
    Y = np.repeat(two, 400, axis=0)[np.random.default_rng(3).permutation(800)]
    X = np.concatenate([two[:1] - np.array(t), two[1:] + np.array(t), two[:1] - np.array([0, 0, 96])])
    n_w, _ = _unique_witness(X, two)
    assert list(n_w) == [1, 1, 0] and (cell_index(Y * U, Y.min(0) * U, VS_LATTICE) == 0).all()
    pairs.append((len(ints), len(ints) + 1))
    ints += [X, Y]
    return Case("piles_" + place, VS_LATTICE, ints=ints, pairs=pairs)


@functools.lru_cache(None)
def neighbours(place):
    """a query in the middle cell of a 3 x 3 x 3 grid whose only witness sits in each of the 26 cells around it in turn (two anchor
    points span the grid and are out of reach)"""
    p0 = _place(place)
    anchors = np.array([(0, 0, 0), (290, 290, 290)], np.int64)
    y_of, x_of = {-1: 97, 0: 146, 1: 196}, {-1: 98, 0: 146, 1: 195}
    ints, pairs = [], []
    for d in itertools.product((-1, 0, 1), repeat=3):
        if d == (0, 0, 0):
            continue
        Y = np.concatenate([anchors, [[y_of[q] for q in d]]]) + p0
        X = np.array([[x_of[q] for q in d]], np.int64) + p0
        n_w, who = _unique_witness(X, Y)
        assert n_w[0] == 1 and who[0] == 2
        cy, cx = cell_index(Y * U, Y.min(0) * U, VS_LATTICE), cell_index(X * U, Y.min(0) * U, VS_LATTICE)
        assert (cx[0] == 1).all() and (cy[2] == 1 + np.array(d)).all() and (cy[0] == 0).all() and (cy[1] == 2).all()
        pairs.append((len(ints), len(ints) + 1))
        ints += [X, Y]
    return Case("neighbours_" + place, VS_LATTICE, ints=ints, pairs=pairs)


@functools.lru_cache(None)
def base_delta(place):
    """clouds that GREW after they were indexed: a base grid over the first points (on their box) and a delta grid over the rest, part
    of which lies outside the base box.  Y: 8 points of a 3^3 lattice first, then the other 19, then re-observed copies of four base
    and three delta points -- so a query finds its witness in the base grid only, in the delta grid only, or in both.  X: the
    queries around the base points first.  Each cloud once whole and once split; all four combinations must count alike."""
    X, Y, cls, owner = knife_clouds(place, seed=2)
    g = (Y - _place(place)) // 256
    first = (g < 2).all(1)
    oy = np.concatenate([np.flatnonzero(first), np.flatnonzero(~first)])
    nby = int(first.sum())
    assert nby == 8
    Yo = Y[oy]
    Ys = np.concatenate([Yo, Yo[[0, 3, 5, 6]], Yo[[9, 14, 20]]])
    in_base = first[owner]
    ox = np.concatenate([np.flatnonzero(in_base), np.flatnonzero(~in_base)])
    Xs, cls_s, nbx = X[ox], cls[ox], int(in_base.sum())
    # delta points partly outside the base box (the cloud grew), partly inside it
    for P, nb in ((Ys, nby), (Xs, nbx)):
        lo, hi = P[:nb].min(0), P[:nb].max(0)
        out = ((P[nb:] < lo) | (P[nb:] > hi)).any(1)
        assert out.any() and (P is Xs or (~out).any())
    hb, hd = model_hits(Xs, Ys[:nby]), model_hits(Xs, Ys[nby:])
    assert (hb & ~hd).sum() > 20 and (~hb & hd).sum() > 20 and (hb & hd).sum() > 20       # base only, delta only, both
    ints = [Xs, Xs.copy(), Ys, Ys.copy()]
    c = Case("base_delta_" + place, VS_LATTICE, ints=ints, pairs=[(0, 2), (1, 2), (0, 3), (1, 3)], n_base=[None, nbx, None, nby])
    return c


# ---- realistic radius
def patch(rng, n, shift):
    """a re-observed surface (cloud(rng, n, 1) of tests/test_dbscan_hook.py): half the points on exact 5 cm lattice sites"""
    p = np.zeros((n, 3))
    p[:, 0], p[:, 1], p[:, 2] = rng.uniform(0, 1.5, n), rng.uniform(0, 1.0, n), rng.normal(0, 0.004, n)
    m = rng.random(n) < 0.5
    p[m] = (np.round(p / 0.05) * 0.05)[m]
    return p + np.asarray(shift, np.float64)


@functools.lru_cache(None)
def realistic(place):
    rng = np.random.default_rng(77)
    p0 = np.array(PLACES[place], np.float64) * U
    A = patch(rng, 1200, p0)
    A = A[np.argsort(A[:, 0], kind="stable")]                             # (so that the points behind n_base extend the box)
    B = np.concatenate([A[rng.integers(0, len(A), 500)] + rng.normal(0, 0.02, (500, 3)), patch(rng, 300, p0 + [0.9, 0.4, 0.03])])
    Cc = patch(rng, 700, p0 + [0.7, 0.3, 0.02])
    Dd = patch(rng, 150, p0 + [0.2, 0.2, 0.07])                           # 7 cm above A: around the radius
    Dd[:, :2] = p0[:2] + 0.2 + (Dd[:, :2] - p0[:2] - 0.2) * 0.4
    small = [patch(rng, n, p0 + [0.5, 0.5, 0.06]) for n in (19, 20, 21)]
    for s in small:
        s[:, :2] = p0[:2] + 0.5 + (s[:, :2] - p0[:2] - 0.5) * 0.2
    clouds = [A, B, Cc, Dd] + small + [A.copy(), B.copy()]
    nb = [None] * 7 + [900, 500]
    pairs = [(a, b) for a in range(7) for b in range(a + 1, 7)] + [(7, 1), (0, 8), (7, 8), (3, 7), (8, 4), (5, 8)]
    return Case("realistic_" + place, VS_REAL, clouds=clouds, pairs=pairs, n_base=nb)


@functools.lru_cache(None)
def lattice_small(place):
    """lattice query clouds of 19, 20 and 21 points (faiss's switch between its two forms) and a full one"""
    X, Y, cls, _ = knife_clouds(place, seed=3)
    ints = [Y, X[:19], X[100:120], X[200:221], X]
    return Case("lattice_small_" + place, VS_LATTICE, ints=ints, pairs=[(k, 0) for k in range(1, 5)])


def forms_differ(case):
    """point decisions of the case on which the two distance forms differ"""
    n = 0
    for a, b in case.pairs:
        for x, y in ((a, b), (b, a)):
            n += int((case.hits(x, y, FORM_DIRECT) != case.hits(x, y, FORM_BLAS)).sum())
    return n


# ---- decision mode
THRESHOLDS = (0.0, 0.25, 0.75, 0.9999)
N_SITES = 24
SMALL_KINDS = ("all4", "3of4", "1of4", "0of4", "chair", "wide", "spots")
P_EDGES = (1, 255, 256, 257, 640)


@functools.lru_cache(None)
def decision_pool():
    """24 sites 1500 u apart.  Per site a FLOOR (300 points, 20 x 15 at 40 u), at four sites a second large cloud of three piles
    of 100 points, and seven small clouds of 4 points:
      all4 / 3of4 / 1of4 / 0of4   the floor's corners lifted by 95 u (a witness below) or 96 u (none): first ratios 1, 0.75, 0.25
                                  and 0 -- EXACTLY the thresholds; their box covers the floor, so no bound: the floor is scanned
                                  and few of its points count
      chair                       4 points over one corner: first ratio 0.25, and few floor points near its box: the bound decides
      wide                        no witness anywhere and a box over ALL sites: every floor is scanned against it (2 chunks each)
      spots                       3 points in the piles of the second large cloud + 1 far off: first ratio 0.75 and EVERY point of
                                  the larger cloud counts: the second direction decides
    -> Case whose pairs are: every same-site pair, wide x every floor (16 wides), and cross-site pairs to fill up; shuffled."""
    rng = np.random.default_rng(11)
    gx, gy = np.meshgrid(np.arange(20) * 40, np.arange(15) * 40, indexing="ij")
    floor = np.stack([gx.ravel(), gy.ravel(), np.zeros(300, np.int64)], -1).astype(np.int64)
    cor = np.array([(0, 0), (760, 0), (0, 560), (760, 560)], np.int64)
    lift = {"all4": (95, 95, 95, 95), "3of4": (95, 95, 95, 96), "1of4": (95, 96, 96, 96), "0of4": (96, 96, 96, 96)}
    ints, kind, site = [], [], []
    span_lo, span_hi = np.array([-3900, -2400]), np.array([4700, 3000])       # (around every site)
    for j in range(N_SITES):
        off = np.array([(j % 6) * 1500 - 3750, (j // 6) * 1500 - 2250, 0], np.int64)
        ints.append(floor + off), kind.append("floor"), site.append(j)
        if j < 4:
            spots = np.array([(0, 0, 2000), (300, 0, 2000), (0, 300, 2000)], np.int64)
            ints.append(np.repeat(spots, 100, axis=0)[rng.permutation(300)] + off), kind.append("spots_large"), site.append(j)
        for kd in SMALL_KINDS:
            if kd in lift:
                p = np.concatenate([cor, np.array(lift[kd])[:, None]], 1)
            elif kd == "chair":
                p = np.array([(0, 0, 95), (40, 0, 96), (0, 40, 96), (40, 40, 96)], np.int64)
            elif kd == "wide":
                p = np.array([(0, 0, 96), (40, 40, 96), (0, 0, 500), (0, 0, 500)], np.int64)
                p[2, :2], p[3, :2] = span_lo - off[:2], span_hi - off[:2]
            else:
                if j >= 4:
                    continue
                p = np.array([(0, 0, 2095), (300, 0, 1905), (0, 395, 2000), (900, 900, 3000)], np.int64)
            ints.append(p + off), kind.append(kd), site.append(j)
    kind, site = np.array(kind), np.array(site)
    large = np.flatnonzero((kind == "floor") | (kind == "spots_large"))
    small = np.flatnonzero((kind != "floor") & (kind != "spots_large"))
    pairs = [(s, l) for s in small for l in large if site[s] == site[l]]
    wides = [s for s in small if kind[s] == "wide"][:16]
    pairs += [(s, l) for s in wides for l in large if kind[l] == "floor" and site[s] != site[l]]
    seen = set(pairs)
    while len(pairs) < 640:
        s, l = int(rng.choice(small)), int(rng.choice(large))
        if (s, l) not in seen and kind[s] != "wide":
            seen.add((s, l)), pairs.append((s, l))
    pairs = [pairs[i] for i in rng.permutation(len(pairs))]
    pairs = [(b, a) if rng.random() < 0.5 else (a, b) for a, b in pairs]
    nb = [None] * len(ints)
    nb[0], nb[1] = 200, 120                                  # a floor and a pile cloud that grew
    c = Case("decision_pool", VS_LATTICE, ints=ints, pairs=pairs, n_base=nb)
    c.kind, c.site = kind, site
    return c


@functools.lru_cache(None)
def many_small():
    """all 2080 pairs of 65 ten-point clouds strung along a line, neighbours overlapping: more pairs than the planned second launch
    takes (OV2_MAX_PAIRS = 2048), so the default path falls back to a workgroup per chunk"""
    rng = np.random.default_rng(5)
    ints = [np.array([i * 60, 0, 0]) + rng.integers(-50, 51, (10, 3)) for i in range(65)]
    pairs = [(a, b) for a in range(65) for b in range(a + 1, 65)]
    assert len(pairs) == 2080
    return Case("many_small", VS_LATTICE, ints=ints, pairs=pairs)


def lattice_value_cases():
    """every lattice set of the value-mode test, direct form"""
    out = [knife(p) for p in PLACES] + [knife_sizes()]
    for p in ("origin", "far"):
        out += [faces(p), degenerate(p), piles(p), neighbours(p), base_delta(p), lattice_small(p)]
    out += [faces("binade_edges"), faces("negative"), base_delta("across_zero"), decision_pool(), many_small()]
    return out
