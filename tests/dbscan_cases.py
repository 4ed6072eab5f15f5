"""Inputs for the batched cosine DBSCAN (feats_denoise_dbscan, utils/graph_utils.py:682-728) whose answer is known EXACTLY.

A set is built from an integer model, so that who is whose neighbour never depends on floating point:

  lattice arcs   rows are unit vectors at integer positions p on great-circle arcs, angle p * step with
                 step = arccos(1 - eps) / (m + 0.5), one arc per `group` (mutually orthogonal planes; the negated rows of a plane
                 are a group of their own).  Two rows are neighbours iff they share the group and |dp| <= m.  The set is rotated
                 by a random orthogonal matrix, every row scaled by a factor in [0.25, 4] and the rows permuted.
  knife edge     rows in {+-1/16}^256 (times a power of two): norms, products and every partial sum are exact in float32 in any
                 order, the cosine distance is h / 128 for Hamming distance h -- a pair may sit exactly ON eps.

From the neighbour relation the rest is sklearn's algorithm restated on integers (`expect`): core rows, dbscan_inner's labels
(clusters numbered by their first core row, a border row to the first cluster that reaches it), Counter.most_common, and the
representative as the sum of the chosen rows in row order in the input dtype, divided once -- asserted equal to np.mean(axis=0),
the call the reference program makes.

Every builder calls `check_margin`: the float64 cosine distances of the rows it returns must give the integer model's relation,
and no distance may lie within 4 * tau of eps, tau = (D + 8) * u (u = 2^-24 / 2^-53: the worst-case error of a length-D fma
chain on unit rows plus the normalisation).  Nothing is left out for a small margin: a builder that cannot keep it fails."""
from collections import Counter

import numpy as np

GAPS_DEFAULT = (0, 1, 2, "m", "m+1", "2m+1")


def unit_roundoff(dtype):
    return 2.0 ** -24 if np.dtype(dtype) == np.float32 else 2.0 ** -53


def eps_as_seen(eps, dtype):
    """the threshold the kernels compare with: the float32 path takes (float)eps"""
    return float(np.float32(eps)) if np.dtype(dtype) == np.float32 else float(eps)


def model_adjacency(group, pos, m):
    group, pos = np.asarray(group, np.int64), np.asarray(pos, np.int64)
    return (group[:, None] == group[None, :]) & (np.abs(pos[:, None] - pos[None, :]) <= m)


def float64_distances(X, dtype):
    """sklearn's cosine_distances of the rows, in float64: normalise (a zero row stays zero), 1 - X^ X^T clipped to [0, 2], diagonal 0.
    A row whose squared norm overflows the input dtype has an infinite norm there and normalises to zero (nan_to_num's +-max)."""
    X64 = np.asarray(X, np.float64)
    n2 = np.einsum("ij,ij->i", X64, X64)
    nrm = np.sqrt(n2)
    over = n2 > float(np.finfo(dtype).max)
    nrm[nrm == 0] = 1.0
    Xn = X64 / nrm[:, None]
    Xn[over] = 0.0
    d = np.clip(1.0 - Xn @ Xn.T, 0.0, 2.0)
    np.fill_diagonal(d, 0.0)
    return d


def check_margin(X, adj, eps, dtype):
    """-> margin / tau (>= 4, asserted) after asserting that the float64 relation is the integer model's"""
    D = X.shape[1]
    e = eps_as_seen(eps, dtype)
    d = float64_distances(X, dtype)
    assert np.array_equal(d <= e, adj), "the float64 adjacency is not the integer model's"
    off = ~np.eye(len(X), dtype=bool)
    if not off.any():
        return np.inf
    tau = (D + 8) * unit_roundoff(dtype)
    margin = float(np.min(np.abs(d - e)[off]))
    assert margin >= 4 * tau, "margin %.3g < 4 tau = %.3g (D %d, eps %g)" % (margin, 4 * tau, D, eps)
    return margin / tau


def dbscan_inner(adj, core):
    """sklearn/cluster/_dbscan_inner.pyx restated: depth-first over the core rows, labels in order of discovery"""
    n = len(adj)
    labels = np.full(n, -1, np.int64)
    nbrs = [None] * n
    label_num = 0
    for start in range(n):
        if labels[start] != -1 or not core[start]:
            continue
        i, stack = start, []
        while True:
            if labels[i] == -1:
                labels[i] = label_num
                if core[i]:
                    if nbrs[i] is None:
                        nbrs[i] = np.flatnonzero(adj[i])
                    stack.extend(int(v) for v in nbrs[i] if labels[v] == -1)
            if not stack:
                break
            i = stack.pop()
        label_num += 1
    return labels


def sequential_mean(rows):
    """sum in row order in the rows' dtype, one division: what np.mean(axis=0) does on a C-contiguous [n, D] array (asserted)"""
    rows = np.ascontiguousarray(rows)
    acc = rows[0].copy()
    for r in rows[1:]:
        acc = acc + r
    assert acc.dtype == rows.dtype
    out = acc / rows.dtype.type(len(rows)) if len(rows) > 1 else acc
    with np.errstate(over="ignore", invalid="ignore"):
        ref = np.mean(rows, axis=0)
    assert ref.dtype == rows.dtype and np.array_equal(bits(out), bits(ref)), "np.mean(axis=0) is not the sequential sum"
    return out


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


class Expected:
    pass


def expect(X, adj, min_samples):
    """feats_denoise_dbscan from the neighbour relation: -> .rep, .n_in_cluster (0 = no cluster), .labels, .core, .chosen"""
    e = Expected()
    e.core = adj.sum(axis=1) >= min_samples
    e.labels = dbscan_inner(adj, e.core)
    c = Counter(int(v) for v in e.labels)
    c.pop(-1, None)
    if c:
        e.chosen = e.labels == c.most_common(1)[0][0]
        e.n_in_cluster = int(e.chosen.sum())
    else:
        e.chosen = np.ones(len(X), bool)
        e.n_in_cluster = 0
    e.rep = sequential_mean(X[e.chosen])
    e.n_clusters = len(c)
    return e


class Case:
    """one set: .X rows, .adj the exact relation, .eps, .dtype, .ratio (margin / tau), .group / .pos / .m for lattice sets"""

    def expect(self, min_samples):
        return expect(self.X, self.adj, min_samples)


def random_orthogonal(rng, D):
    q, r = np.linalg.qr(rng.standard_normal((D, D)))
    return q * np.sign(np.diag(r))[None, :]


def lattice_limits(eps, m):
    a = np.arccos(1.0 - eps)
    step = a / (m + 0.5)
    return step, int(np.floor((2 * np.pi - 2 * a) / step)) - 1       # positions stay below (2 pi - 2 a) / step: nothing wraps


def draw_positions(rng, n, m, pmax, gaps=GAPS_DEFAULT, weights=None):
    """n positions in [0, pmax] from cumulative gaps; once the arc is full the remaining rows repeat earlier positions"""
    val = {"m": m, "m+1": m + 1, "2m+1": 2 * m + 1}
    g = np.array([val.get(x, x) for x in gaps], np.int64)
    p = np.cumsum(g[rng.choice(len(g), n, p=weights)])
    p -= p[0]
    late = p > pmax
    if late.any():
        first = int(np.argmax(late))
        p[first:] = p[rng.integers(0, first, n - first)]
    return p


def lattice_from_model(rng, group, pos, D, eps, m, dtype, planes=None, zero=None):
    """rows for the integer model.  group g < planes: the arc in plane g; planes <= g < 2 * planes: the NEGATED rows of plane
    g - planes (antipodal to it, never its neighbours); rows flagged in `zero` become all-zero rows: they stay zero, have d = 1 to
    everything and count only themselves (the model gives each a group of its own)."""
    group, pos = np.array(group, np.int64), np.array(pos, np.int64)
    n = len(group)
    zero = np.zeros(n, bool) if zero is None else np.asarray(zero, bool)
    if planes is None:
        planes = int(group[~zero].max()) + 1 if (~zero).any() else 1
    assert 2 * planes <= D, "a set needs 2 * planes <= D"
    step, pmax = lattice_limits(eps, m)
    if (group[~zero] >= planes).any():                  # +x at p and -x at p' must not meet: keep the arcs below half a turn
        pmax = int(np.floor((np.pi - 2 * np.arccos(1.0 - eps)) / step)) - 1
    assert (group[~zero] < 2 * planes).all() and pos.min() >= 0 and pos.max() <= pmax, "positions wrap"
    group[zero] = 2 * planes + np.arange(int(zero.sum()))
    plane = np.where(zero, 0, group % planes)
    sign = np.where(group >= planes, -1.0, 1.0)
    U = np.zeros((n, D))
    U[np.arange(n), 2 * plane] = sign * np.cos(pos * step)
    U[np.arange(n), 2 * plane + 1] = sign * np.sin(pos * step)
    U = U @ random_orthogonal(rng, D).T
    U *= rng.uniform(0.25, 4.0, n)[:, None]
    X = np.ascontiguousarray(U.astype(dtype))
    X[zero] = 0
    first = {}
    for i in range(n):                                  # about half of the repeats of a position are EXACT copies, the rest scaled ones
        j = first.setdefault((int(group[i]), int(pos[i])), i)
        if j != i and rng.random() < 0.5:
            X[i] = X[j]
    c = Case()
    c.X, c.group, c.pos, c.m, c.eps, c.dtype = X, group, pos, m, eps, np.dtype(dtype)
    c.adj = model_adjacency(group, pos, m)
    c.ratio = check_margin(X, c.adj, eps, dtype)
    return c


def lattice(seed, n, D, eps, m, dtype, planes=None, weights=None, order="perm", n_zero=0, antipodal=False):
    """a random lattice set: rows dealt to the planes, cumulative gaps from {0, 1, 2, m, m + 1, 2m + 1} inside a plane (0: duplicates,
    m: sparse runs, above m: the chain breaks).  order: "perm" (rows permuted), "sorted" (group, position), "reverse".  antipodal:
    a fifth of the rows negated, among them the exact negative of row 0's direction.  n_zero: all-zero rows."""
    rng = np.random.default_rng(seed)
    step, pmax = lattice_limits(eps, m)
    if antipodal:
        pmax = int(np.floor((np.pi - 2 * np.arccos(1.0 - eps)) / step)) - 1
    if planes is None:
        planes = max(1, min(D // 2, 1 + n // 48))
    n_zero = min(n_zero, max(n - 1, 0))
    n_l = n - n_zero
    per = np.bincount(rng.integers(0, planes, n_l), minlength=planes)
    group, pos = [], []
    for g in range(planes):
        if per[g]:
            group += [g] * int(per[g])
            pos += list(draw_positions(rng, int(per[g]), m, pmax, weights=weights))
    group, pos = np.array(group, np.int64), np.array(pos, np.int64)
    if antipodal and n_l >= 2:
        flip = rng.random(n_l) < 0.2
        flip[:2] = (False, True)
        group[1], pos[1] = group[0], pos[0]             # rows 0 and 1: an antipodal pair
        group = np.where(flip, group + planes, group)
    group = np.concatenate([group, np.zeros(n_zero, np.int64)])
    pos = np.concatenate([pos, np.zeros(n_zero, np.int64)])
    zero = np.arange(n) >= n_l
    if order == "perm":
        o = rng.permutation(n)
    else:
        o = np.lexsort((pos, group))
        if order == "reverse":
            o = o[::-1]
    return lattice_from_model(rng, group[o], pos[o], D, eps, m, dtype, planes=planes, zero=zero[o])


# ---- the exact knife edge
KNIFE_D = 256
KNIFE_EPS = 2.0 ** -6


def knife_edge(seed, chain, n_noise, dtype, eps=KNIFE_EPS, n_dup=0, order="perm"):
    """a chain of `chain` rows in {+-1/16}^256 in which consecutive rows differ in two coordinates (d = 2 / 128 = 2^-6 exactly, rows
    further apart 4 / 128 and more), n_dup exact copies of chain rows, n_noise unrelated random sign rows; every row times a power
    of two.  The relation is h / 128 <= eps on the Hamming matrix, evaluated exactly (both sides are dyadic)."""
    rng = np.random.default_rng(seed)
    assert 2 * (chain - 1) <= KNIFE_D
    S = np.empty((chain + n_dup + n_noise, KNIFE_D), np.int8)
    S[0] = rng.choice([-1, 1], KNIFE_D)
    flips = rng.permutation(KNIFE_D)
    for i in range(1, chain):
        S[i] = S[i - 1]
        S[i, flips[2 * (i - 1):2 * i]] *= -1
    S[chain:chain + n_dup] = S[rng.integers(0, chain, n_dup)]
    S[chain + n_dup:] = rng.choice([-1, 1], (n_noise, KNIFE_D))
    if order == "perm":
        S = S[rng.permutation(len(S))]
    H = (KNIFE_D - S.astype(np.int64) @ S.astype(np.int64).T) // 2
    scale = 2.0 ** rng.integers(-2, 3, len(S))
    c = Case()
    c.X = np.ascontiguousarray((S / 16.0 * scale[:, None]).astype(dtype))
    assert np.array_equal(c.X.astype(np.float64), S / 16.0 * scale[:, None])          # exact in the dtype
    e = eps_as_seen(eps, dtype)
    c.adj = (H / 128.0) <= e                                                             # h / 128 and e are exact doubles
    c.H, c.eps, c.dtype, c.m = H, eps, np.dtype(dtype), None
    # no margin here BY DESIGN (links sit on eps); what is asserted instead is that float64 reproduces the exact distances
    assert np.array_equal(float64_distances(c.X, dtype), H / 128.0)
    c.ratio = 0.0
    return c


# ---- what a set contains (asserted by the structure tests)
def structure(case, min_samples):
    """-> dict: clusters, borders, borders_between (border rows adjacent to cores of two clusters), noise, top_tie (the two largest
    clusters have equal size), border_decides_size / border_decides_order (see the tests), hops (longest shortest path between
    core rows of one cluster, in steps of the relation)"""
    e = case.expect(min_samples)
    adj, core, lab = case.adj, e.core, e.labels
    s = dict(clusters=e.n_clusters, borders=int(((lab >= 0) & ~core).sum()), noise=int((lab < 0).sum()), cores=int(core.sum()))
    between = 0
    for i in np.flatnonzero((lab >= 0) & ~core):
        between += len(set(lab[np.flatnonzero(adj[i] & core)])) >= 2
    s["borders_between"] = int(between)
    sizes = Counter(int(v) for v in lab if v >= 0)
    core_sizes = Counter(int(v) for v in lab[core])
    top = sizes.most_common(2)
    s["top_tie"] = len(top) == 2 and top[0][1] == top[1][1]
    # the largest cluster is strictly larger than the runner-up only through its border rows
    s["border_decides_size"] = len(top) == 2 and top[0][1] > top[1][1] and core_sizes[top[0][0]] <= core_sizes[top[1][0]]
    # on a tie, the winner (first to appear in row order) is not the tied cluster with the smallest label: a border row appears first
    s["border_decides_order"] = s["top_tie"] and sizes.most_common(1)[0][0] != min(k for k, v in sizes.items() if v == top[0][1])
    return s


def hops(case, min_samples):
    """eccentricity of the lowest core row inside its cluster (breadth-first over core rows)"""
    e = case.expect(min_samples)
    cores = np.flatnonzero(e.core)
    if not len(cores):
        return 0
    seen = np.zeros(len(case.X), bool)
    front = np.zeros(len(case.X), bool)
    front[cores[0]] = seen[cores[0]] = True
    h = 0
    while True:
        nxt = case.adj[front].any(axis=0) & e.core & ~seen
        if not nxt.any():
            return h
        seen |= nxt
        front = nxt
        h += 1
