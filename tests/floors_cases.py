"""Inputs and references for the storeys of the map (hmsg_segment_floors, include/hmsg.h: the kernels k_fl_yrange / k_fl_hist /
k_fl_crop of holoagent_amd/csrc/hmsg_floors.hip, the host half in hmsg_floors_host.h; the Python mirror
Graph._segment_floors_host) -- Graph.segment_floors_manually of the reference (graph.py:624-787).

  reference(counts, ymin, ymax)   from a height histogram to the slabs with scipy and numpy themselves: gaussian_filter1d on the
                 int64 counts, np.percentile, find_peaks, chains of gaps <= 1, the pick and the adjust rules.  Two orders are the
                 LIBRARY's definitions (scipy and the reference sort with numpy's default argsort, which defines nothing among equal
                 values): find_peaks' distance rule visits equally high peaks from the higher position down, and the pick of a chain's
                 highest peaks keeps the higher positions among equals.  ties="numpy" is plain find_peaks(distance=20.0) and default
                 argsort instead; where a histogram has no tie the two must agree, and `Ref.pick_tie` / `Ref.dist_tie` say whether it
                 has one.
  exact family   clouds in which every 5 cm voxel of the re-sampling grid (Open3D voxel_down_sample, graph.py:633) holds exactly
                 one point: every point has an (x, z) column of its own, 10 cm from the next.  The re-sampled cloud is then the
                 cloud itself bit for bit, and `reference_floors` is the whole answer with no tolerance: np.histogram, `reference`,
                 numpy crops.  The heights are what is hostile: on bin edges computed as the kernel computes them and one ulp either
                 side, at ymax, on shared slab edges, across zero, -0.0, all negative.
  general family many points per voxel: the re-sampling averages, so the C ABI is compared with the mirror (which re-samples through
                 the library; that step is pinned elsewhere).  `general_analysis` re-samples with the oracle to say which cases hold
                 a tie.

Seeds are PCG64 (np.random.default_rng); no cloud has more than 30 000 points.  Builders assert what a case is meant to contain,
without the code under test."""
import functools

import numpy as np
from scipy.ndimage import gaussian_filter1d
from scipy.signal import find_peaks

from oracle import hmsg_oracle as O

MAX_POINTS = 30000
DISTANCE = 0.2 / 0.01                    # find_peaks' distance, in bins (graph.py:648)


def distance_rule(peaks, heights, distance, reverse_ties=False):
    """find_peaks' distance rule as scipy documents it: the highest peak first, and every peak that is kept removes all others
    closer than ceil(distance).  Equal heights: the higher position first (reverse_ties: the lower, to see whether it matters)."""
    peaks, heights = np.asarray(peaks, np.int64), np.asarray(heights, np.int64)
    d = int(np.ceil(distance))
    pos = np.arange(len(peaks))
    order = sorted(pos.tolist(), key=lambda i: (-int(heights[i]), i if reverse_ties else -i))
    alive = np.ones(len(peaks), bool)
    for i in order:
        if alive[i]:
            alive &= (np.abs(peaks - peaks[i]) >= d) | (pos == i)
    return peaks[alive]


class Ref:
    pass


def reference(counts, ymin, ymax, ties="library"):
    """-> Ref: smooth int64 [bins], peaks int64 [m], slabs float64 [n_floors][2], chains (list of peak arrays), picks, and
    pick_tie: a chain has more peaks than it may keep and the lowest height kept is also the highest height dropped;
    dist_tie: two peaks of equal height at or above the percentile are closer than 20 bins;
    dist_tie_decides: ... and visiting them the other way round keeps other peaks"""
    counts = np.asarray(counts, np.int64)
    bins = len(counts)
    edges = np.linspace(ymin, ymax, bins + 1)                # np.histogram's edges for bins = an int
    r = Ref()
    r.edges = edges
    r.smooth = gaussian_filter1d(counts, sigma=2)
    assert r.smooth.dtype == np.int64
    r.height = np.percentile(r.smooth, 90)
    cand, _ = find_peaks(r.smooth, height=r.height)
    r.candidates = cand
    near = [(a, b) for i, a in enumerate(cand) for b in cand[i + 1:] if b - a < np.ceil(DISTANCE) and r.smooth[a] == r.smooth[b]]
    r.dist_tie = bool(near)
    lib_peaks = distance_rule(cand, r.smooth[cand], DISTANCE)
    r.dist_tie_decides = not np.array_equal(lib_peaks, distance_rule(cand, r.smooth[cand], DISTANCE, reverse_ties=True))
    if ties == "numpy":
        r.peaks, _ = find_peaks(r.smooth, distance=DISTANCE, height=r.height)
    else:
        r.peaks = lib_peaks
    locs = edges[r.peaks]
    r.chains = np.split(r.peaks, np.flatnonzero(np.diff(locs) > 1) + 1) if len(locs) else []
    r.pick_tie = False
    picks = []
    for c, pk in enumerate(r.chains):
        take = 1 if c in (0, len(r.chains) - 1) else 2
        h = r.smooth[pk]
        o = np.argsort(h) if ties == "numpy" else np.argsort(h, kind="stable")
        picks += edges[pk[o[-take:]]].tolist()
        hs = np.sort(h)
        if len(hs) > take and hs[-take] == hs[-take - 1]:
            r.pick_tie = True
    r.picks = np.sort(np.array(picks, np.float64))
    adj = []
    for a, b in zip(r.picks[:-1], r.picks[1:]):
        adj.append(a)
        if b - a >= 2.5:
            adj.append(b - 0.2)
    adj += r.picks[-1:].tolist()
    slabs = [[a, b] for a, b in zip(adj[:-1], adj[1:])] or [[edges[0], edges[-1]]]
    slabs[0][0] = (slabs[0][0] + ymin) / 2
    slabs[-1][1] = ymax
    r.slabs = np.array(slabs, np.float64)
    return r


def histogram(y):
    """graph.py:640-642 -> counts, ymin, ymax"""
    y = np.asarray(y, np.float64)
    ymin, ymax = np.min(y), np.max(y)
    bins = int(np.abs(ymax - ymin) / 0.01)
    counts, edges = np.histogram(y, bins=bins)
    assert np.array_equal(edges, np.linspace(ymin, ymax, bins + 1))
    return counts.astype(np.int64), float(ymin), float(ymax)


def crops(points, slabs):
    """graph.py:769-787 -> list of dicts like Scene.segment_floors'"""
    y = points[:, 1]
    out = []
    for lo, hi in slabs:
        sel = points[(y >= lo) & (y <= hi)]
        zero = float(sel[:, 1].min()) if len(sel) else float(lo)
        out.append(dict(y_lo=float(lo), y_hi=float(hi), n_points=len(sel), zero_level=zero, height=float(hi - zero),
                        bbox_min=sel.min(0) if len(sel) else np.zeros(3), bbox_max=sel.max(0) if len(sel) else np.zeros(3)))
    return out


def reference_floors(points, ties="library"):
    """the whole answer for a cloud that its 5 cm re-sampling leaves as it is -> (floors, Ref)"""
    r = reference(*histogram(points[:, 1]), ties=ties)
    return crops(points, r.slabs), r


# ------------------------------------------------------------------------------------------------ exact family
def one_per_voxel(points):
    keys, _ = O.o3d_voxel_keys(np.asarray(points, np.float64), 0.05)
    return len(np.unique(keys, axis=0)) == len(points)


def columns(ys, seed, x0=-3.0, z0=1.0):
    """a cloud with the heights ys, every point in an (x, z) column of its own 10 cm from the next, in shuffled order"""
    ys = np.asarray(ys, np.float64)
    n = len(ys)
    assert 2 <= n <= MAX_POINTS
    side = int(np.ceil(np.sqrt(n)))
    k = np.random.default_rng(seed).permutation(n)
    pts = np.stack([x0 + (k % side) * 0.1, ys, z0 + (k // side) * 0.1], axis=1)
    assert one_per_voxel(pts)
    return np.ascontiguousarray(pts)


def edge_of(j, lo, hi):
    """the lower edge of bin j as np.linspace (and k_fl_hist) compute it"""
    bins = int(np.abs(hi - lo) / 0.01)
    step = (hi - lo) / bins
    return j * step + lo


def heights(seed, n, lo, hi, levels, sigma, wall=0.0, on_edges=(), extra=(), n_top=2):
    """n heights between lo and hi (both taken, hi n_top times: ymax belongs to the last bin): `levels` with n_level points each
    (normal(level, sigma) clipped into the range; sigma 0: the level itself), a share `wall` of uniform ones, three heights for
    every j of on_edges (edge j of the histogram, the double below it and the double above it) and `extra` as given"""
    rng = np.random.default_rng(seed)
    bins = int(np.abs(hi - lo) / 0.01)
    ys = [lo] + [hi] * n_top + list(extra)
    for j in on_edges:
        assert 0 < j < bins
        e = edge_of(j, lo, hi)
        ys += [e, np.nextafter(e, -np.inf), np.nextafter(e, np.inf)]
    m = n - len(ys)
    assert m >= 0
    n_wall = int(m * wall)
    per = (m - n_wall) // max(len(levels), 1)
    for L in levels:
        ys += np.clip(rng.normal(L, sigma, per), lo, hi).tolist() if sigma else [float(L)] * per
    ys += rng.uniform(lo, hi, n - len(ys)).tolist()
    ys = np.array(ys, np.float64)
    assert len(ys) == n and ys.min() == lo and ys.max() == hi
    return ys


class Case:
    def __init__(self, name, points):
        self.name, self.points = name, np.ascontiguousarray(points, np.float64)
        assert self.points.ndim == 2 and 2 <= len(self.points) <= MAX_POINTS, name

    def __repr__(self):
        return self.name


def _size_case(n):
    """two storeys and a few bin edges; cloud sizes around the 64 lanes of a wave and the 256 threads of a workgroup"""
    lo, hi = 0.13, 2.37
    if n == 2:
        return Case("size_2", columns([lo, hi], 2))
    ys = heights(100 + n, n, lo, hi, [0.52, 1.93], 0.005, on_edges=(39, 40, 180), extra=(0.52, 1.93))
    return Case("size_%d" % n, columns(ys, n))


SIZES = (2, 63, 64, 65, 255, 256, 257)
EDGE_LEVELS_RANGE = (0.13, 4.91)
EXACT_NAMES = tuple("size_%d" % n for n in SIZES) + ("one_bin", "tall_20000", "across_zero", "all_negative", "empty_slab", "twin_levels",
                                                      "five_equals", "ceiling_at_ymax", "peak_at_percentile", "levels_on_edges")


@functools.lru_cache(None)
def exact_cases():
    out = [_size_case(n) for n in SIZES]
    # one bin: a map 1.37 cm high (np.histogram with bins = 1, a filter longer than its input, the fallback slab)
    out.append(Case("one_bin", columns([0.3, 0.3 + 0.0137], 3)))
    # about 20 000 points, three storeys with walls, EVERY bin edge with its two neighbours
    lo, hi = 0.07, 7.52
    bins = int(np.abs(hi - lo) / 0.01)
    ys = heights(1, 20011, lo, hi, [0.61, 3.43, 6.38], 0.03, wall=0.2, on_edges=range(1, bins), n_top=5)
    out.append(Case("tall_20000", columns(ys, 4)))
    # heights across zero, with both zeros
    lo, hi = -1.31, 2.94
    bins = int(np.abs(hi - lo) / 0.01)
    ys = heights(2, 6000, lo, hi, [-0.9, 0.0, 1.6], 0.02, wall=0.15, on_edges=range(1, bins), extra=(-0.0, 0.0, -0.0, 5e-324, -5e-324))
    assert np.signbit(ys).any() and (ys == 0).sum() >= 3
    out.append(Case("across_zero", columns(ys, 5)))
    # all heights negative
    lo, hi = -7.43, -0.21
    bins = int(np.abs(hi - lo) / 0.01)
    ys = heights(3, 5000, lo, hi, [-6.9, -3.8, -1.0], 0.03, wall=0.1, on_edges=range(1, bins, 3))
    out.append(Case("all_negative", columns(ys, 6, x0=-40.0, z0=-17.0)))
    # no walls, levels as single heights 3.1 m apart: each pick gets a ceiling 0.2 m under it, and the slab between that ceiling and
    # the pick -- the pick is the LOWER edge of the level's bin, the level lies inside the bin -- holds no point
    lo, hi = 0.0, 7.2
    ys = heights(4, 1503, lo, hi, [0.505, 3.605, 6.705], 0.0)
    out.append(Case("empty_slab", columns(ys, 7)))
    # two levels of equally many points 15 bins apart (and a third storey): equal smoothed peaks closer than find_peaks' distance
    lo, hi = 0.0, 4.0
    ys = heights(5, 1204, lo, hi, [1.005, 1.155, 3.005], 0.0, n_top=3)
    out.append(Case("twin_levels", columns(ys, 8)))
    # a chain of five equally high peaks 0.3 m apart between two storeys further off: the middle chain keeps two of five equals
    lo, hi = 0.0, 8.0
    ys = heights(6, 2104, lo, hi, [0.805, 2.505, 2.805, 3.105, 3.405, 3.705, 6.005], 0.0, n_top=3)
    out.append(Case("five_equals", columns(ys, 9)))
    # a ceiling AT ymax: 400 points in the last bin because its upper edge belongs to it.  They bury the level four bins below (no
    # peak there: the smoothed counts rise to the end); without them that level would be a peak and another storey
    lo, hi = 0.0, 5.0
    ys = heights(7, 1201, lo, hi, [0.505, 2.505, hi - 0.045], 0.0, n_top=400)
    out.append(Case("ceiling_at_ymax", columns(ys, 10)))
    # 311 bins, so np.percentile(.., 90) is EXACTLY the 280th smallest smoothed count (virtual index 310 * 0.9 = 279.0; the
    # algebraically equal 311 * 0.9 + 0.1 - 1 is 279.00000000000006 and interpolates a hair upwards).  Three large levels hold the 31
    # counts above it, and a small level on its own chain peaks exactly AT it: find_peaks keeps it, and it is the lower pick
    lo, hi = 0.0, 3.115
    step = (hi - lo) / 311
    ys = np.concatenate([[lo, hi, hi]] + [np.full(n, (j + 0.5) * step) for j, n in ((30, 26), (140, 1000), (200, 1010), (260, 400))])
    out.append(Case("peak_at_percentile", columns(ys, 11)))
    # whole levels ON bin edges, so that the bin of an edge point decides a slab edge: 300 points at exactly edge 209 (they belong to
    # bin 209; floor((v - lo) / step) alone says 208) and 300 at the double below edge 330 (bin 329; the same expression says 330),
    # between a level inside bin 60 and one inside bin 445.  Four chains of one peak: the slabs meet at edge 209 and at edge 329
    lo, hi = EDGE_LEVELS_RANGE
    step = (hi - lo) / int(np.abs(hi - lo) / 0.01)
    on, under = edge_of(209, lo, hi), np.nextafter(edge_of(330, lo, hi), -np.inf)
    assert np.floor((on - lo) / step) == 208 and np.floor((under - lo) / step) == 330
    ys = heights(8, 1203, lo, hi, [60.5 * step + lo, on, under, 445.5 * step + lo], 0.0)
    out.append(Case("levels_on_edges", columns(ys, 12)))
    assert tuple(c.name for c in out) == EXACT_NAMES
    return out


# ------------------------------------------------------------------------------------------------ general family
def storeys(seed, levels, sigma, per_level, wall=0, side=1.5):
    """levels of per_level points each over a side x side square (many per 5 cm voxel), normal(level, sigma) in height, and `wall`
    points uniform in height along one side"""
    rng = np.random.default_rng(seed)
    parts = []
    for L in levels:
        p = np.empty((per_level, 3))
        p[:, 0], p[:, 2] = rng.uniform(0, side, per_level), rng.uniform(0, side, per_level)
        p[:, 1] = rng.normal(L, sigma, per_level) if sigma else L
        parts.append(p)
    if wall:
        w = np.empty((wall, 3))
        w[:, 0], w[:, 2] = rng.uniform(0, 0.04, wall), rng.uniform(0, side, wall)
        w[:, 1] = rng.uniform(min(levels) - 0.1, max(levels) + 0.1, wall)
        parts.append(w)
    pts = np.concatenate(parts)
    return np.ascontiguousarray(pts[rng.permutation(len(pts))])


REPRO_LEVELS = (0.608, 1.523, 2.110, 4.935, 5.709, 6.416, 7.318)

# the reproduction: seven levels of 1627 points, sigma 0.03, one wall.  Seeds chosen on the CPU (general_analysis): every one has two
# equally high peaks in a chain that may keep only one of them; with the first, numpy 2.2.6's default argsort on an AVX-512 CPU picks
# the other one (smoothed heights [123, 125, 125 | 124, 124, 118, 123]: np.argsort([124, 124, 118, 123]) = [2 3 1 0])
REPRO_SEEDS = (87, 2, 16)


def _levels(seed, n):
    rng = np.random.default_rng(9000 + seed)
    return np.round(np.cumsum(rng.uniform(0.45, 1.6, n)), 3).tolist()


def _general_specs():
    """(name, seed, levels, sigma, points per level, wall points)"""
    specs = []
    for seed in REPRO_SEEDS:
        specs.append(("repro_%d" % seed, seed, REPRO_LEVELS, 0.03, 1627, 1200))
    k = 0
    for n in (2, 3, 4, 5, 6, 7):
        for sigma in (0.0, 0.005, 0.03):
            specs.append(("storeys_%d_s%g" % (n, sigma), 300 + k, _levels(k, n), sigma, 1500, 400 + 100 * (k % 4) if k % 3 else 0))
            k += 1
    specs.append(("twenty_levels", 41, [0.4 + 0.3 * i for i in range(20)], 0.005, 1200, 800))
    specs.append(("levels_1p5_apart", 42, [0.5 + 1.5 * i for i in range(6)], 0.03, 1500, 500))
    return specs


GENERAL_NAMES = tuple(s[0] for s in _general_specs())


@functools.lru_cache(None)
def general_cases():
    out = []
    for name, seed, levels, sigma, per, wall in _general_specs():
        c = Case(name, storeys(seed, levels, sigma, per, wall))
        assert not one_per_voxel(c.points), name
        out.append(c)
    return out


@functools.lru_cache(None)
def general_analysis(name):
    """`reference` (both tie modes) on the oracle's re-sampling of a general case"""
    c = {c.name: c for c in general_cases()}[name]
    down = O.o3d_voxel_down_sample(c.points, None, 0.05)[0]
    h = histogram(down[:, 1])
    return reference(*h), reference(*h, ties="numpy")
