"""The batched cosine DBSCAN (k_pool_gram / k_rn_gram_f64 -> pool_cluster -> k_pool_mean / k_rn_mean_f64) against the exact integer
reference of tests/dbscan_cases.py, through hmsg_denoise_feats_batch (eps and min_samples are arguments) in float32 and float64,
and the pooling front (valid scan -> row offsets -> gather with nan_to_num) through the hmsg_test_pool_rows hook.

n_in_cluster is compared exactly and the representative bit for bit.  Every builder asserts that the float64 adjacency of its
rows is the integer model's and that no distance lies within 4 tau of eps (dbscan_cases.check_margin); no case is left out.

  shape sweep   n on the edges of the 32 / 64 / 128-row tiles and of gram_tile_of's super-tiles (1024 / 1025, 2049, 3000), D on the
                staging paths of k_pool_gram (D % 4 != 0, D % 32 == 4, D < 32), min_samples 2 .. 100, eps 0.02 .. 1e-4
  structure     a border row between two clusters; equal largest clusters ordered by a border row; 40+ clusters; a 400-hop chain
                permuted, in position order and reversed
  knife edge    links exactly ON eps = 2^-6 (exact arithmetic in any order); one float32 ulp lower there is no cluster
  batch         300 sets, again in another order at a non-zero set_off[0], and under HMSG_DEBUG_POOL_ALL_ROWS=1 in a child process
  pooling front instances without a valid row (first, last, three in a row), NaN / +-inf in the table, one voxel repeated, the
                defaults eps 0.01 / min 100

The simulator twins take the cases up to about 1100 rows (HMSG_EMU_SLOW=1: all of them); -m gpu takes every case and one batch of
about 1e5 rows with a 6000-row set at D = 512."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import dbscan_cases as DC
from tests import parity_common as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
needs_emu = pytest.mark.skipif(not os.path.exists(PC.EMU_PATH), reason="kernel simulator not built")
EMU_SLOW = bool(os.environ.get("HMSG_EMU_SLOW"))
DTYPES = (np.float32, np.float64)

NS = (1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 257, 1023, 1024, 1025, 2049, 3000)
DS = (2, 3, 5, 16, 30, 36, 48, 64, 100, 512, 1024)
MIN_SAMPLES = (2, 3, 5, 8, 20, 100)
EPS = (0.02, 0.01, 1e-3, 1e-4)


def eps_allowed(D):
    """the margin rule (margin ~ 2 eps / (2m + 1) against 4 tau = 4 (D + 8) 2^-24): eps 1e-4 up to D = 36, 1e-3 up to 512"""
    return EPS if D <= 36 else EPS[:3] if D <= 512 else EPS[:2]


def gap_weights(min_samples):
    """more duplicates for a larger min_samples, so that cores exist where the set is large enough"""
    if min_samples >= 100:
        return (0.955, 0.02, 0.01, 0.005, 0.005, 0.005)
    if min_samples >= 20:
        return (0.82, 0.08, 0.04, 0.03, 0.02, 0.01)
    if min_samples >= 5:
        return (0.45, 0.2, 0.15, 0.1, 0.05, 0.05)
    return (0.2, 0.2, 0.2, 0.2, 0.1, 0.1)


def sweep():
    """every n with three D, every D with at least four n; eps and min_samples cycle.  (n, D, eps, m, min_samples, seed)"""
    out = []
    for i, n in enumerate(NS):
        for j in range(3):
            D = DS[(4 * i + 5 * j + i // 11) % len(DS)]
            allowed = eps_allowed(D)
            eps = allowed[(i + 2 * j) % len(allowed)]
            out.append((n, D, eps, 4 if D == 512 and eps >= 0.01 else 3, MIN_SAMPLES[(i + j) % len(MIN_SAMPLES)], 1000 + 3 * i + j))
    return out


SWEEP = sweep()


def on_simulator(n, D):
    return EMU_SLOW or (n <= 1100 and n * n * D <= 1100 * 1100 * 64)


def raw_batch(L, X, off, eps, min_samples):
    """hmsg_denoise_feats_batch as a C host calls it: X all rows, off the sets' row offsets (off[0] may be > 0)"""
    X, off = np.ascontiguousarray(X), np.ascontiguousarray(off, np.int64)
    K, D = len(off) - 1, X.shape[1]
    out, ncl = np.zeros((K, D), X.dtype), np.full(K, -7, np.int32)
    rc = L.c.hmsg_denoise_feats_batch(0, K, off.ctypes.data, X.ctypes.data, int(X.dtype == np.float64), D, float(eps), int(min_samples),
                                      out.ctypes.data, ncl.ctypes.data)
    assert rc == 0
    return out, ncl


def assert_exact(got_rep, got_ncl, case, min_samples, what):
    e = case.expect(min_samples)
    print("%s: n %d D %d %s eps %g min %d ratio %.1f -> clusters %d, n_in_cluster %d (got %d)"
          % (what, len(case.X), case.X.shape[1], case.dtype, case.eps, min_samples, case.ratio, e.n_clusters, e.n_in_cluster, got_ncl))
    assert got_rep.dtype == case.X.dtype
    assert int(got_ncl) == e.n_in_cluster, what
    assert np.array_equal(DC.bits(got_rep), DC.bits(e.rep)), what
    return e


def run_one(L, case, min_samples, what=""):
    rep, ncl = raw_batch(L, case.X, [0, len(case.X)], case.eps, min_samples)
    return assert_exact(rep[0], ncl[0], case, min_samples, what)


# ---- shape sweep
def check_sweep(L, k, simulator):
    n, D, eps, m, ms, seed = SWEEP[k]
    if simulator and not on_simulator(n, D):
        return 0
    for dt in DTYPES:
        c = DC.lattice(seed, n, D, eps, m, dt, weights=gap_weights(ms), n_zero=(k % 4 == 1) * 2, antipodal=(k % 3 == 0))
        run_one(L, c, ms, "sweep %d" % k)
    return 1


def test_sweep_covers_the_issue():
    assert {c[0] for c in SWEEP} == set(NS) and {c[1] for c in SWEEP} == set(DS)
    assert {c[2] for c in SWEEP} == set(EPS) and {c[4] for c in SWEEP} == set(MIN_SAMPLES)
    sim = [c for c in SWEEP if c[0] <= 1100 and c[0] * c[0] * c[1] <= 1100 * 1100 * 64]
    assert {c[0] for c in sim} >= set(NS[:16]) and {c[1] for c in sim} == set(DS)          # the default simulator share
    assert any(c[1] % 4 != 0 for c in sim) and any(c[1] % 32 == 4 and c[1] > 32 for c in sim)
    # structure across the sweep, by the integer model: borders, noise, all-noise sets, min_samples above every neighbourhood
    borders = noise_only = 0
    for (n, D, eps, m, ms, seed) in SWEEP:
        if n <= 300:
            s = DC.structure(DC.lattice(seed, n, D, eps, m, np.float64, weights=gap_weights(ms)), ms)
            borders += s["borders"] > 0
            noise_only += s["clusters"] == 0
    assert borders >= 5 and noise_only >= 3


def test_reference_agrees_with_sklearn():
    """the labels of the integer reference are sklearn's own (where scikit-learn is installed); the reference stays what is asserted"""
    try:
        from sklearn.cluster import DBSCAN
    except Exception:
        return
    cases = [(DC.lattice(seed, n, D, eps, m, dt, weights=gap_weights(ms), n_zero=1, antipodal=True), ms)
             for (n, D, eps, m, ms, seed) in SWEEP if 2 <= n <= 300 and D <= 100 for dt in DTYPES]
    cases += [(DC.knife_edge(5, 40, 30, dt, n_dup=4), ms) for dt in DTYPES for ms in (2, 3)]
    cases += [(c, ms) for c, ms, _ in structure_cases(np.float64) if len(c.X) < 400]
    for c, ms in cases:
        lab = DBSCAN(eps=DC.eps_as_seen(c.eps, c.dtype), min_samples=ms, metric="cosine").fit(c.X).labels_
        assert np.array_equal(lab, c.expect(ms).labels)


@needs_emu
@pytest.mark.parametrize("k", range(len(SWEEP)))
def test_sweep_on_the_simulator(k):
    from holoagent_amd._lib import HmsgLib
    check_sweep(HmsgLib(PC.EMU_PATH), k, True)


@pytest.mark.gpu
def test_sweep_gpu():
    from holoagent_amd._lib import HmsgLib
    L = HmsgLib()
    assert sum(check_sweep(L, k, False) for k in range(len(SWEEP))) == len(SWEEP)


# ---- structure
def structure_cases(dt):
    """-> [(case, min_samples, what)], every one asserted to contain what it is there for"""
    out = []
    rng = np.random.default_rng(77)
    A, B = [0, 0, 1, 1, 2], [8, 8, 9, 9, 10]
    # a border row (position 5) adjacent to cores of two clusters (2 and 8; m = 3, min_samples 5): it decides which is larger
    for tag, pos in (("A first", A + [5] + B), ("B first", B + [5] + A), ("border first", [5] + B + A)):
        c = DC.lattice_from_model(rng, [0] * 11 + [1] * 4, pos + [0, 4, 8, 12], 16, 0.01, 3, dt)
        s = DC.structure(c, 5)
        assert s["clusters"] == 2 and s["borders_between"] == 1 and s["border_decides_size"] and s["noise"] == 4
        out.append((c, 5, "border between two clusters, " + tag))
    # two largest clusters of equal size; the one that appears first in row order does so with a BORDER row, its cores come later
    Bp = [0, 0, 0, 1, 1, 2]
    for tag, group, pos in (("border row first", [0] + [1] * 6 + [0] * 5, [5] + Bp + A),
                            ("core rows first", [1] * 6 + [0] * 5 + [0], Bp + A + [5])):
        c = DC.lattice_from_model(rng, group, pos, 16, 0.01, 3, dt)
        s = DC.structure(c, 5)
        assert s["clusters"] == 2 and s["top_tie"] and s["borders"] == 1 and s["border_decides_order"] == (tag == "border row first")
        out.append((c, 5, "tie of the two largest clusters, " + tag))
    # 40 and more clusters in one set
    for ms in (2, 3):
        c = DC.lattice(31, 1025, 64, 0.01, 3, dt)
        assert DC.structure(c, ms)["clusters"] >= 40
        out.append((c, ms, "many clusters"))
    # one chain of 400 and more hops (eps 1e-4 on one plane): permuted, in position order (the first-round shortcut's best case) and
    # reversed (its worst)
    _, pmax = DC.lattice_limits(1e-4, 3)
    pos = np.cumsum(rng.choice([1, 2, 3], 700, p=[0.05, 0.1, 0.85]))
    pos = pos[pos <= pmax]
    for order in ("perm", "sorted", "reverse"):
        o = {"perm": rng.permutation(len(pos)), "sorted": np.arange(len(pos)), "reverse": np.arange(len(pos))[::-1]}[order]
        c = DC.lattice_from_model(rng, np.zeros(len(pos), np.int64), pos[o], 16, 1e-4, 3, dt)
        for ms in (2, 3) if order == "perm" else (2,):
            h = DC.hops(c, ms)
            assert h >= 400 and c.expect(ms).n_clusters == 1
            out.append((c, ms, "chain of %d hops, %s" % (h, order)))
    # edge rows inside an ordinary set: all-zero rows, exact duplicates, an antipodal pair; a set of one row; an all-noise set
    c = DC.lattice(41, 200, 30, 0.02, 3, dt, n_zero=3, antipodal=True, weights=gap_weights(5))
    z = np.flatnonzero(~c.X.any(axis=1))
    d = DC.float64_distances(c.X, dt)
    assert len(z) == 3 and (c.adj[z].sum(axis=1) == 1).all() and np.allclose(d[z][:, np.flatnonzero(c.X.any(axis=1))], 1.0)
    same = (c.X[:, None, :] == c.X[None, :, :]).all(axis=2)
    assert same.sum() >= len(c.X) + 10 and (d > 2 - 1e-9).any()          # exact duplicates (the clip-to-0 path) and an antipodal pair
    for ms in (2, 5):
        out.append((c, ms, "zero rows, duplicates, antipodal pair"))
    out.append((DC.lattice(42, 1, 30, 0.02, 3, dt), 2, "one row"))
    c = DC.lattice(43, 90, 36, 0.01, 3, dt)
    assert DC.structure(c, 20)["clusters"] == 0
    out.append((c, 20, "every row noise"))
    return out


def check_structure(L):
    for dt in DTYPES:
        for c, ms, what in structure_cases(dt):
            run_one(L, c, ms, what)


@needs_emu
def test_structure_on_the_simulator():
    from holoagent_amd._lib import HmsgLib
    check_structure(HmsgLib(PC.EMU_PATH))


@pytest.mark.gpu
def test_structure_gpu():
    from holoagent_amd._lib import HmsgLib
    check_structure(HmsgLib())


# ---- the exact knife edge
def check_knife_edge(L, big):
    below = float(np.nextafter(np.float32(DC.KNIFE_EPS), np.float32(0)))
    for dt in DTYPES:
        for chain, noise, dup in ((60, 40, 0), (129, 200, 30) if big else (100, 70, 10)):
            c = DC.knife_edge(chain, chain, noise, dt, n_dup=dup)
            s2, s3 = DC.structure(c, 2), DC.structure(c, 3)
            # every link lies exactly on eps and is a neighbour: one cluster of the whole chain; with min_samples 3 its two ends are
            # border rows (an end with a duplicate is a core row)
            assert s2["clusters"] == 1 and s2["borders"] == 0 and s2["noise"] == noise
            assert s3["clusters"] == 1 and s3["noise"] == noise and (s3["borders"] == 2 if dup == 0 else s3["borders"] <= 2)
            e = run_one(L, c, 2, "knife edge")
            assert e.n_in_cluster == chain + dup
            run_one(L, c, 3, "knife edge, border ends")
            lo = DC.knife_edge(chain, chain, noise, dt, eps=below, n_dup=dup)  # one float32 ulp lower: no link left, only copies pair up
            s = DC.structure(lo, 2)
            assert s["clusters"] == 0 if dup == 0 else s["cores"] <= 2 * dup
            e = run_one(L, lo, 2, "knife edge, eps one ulp lower")
            assert e.n_in_cluster == 0 if dup == 0 else e.n_in_cluster <= dup + 1


@needs_emu
def test_knife_edge_on_the_simulator():
    from holoagent_amd._lib import HmsgLib
    check_knife_edge(HmsgLib(PC.EMU_PATH), EMU_SLOW)


@pytest.mark.gpu
def test_knife_edge_gpu():
    from holoagent_amd._lib import HmsgLib
    check_knife_edge(HmsgLib(), True)


# ---- batches
def batch_sets(dt, sizes, D, eps, m, seed):
    return [DC.lattice(seed + k, int(n), D, eps, m, dt, weights=gap_weights(5), n_zero=int(k % 7 == 0), antipodal=(k % 5 == 0))
            for k, n in enumerate(sizes)]


def pack(sets, order, lead):
    """rows of sets[order] behind `lead` rows that belong to no set -> X, off (off[0] = lead)"""
    D, dt = sets[0].X.shape[1], sets[0].X.dtype
    X = np.concatenate([np.full((lead, D), 3.0, dt)] + [sets[k].X for k in order])
    off = lead + np.concatenate([[0], np.cumsum([len(sets[k].X) for k in order])])
    return np.ascontiguousarray(X), off.astype(np.int64)


def child_main(lib_path, path_in, path_out):
    """(child process) run the batches of path_in and save the answers"""
    import torch  # noqa: F401  (before the library, as tests/conftest.py does)
    from holoagent_amd._lib import HmsgLib
    L = HmsgLib(lib_path or None)
    z = np.load(path_in)
    res = {}
    for tag in ("a", "b"):
        rep, ncl = raw_batch(L, z["X" + tag], z["off" + tag], float(z["eps"]), int(z["ms"]))
        res["rep" + tag], res["ncl" + tag] = rep, ncl
    np.savez(path_out, **res)


def check_batch(L, lib_path, tmp_path, sizes, D=16, eps=0.01, m=3, ms=3):
    rng = np.random.default_rng(5)
    for dt in DTYPES:
        sets = batch_sets(dt, sizes, D, eps, m, 9000)
        want = [c.expect(ms) for c in sets]
        assert sum(e.n_clusters > 1 for e in want) >= 20 and sum(e.n_in_cluster == 0 for e in want) >= 3
        a = np.arange(len(sets))
        b = rng.permutation(len(sets))
        Xa, offa = pack(sets, a, 0)
        Xb, offb = pack(sets, b, 37)                         # another order, and set_off[0] != 0
        for tag, X, off, order in (("a", Xa, offa, a), ("b", Xb, offb, b)):
            rep, ncl = raw_batch(L, X, off, eps, ms)
            for slot, k in enumerate(order):                  # a set's answer does not depend on its neighbours in the batch
                assert int(ncl[slot]) == want[k].n_in_cluster, (tag, k)
                assert np.array_equal(DC.bits(rep[slot]), DC.bits(want[k].rep)), (tag, k)
        # the same under HMSG_DEBUG_POOL_ALL_ROWS=1 (read once per process: a child)
        pin, pout = str(tmp_path / ("in_%s.npz" % np.dtype(dt).name)), str(tmp_path / ("out_%s.npz" % np.dtype(dt).name))
        np.savez(pin, Xa=Xa, offa=offa, Xb=Xb, offb=offb, eps=eps, ms=ms)
        env = dict(os.environ, HMSG_DEBUG_POOL_ALL_ROWS="1", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
        code = "from tests.test_feats_dbscan_exact import child_main; child_main(%r, %r, %r)" % (lib_path, pin, pout)
        subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, check=True, timeout=900)
        z = np.load(pout)
        for tag, order in (("a", a), ("b", b)):
            for slot, k in enumerate(order):
                assert int(z["ncl" + tag][slot]) == want[k].n_in_cluster, ("all rows", tag, k)
                assert np.array_equal(DC.bits(z["rep" + tag][slot]), DC.bits(want[k].rep)), ("all rows", tag, k)


@needs_emu
def test_batch_on_the_simulator(tmp_path):
    from holoagent_amd._lib import HmsgLib
    rng = np.random.default_rng(3)
    sizes = np.maximum(1, (400 ** rng.random(300) if EMU_SLOW else 60 ** rng.random(300)).astype(int))  # 300 sets, most of them small
    sizes[:4] = (1, 400, 2, 129)                                     # (1 .. 400 rows)
    check_batch(HmsgLib(PC.EMU_PATH), PC.EMU_PATH, tmp_path, sizes)


@pytest.mark.gpu
def test_batch_gpu(tmp_path):
    from holoagent_amd._lib import HmsgLib
    sizes = np.random.default_rng(3).integers(1, 401, 300)
    sizes[:4] = (1, 400, 2, 129)
    check_batch(HmsgLib(), "", tmp_path, sizes)


@pytest.mark.gpu
def test_large_batch_exact_gpu():
    """about 1e5 rows at D = 512 in one call, one set of 6000 rows (47 tiles a side: six super-columns of gram_tile_of)"""
    from holoagent_amd._lib import HmsgLib
    L = HmsgLib()
    rng = np.random.default_rng(8)
    sizes = [6000] + [int(v) for v in rng.integers(1500, 2600, 46)]
    assert 9e4 <= sum(sizes) <= 1.3e5
    for dt in DTYPES:
        sets = [DC.lattice(12000 + k, n, 512, 0.01, 4, dt, planes=8 + k % 5, weights=gap_weights((5, 20, 100)[k % 3]), n_zero=k % 2)
                for k, n in enumerate(sizes)]
        X, off = pack(sets, range(len(sets)), 0)
        for ms in (5, 100):
            rep, ncl = raw_batch(L, X, off, 0.01, ms)
            for k, c in enumerate(sets):
                assert_exact(rep[k], ncl[k], c, ms, "large batch set %d" % k)


# ---- the pooling front (hmsg_test_pool_rows)
def pool_rows(L, counts, idx, valid, table, eps, ms):
    counts, idx = np.ascontiguousarray(counts, np.int32), np.ascontiguousarray(idx, np.int32)
    valid, table = np.ascontiguousarray(valid, np.uint8), np.ascontiguousarray(table, np.float32)
    out = np.full((len(counts), table.shape[1]), 7.0, np.float32)
    rc = L.c.hmsg_test_pool_rows(0, len(counts), counts.ctypes.data, idx.ctypes.data, valid.ctypes.data, table.ctypes.data, len(table),
                                 table.shape[1], float(eps), int(ms), out.ctypes.data)
    assert rc == 0
    return out


def pool_case(rng, sets, D, specials=False, repeat=False):
    """instances from lattice sets (None: an instance without a valid row; an int: that many points, none valid): a table holding the
    sets' rows in shuffled places between rows no instance uses, idx / valid with invalid points sprinkled in.
    -> counts, idx, valid, table, [(rows after nan_to_num, adjacency) or None per instance]"""
    rows = [c.X for c in sets if isinstance(c, DC.Case)]
    n_rows = sum(len(r) for r in rows)
    table = rng.standard_normal((n_rows + 50, D)).astype(np.float32)
    place = rng.permutation(len(table))[:n_rows]
    counts, idx, valid, ref, at = [], [], [], [], 0
    for c in sets:
        if not isinstance(c, DC.Case):
            k = int(c or 0)
            counts.append(k)
            idx += list(rng.integers(-1, len(table), k))           # (-1: no voxel found, as k_pool_nn leaves it)
            valid += [0] * k
            ref.append(None)
            continue
        n = len(c.X)
        p = place[at:at + n]
        at += n
        table[p] = c.X
        X, adj = c.X.copy(), c.adj.copy()
        if specials and n >= 8:
            # rows 1 / 2 / 3 of the instance: NaN in every place (-> a zero row), one +inf, one -inf (-> +-max: the norm overflows
            # float32, the normalised row is zero): each is its own neighbour only
            table[p[1]] = np.nan
            table[p[2], 0] = np.inf
            table[p[3], D - 1] = -np.inf
            table[p[4], 1] = np.nan                                  # one NaN entry of an ordinary row -> 0: checked below
            X[[1, 2, 3, 4]] = np.nan_to_num(table[p[[1, 2, 3, 4]]])
            assert not X[1].any() and X[2, 0] == np.finfo(np.float32).max and X[3, D - 1] == -np.finfo(np.float32).max
            for r in (1, 2, 3):
                adj[r, :] = adj[:, r] = False
                adj[r, r] = True
            adj = adj_after_edit(X, adj, 4, c.eps)
            DC.check_margin(X, adj, c.eps, np.float32)
        ii, vv = [], []
        for r in range(n):
            while rng.random() < 0.15:                               # an invalid point in between
                ii.append(int(rng.integers(-1, len(table))))
                vv.append(0)
            ii.append(int(p[r]))
            vv.append(1)
        if repeat:                                                   # one voxel many times: exact duplicates
            ii += [int(p[0])] * 40
            vv += [1] * 40
            X = np.concatenate([X, np.repeat(X[:1], 40, axis=0)])
            src = np.concatenate([np.arange(n), np.zeros(40, np.int64)])
            adj = adj[src][:, src]
        counts.append(len(ii))
        idx += ii
        valid += vv
        ref.append((X, adj))
    return counts, idx, valid, table, ref


def adj_after_edit(X, adj, r, eps):
    """row r lost one entry (NaN -> 0): its relation to the others is recomputed in float64 (check_margin asserts the margin)"""
    d = DC.float64_distances(X, np.float32)
    adj = adj.copy()
    adj[r, :] = adj[:, r] = d[r] <= DC.eps_as_seen(eps, np.float32)
    return adj


def check_pool_rows(L, big):
    rng = np.random.default_rng(21)
    f32 = np.float32
    # instances without a valid row: first, last, three in a row (points without a voxel, and no points at all)
    D, eps, ms = 36, 0.01, 3
    sets = [5, DC.lattice(1, 70, D, eps, 3, f32, weights=gap_weights(5)), 0, 4, None, DC.lattice(2, 129, D, eps, 3, f32, weights=gap_weights(5)),
            DC.lattice(3, 1, D, eps, 3, f32), 3, DC.lattice(4, 33, D, eps, 3, f32, n_zero=1), 0, 6]
    todo = [(sets, D, eps, ms, False, False)]
    # NaN / +inf / -inf in the table; one voxel repeated
    D = 30
    todo.append(([DC.lattice(5, 90, D, eps, 3, f32, weights=gap_weights(5)), DC.lattice(6, 12, D, eps, 3, f32),
                  DC.lattice(7, 200, D, eps, 3, f32, weights=gap_weights(5))], D, eps, 3, True, False))
    todo.append(([DC.lattice(5, 9, D, eps, 3, f32, weights=(0, 0, 0, 0, 0, 1))], D, eps, 3, True, False))      # every row noise: the clamp shows in the mean
    todo.append(([DC.lattice(8, 60, D, eps, 3, f32, weights=gap_weights(5)), None, DC.lattice(9, 100, D, eps, 3, f32)], D, eps, 5, False, True))
    # the defaults eps 0.01, min_samples 100 on a set with cores, borders and noise at that setting
    n = 3000 if big else 1100
    c = DC.lattice(10, n, 16, 0.01, 3, f32, planes=2, weights=(0.93, 0.03, 0.015, 0.01, 0.01, 0.005))
    s = DC.structure(c, 100)
    assert s["cores"] > 100 and s["borders"] > 0 and s["noise"] > 0, s
    todo.append(([None, c, DC.lattice(11, 40, 16, 0.01, 3, f32)], 16, 0.01, 100, False, False))
    for sets, D, eps, ms, specials, repeat in todo:
        counts, idx, valid, table, ref = pool_case(rng, sets, D, specials, repeat)
        out = pool_rows(L, counts, idx, valid, table, eps, ms)
        for k, r in enumerate(ref):
            if r is None:
                assert not out[k].any() and not np.signbit(out[k]).any(), k       # graph.py:479-483: zeros
                continue
            with np.errstate(over="ignore"):
                e = DC.expect(r[0], r[1], ms)
            print("pool_rows instance %d: n %d min %d -> clusters %d, n_in_cluster %d" % (k, len(r[0]), ms, e.n_clusters, e.n_in_cluster))
            assert np.array_equal(DC.bits(out[k]), DC.bits(e.rep)), k


@needs_emu
def test_pool_rows_on_the_simulator():
    from holoagent_amd._lib import HmsgLib
    check_pool_rows(HmsgLib(PC.EMU_PATH), EMU_SLOW)


@pytest.mark.gpu
def test_pool_rows_gpu():
    from holoagent_amd._lib import HmsgLib
    check_pool_rows(HmsgLib(), True)
