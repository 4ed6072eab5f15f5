"""hmsg_kmeans_batch (include/hmsg.h; holoagent_amd/csrc/hmsg_kmeans_device.hip) against hmsg_kmeans called once per set: labels,
centres, inertia and n_iter BIT FOR BIT, and one Lloyd iteration from given centres (hmsg_test_kmeans_lloyd) device against host.
hmsg_kmeans itself is held to scikit-learn by tests/test_kmeans_cabi.py; the simulator runs here check the labels against
scikit-learn once more.

Every check runs once on the kernel simulator and once on the GPU.  The shapes are the smallest that take a distinct branch:

  (24, 16, 24)     n == k, every point a centre                      (6, 16, 5)       what the small graph scenes produce
  (70, 13, 5)      D a multiple of neither 4 nor 8 (both tails), k < 8 in the pairwise sum
  (257, 200, 24)   crosses the 256-row chunk; D > 128: the pairwise sum's recursion with its n2 -= n2 % 8 split
  (300, 512, 24)   the workload's D and k                            (600, 64, 5)     X[::3] = X[0]: repeated rows
  (300, 64, 24) with max_iter = 2: stops unconverged, the extra E-step runs"""
import os
import warnings

import numpy as np
import pytest

from tests import parity_common as PC

needs_emu = pytest.mark.skipif(not os.path.exists(PC.EMU_PATH), reason="kernel simulator not built")
HMSG_ERR_INVALID = -1


def make(kind, n, D, seed):
    """the three kinds of tests/test_kmeans_cabi.py::_cases: (a) normal, (b) unit rows around a few directions, (c) repeated rows"""
    rng = np.random.default_rng(seed)
    if kind == "a":
        X = rng.standard_normal((n, D))
    elif kind == "b":
        c = rng.standard_normal((7, D))
        X = c[rng.integers(0, 7, n)] + 0.3 * rng.standard_normal((n, D))
        X /= np.linalg.norm(X, axis=1, keepdims=True)
    else:
        X = rng.standard_normal((n, D))
        X[::3] = X[0]
    return np.ascontiguousarray(X, np.float32)


#        n,   D,  k, kind, max_iter, no cluster may be empty
CASES = ((24, 16, 24, "a", 100, True),
         (6, 16, 5, "b", 100, False),
         (70, 13, 5, "a", 100, False),
         (257, 200, 24, "b", 100, False),
         (300, 512, 24, "b", 100, True),
         (600, 64, 5, "c", 100, False),
         (300, 64, 24, "a", 2, False))

_REF = {}


def reference(k_case):
    """hmsg_kmeans on the case (host code: computed once, shared by the simulator and the GPU run)"""
    if k_case not in _REF:
        from holoagent_amd._lib import HmsgLib, kmeans
        n, D, k, kind, max_iter, _ = CASES[k_case]
        X = make(kind, n, D, 100 + k_case)
        L = HmsgLib(PC.EMU_PATH if os.path.exists(PC.EMU_PATH) else None)
        _REF[k_case] = (X, kmeans(X, k, max_iter=max_iter, lib_=L))
    return _REF[k_case]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_same_fit(got, want, what):
    assert np.array_equal(np.asarray(got[0]), np.asarray(want[0])), ("labels", what)
    assert np.array_equal(bits(got[1]), bits(want[1])), ("centres", what)
    assert np.array_equal(bits(np.float32(got[2])), bits(np.float32(want[2]))), ("inertia", what, got[2], want[2])
    assert got[3] == want[3], ("n_iter", what, got[3], want[3])


def check_case(L, k_case, simulator):
    from holoagent_amd._lib import kmeans_batch
    n, D, k, kind, max_iter, full = CASES[k_case]
    X, want = reference(k_case)
    if full:                                   # (the case is there for the path WITHOUT an empty cluster: it must not pass by another)
        assert len(np.unique(want[0])) == k
    if max_iter == 2:
        assert want[3] == 2                    # stopped by max_iter: the extra E-step ran
    got = kmeans_batch([X], k, max_iter=max_iter, lib_=L)[0]
    print("case %s: n_iter %d inertia %r" % (CASES[k_case][:3], got[3], got[2]))
    assert_same_fit(got, want, CASES[k_case])
    if simulator:
        from sklearn.cluster import KMeans
        from threadpoolctl import threadpool_limits
        with threadpool_limits(limits=1), warnings.catch_warnings():
            warnings.simplefilter("ignore")
            km = KMeans(n_clusters=k, max_iter=max_iter, n_init=5, random_state=0).fit(X)
        assert np.array_equal(got[0], km.labels_)


@needs_emu
@pytest.mark.parametrize("k_case", range(len(CASES)))
def test_cases_on_the_simulator(k_case):
    from holoagent_amd._lib import HmsgLib
    check_case(HmsgLib(PC.EMU_PATH), k_case, True)


@pytest.mark.gpu
@pytest.mark.parametrize("k_case", range(len(CASES)))
def test_cases_gpu(k_case):
    from holoagent_amd._lib import HmsgLib
    check_case(HmsgLib(), k_case, False)


# ---- one batched call
BATCH_SIZES = (5, 6, 70, 257, 600)


def check_batch(L):
    from holoagent_amd._lib import kmeans, kmeans_batch
    sets = [make("abc"[i % 3], n, 64, 300 + i) for i, n in enumerate(BATCH_SIZES)]
    a = kmeans_batch(sets, 5, lib_=L)
    b = kmeans_batch(sets, 5, lib_=L)
    for i, X in enumerate(sets):
        assert_same_fit(a[i], kmeans(X, 5, lib_=L), ("host", i))
        assert_same_fit(a[i], kmeans_batch([X], 5, lib_=L)[0], ("alone", i))
        assert_same_fit(a[i], b[i], ("again", i))


@needs_emu
def test_batch_on_the_simulator():
    from holoagent_amd._lib import HmsgLib
    check_batch(HmsgLib(PC.EMU_PATH))


@pytest.mark.gpu
def test_batch_gpu():
    from holoagent_amd._lib import HmsgLib
    check_batch(HmsgLib())


# ---- one Lloyd step from given centres
def lloyd(L, on_device, X, C):
    n, D = X.shape
    k = len(C)
    labels, out, shift = np.full(n, -9, np.int32), np.full((k, D), 7.0, np.float32), np.full(k, 7.0, np.float32)
    rc = L.c.hmsg_test_kmeans_lloyd(int(on_device), 0, X.ctypes.data, n, D, k, C.ctypes.data, labels.ctypes.data, out.ctypes.data,
                                    shift.ctypes.data)
    assert rc == 0
    return labels, out, shift


def e_step(X, C):
    """labels of the E-step in float64 (the tests below only use them where they are the host's)"""
    X64, C64 = X.astype(np.float64), C.astype(np.float64)
    return np.argmin((C64 * C64).sum(1)[None, :] - 2.0 * X64 @ C64.T, axis=1)


def lloyd_inputs():
    """-> [(what, X, centres, least number of empty clusters)]"""
    rng = np.random.default_rng(11)
    out = []
    # one centre far from all data: one empty cluster, a non-zero farthest distance
    X = make("a", 150, 32, 1)
    C = X[rng.choice(150, 6, replace=False)].copy()
    C[3] = 1e3
    out.append(("one far centre", X, C, 1))
    # three far centres, the two farthest rows duplicated: several empties and a tie in the stable order
    X = make("a", 150, 32, 2)
    C = X[rng.choice(150, 7, replace=False)].copy()
    C[[1, 4, 6]] = np.array([[1e3], [-1e3], [2e3]], np.float32)
    out.append(("three far centres", X, C, 3))
    # all rows identical: dmax == 0, no relocation, the empty clusters copy the heaviest centre
    X = np.ascontiguousarray(np.repeat(make("a", 1, 32, 3), 40, axis=0))
    C = np.ascontiguousarray(np.stack([X[0], X[0] + 1.0, X[0] - 2.0, X[0] + 3.0]).astype(np.float32))
    out.append(("identical rows", X, C, 1))
    # D = 13 and D = 200: the tails of the shift's four-terms-per-step distance
    for D in (13, 200):
        X = make("b", 90, D, 4 + D)
        out.append(("D = %d" % D, X, X[rng.choice(90, 5, replace=False)].copy() + np.float32(0.01), 0))
    return out


def check_lloyd(L):
    for what, X, C, min_empty in lloyd_inputs():
        if what == "three far centres":
            # the two farthest rows (by the host's own distances to their centres), each twice
            lab = e_step(X, C)
            d = ((X - C[lab]) ** 2).sum(axis=1)
            far = np.argsort(-d, kind="stable")[:2]
            X = np.ascontiguousarray(np.concatenate([X, X[far]]))
        C = np.ascontiguousarray(C, np.float32)
        h = lloyd(L, 0, X, C)
        d = lloyd(L, 1, X, C)
        k = len(C)
        empty = [j for j in range(k) if not (h[0] == j).any()]
        print("%s: empty clusters %s" % (what, empty))
        assert len(empty) >= min_empty, what
        assert np.array_equal(d[0], h[0]), ("labels", what)
        assert np.array_equal(bits(d[1]), bits(h[1])), ("centres", what)
        assert np.array_equal(bits(d[2]), bits(h[2])), ("shift", what)
        if what == "one far centre":
            # the relocated centre is the farthest row, and its old cluster's sum lost that row
            assert empty == [3]
            dist = ((X - C[h[0]]) ** 2).sum(axis=1)
            far = int(np.argmax(dist))
            assert np.array_equal(bits(d[1][3]), bits(X[far]))
            old = int(h[0][far])
            rest = [i for i in np.flatnonzero(h[0] == old) if i != far]
            np.testing.assert_allclose(d[1][old], X[rest].astype(np.float64).mean(axis=0), rtol=0, atol=1e-5)
        if what == "identical rows":
            heavy = int(h[0][0])
            assert (h[0] == heavy).all()
            for j in empty:
                assert np.array_equal(bits(d[1][j]), bits(d[1][heavy]))


@needs_emu
def test_lloyd_step_on_the_simulator():
    from holoagent_amd._lib import HmsgLib
    check_lloyd(HmsgLib(PC.EMU_PATH))


@pytest.mark.gpu
def test_lloyd_step_gpu():
    from holoagent_amd._lib import HmsgLib
    check_lloyd(HmsgLib())


# ---- errors
def check_errors(L):
    X = make("a", 5 + 3 + 9, 16, 9)
    off = np.array([0, 5, 8, 17], np.int64)                      # the middle set has 3 rows: fewer than k = 5
    labels, centers = np.full(17, -7, np.int32), np.full((3, 5, 16), 7.0, np.float32)
    inertia, n_iter = np.full(3, 7.0, np.float32), np.full(3, -7, np.int32)
    rc = L.c.hmsg_kmeans_batch(0, 3, off.ctypes.data, X.ctypes.data, 16, 5, 5, 100, 0, labels.ctypes.data, centers.ctypes.data,
                               inertia.ctypes.data, n_iter.ctypes.data)
    assert rc == HMSG_ERR_INVALID
    assert (labels == -7).all() and (centers == 7.0).all() and (inertia == 7.0).all() and (n_iter == -7).all()
    off = np.array([0, 5, 5, 17], np.int64)                      # an empty set
    assert L.c.hmsg_kmeans_batch(0, 3, off.ctypes.data, X.ctypes.data, 16, 5, 5, 100, 0, labels.ctypes.data, centers.ctypes.data, None,
                                 None) == HMSG_ERR_INVALID
    assert (labels == -7).all() and (centers == 7.0).all()
    assert L.c.hmsg_kmeans_batch(0, 0, None, None, 16, 5, 5, 100, 0, None, None, None, None) == 0


@needs_emu
def test_errors_on_the_simulator():
    from holoagent_amd._lib import HmsgLib
    check_errors(HmsgLib(PC.EMU_PATH))


@pytest.mark.gpu
def test_errors_gpu():
    from holoagent_amd._lib import HmsgLib
    check_errors(HmsgLib())


# ---- GPU only
@pytest.mark.gpu
def test_device_tensors_give_the_same_bits_gpu():
    import torch
    from holoagent_amd._lib import HmsgLib, kmeans_batch
    L = HmsgLib()
    sets = [make("b", 257, 64, 41), make("a", 70, 64, 42)]
    host = kmeans_batch(sets, 5, lib_=L)
    dev = kmeans_batch([torch.from_numpy(x).to("cuda:0") for x in sets], 5, lib_=L)
    for h, d in zip(host, dev):
        assert d[0].is_cuda and d[1].is_cuda
        assert_same_fit((d[0].cpu().numpy(), d[1].cpu().numpy(), d[2], d[3]), h, "device tensors")


@pytest.mark.gpu
def test_more_rows_than_one_workgroup_gpu():
    from holoagent_amd._lib import HmsgLib, kmeans, kmeans_batch
    L = HmsgLib()
    X = make("b", 3000, 64, 43)
    assert_same_fit(kmeans_batch([X], 24, lib_=L)[0], kmeans(X, 24, lib_=L), "3000 x 64")
