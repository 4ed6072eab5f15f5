"""The semantic segmentation score (include/hmsg.h: hmsg_semseg_instance_labels, hmsg_knn_labels, hmsg_semseg_confusion,
hmsg_semseg_metrics; holoagent_amd/csrc/hmsg_semseg.hip) on the kernel simulator; tests/test_semseg_gpu.py runs the same checks on
the library, from host arrays and from torch device tensors.

  * the k-NN vote against scikit-learn's BallTree + np.bincount (knn_interpolation's own calls) on clouds where the test ASSERTS,
    from a k + 1 query, that no query's k-th and (k + 1)-th distance are equal -- there the reference's answer is defined -- and
    against the (d2, index) model of tests/semseg_reference.py; the lattice walk and the scan (HMSG_DEBUG_KNN_BRUTE=1) must agree in
    labels and neighbour lists;
  * exact ties (a lattice with every point twice) against the model alone: BallTree has no rule there;
  * the float32 cosine labels on tables whose best and second-best cosine differ by more than 1e-3 in float64 (asserted): the error
    of a float32 dot product of normalised rows is at most 2 (D + 2) 2^-24, 6.2e-5 for D = 512;
  * the confusion matrix against np.add.at; the metrics to the bit against the reference's own metric.py (tests/golden/
    semseg_metrics.npz, recorded by scripts/gen_semseg_golden.py).
"""
import ctypes as C
import os

import numpy as np
import pytest

from tests import parity_common as PC
from tests import semseg_reference as R
from tests import test_eval_semantics as TS

HMSG_ERR_INVALID = -1
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "semseg_metrics.npz")
KNN_SHAPES = [(4000, 3000, 5, 12), (300, 500, 1, 3), (64, 257, 16, 40), (5, 100, 5, 4)]            # (n, m, k, classes); the last: n == k
LABEL_SHAPES = [(8, 3, 33), (8, 40, 33), (8, 1030, 1), (512, 3, 33), (512, 40, 33), (512, 1030, 1)]  # (D, C, n)
CONF_SHAPES = [(L, m) for L in (1, 40, 1030) for m in (1, 257, 100003)] + [(110, 257), (111, 257)]   # (the LDS form ends at L = 110)


class Hook:
    def __init__(self, L, wrap=None):
        from holoagent_amd._lib import Scene
        self.L, self.wrap = L, wrap or (lambda a: a)
        self.scene = Scene(lib_=L, height=8, width=8, max_frames=1, max_masks=1, feat_dim=16)

    def close(self):
        self.scene.close()

    def knn(self, pts, lab, q, k, brute=False):
        w = self.wrap
        old = os.environ.pop("HMSG_DEBUG_KNN_BRUTE", None)
        if brute:
            os.environ["HMSG_DEBUG_KNN_BRUTE"] = "1"
        try:
            out, nn = self.scene.knn_labels(w(np.ascontiguousarray(pts, np.float64)), w(np.ascontiguousarray(lab, np.int32)),
                                            w(np.ascontiguousarray(q, np.float64)), k, return_index=True)
        finally:
            os.environ.pop("HMSG_DEBUG_KNN_BRUTE", None)
            if old is not None:
                os.environ["HMSG_DEBUG_KNN_BRUTE"] = old
        return out, nn, self.scene.knn_last_phase2()

    def labels(self, emb, text, cl):
        w = self.wrap
        return self.scene.semseg_instance_labels(w(np.ascontiguousarray(emb)), w(np.ascontiguousarray(text, np.float32)),
                                                 w(np.ascontiguousarray(cl, np.int32)))

    def confusion(self, gt, pred, L):
        w = self.wrap
        return self.scene.semseg_confusion(w(np.ascontiguousarray(gt, np.int32)), w(np.ascontiguousarray(pred, np.int32)), L)


# ------------------------------------------------------------------------------------------------ the k-NN vote
def two_boxes(n, m, k, classes, seed):
    """labelled points uniform in two unit boxes 3 m apart; queries in the boxes, in the gap between them and in a margin of 2.5 m
    around everything (the gap and the margin are what the lattice walk gives up on)"""
    rng = np.random.default_rng(seed)
    pts = rng.random((n, 3))
    pts[n // 2:, 0] += 4.0
    lab = rng.integers(0, classes, n).astype(np.int32)
    lab[:min(classes, n)] = np.arange(min(classes, n))                # (every class is there when n allows)
    a = m // 3
    q_box = rng.random((a, 3))
    q_box[:, 0] += 4.0 * rng.integers(0, 2, a)
    q_gap = rng.random((a, 3))
    q_gap[:, 0] = 1.0 + 3.0 * q_gap[:, 0]
    q_out = rng.random((m - 2 * a, 3)) * np.array([10.0, 6.0, 6.0]) - 2.5
    return pts, lab, np.concatenate([q_box, q_gap, q_out])


_sk_cache = {}


def sklearn_case(n, m, k, classes):
    """-> pts, lab, q, sklearn's labels, the model's labels and neighbour lists: computed once per shape"""
    key = (n, m, k, classes)
    if key not in _sk_cache:
        from sklearn.neighbors import BallTree
        pts, lab, q = two_boxes(n, m, k, classes, seed=n + m + k)
        tree = BallTree(pts, metric="minkowski")
        if n > k:                                          # the k-th and (k + 1)-th distance differ for EVERY query (n == k: there is no (k + 1)-th)
            dist = tree.query(q, k=k + 1)[0]
            assert (dist[:, k] > dist[:, k - 1]).all()
        knn_classes = lab[tree.query(q, k=k)[1]].astype(int)
        sk = np.array([np.bincount(row).argmax() for row in knn_classes], np.int32)
        want, nn, _ = R.knn_vote(pts, lab, q, k)
        assert np.array_equal(sk, want)                    # where there is no tie at the k-th place the rule IS the reference's answer
        _sk_cache[key] = (pts, lab, q, sk, want, nn)
    return _sk_cache[key]


def knn_against_sklearn(hk, n, m, k, classes):
    pts, lab, q, sk, want, nn = sklearn_case(n, m, k, classes)
    got, got_nn, n2 = hk.knn(pts, lab, q, k)
    assert np.array_equal(got, sk)
    assert np.array_equal(got_nn, nn)
    # The gap and the margin force phase 2 only where the lattice has many cells: the shapes with n >= 300.  For n = 64 and n = 5 the
    # lattice is a few cells, the walk's cube covers it within its rings and answers every query itself (n2 == 0, legitimately);
    # for those two shapes only the HMSG_DEBUG_KNN_BRUTE run below goes through the scan, and nothing here tests the hand-over.
    assert n2 < m and (n2 > 0 or n < 300), n2
    b, b_nn, nb = hk.knn(pts, lab, q, k, brute=True)
    assert nb == m
    assert np.array_equal(b, got) and np.array_equal(b_nn, got_nn)
    assert n == k or len(set(got.tolist())) > 1              # (n == k: every query sees the same k rows)


def knn_exact_ties(hk):
    """an 8 x 8 x 8 lattice at 0.05, two classes, every point twice; queries on the lattice points and the cell centres: every query
    has tied candidates (at least the two copies), decided by the index"""
    g = np.arange(8) * 0.05
    lat = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    pts = np.concatenate([lat, lat])
    rng = np.random.default_rng(3)
    perm = rng.permutation(len(pts))
    pts = pts[perm]
    lab = (pts[:, 0] > 0.16).astype(np.int32) * 3 + 2          # classes 2 and 5
    c = (np.arange(7) + 0.5) * 0.05
    q = np.concatenate([lat, np.stack(np.meshgrid(c, c, c, indexing="ij"), -1).reshape(-1, 3)])
    for k in (1, 5, 8, 16):
        want, nn, dk = R.knn_vote(pts, lab, q, k)
        assert k % 2 == 0 or (dk[:, k] == dk[:, k - 1]).mean() > 0.3       # odd k: the k-th place splits a pair of copies
        got, got_nn, _ = hk.knn(pts, lab, q, k)
        assert np.array_equal(got, want) and np.array_equal(got_nn, nn), k
        b, b_nn, _ = hk.knn(pts, lab, q, k, brute=True)
        assert np.array_equal(b, want) and np.array_equal(b_nn, nn), k


def knn_dropped_rows(hk):
    pts, lab, q = two_boxes(600, 300, 5, 7, seed=11)
    lab = lab.copy()
    lab[::3] = -1
    want, nn, _ = R.knn_vote(pts, lab, q, 5)
    got, got_nn, _ = hk.knn(pts, lab, q, 5)
    assert np.array_equal(got, want) and np.array_equal(got_nn, nn)
    assert got_nn.max() < (lab != -1).sum() and got_nn.min() >= 0      # positions AFTER the drop
    kept = np.flatnonzero(lab != -1)
    assert (lab[kept[got_nn]] != -1).all()
    # a degenerate cloud: all kept rows at one point, and rows on a line
    one = np.tile([[1.0, 2.0, 3.0]], (9, 1))
    got, got_nn, _ = hk.knn(one, np.arange(9) % 2, q[:50], 3)
    assert (got == 0).all() and (got_nn == np.arange(3)).all()
    line = np.zeros((200, 3))
    line[:, 1] = np.linspace(0, 5, 200)
    ll = (np.arange(200) // 50).astype(np.int32)
    want, nn, _ = R.knn_vote(line, ll, q, 4)
    got, got_nn, _ = hk.knn(line, ll, q, 4)
    assert np.array_equal(got, want) and np.array_equal(got_nn, nn)


def knn_refusals(hk):
    pts, lab, q = two_boxes(20, 10, 5, 3, seed=1)
    out, nn = np.full(10, 77, np.int32), np.full(160, 77, np.int32)
    f, h = hk.L.c.hmsg_knn_labels, hk.scene.h

    def call(p=pts, l=lab, qq=q, k=5, n=20):
        p, l, qq = np.ascontiguousarray(p), np.ascontiguousarray(l, np.int32), np.ascontiguousarray(qq)
        return f(h, n, p.ctypes.data, l.ctypes.data, 10, qq.ctypes.data, k, out.ctypes.data, nn.ctypes.data)
    assert call(k=0) == HMSG_ERR_INVALID
    assert call(k=17) == HMSG_ERR_INVALID
    assert call(n=4) == HMSG_ERR_INVALID                                  # n < k
    few = lab.copy()
    few[4:] = -1
    assert call(l=few) == HMSG_ERR_INVALID                                # ... after the drop
    bad = pts.copy()
    bad[7, 1] = np.nan
    assert call(p=bad) == HMSG_ERR_INVALID
    badq = q.copy()
    badq[3, 2] = np.inf
    assert call(qq=badq) == HMSG_ERR_INVALID
    neg = lab.copy()
    neg[5] = -2
    assert call(l=neg) == HMSG_ERR_INVALID
    assert (out == 77).all() and (nn == 77).all() and len(hk.L.c.hmsg_last_error(h)) > 0
    assert f(None, 20, pts.ctypes.data, lab.ctypes.data, 10, q.ctypes.data, 5, out.ctypes.data, None) == HMSG_ERR_INVALID
    assert f(h, 20, pts.ctypes.data, lab.ctypes.data, 0, None, 5, None, None) == 0           # m == 0
    assert f(h, 3, pts.ctypes.data, lab.ctypes.data, 0, None, 5, None, None) == 0            # ... is success whatever n is,
    assert f(h, 3, pts.ctypes.data, lab.ctypes.data, 0, None, 17, None, None) == HMSG_ERR_INVALID      # but k is checked first
    assert (out == 77).all() and (nn == 77).all()
    dropped = lab.copy()
    dropped[7] = -1                                        # a row that is dropped may hold anything: the reference never sees it
    assert call(p=bad, l=dropped) == 0 and (out != 77).all()
    want = R.knn_vote(np.nan_to_num(bad), dropped, q, 5)[0]
    assert np.array_equal(out, want)
    out[:], nn[:] = 77, 77
    assert call() == 0 and (out != 77).all() and (nn[:50] != 77).all() and (nn[50:] == 77).all()


# ------------------------------------------------------------------------------------------------ instance labels
def instance_labels(hk, D, C_, n):
    emb, text, names, _ = TS.table(D, C_, n, seed=D + C_ + n)
    cl = (names * 3 + 1).astype(np.int32)
    want, sims = R.instance_labels(emb, text, cl)
    top = np.sort(sims, axis=1)
    assert C_ < 2 or (top[:, -1] - top[:, -2] > 1e-3).all()
    assert np.array_equal(hk.labels(emb, text, cl), want)
    assert np.array_equal(hk.labels(emb.astype(np.float64), text, cl), want)       # float64 embeddings are cast to float32 first


def instance_labels_ties_and_zero(hk):
    D, C_ = 8, 40
    emb, text, names, _ = TS.table(D, C_, 4, seed=5)
    cl = (names + 100).astype(np.int32)
    s = R.instance_labels(emb[:1], text, cl)[1][0]
    best, other = int(s.argmax()), int((s.argmax() + 7) % C_)
    text2 = text.copy()
    text2[other] = text[best]                                  # two classes with rows of the same bits: the smaller index wins
    assert hk.labels(emb[:1], text2, cl).tolist() == [100 + min(best, other)]
    zero = np.zeros((3, D), np.float32)                        # graph.py:479-483: an empty instance's zeros(1, D) gets class 0
    assert hk.labels(zero, text, cl).tolist() == [100, 100, 100]
    mixed = np.concatenate([zero[:1], emb[:2]])
    assert hk.labels(mixed, text, cl).tolist() == [100] + R.instance_labels(emb[:2], text, cl)[0].tolist()


# ------------------------------------------------------------------------------------------------ confusion matrix
def confusion_case(hk, L, m):
    rng = np.random.default_rng(L * 7 + m)
    gt, pred = rng.integers(0, L, m).astype(np.int32), rng.integers(0, L, m).astype(np.int32)
    pred[: m // 2] = gt[: m // 2]
    want = R.confusion(gt, pred, L)
    got = hk.confusion(gt, pred, L)
    assert got.dtype == np.int64 and np.array_equal(got, want) and got.sum() == m
    assert np.array_equal(hk.confusion(gt, pred, L), want)                 # two calls give the same matrix
    bad = pred.copy()
    bad[m // 2] = L                                                        # a label equal to L is refused, conf untouched
    conf = np.full((L, L), 77, np.int64)
    for g, p in ((gt, bad), (bad, pred)):
        rc = hk.L.c.hmsg_semseg_confusion(hk.scene.h, m, g.ctypes.data, p.ctypes.data, L, conf.ctypes.data)
        assert rc == HMSG_ERR_INVALID and (conf == 77).all()


# ------------------------------------------------------------------------------------------------ metrics
def golden_cases():
    fx = np.load(GOLDEN)
    for i in range(int(fx["n_cases"])):
        yield i, fx["gt_%d" % i], fx["pred_%d" % i], fx["ignore_%d" % i], fx["scores_%d" % i], fx["classes_%d" % i], fx["per_class_%d" % i]


def metrics_golden(hk):
    """bit for bit the reference's metric.py on its own label arrays: pixel_accuracy, mean_accuracy, mean_iou, frequency_weighted_iou
    and per_class_iou (a list over the union's classes)"""
    from holoagent_amd import semseg as S
    from holoagent_amd._lib import semseg_metrics
    seen = set()
    for i, gt, pred, ignore, scores, classes, per_class in golden_cases():
        L = int(max(gt.max(), pred.max())) + 2                # (one class beyond the largest: on neither side)
        conf = hk.confusion(gt.reshape(-1), pred.reshape(-1), L)
        d = semseg_metrics(conf, ignore.tolist(), lib_=hk.L)
        got = np.array([d["acc"], d["macc"], d["miou"], d["fmiou"]])
        assert np.array_equal(got, scores, equal_nan=True), (i, got, scores)
        assert np.array_equal(d["per_class_iou"][classes], per_class), i
        rest = np.setdiff1d(np.arange(L), classes)
        assert np.isnan(d["per_class_iou"][rest]).all() and len(rest) >= 1
        m = R.metrics(conf, ignore.tolist())                  # the numpy model says the same
        assert np.array_equal(np.array([m["acc"], m["macc"], m["miou"], m["fmiou"]]), scores, equal_nan=True), i
        # the reference's names and signatures, through the library
        ig = ignore.tolist()
        with S.using(hk.L):
            got2 = np.array([S.pixel_accuracy(pred, gt, ig), S.mean_accuracy(pred, gt, ig), S.mean_iou(pred, gt, ig),
                             S.frequency_weighted_iou(pred, gt, ig)])
            assert np.array_equal(got2, scores, equal_nan=True), i
            assert np.array_equal(np.asarray(S.per_class_iou(pred, gt, ig), np.float64), per_class), i
        seen.add(len(np.unique(gt)))
    assert {1, 7, 9, 200} <= seen                             # numpy's pairwise sum changes its path at 8 and at 128 terms
    fx = np.load(GOLDEN)                                      # the recorded knn_interpolation run
    got, _, _ = hk.knn(fx["knn_pts"], fx["knn_lab"], fx["knn_q"], int(fx["knn_k"]))
    assert np.array_equal(got, fx["knn_out"].astype(np.int32))


needs_emu = pytest.mark.skipif(not os.path.exists(PC.EMU_PATH), reason="kernel simulator not built")


@pytest.fixture(scope="module")
def emu():
    from holoagent_amd._lib import HmsgLib
    hk = Hook(HmsgLib(PC.EMU_PATH))
    yield hk
    hk.close()


@needs_emu
@pytest.mark.parametrize("n,m,k,classes", KNN_SHAPES)
def test_knn_against_sklearn_simulator(emu, n, m, k, classes):
    knn_against_sklearn(emu, n, m, k, classes)


@needs_emu
def test_knn_exact_ties_simulator(emu):
    knn_exact_ties(emu)


@needs_emu
def test_knn_dropped_rows_simulator(emu):
    knn_dropped_rows(emu)


@needs_emu
def test_knn_refusals_simulator(emu):
    knn_refusals(emu)


@needs_emu
@pytest.mark.parametrize("D,C_,n", LABEL_SHAPES)
def test_instance_labels_simulator(emu, D, C_, n):
    instance_labels(emu, D, C_, n)


@needs_emu
def test_instance_labels_ties_and_zero_simulator(emu):
    instance_labels_ties_and_zero(emu)


@needs_emu
@pytest.mark.parametrize("L,m", CONF_SHAPES)
def test_confusion_simulator(emu, L, m):
    confusion_case(emu, L, m)


@needs_emu
def test_metrics_golden_simulator(emu):
    metrics_golden(emu)
