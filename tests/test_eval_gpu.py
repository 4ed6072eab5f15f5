"""hmsg_cloud_set_overlaps / hmsg_cloud_set_overlaps_kd / hmsg_lsap on the GPU build of the library: the exact sets of
tests/test_eval_overlaps.py from host arrays and from torch device tensors, one call of use-like shape (64 predicted against 48
ground-truth object clouds of up to 5 000 points, the pairs behind the evaluator's box gate) compared count for count with the
exhaustive route hmsg_pair_overlaps, and two calls on the same inputs compared with each other."""
import numpy as np
import pytest

from tests import overlap_cases as OC
from tests import test_eval_overlaps as T

pytestmark = pytest.mark.gpu


def _device(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module", params=["host", "device"])
def hk(request):
    from holoagent_amd._lib import HmsgLib
    h = T.Hook(HmsgLib(), wrap=_device if request.param == "device" else None)
    yield h
    h.close()


@pytest.mark.parametrize("form", [OC.FORM_DIRECT, OC.FORM_BLAS])
@pytest.mark.parametrize("family", list(T.LATTICE))
def test_lattice_sets_gpu(hk, family, form):
    T.lattice(hk, family, form)


@pytest.mark.parametrize("form", [OC.FORM_DIRECT, OC.FORM_BLAS])
@pytest.mark.parametrize("place", ["origin", "far"])
def test_realistic_sets_gpu(hk, place, form):
    T.realistic(hk, place, form)


@pytest.mark.parametrize("form", [OC.FORM_DIRECT, OC.FORM_BLAS])
def test_cloud_sizes_gpu(hk, form):
    T.sizes(hk, form)


def test_shapes_of_the_pair_list_gpu(hk):
    T.shapes_of_the_pair_list(hk)


def test_wide_span_gpu(hk):
    T.wide_span(hk)


def test_kd_comparison_gpu(hk):
    T.kd_mode(hk)


def test_bad_arguments_gpu():
    from holoagent_amd._lib import HmsgLib
    h = T.Hook(HmsgLib())
    T.bad_arguments(h)
    h.close()


def test_lsap_gpu_build():
    """the host solver as the product library exports it"""
    from scipy.optimize import linear_sum_assignment
    from holoagent_amd._lib import HmsgLib, lsap
    L = HmsgLib()
    rng = np.random.default_rng(5)
    for nr, nc in ((40, 60), (60, 40), (33, 33)):
        m = np.round(rng.random((nr, nc)), 1) * (rng.random((nr, nc)) < 0.1)
        for mx in (False, True):
            r0, c0 = linear_sum_assignment(m, maximize=mx)
            r1, c1 = lsap(m, maximize=mx, lib_=L)
            assert np.array_equal(r0, r1) and np.array_equal(c0, c1)


def box_surface(rng, lo, hi, n):
    """n points on the surface of the box [lo, hi]"""
    p = rng.uniform(lo, hi, (n, 3))
    axis = rng.integers(0, 3, n)
    side = rng.integers(0, 2, n)
    p[np.arange(n), axis] = np.where(side == 0, lo[axis], hi[axis])
    return p


def use_like_scene(seed=4):
    """48 ground-truth objects (box surfaces, 500 .. 5 000 samples) in a 10 x 3 x 8 m storey and 64 predictions: most of them a
    ground-truth object seen again (shifted by up to 3 cm, partly cut off), the last 8 spurious (inside an object, far from its surface).
    -> pred clouds, gt clouds, pairs whose axis-aligned boxes intersect"""
    rng = np.random.default_rng(seed)
    gt, gbox = [], []
    for _ in range(48):
        c = rng.uniform((0.5, 0.2, 0.5), (9.5, 2.0, 7.5))
        half = rng.uniform(0.15, 0.75, 3)
        lo, hi = c - half, c + half
        gt.append(box_surface(rng, lo, hi, int(rng.integers(500, 5001))))
        gbox.append((lo, hi))
    pred = []
    for k in range(64):
        if k < 56:
            lo, hi = gbox[k % 48]
            p = box_surface(rng, lo, hi, int(rng.integers(300, 5001))) + rng.uniform(-0.03, 0.03, 3) + rng.normal(0, 0.01, (1, 3))
            if k % 3 == 0:                                   # seen from one side only
                p = p[p[:, 0] < np.median(p[:, 0])]
        else:
            lo, hi = gbox[k - 56]                            # spurious: a small thing in the middle of an object, 10 cm from its surface
            c = (lo + hi) / 2
            p = box_surface(rng, c - 0.05, c + 0.05, int(rng.integers(50, 800)))
        pred.append(p)
    pairs = []
    for a, p in enumerate(pred):
        plo, phi = p.min(0), p.max(0)
        for b, g in enumerate(gt):
            if (plo <= g.max(0)).all() and (g.min(0) <= phi).all():
                pairs.append((a, b))
    return pred, gt, np.array(pairs, np.int32)


def test_use_like_shape_equals_the_exhaustive_route():
    from holoagent_amd._lib import HmsgLib
    L = HmsgLib()
    h = T.Hook(L)
    pred, gt, pairs = use_like_scene()
    assert len(pred) == 64 and len(gt) == 48 and len(pairs) >= 64 and max(len(g) for g in gt) > 4000
    radius = 0.02
    got = h.counts(0, pred, gt, pairs, radius)
    again = h.counts(0, pred, gt, pairs, radius)
    assert np.array_equal(got, again), "two calls on the same inputs differ"
    pts, off = T.csr(pred + gt)
    joint = np.ascontiguousarray(pairs + np.array([0, len(pred)], np.int32))
    ref = np.full((len(pairs), 2), 0xDEADBEEF, np.uint32)
    rc = L.c.hmsg_test_pair_overlaps(h.scene(0).h, len(pred) + len(gt), pts.ctypes.data, off.ctypes.data, len(pairs), joint.ctypes.data, radius,
                                     ref.ctypes.data)
    assert rc == 0
    assert np.array_equal(got, ref.astype(np.int64)), np.flatnonzero((got != ref).any(1))[:10].tolist()
    n_a = np.array([len(pred[a]) for a, _ in pairs])
    assert (got[:, 0] > 0).sum() >= 30 and ((got[:, 0] > 0) & (got[:, 0] < n_a)).sum() >= 20 and (got.sum(1) == 0).sum() >= 5
    # the same from device tensors
    hd = T.Hook(L, wrap=_device)
    assert np.array_equal(hd.counts(0, pred, gt, pairs, radius), got)
    hd.close()
    # ... and with the pair list and the counts in device memory as well (the C call itself: the wrapper's counts are a host array)
    import torch
    pa, oa = T.csr(pred)
    pb, ob = T.csr(gt)
    d = [_device(v) for v in (pa, oa, pb, ob, pairs)]
    out = torch.full((len(pairs), 2), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    rc = L.c.hmsg_cloud_set_overlaps(h.scene(0).h, len(pred), d[0].data_ptr(), d[1].data_ptr(), len(gt), d[2].data_ptr(), d[3].data_ptr(), len(pairs),
                                     d[4].data_ptr(), radius, out.data_ptr())
    assert rc == 0 and np.array_equal(out.cpu().numpy().astype(np.int64), got)
    h.close()
