"""hmsg_eval_object_matrices (include/hmsg.h; holoagent_amd/csrc/hmsg_eval.hip) against a literal numpy restatement of
evaluate_objects' matrix loop (memory/hmsg/eval/hm3dsem_evaluator.py:429-458): the predicted box through Open3D's corner order
(oracle/refdrive/fake_backends.py) and find_box_center_and_dims, get_3d_iou in float64, find_overlapping_ratio_faiss in float32 only
where iou > 0.  Both matrices must be EQUAL to the restatement's, bit for bit: they are the same float64 operations on the same
integers.  Simulator here, the library under `gpu`."""
import os

import numpy as np
import pytest

from oracle.refdrive.fake_backends import _AABB
from tests import overlap_cases as OC
from tests import parity_common as PC

HMSG_ERR_INVALID = -1


def find_box_center_and_dims(box_3d):                      # utils/eval_utils.py:413-417
    a = np.array(box_3d)
    return np.mean(a, axis=0), np.ptp(a, axis=0)


def get_3d_iou(c1, d1, c2, d2):                            # utils/eval_utils.py:169-200
    e1, e2 = [d / 2 for d in d1], [d / 2 for d in d2]
    mn1, mx1 = [c1[i] - e1[i] for i in range(3)], [c1[i] + e1[i] for i in range(3)]
    mn2, mx2 = [c2[i] - e2[i] for i in range(3)], [c2[i] + e2[i] for i in range(3)]
    imn, imx = [max(mn1[i], mn2[i]) for i in range(3)], [min(mx1[i], mx2[i]) for i in range(3)]
    inter = max(0, imx[0] - imn[0]) * max(0, imx[1] - imn[1]) * max(0, imx[2] - imn[2])
    union = d1[0] * d1[1] * d1[2] + d2[0] * d2[1] * d2[2] - inter
    return inter / union if union > 0 else 0.0


def overlap_ratio(a, b, radius):                           # utils/graph_utils.py:620-664, direct distance form
    if len(a) == 0 or len(b) == 0:
        return 0
    r2 = np.float32(radius * radius)
    return np.max([np.sum(OC.brute_f32(a, b, r2)) / a.shape[0], np.sum(OC.brute_f32(b, a, r2)) / b.shape[0]])


def restated(pred, gt, gc, gd, radius):
    iou_m, ov_m = np.zeros((len(pred), len(gt))), np.zeros((len(pred), len(gt)))
    for g in range(len(gt)):
        for p in range(len(pred)):
            pts = pred[p]
            box = _AABB(pts.min(0), pts.max(0)) if len(pts) else _AABB(np.zeros(3), np.zeros(3))
            pc, pd = find_box_center_and_dims(box.get_box_points())
            iou = get_3d_iou(gc[g], gd[g], pc, pd)
            iou_m[p][g] = iou
            if iou > 0.0:
                ov_m[p][g] = overlap_ratio(pts, gt[g], radius)
    return iou_m, ov_m


def box_surface(rng, lo, hi, n):
    p = rng.uniform(lo, hi, (n, 3))
    axis, side = rng.integers(0, 3, n), rng.integers(0, 2, n)
    p[np.arange(n), axis] = np.where(side == 0, lo[axis], hi[axis])
    return p


def scene(seed=2, n_gt=14, n_pred=18):
    """ground-truth boxes sampled on their surfaces at 2 .. 3 cm, predictions: the objects seen again (shifted a little, a third from
    one side only), three spurious ones far from everything, one inside an object (gate open, no overlap), one empty, one of one point;
    coordinates such as 0.1 * k that float64 does not hold exactly, a few metres from the origin"""
    rng = np.random.default_rng(seed)
    gt, gc, gd = [], [], []
    for _ in range(n_gt):
        c = rng.uniform((3.5, 0.2, -6.5), (9.5, 2.0, -1.5))
        half = rng.uniform(0.1, 0.35, 3)
        gt.append(box_surface(rng, c - half, c + half, int(rng.integers(300, 1400))))
        gc.append(c + rng.normal(0, 0.01, 3))              # (an oriented box's centre and dims: near the cloud's, not equal)
        gd.append(2 * half * rng.uniform(0.95, 1.1, 3))
    pred = []
    for k in range(n_pred):
        if k < n_pred - 6:
            g = gt[k % n_gt]
            p = box_surface(rng, g.min(0), g.max(0), int(rng.integers(200, 1200))) + rng.uniform(-0.02, 0.02, 3)
            if k % 3 == 0:
                p = p[p[:, 0] < np.median(p[:, 0])]
        elif k < n_pred - 3:
            c = rng.uniform((20.0, 0.2, 5.0), (25.0, 2.0, 9.0))
            p = box_surface(rng, c - 0.2, c + 0.2, 150)
        elif k == n_pred - 3:
            c = (gt[0].min(0) + gt[0].max(0)) / 2
            p = box_surface(rng, c - 0.02, c + 0.02, 80)
        elif k == n_pred - 2:
            p = np.zeros((0, 3))
        else:
            p = gt[1][:1] + 0.003
        pred.append(np.round(p, 3))
    return pred, [np.round(g, 3) for g in gt], np.array(gc), np.array(gd)


def check(L):
    from holoagent_amd._lib import Scene
    sc = Scene(lib_=L, height=8, width=8, max_frames=1, max_masks=1, feat_dim=16)
    pred, gt, gc, gd = scene()
    want_iou, want_ov = restated(pred, gt, gc, gd, 0.02)
    gate = want_iou > 0
    # conditions on the inputs: gated pairs with and without overlap, closed gates, ratios on either side of 0.5
    # (12 objects seen again + the one inside an object; a one-point cloud has a box without volume: its gate stays closed)
    assert gate.sum() >= 13 and (~gate).sum() >= 100 and (want_ov[gate] == 0).sum() >= 1 and (want_ov > 0.5).sum() >= 3
    assert ((want_ov > 0) & (want_ov < 0.5)).sum() >= 3 and not gate[-2].any() and not gate[-1].any()
    iou, ov, n = sc.eval_object_matrices(pred, gt, gc, gd, 0.02)
    assert n == int(gate.sum())
    assert np.array_equal(iou.view(np.uint64), want_iou.view(np.uint64)), np.argwhere(iou != want_iou)[:5].tolist()
    assert np.array_equal(ov.view(np.uint64), want_ov.view(np.uint64)), np.argwhere(ov != want_ov)[:5].tolist()
    # no predictions / no ground truth: refused, as the reference's metrics divide by zero there
    for p_, g_ in (([], gt), (pred, [])):
        from holoagent_amd._lib import HmsgError
        with pytest.raises(HmsgError):
            sc.eval_object_matrices(p_, g_, gc[:len(g_)], gd[:len(g_)], 0.02)
    sc.close()


@pytest.mark.skipif(not os.path.exists(PC.EMU_PATH), reason="kernel simulator not built")
def test_object_matrices_simulator():
    from holoagent_amd._lib import HmsgLib
    check(HmsgLib(PC.EMU_PATH))


@pytest.mark.gpu
def test_object_matrices_gpu():
    from holoagent_amd._lib import HmsgLib
    check(HmsgLib())
