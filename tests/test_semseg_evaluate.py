"""hmsg_evaluate_semseg (include/hmsg.h) on a scene built from a few synthetic frames: the one call must equal the composition of
the four calls it is made of, fed with the instance points and pooled features READ BACK from the scene -- scores, per-class IoU
and confusion matrix exact -- and Graph.evaluate_semseg must give the same dict.  CPU: the kernel simulator; -m gpu: libhmsg.so."""
import os

import numpy as np
import pytest

from tests import parity_common as PC

WORDS = ["wall", "chair", "table", "floor", "sofa", "lamp"]
IDS = [3, 10, 11, 40, 41, 7]                                   # arbitrary class ids; 99 below is a ground-truth class without a text row


def build_graph(L):
    from holoagent_amd.graph import Graph
    from tests.graph_fixture import SynthDataset, SynthEncoders, tiny_scene
    scn = tiny_scene(4, 32)
    ds = SynthDataset(scn)
    enc = SynthEncoders(ds, ["background"] + WORDS)
    cfg = dict(main=dict(device_id=0), models=dict(clip=dict(type="ViT-B/32", feat_dim=32)),
               pipeline=dict(voxel_size=0.05, skip_frames=1, merge_type="sequential", max_masks=8))
    g = Graph(cfg, dataset=ds, encoders=enc, lib=L)
    g.create_feature_map()
    return g


def ground_truth(pts, rng, m=5000):
    """m labelled points: most beside the mapped points, the rest anywhere in a box 1 m larger than the map's (nothing mapped there)"""
    near = pts[rng.integers(0, len(pts), m * 9 // 10)] + 0.03 * rng.standard_normal((m * 9 // 10, 3))
    lo, hi = pts.min(0) - 1.0, pts.max(0) + 1.0
    far = lo + (hi - lo) * rng.random((m - len(near), 3))
    gt = np.ascontiguousarray(np.concatenate([near, far]))
    return gt, rng.choice(IDS + [99], m).astype(np.int64)


def same(a, b):
    for key in ("miou", "fmiou", "acc", "macc"):
        assert np.array_equal(a[key], b[key], equal_nan=True), (key, a[key], b[key])
    assert np.array_equal(a["confusion"], b["confusion"]) and np.array_equal(a["classes"], b["classes"])
    assert a["per_class_iou"].keys() == b["per_class_iou"].keys()
    for c in a["per_class_iou"]:
        assert np.array_equal(a["per_class_iou"][c], b["per_class_iou"][c], equal_nan=True), c


def whole_evaluation(L, wrap=lambda a: a):
    from holoagent_amd._lib import HmsgError, Scene, semseg_metrics
    g = build_graph(L)
    sc = g.scene
    sizes = sc.instance_sizes()
    assert len(sizes) >= 2 and sizes.sum() > 100
    pts = np.empty((int(sizes.sum()), 3))
    sc.instance_points_into(pts)
    feats = np.ascontiguousarray(sc.instance_feats(), np.float32)
    rng = np.random.default_rng(17)
    gt_pts, gt_lab = ground_truth(pts, rng)
    text = g.get_text_feats_multiple_templates(WORDS)
    ignore = [3, 55]                                          # a class with a text row, and one that is nowhere
    for k in (5, 1):
        got = sc.evaluate_semseg(wrap(text), IDS, wrap(gt_pts), gt_lab, k=k, ignore=ignore)
        # ---- the composition, on what the scene hands back
        classes = np.unique(np.concatenate([IDS, gt_lab, ignore]))
        cl = np.searchsorted(classes, IDS).astype(np.int32)
        inst = sc.semseg_instance_labels(feats, text, cl)
        paint = np.repeat(inst, sizes).astype(np.int32)       # instances in order, duplicates kept
        pred = sc.knn_labels(pts, paint, gt_pts, k)
        conf = sc.semseg_confusion(np.searchsorted(classes, gt_lab).astype(np.int32), pred, len(classes))
        m = semseg_metrics(conf, np.searchsorted(classes, ignore).tolist(), lib_=L)
        want = dict(m, confusion=conf, classes=classes, per_class_iou={int(c): float(v) for c, v in zip(classes, m["per_class_iou"])})
        same(got, want)
        assert got["confusion"].sum() == len(gt_pts) and got["confusion"][np.searchsorted(classes, 55)].sum() == 0
        assert sc.knn_last_phase2() > 0                       # the far ground-truth points went through the scan
        assert 0.0 <= got["acc"] <= 1.0 and np.isnan(got["per_class_iou"][55])
        # ---- the mirror: class names (text features from get_text_feats_multiple_templates), and the features themselves
        same(g.evaluate_semseg(gt_pts, gt_lab, WORDS, k=k, ignore=ignore, class_ids=IDS), got)
        same(g.evaluate_semseg(gt_pts, gt_lab, dict(zip(IDS, WORDS)), k=k, ignore=ignore), got)
        same(g.evaluate_semseg(gt_pts, gt_lab, text, k=k, ignore=ignore, class_ids=IDS), got)
    # a scene without pooled instances is refused
    bare = Scene(lib_=L, height=8, width=8, max_frames=1, max_masks=1, feat_dim=32)
    with pytest.raises(HmsgError, match="pooled"):
        bare.evaluate_semseg(text, IDS, gt_pts, gt_lab)
    bare.close()
    sc.close()


@pytest.mark.skipif(not os.path.exists(PC.EMU_PATH), reason="kernel simulator not built")
def test_evaluate_semseg_simulator():
    from holoagent_amd._lib import HmsgLib
    whole_evaluation(HmsgLib(PC.EMU_PATH))


@pytest.mark.gpu
@pytest.mark.parametrize("where", ["host", "device"])
def test_evaluate_semseg_gpu(where):
    from holoagent_amd._lib import HmsgLib

    def dev(a):
        import torch
        return torch.from_numpy(np.ascontiguousarray(a)).cuda()
    whole_evaluation(HmsgLib(), wrap=dev if where == "device" else (lambda a: a))
