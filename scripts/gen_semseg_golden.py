"""Golden generator for the semantic segmentation score: runs the REFERENCE's own utils/metric.py (pixel_accuracy, mean_accuracy,
mean_iou, frequency_weighted_iou, per_class_iou) and eval_utils.knn_interpolation on seeded label arrays and a small cloud, and stores
inputs + answers as tests/golden/semseg_metrics.npz.  Nothing of the reference travels: only data.

    python scripts/gen_semseg_golden.py [output.npz]          # from the repo root, where the reference checkout exists

The reference is imported with the recipe of oracle/refdrive/gen_golden.py (SURVEY.md's appendix); eval_utils.py additionally imports
`hmsg.utils.clip_utils`, which is given a stand-in (no text encoder is called here).  scikit-learn and scipy are the real ones.

Cases (numpy's pairwise sum changes its path at 8 and at 128 terms, hence 1, 7, 9 and 200 present classes): see CASES.  The k-NN case
is drawn so that no query's 5th and 6th neighbour are equally far: there BallTree's answer is defined.
"""
from __future__ import annotations

import os
import sys
import warnings
from unittest.mock import MagicMock

import numpy as np

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, REPO)


def noisy(rng, gt, classes, rate=0.3):
    pred = gt.copy()
    flip = rng.random(gt.shape) < rate
    pred[flip] = rng.choice(classes, int(flip.sum()))
    return pred


def cases(rng):
    """-> [(gt [1, N], pred [1, N], ignore)]"""
    out = []
    for n_cl, N in ((1, 50), (7, 400), (9, 500), (200, 6000)):
        cl = np.sort(rng.choice(np.arange(1, 260), n_cl, replace=False))
        gt = rng.choice(cl, (1, N))
        gt[0, :n_cl] = cl                                                   # every class is present
        out.append((gt, noisy(rng, gt, cl), []))
    cl = np.array([2, 3, 5, 8, 13])
    gt = rng.choice(cl, (1, 300))
    pred = noisy(rng, gt, cl)
    pred[0, ::17] = 21                                                      # a class predicted but absent from the ground truth
    out.append((gt, pred, []))
    pred = noisy(rng, gt, cl)
    pred[pred == 8] = 3                                                     # a ground-truth class never predicted
    out.append((gt, pred, []))
    out.append((gt, noisy(rng, gt, cl), [0, 5]))                            # an ignore list naming a present class (and an absent one)
    out.append((gt, noisy(rng, gt, cl), [4, 99]))                           # ... naming absent classes only
    out.append((gt, noisy(rng, gt, cl), [2, 3, 5, 8, 13]))                  # every ground-truth class ignored: the divisions by zero
    pred = noisy(rng, gt, cl)
    pred[0, ::11] = 21
    out.append((gt, pred, [21, 13]))                                        # an ignored class that is only predicted
    return out


def knn_case(rng):
    while True:
        pts = rng.random((400, 3))
        pts[200:, 0] += 4.0
        lab = rng.integers(0, 9, 400).astype(np.float64)
        lab[::5] = -1
        q = np.concatenate([rng.random((150, 3)) * np.array([5.0, 1.0, 1.0]), rng.random((150, 3)) * np.array([9.0, 5.0, 5.0]) - 2.0])
        kept = pts[lab != -1]
        d = q[:, None, :] - kept[None, :, :]
        d2 = np.sort((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2], axis=1)
        if (d2[:, 5] > d2[:, 4] * (1 + 1e-9)).all():
            return pts, lab, q


def main(path):
    from oracle.refdrive.gen_golden import import_reference
    import_reference()
    for m in ("hmsg", "hmsg.utils", "hmsg.utils.clip_utils"):
        sys.modules.setdefault(m, MagicMock())
    import memory.hmsg.utils.eval_utils as EU
    import memory.hmsg.utils.metric as M
    rng = np.random.Generator(np.random.PCG64(20261020))
    out = {}
    cs = cases(rng)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for i, (gt, pred, ignore) in enumerate(cs):
            scores = [M.pixel_accuracy(pred, gt, ignore), M.mean_accuracy(pred, gt, ignore), M.mean_iou(pred, gt, ignore),
                      M.frequency_weighted_iou(pred, gt, ignore)]
            out["gt_%d" % i], out["pred_%d" % i] = gt.astype(np.int64), pred.astype(np.int64)
            out["ignore_%d" % i] = np.asarray(ignore, np.int64)
            out["scores_%d" % i] = np.asarray([float(s) for s in scores], np.float64)
            out["classes_%d" % i] = np.union1d(np.unique(pred), np.unique(gt)).astype(np.int64)
            out["per_class_%d" % i] = np.asarray([float(v) for v in M.per_class_iou(pred, gt, ignore)], np.float64)
    out["n_cases"] = np.int64(len(cs))
    pts, lab, q = knn_case(rng)
    devnull = open(os.devnull, "w")
    old, sys.stdout = sys.stdout, devnull                                   # (knn_interpolation prints)
    try:
        res = EU.knn_interpolation(np.column_stack([pts, lab]), q, 5)
    finally:
        sys.stdout = old
        devnull.close()
    out.update(knn_pts=pts, knn_lab=lab.astype(np.int32), knn_q=q, knn_k=np.int64(5), knn_out=res[:, -1].astype(np.int64))
    np.savez_compressed(path, **out)
    print("semseg_metrics ok:", len(cs), "cases,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(REPO, "tests", "golden", "semseg_metrics.npz"))
