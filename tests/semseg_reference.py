"""numpy models of the semantic segmentation score (include/hmsg.h: hmsg_semseg_instance_labels, hmsg_knn_labels, hmsg_semseg_metrics),
written from the header's rules -- what the library is compared with where scikit-learn has no rule (exact ties) and where the
kernel's float32 needs a separated input (the cosine labels)."""
import numpy as np


def knn_vote(points, labels, queries, k, chunk=512):
    """the k rows smallest by (d2, index) among the rows with label != -1, d2 = ((dx*dx) + (dy*dy)) + (dz*dz) in float64, index = the
    position after the drop; the vote is np.bincount(...).argmax().  -> (label int32 [m], nn_index int32 [m, k], d2 of the k + 1 smallest
    float64 [m, min(k + 1, n)])"""
    points, labels = np.asarray(points, np.float64).reshape(-1, 3), np.asarray(labels).reshape(-1)
    kept = labels != -1
    p, l = points[kept], labels[kept].astype(np.int64)
    q = np.asarray(queries, np.float64).reshape(-1, 3)
    n, m = len(p), len(q)
    out, nn, dk = np.zeros(m, np.int32), np.zeros((m, k), np.int32), np.zeros((m, min(k + 1, n)))
    idx = np.arange(n)
    for a in range(0, m, chunk):
        d = q[a:a + chunk, None, :] - p[None, :, :]
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        for r in range(d2.shape[0]):
            order = np.lexsort((idx, d2[r]))                 # (d2, index)
            nn[a + r] = order[:k]
            dk[a + r] = d2[r][order[:dk.shape[1]]]
            out[a + r] = np.bincount(l[order[:k]]).argmax()
    return out, nn, dk


def instance_labels(emb, text, class_label):
    """cosine in float64 of the float32 values, rows divided by max(norm, 1e-8); -> (labels, sims [n, C]): the first of the largest"""
    x = np.asarray(emb).astype(np.float32).astype(np.float64)
    t = np.asarray(text, np.float32).astype(np.float64)
    xn = x / np.maximum(np.linalg.norm(x, axis=1, keepdims=True), 1e-8)
    tn = t / np.maximum(np.linalg.norm(t, axis=1, keepdims=True), 1e-8)
    s = xn @ tn.T
    return np.asarray(class_label)[s.argmax(axis=1)].astype(np.int32), s


def confusion(gt, pred, L):
    conf = np.zeros((L, L), np.int64)
    np.add.at(conf, (np.asarray(gt, np.int64), np.asarray(pred, np.int64)), 1)
    return conf


def metrics(conf, ignore=()):
    """the header's statement of the five numbers, from a confusion matrix (rows ground truth); sums by np.sum of float64 arrays in
    ascending class order.  -> dict(miou, fmiou, acc, macc, per_class_iou [L])"""
    conf = np.asarray(conf, np.int64)
    L = len(conf)
    t, p, d = conf.sum(1).astype(np.float64), conf.sum(0).astype(np.float64), np.diag(conf).astype(np.float64)
    m = float(conf.sum())
    ign = np.isin(np.arange(L), list(ignore))
    in_gt, in_un = t > 0, (t > 0) | (p > 0)
    with np.errstate(all="ignore"):
        iou = d / (t + p - d)
        per_class = np.where(~in_un, np.nan, np.where(ign, 0.0, iou))
        acc_terms = np.where(ign, 0.0, d / t)[in_gt]
        skip = ign | (t == 0) | (p == 0)
        iou_terms = np.where(skip, 0.0, iou)[in_un]
        fw_terms = np.where(skip, 0.0, (t * d) / (t + p - d))[in_un]
        n_cl = float(in_gt.sum() - (in_gt & ign).sum())
        st = t[in_gt & ~ign].sum()
        return dict(acc=0.0 if st == 0 else float(d[in_gt & ~ign].sum() / st),
                    macc=float(np.float64(np.sum(acc_terms)) / np.float64(n_cl)),
                    miou=float(np.float64(np.sum(iou_terms)) / np.float64(n_cl)),
                    fmiou=float(np.float64(np.sum(fw_terms)) / np.float64(m - t[ign].sum())), per_class_iou=per_class)
