"""The reference's evaluator (memory/hmsg/eval/hm3dsem_evaluator.py:193-589) restated literally in numpy / scipy, quirks included,
for the tests of hmsg_eval_rooms, hmsg_eval_semantic_ranks, the metrics header and hmsg_graph_evaluate.  Open3D's
voxel_down_sample is oracle.hmsg_oracle.o3d_voxel_down_sample (canonical ascending voxel order), find_overlapping_ratio_faiss's
distance is tests.overlap_cases.brute_f32, find_intersection_share is scipy's cKDTree."""
import numpy as np
from scipy.optimize import linear_sum_assignment
from scipy.spatial import cKDTree

from oracle.hmsg_oracle import o3d_voxel_down_sample
from tests import overlap_cases as OC

trapz = getattr(np, "trapezoid", None) or np.trapz          # (np.trapz under its name since numpy 2.0)


def vds(p, voxel):
    return o3d_voxel_down_sample(np.ascontiguousarray(p, np.float64).reshape(-1, 3), None, voxel)[0]


def overlapping_ratio_faiss(a, b, radius):
    """find_overlapping_ratio_faiss (utils/graph_utils.py:620-662), the direct float32 distance form"""
    if len(a) == 0 or len(b) == 0:
        return 0.0
    r2 = np.float32(radius * radius)
    return max(float(OC.brute_f32(a, b, r2).sum()) / len(a), float(OC.brute_f32(b, a, r2).sum()) / len(b))


def intersection_share(map_points, obj_points, radius):
    """find_intersection_share (utils/graph_utils.py:160-189): the points of `map_points` with a point of `obj_points` inside the
    bound, over the number of `obj_points` -- so it can exceed 1"""
    if len(map_points) == 0 or len(obj_points) == 0:
        return 0
    _, idx = cKDTree(obj_points).query(map_points, k=1, distance_upper_bound=radius, p=2)
    return int((idx != len(obj_points)).sum()) / len(obj_points)


def room_matrices(pred, zero_level, height, gt, min_h, max_h, mean_h, lower, upper, voxel=0.05, radius=0.05):
    """:278-341.  pred / gt: lists of float64 [n][3]; -> assoc, over_pred, over_gt [P][G], visits in loop 1 per gt room.
    The predicted clouds are NOT written to (the reference writes the flattened y into them; nothing reads it afterwards)."""
    P, G = len(pred), len(gt)
    bev = [np.array(g, np.float64).reshape(-1, 3) for g in gt]               # gt_room.bev_pcd, replaced at every visit
    assoc, over_pred, over_gt = np.zeros((P, G)), np.zeros((P, G)), np.zeros((P, G))
    visits = np.zeros(G, np.int64)
    for loop in (1, 2):
        for f in range(len(lower)):
            for g in range(G):
                if mean_h[g] > lower[f] and mean_h[g] < upper[f]:
                    for p in range(P):
                        pm = zero_level[p] + height[p] / 2
                        if pm > min_h[g] and pm < max_h[g]:
                            pts = np.array(pred[p], np.float64).reshape(-1, 3)
                            pts[:, 1] = min_h[g]
                            bev[g] = vds(bev[g], voxel)
                            pb = vds(pts, voxel)
                            if loop == 1:
                                visits[g] += 1
                                assoc[p][g] = overlapping_ratio_faiss(pb, bev[g], radius)
                            else:
                                over_pred[p][g] = min(intersection_share(bev[g], pb, radius), 1.0)
                                over_gt[p][g] = min(intersection_share(pb, bev[g], radius), 1.0)
    return assoc, over_pred, over_gt, visits


def sweep(M, row, col, P, G):
    """:364-383 / :467-484 -> dict(acc, prec, rec (sorted), tp, ap)"""
    acc, prec, rec, tps = [], [], [], []
    for thresh in np.linspace(0.0, 1.0, 11, endpoint=True):
        TP, TN = np.sum(M[row, col] > thresh), 0
        FP, FN = P - TP, G - TP
        prec.append(TP / (TP + FP) if (TP + FP) > 0 else 0)
        rec.append(TP / (TP + FN) if (TP + FN) > 0 else 0)
        acc.append((TP + TN) / (TP + TN + FP + FN) if (TP + TN + FP + FN) > 0 else 0)
        tps.append(int(TP))
    rec.sort()
    return dict(acc=acc, prec=prec, rec=rec, tp=tps, ap=trapz(prec, rec))


def counts_at(M, row, col, P, G, threshold=0.5):
    """:497-506"""
    TP, TN = np.sum(M[row, col] > threshold), 0
    FP, FN = P - TP, G - TP
    precision = TP / (TP + FP) if (TP + FP) > 0 else 0
    recall = TP / (TP + FN) if (TP + FN) > 0 else 0
    accuracy = (TP + TN) / (TP + TN + FP + FN) if (TP + TN + FP + FN) > 0 else 0
    return dict(acc=accuracy, prec=precision, recall=recall, tp=int(TP), fp=int(FP), fn=int(FN))


def hydra(over_pred, over_gt):
    """:343-356"""
    hp = hr = 0.0
    for i in range(over_pred.shape[0]):
        hp += np.max(over_pred[i, :])
    for j in range(over_gt.shape[1]):
        hr += np.max(over_gt[:, j])
    return hp / over_pred.shape[0], hr / over_gt.shape[1]


def floors(lower, upper, verts):
    """:193-263.  verts [Fp][8][3].  Raises ValueError (numpy's broadcast error) on unequal floor counts."""
    def bounds(pairs):
        b = sorted([y for x in pairs for y in x])
        return [b[0]] + [(b[i] + b[i + 1]) / 2 for i in range(1, len(b) - 1, 2)] + [b[-1]]
    gb = bounds([[lo, up] for lo, up in zip(lower, upper)])
    pb = []
    for v in verts:
        box = np.array(v)
        c, d = np.mean(box, axis=0), np.ptp(box, axis=0)
        pb.append([c[1] - d[1] / 2, c[1] + d[1] / 2])
    pb = bounds(pb)
    dist = np.abs(np.array(gb) - np.array(pb))
    TP, TN = 0, 0
    for i in range(len(dist)):
        if dist[i] < 0.5:
            TP += 1
    FP, FN = len(pb) - TP, len(gb) - TP
    precision = TP / (TP + FP) if (TP + FP) > 0 else 0
    recall = TP / (TP + FN) if (TP + FN) > 0 else 0
    accuracy = (TP + TN) / (TP + TN + FP + FN) if (TP + TN + FP + FN) > 0 else 0
    return dict(tp=TP, tn=TN, fp=FP, fn=FN, acc=accuracy, prec=precision, recall=recall)


def top_k_from_ranks(rank, ks, C):
    """:585-588 once `category in top_k_classes` is known to be rank < k"""
    rank = np.asarray(rank)
    acc = {int(k): int((rank < k).sum()) / len(rank) for k in ks}
    multi = [int((rank < k).sum()) / len(rank) for k in range(0, C, 10)]
    return acc, trapz(multi, [k / C for k in range(0, C, 10)])


def semantic_ranks(emb, text, class_name_id, target_name_id):
    """float64 model of hmsg_eval_semantic_ranks (include/hmsg.h): cosine of every class, rank of the best class that carries the
    target's name in the order of a stable ascending argsort read from its end.  Rows of the same bits get the same cosine (they are
    computed once).  A row of norm zero gives NaN, which numpy sorts above every number.  -> rank [n], cosines [n][C]"""
    emb, text = np.asarray(emb, np.float64), np.asarray(text, np.float64)
    C = len(text)
    uniq, inv = np.unique(text, axis=0, return_inverse=True)
    inv = np.asarray(inv).reshape(-1)
    names = np.asarray(class_name_id)
    ranks, sims = [], []
    with np.errstate(invalid="ignore", divide="ignore"):
        un = uniq / np.linalg.norm(uniq, axis=1, keepdims=True)
        for e, t in zip(emb, target_name_id):
            s = (un * (e / np.linalg.norm(e))[None, :]).sum(1)[inv]
            order = np.argsort(s, kind="stable")[::-1]
            where = np.flatnonzero(names[order] == t) if t >= 0 else []
            ranks.append(int(where[0]) if len(where) else C)
            sims.append(s)
    return np.array(ranks, np.int32), np.array(sims)
