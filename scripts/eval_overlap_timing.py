#!/usr/bin/env python
"""Times hmsg_cloud_set_overlaps (holoagent_amd/csrc/hmsg_eval.hip: both sets sorted once by (cloud, cell), a 27-cell probe per query
point) against the only route the library had for find_overlapping_ratio_faiss on arbitrary clouds, the exhaustive
hmsg_pair_overlaps (hmsg_objmerge.hip, behind the hook hmsg_test_pair_overlaps), on the same pairs of one synthetic evaluation:
predicted object clouds against ground-truth mesh samples, the pairs those whose axis-aligned boxes intersect, radius 0.02 as in
evaluate_objects (memory/hmsg/eval/hm3dsem_evaluator.py).

Both routes run in one process, alternating, `--rounds` rounds after a warm-up; each call ends in a stream synchronise inside the
library and is timed with the host clock around it; the points are in device memory for both.  Both must return the same counts
before a time is reported.  One more call with the library's event brackets on gives the probe kernel's own time, set against the
bytes computed from the shapes.  Writes profiles/eval_overlap_timing.json.  Needs the GPU: there is no CPU path."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def box_surface(rng, lo, hi, n):
    p = rng.uniform(lo, hi, (n, 3))
    axis, side = rng.integers(0, 3, n), rng.integers(0, 2, n)
    p[np.arange(n), axis] = np.where(side == 0, lo[axis], hi[axis])
    return p


def scene(n_gt, n_pred, gt_points, pred_points, seed):
    """ground truth: box surfaces sampled with gt_points[0] .. gt_points[1] points in a 20 x 3 x 16 m storey; predictions: the
    objects seen again (shifted by up to 3 cm, a third of them from one side only) with pred_points[0] .. [1] points"""
    rng = np.random.default_rng(seed)
    gt, box = [], []
    for _ in range(n_gt):
        c = rng.uniform((0.5, 0.2, 0.5), (19.5, 2.0, 15.5))
        half = rng.uniform(0.15, 0.75, 3)
        gt.append(box_surface(rng, c - half, c + half, int(rng.integers(gt_points[0], gt_points[1] + 1))))
        box.append((c - half, c + half))
    pred = []
    for k in range(n_pred):
        lo, hi = box[k % n_gt]
        p = box_surface(rng, lo, hi, int(rng.integers(pred_points[0], pred_points[1] + 1))) + rng.uniform(-0.03, 0.03, 3)
        if k % 3 == 0:
            p = p[p[:, 0] < np.median(p[:, 0])]
        pred.append(p)
    pairs = []
    glo, ghi = np.array([g.min(0) for g in gt]), np.array([g.max(0) for g in gt])
    for a, p in enumerate(pred):
        hit = ((p.min(0) <= ghi) & (glo <= p.max(0))).all(1)
        pairs += [(a, int(b)) for b in np.flatnonzero(hit)]
    return pred, gt, np.array(pairs, np.int32)


def csr(clouds):
    off = np.zeros(len(clouds) + 1, np.int64)
    off[1:] = np.cumsum([len(c) for c in clouds])
    return np.ascontiguousarray(np.concatenate(clouds), np.float64), off


def quantiles(ms):
    v = np.sort(np.asarray(ms, np.float64))
    return {"median_ms": float(np.median(v)), "p10_ms": float(np.quantile(v, 0.1)), "p90_ms": float(np.quantile(v, 0.9)), "samples_ms": [float(x) for x in ms]}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--gt", type=int, default=192)
    ap.add_argument("--pred", type=int, default=256)
    ap.add_argument("--gt-points", type=int, nargs=2, default=(10000, 40000))
    ap.add_argument("--pred-points", type=int, nargs=2, default=(2000, 8000))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval_overlap_timing.json"))
    args = ap.parse_args()

    import torch
    from holoagent_amd._lib import HmsgLib, Scene
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this script measures, it does not fall back")
    L = HmsgLib()
    sc = Scene(lib_=L, height=8, width=8, max_frames=1, max_masks=1, feat_dim=16)       # default distance form
    pred, gt, pairs = scene(args.gt, args.pred, args.gt_points, args.pred_points, args.seed)
    radius = 0.02
    pa, oa = csr(pred)
    pb, ob = csr(gt)
    joint_pts = torch.from_numpy(np.concatenate([pa, pb])).cuda()
    d_pa, d_pb = joint_pts[:len(pa)], joint_pts[len(pa):]
    joint_off = np.concatenate([oa, ob[1:] + oa[-1]])
    joint_pairs = np.ascontiguousarray(pairs + np.array([0, len(pred)], np.int32))
    torch.cuda.synchronize()

    def new_route():
        return sc.cloud_set_overlaps(d_pa, oa, d_pb, ob, pairs, radius)

    def old_route():
        out = np.zeros((len(pairs), 2), np.uint32)
        rc = L.c.hmsg_test_pair_overlaps(sc.h, len(pred) + len(gt), joint_pts.data_ptr(), joint_off.ctypes.data, len(pairs), joint_pairs.ctypes.data,
                                         radius, out.ctypes.data)
        if rc != 0:
            raise SystemExit("hmsg_test_pair_overlaps failed: %d" % rc)
        return out

    a, b = new_route(), old_route()                     # warm-up, and the check that comes before any time
    if not np.array_equal(a, b):
        bad = np.flatnonzero((a != b).any(1))
        raise SystemExit("the two routes disagree on %d of %d pairs, first %s: %s against %s" % (len(bad), len(pairs), pairs[bad[0]].tolist(),
                                                                                                a[bad[0]].tolist(), b[bad[0]].tolist()))
    t_new, t_old = [], []
    for _ in range(args.rounds):
        t0 = time.perf_counter()
        new_route()
        t1 = time.perf_counter()
        old_route()
        t2 = time.perf_counter()
        t_new.append((t1 - t0) * 1e3)
        t_old.append((t2 - t1) * 1e3)
    sc.set_profiling(True)
    new_route()
    prof = {k: {"launches": v[0], "ms": v[1], "bytes": v[2]} for k, v in sc.profile().items() if k.startswith("k_ev_")}
    sc.set_profiling(False)
    n_a = np.array([len(pred[i]) for i in pairs[:, 0]], np.float64)
    n_b = np.array([len(gt[i]) for i in pairs[:, 1]], np.float64)
    res = {
        "what": "hmsg_cloud_set_overlaps against hmsg_pair_overlaps on the same pairs, alternating in one process, default distance form",
        "device": torch.cuda.get_device_name(0),
        "radius": radius,
        "clouds": {"pred": len(pred), "gt": len(gt), "pred_points": int(oa[-1]), "gt_points": int(ob[-1])},
        "pairs": int(len(pairs)),
        "points_per_side_of_a_pair": {"pred_median": float(np.median(n_a)), "gt_median": float(np.median(n_b)),
                                      "exhaustive_distance_evaluations": float(2.0 * (n_a * n_b).sum())},
        "counts_equal": True,
        "pairs_with_overlap": int((a.sum(1) > 0).sum()),
        "rounds": args.rounds,
        "cloud_set_overlaps": quantiles(t_new),
        "pair_overlaps": quantiles(t_old),
        "kernels": prof,
    }
    res["new_p90_below_old_p10"] = res["cloud_set_overlaps"]["p90_ms"] < res["pair_overlaps"]["p10_ms"]
    res["ratio_of_medians"] = res["pair_overlaps"]["median_ms"] / res["cloud_set_overlaps"]["median_ms"]
    if "k_ev_probe" in prof and prof["k_ev_probe"]["ms"] > 0:
        k = prof["k_ev_probe"]
        res["probe_bytes_per_second"] = k["bytes"] / (k["ms"] * 1e-3)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    sc.close()


if __name__ == "__main__":
    main()
