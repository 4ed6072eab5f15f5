"""Timing of the k-NN label transfer of the semantic segmentation score (include/hmsg.h: hmsg_knn_labels) against the reference's
route on the same host: sklearn's BallTree.query plus the np.bincount loop of knn_interpolation (eval_utils.py:308-339).  To be run
on the MI355X, outside the test suite:

    python scripts/bench_semseg_eval.py [--n 1000000] [--m 3000000] [--k 5] [--classes 40] [--reps 3] [--no-sklearn]

Scene: n labelled points uniform in two boxes of 4 x 3 x 4 m with 4 m of empty space between them, m queries uniform over the
bounding box of both (a third of them in the empty region: ground-truth vertices where nothing was mapped).  The library is timed with
device tensors in and out (wall time of the call, which returns when the labels are complete; the best of --reps after a warm-up).
The labels of both routes are compared; the share of queries that the lattice walk handed to the scan (phase 2) is reported.
Writes profiles/semseg_eval.json.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, REPO)


def scene(n, m, classes, seed=7):
    rng = np.random.default_rng(seed)
    pts = rng.random((n, 3)) * np.array([4.0, 3.0, 4.0])
    pts[n // 2:, 0] += 8.0
    lab = rng.integers(0, classes, n).astype(np.int32)
    q = rng.random((m, 3)) * np.array([12.0, 3.0, 4.0])
    return pts, lab, q


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1000000)
    ap.add_argument("--m", type=int, default=3000000)
    ap.add_argument("--k", type=int, default=5)
    ap.add_argument("--classes", type=int, default=40)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-sklearn", action="store_true")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "semseg_eval.json"))
    a = ap.parse_args()
    import torch
    from holoagent_amd._lib import HmsgLib, Scene
    pts, lab, q = scene(a.n, a.m, a.classes)
    sc = Scene(lib_=HmsgLib(), height=8, width=8, max_frames=1, max_masks=1, feat_dim=16)
    d_pts, d_lab, d_q = torch.from_numpy(pts).cuda(), torch.from_numpy(lab).cuda(), torch.from_numpy(q).cuda()
    d_out = torch.empty(a.m, dtype=torch.int32, device="cuda")
    sc.set_profiling(True)
    times = []
    for rep in range(a.reps + 1):                             # (the first call pays for the allocations)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        sc.knn_labels(d_pts, d_lab, d_q, a.k, out=d_out)
        times.append((time.perf_counter() - t0) * 1e3)
    phase2 = sc.knn_last_phase2()
    print("hmsg_knn_labels: %s ms, %d of %d queries in phase 2" % (["%.1f" % t for t in times], phase2, a.m), flush=True)
    got = d_out.cpu().numpy()
    res = dict(n=a.n, m=a.m, k=a.k, classes=a.classes, device=torch.cuda.get_device_name(0), knn_labels_ms=min(times[1:]),
               knn_labels_first_call_ms=times[0], knn_labels_all_ms=times, phase2_queries=int(phase2), phase2_share=phase2 / a.m)
    if hasattr(sc, "profile"):
        try:
            res["kernels_ms"] = {k: v for k, v in sc.profile().items() if k.startswith("k_ss_")}
        except Exception:
            pass
    if not a.no_sklearn:
        from sklearn.neighbors import BallTree
        threads = int(os.environ.get("OMP_NUM_THREADS", "0")) or None
        t0 = time.perf_counter()
        tree = BallTree(pts, metric="minkowski")
        t1 = time.perf_counter()
        idx = np.empty((a.m, a.k), np.int64)
        for c0 in range(0, a.m, 250000):                      # (in chunks only to show progress; the tree is built once)
            idx[c0:c0 + 250000] = tree.query(q[c0:c0 + 250000], k=a.k)[1]
            print("sklearn: %d of %d queries, %.1f s" % (min(c0 + 250000, a.m), a.m, time.perf_counter() - t1), flush=True)
        t2 = time.perf_counter()
        knn_classes = lab[idx].astype(int)
        ref = np.zeros(a.m, np.int32)
        for i in range(a.m):
            ref[i] = np.bincount(knn_classes[i]).argmax()
        t3 = time.perf_counter()
        res.update(sklearn_build_ms=(t1 - t0) * 1e3, sklearn_query_ms=(t2 - t1) * 1e3, sklearn_vote_loop_ms=(t3 - t2) * 1e3,
                   sklearn_total_ms=(t3 - t0) * 1e3, sklearn_threads="BallTree.query is single-threaded (OMP_NUM_THREADS=%s)" % threads,
                   labels_equal=bool(np.array_equal(got, ref)), labels_differ=int((got != ref).sum()),
                   speedup=(t3 - t0) * 1e3 / min(times[1:]))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))
    sc.close()


if __name__ == "__main__":
    main()
