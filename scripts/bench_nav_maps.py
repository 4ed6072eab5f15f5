"""Timing of the navigation maps of one storey (include/hmsg.h: hmsg_nav_floor_maps) against the reference's route on the same host:
the numpy / scipy restatement of tests/navmap_reference.py, its per-point Python loop for the top-down image included.  To be run
on the MI355X, outside the test suite:

    python scripts/bench_nav_maps.py [--n 1000000] [--reps 10] [--batch 100] [--no-reference] [--kernel-stats <rocprofv3 kernel_stats.csv>]

Scene: a walled storey of 24 x 15 m with cupboards, n points, 40 poses; 3 cm cells (about 800 x 500).  The library is timed with
device tensors in and out.  A call returns when every map is complete, so a sample is the host clock around --batch calls in a row
(a fifth of a second at the default: one call of 2 ms would measure the clock and the scheduler as much as the stage) divided by
their number; the best, the median and the spread of --reps samples after a warm-up batch are reported.  Both routes must return
the same arrays, or the script fails.  Kernel times come from a run of their own
under `rocprofv3 --kernel-trace --stats -- python scripts/bench_nav_maps.py --no-reference`, whose csv a second call folds in with
--kernel-stats.  Writes profiles/nav_maps.json.
"""
from __future__ import annotations

import argparse
import csv
import json
import os
import sys
import time

import numpy as np

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, REPO)


def storey(n, seed=3, size_x=24.0, size_z=15.0):
    rng = np.random.default_rng(seed)
    nf, nw = n * 6 // 10, n * 3 // 10
    nb = n - nf - nw
    fl = np.c_[rng.uniform(0, size_x, nf), rng.uniform(0.0, 0.03, nf), rng.uniform(0, size_z, nf)]
    t, side = rng.uniform(0, 1, nw), rng.integers(0, 6, nw)                           # four outer walls and two inner ones with a door
    wx = np.where(side == 0, 0.0, np.where(side == 1, size_x, np.where(side == 4, size_x / 3, np.where(side == 5, 2 * size_x / 3, t * size_x))))
    wz = np.where((side < 2) | (side > 3), t * size_z, np.where(side == 2, 0.0, size_z))
    wall = np.c_[wx, rng.uniform(0.0, 2.7, nw), wz]
    wall = wall[~((side > 3) & (np.abs(wz - size_z / 2) < 0.5) & (wall[:, 1] < 2.0))]
    c = rng.integers(0, 12, nb)                                                       # cupboards
    box = np.c_[1.5 + (c % 4) * 6.0 + rng.uniform(0, 0.8, nb), rng.uniform(0.0, 2.2, nb), 2.0 + (c // 4) * 4.5 + rng.uniform(0, 1.4, nb)]
    pts = np.concatenate([fl, wall, box])
    pts = np.ascontiguousarray(pts[rng.permutation(len(pts))])
    cols = rng.uniform(0, 1, pts.shape)
    poses = np.tile(np.eye(4), (40, 1, 1))
    poses[:, 0, 3], poses[:, 1, 3], poses[:, 2, 3] = rng.uniform(1, size_x - 1, 40), 0.8 + rng.uniform(-0.01, 0.01, 40), rng.uniform(1, size_z - 1, 40)
    return pts, cols, 0.0, poses


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1000000)
    ap.add_argument("--reps", type=int, default=10, help="timed samples")
    ap.add_argument("--batch", type=int, default=100, help="calls per sample")
    ap.add_argument("--no-reference", action="store_true")
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "nav_maps.json"))
    a = ap.parse_args()
    if a.kernel_stats:                                                                # fold a profiler run into the existing file
        res = json.load(open(a.out))
        rows = [r for r in csv.DictReader(open(a.kernel_stats)) if r["Name"].startswith(("k_nav_", "k_spcc_"))]
        res["kernels"] = {r["Name"].split("(")[0]: dict(calls=int(r["Calls"]), total_us=int(r["TotalDurationNs"]) / 1e3,
                                                         mean_us=float(r["AverageNs"]) / 1e3) for r in rows}
        res["kernels_note"] = "rocprofv3 --kernel-trace --stats over a run of its own; totals are over all its calls"
        json.dump(res, open(a.out, "w"), indent=1)
        print(json.dumps(res["kernels"]))
        return
    import torch
    from holoagent_amd._lib import HmsgLib, nav_floor_maps
    if not torch.cuda.is_available():
        raise SystemExit("bench_nav_maps.py measures on the GPU: none found")
    L = HmsgLib()
    pts, cols, zero, poses = storey(a.n)
    d_pts, d_cols = torch.from_numpy(pts).cuda(), torch.from_numpy(cols).cuda()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    got = nav_floor_maps(d_pts, d_cols, zero, poses, lib_=L)                          # (the first call pays for the allocations)
    first = (time.perf_counter() - t0) * 1e3
    times = []
    for rep in range(a.reps + 1):                                                     # (sample 0 is the warm-up)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.batch):
            got = nav_floor_maps(d_pts, d_cols, zero, poses, lib_=L)                  # (returns after the library's own synchronise)
        times.append((time.perf_counter() - t0) * 1e3 / a.batch)
    times = times[1:]
    print("hmsg_nav_floor_maps: %s ms a call (samples of %d calls), grid %s" % (["%.3f" % t for t in times], a.batch, got["grid"]), flush=True)
    res = dict(n=len(pts), grid=list(got["grid"]), n_boundary=int(len(got["boundary_rc"])), device=torch.cuda.get_device_name(0),
               calls_per_sample=a.batch, call_ms_best=min(times), call_ms_median=float(np.median(times)), call_ms_worst=max(times),
               call_ms_first=first, call_ms_samples=times,
               timing="host clock around calls_per_sample calls in a row with device tensors in and out, divided by their number; every "
                      "call ends in a stream synchronise; a call is hmsg_nav_grid, then hmsg_nav_floor_maps")
    if not a.no_reference:
        from tests import navmap_reference as NR
        t0 = time.perf_counter()
        ref = NR.floor_maps(pts, cols, zero, poses)
        res["reference_ms"] = (time.perf_counter() - t0) * 1e3
        same = {k: bool(np.array_equal(got[k].cpu().numpy(), ref[k])) for k in
                ("obstacle_map", "region_map", "poses_map", "free_map", "main_free_map", "top_down_bgr", "boundary_rc")}
        res.update(arrays_equal=same, speedup=res["reference_ms"] / res["call_ms_best"],
                   reference="tests/navmap_reference.py: numpy / scipy / sklearn, the per-point loop of get_top_down_rgb_map included")
        print("reference: %.0f ms, equal: %s" % (res["reference_ms"], same), flush=True)
        if not all(same.values()):
            raise SystemExit("the two routes differ: %s" % same)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
