"""Timing of N10 (include/hmsg.h: hmsg_nav_height_map, hmsg_nav_viewpoints_h, hmsg_nav_view_route_h), each beside the call it
extends, measured in the same run on the same inputs.  To be run on the MI355X, outside the test suite:

    python scripts/bench_nav_sight.py [--reps 10] [--batch 50] [--goals 1000] [--ref-goals 10] [--no-reference]
                                      [--kernel-stats <rocprofv3 kernel_stats.csv>] [--out profiles/nav_sight.json]

Height map: the storey of scripts/bench_nav_maps.py (10^6 points, 3 cm cells, about 801 x 501), device tensors in and out; a sample
is the host clock around --batch calls in a row divided by their number (a call is hmsg_nav_grid, then the work call, as for
hmsg_nav_floor_maps, which is timed the same way beside it), the best, the median and the worst of --reps samples after a warm-up
batch; the numpy restatement (tests/navsight_reference.py) once on the same host.
Sight: the map and the goals of scripts/bench_nav_view.py (500 x 700 cells, --goals goals), at 3 m (100 cells) and at the 255-cell
limit, hmsg_nav_viewpoints_h on three height maps against hmsg_nav_viewpoints on the flat map in the same run: "binary" (0 / 65535:
no height is read from the map), "mix" (walls at 65535, a twentieth of the free cells furniture of 0.4 to 1.6 m, eye 1.5 m, goals
at 0.2 to 1.8 m) and "between" (every cell's height strictly between the lower and the upper end of every ray and under it all the
way: every cell a line meets is read from the map and none blocks, the longest walks there are).  A sample is the host clock around
one call; two warm-up calls.  hmsg_nav_view_route_h beside hmsg_nav_view_route on the binary map.  Kernel times come from a run of
their own under `rocprofv3 --kernel-trace --stats -- python scripts/bench_nav_sight.py --no-reference`, whose csv a second call
folds in with --kernel-stats.  Writes profiles/nav_sight.json.
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--batch", type=int, default=50, help="calls per sample of the height map")
    ap.add_argument("--n", type=int, default=1000000)
    ap.add_argument("--goals", type=int, default=1000)
    ap.add_argument("--ref-goals", type=int, default=10)
    ap.add_argument("--no-reference", action="store_true")
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "nav_sight.json"))
    a = ap.parse_args()
    if a.kernel_stats:                                                                # fold a profiler run into the existing file
        res = json.load(open(a.out))
        rows = [r for r in csv.DictReader(open(a.kernel_stats)) if "k_nav" in r["Name"]]
        res["kernels"] = {r["Name"].split("(")[0]: dict(calls=int(r["Calls"]), total_us=int(r["TotalDurationNs"]) / 1e3,
                                                         mean_us=float(r["AverageNs"]) / 1e3) for r in rows}
        res["kernels_note"] = "rocprofv3 --kernel-trace --stats over a run of its own; totals are over all its calls"
        json.dump(res, open(a.out, "w"), indent=1)
        print(json.dumps(res["kernels"]))
        return
    import ctypes as C
    import torch
    from bench_nav_maps import storey
    from holoagent_amd import _lib
    from tests import navroute_cases as NC
    from tests import navsight_reference as SR
    if not torch.cuda.is_available():
        raise SystemExit("bench_nav_sight.py measures on the GPU: none found")
    L = _lib.HmsgLib()
    ld, limit = C.c_int32(0), C.c_int32(0)
    L.c.hmsg_test_nav_sight_layout(0, 0, C.byref(ld), C.byref(limit))
    res = dict(device=torch.cuda.get_device_name(0), lds_limit_per_workgroup=limit.value, lds_row_stride=ld.value)
    print("LDS per workgroup %d B, row stride %d" % (limit.value, ld.value), flush=True)

    # ---- the height map
    pts, cols, zero, poses = storey(a.n)
    d_pts, d_cols = torch.from_numpy(pts).cuda(), torch.from_numpy(cols).cuda()

    def batched(fn):
        out, ts = fn(), []
        for rep in range(a.reps + 1):                                                 # (sample 0 is the warm-up)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.batch):
                out = fn()
            ts.append((time.perf_counter() - t0) * 1e3 / a.batch)
        ts = ts[1:]
        return out, dict(ms_best=min(ts), ms_median=float(np.median(ts)), ms_worst=max(ts), samples=len(ts), calls_per_sample=a.batch)

    hm, t_h = batched(lambda: _lib.nav_height_map(d_pts, zero, lib_=L))
    _, t_m = batched(lambda: _lib.nav_floor_maps(d_pts, d_cols, zero, poses, lib_=L))
    _, t_m0 = batched(lambda: _lib.nav_floor_maps(d_pts, None, zero, poses, lib_=L))
    res["height_map"] = dict(n=len(pts), grid=list(hm["grid"]), **t_h, floor_maps=t_m, floor_maps_without_top_down=t_m0,
                             over_floor_maps=t_h["ms_median"] / t_m["ms_median"],
                             timing="host clock around calls_per_sample calls in a row with device tensors in and out, divided by their number; "
                                    "a call is hmsg_nav_grid, then the work call")
    print("height map %.3f ms (%.3f .. %.3f); floor maps %.3f ms, without the top-down image %.3f ms" %
          (t_h["ms_median"], t_h["ms_best"], t_h["ms_worst"], t_m["ms_median"], t_m0["ms_median"]), flush=True)
    if not a.no_reference:
        t0 = time.perf_counter()
        ref = SR.height_map_np(pts, zero, 0.03)
        ms = (time.perf_counter() - t0) * 1e3
        same = bool(np.array_equal(hm["top"].cpu().numpy(), ref[0]) and np.array_equal(hm["known"].cpu().numpy(), ref[1]))
        res["height_map"].update(reference_ms=ms, equal=same, reference="tests/navsight_reference.py: np.maximum.at and scipy's maximum_filter")
        print("reference %.0f ms, equal: %s" % (ms, same), flush=True)
        if not same:
            raise SystemExit("the library's height map differs from the reference's")

    # ---- sight
    m = np.array(NC.rooms_map(500, 700, 6), order="C")
    blk = (m == 0).astype(np.uint8)
    rng = np.random.default_rng(1)
    free = np.argwhere(m != 0)
    starts = free[rng.integers(0, len(free), 64)].astype(np.int32)                    # (the draws of bench_nav_view.py, in its order)
    goals = np.c_[rng.integers(0, 500, a.goals), rng.integers(0, 700, a.goals)].astype(np.int32)
    eye = 150
    tops = dict(binary=np.where(blk != 0, 65535, 0).astype(np.uint16),
                mix=np.where(blk != 0, 65535, np.where(rng.random(m.shape) < 0.05, rng.integers(40, 160, m.shape), 0)).astype(np.uint16),
                between=np.full(m.shape, 31, np.uint16))                              # T = the ray's lower end: "not low", not "tall",
    gh = dict(binary=np.full(a.goals, 90, np.int32), mix=rng.integers(20, 180, a.goals).astype(np.int32),      # under the ray at every inner cell
              between=np.full(a.goals, 33, np.int32))
    eyes = dict(binary=eye, mix=eye, between=31)
    d_m, d_blk, d_goals = torch.from_numpy(m).cuda(), torch.from_numpy(blk).cuda(), torch.from_numpy(goals).cuda()
    d_tops = {k: torch.from_numpy(v).cuda() for k, v in tops.items()}
    d_gh = {k: torch.from_numpy(v).cuda() for k, v in gh.items()}
    f0 = _lib.nav_distance_fields(d_m, [starts[:1]], lib_=L)[0][0]

    def timed(fn):
        for _ in range(2):
            out = fn()
        ts = []
        for _ in range(a.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        return out, dict(ms_best=min(ts), ms_median=float(np.median(ts)), ms_worst=max(ts), samples=len(ts))

    res["sight"] = dict(rows=500, cols=700, goals=a.goals, eye=eye,
                        timing="host clock around one call with device tensors in and out; every call ends in a stream synchronise; two warm-up calls")
    kept = {}
    for name, r_max in (("3m", 100), ("limit", 255)):
        flat, t_flat = timed(lambda: _lib.nav_viewpoints(d_blk, d_m, d_goals, field=f0, lib_=L, r_max2=r_max * r_max))
        everything, t_open = timed(lambda: _lib.nav_viewpoints(torch.zeros_like(d_blk), d_m, d_goals, field=f0, lib_=L, r_max2=r_max * r_max))
        res["sight"]["viewpoints_%s" % name] = dict(t_flat, visible_cells=int(flat["n_visible"].sum().item()))
        res["sight"]["viewpoints_%s_nothing_blocks" % name] = dict(t_open, visible_cells=int(everything["n_visible"].sum().item()))
        for kind in ("binary", "mix", "between"):
            v, t = timed(lambda: _lib.nav_viewpoints_h(d_tops[kind], d_m, d_goals, eyes[kind], d_gh[kind], field=f0, lib_=L, r_max2=r_max * r_max))
            base = t_open if kind == "between" else t_flat
            res["sight"]["viewpoints_h_%s_%s" % (name, kind)] = dict(t, visible_cells=int(v["n_visible"].sum().item()),
                                                                      over_viewpoints=t["ms_median"] / base["ms_median"],
                                                                      beside="viewpoints_%s%s" % (name, "_nothing_blocks" if kind == "between" else ""))
            kept[name, kind] = v
        assert all(bool(torch.equal(kept[name, "binary"][q], flat[q])) for q in ("view_rc", "view_d2", "view_dist", "n_visible"))
        assert bool(torch.equal(kept[name, "between"]["n_visible"], everything["n_visible"]))
    old, t_old = timed(lambda: _lib.nav_view_route(d_m, d_blk, starts[0], d_goals, lib_=L, min_clearance=42, r_max2=100 * 100))
    new, t_new = timed(lambda: _lib.nav_view_route_h(d_m, d_tops["binary"], starts[0], d_goals, eye, d_gh["binary"], lib_=L, min_clearance=42,
                                                     r_max2=100 * 100))
    assert bool(torch.equal(old["goal_cell"], new["goal_cell"])) and bool(torch.equal(old["path_rc"], new["path_rc"]))
    res["sight"]["view_route_3m_min_clearance_42"] = t_old
    res["sight"]["view_route_h_3m_min_clearance_42"] = dict(t_new, over_view_route=t_new["ms_median"] / t_old["ms_median"])
    for k, v in res["sight"].items():
        if isinstance(v, dict) and "ms_median" in v:
            print("%-40s %8.3f ms median (%.3f .. %.3f)%s" % (k, v["ms_median"], v["ms_best"], v["ms_worst"],
                                                             "  x%.2f" % v["over_viewpoints"] if "over_viewpoints" in v else ""), flush=True)
    if not a.no_reference:
        k, h_f = min(a.ref_goals, a.goals), f0.cpu().numpy()
        t0 = time.perf_counter()
        r = SR.viewpoints_h(tops["mix"], m, goals[:k], 0, 100 * 100, eye, gh["mix"][:k], None, h_f, 0)
        ms = (time.perf_counter() - t0) * 1e3
        same = all(bool(np.array_equal(kept["3m", "mix"][q].cpu().numpy()[:k], r[q])) for q in ("view_rc", "view_d2", "view_dist", "n_visible"))
        res["sight"]["reference_3m_mix"] = dict(goals=k, ms=ms, ms_scaled_to_all_goals=ms * a.goals / max(k, 1), equal=same,
                                               what="tests/navsight_reference.py: numpy over the candidates, goal by goal")
        print("reference 3m mix: %d goals %.0f ms, equal: %s" % (k, ms, same), flush=True)
        if not same:
            raise SystemExit("the library's viewpoints differ from the reference's")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
