"""Timing of the viewpoint calls (include/hmsg.h, N8) on one storey of 700 x 500 cells against the vectorised numpy restatement on
the same map on the same host (tests/navview_reference.py, never the code under test).  To be run on the MI355X, outside the test
suite:

    python scripts/bench_nav_view.py [--reps 10] [--goals 1000] [--ref-goals 20] [--no-reference] [--out profiles/nav_view.json]

Map and goals: those of scripts/bench_nav_route.py (the rooms-and-doors generator of tests/navroute_cases.py at 500 rows x 700
columns, --goals goals anywhere in the image); what blocks the sight is the map's complement.  Timed with device tensors in and out:
hmsg_nav_viewpoints on the start's field with a range of 3 m (100 cells) and at the 255-cell limit, with and without the field;
hmsg_nav_view_route at the 3 m range beside hmsg_nav_route on the same inputs, at min_clearance 0 and 42 (0.25 m).  A call returns
when its outputs are complete (it ends in a stream synchronise), so a sample is the host clock around one call; after two warm-up
calls the best, the median and the worst of --reps samples are reported.  Beside them -- unless --no-reference -- the restatement's
time for the first --ref-goals goals at each range, scaled to --goals, and whether it equals the library's answer for them.
Writes profiles/nav_view.json.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--goals", type=int, default=1000)
    ap.add_argument("--ref-goals", type=int, default=20)
    ap.add_argument("--no-reference", action="store_true")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "nav_view.json"))
    a = ap.parse_args()
    import torch
    from holoagent_amd import _lib
    from tests import navroute_cases as NC
    from tests import navroute_reference as RR
    from tests import navview_reference as VR
    if not torch.cuda.is_available():
        raise SystemExit("bench_nav_view.py measures on the GPU: none found")
    L = _lib.HmsgLib()
    m = np.array(NC.rooms_map(500, 700, 6), order="C")                               # (a copy: the shared map is read-only)
    blk = (m == 0).astype(np.uint8)
    rng = np.random.default_rng(1)
    free = np.argwhere(m != 0)
    starts = free[rng.integers(0, len(free), 64)].astype(np.int32)                    # (the draws of bench_nav_route.py, in its order)
    goals = np.c_[rng.integers(0, 500, a.goals), rng.integers(0, 700, a.goals)].astype(np.int32)
    d_m, d_blk, d_goals = torch.from_numpy(m).cuda(), torch.from_numpy(blk).cuda(), torch.from_numpy(goals).cuda()
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

    res = dict(rows=500, cols=700, passable_cells=int((m != 0).sum()), goals=a.goals, device=torch.cuda.get_device_name(0),
               timing="host clock around one call with device tensors in and out; every call ends in a stream synchronise; two warm-up calls")
    views = {}
    for name, r_max in (("3m", 100), ("limit", 255)):
        for fld, tag in ((f0, "field"), (None, "no_field")):
            key = "viewpoints_%s_%s" % (name, tag)
            v, res[key] = timed(lambda: _lib.nav_viewpoints(d_blk, d_m, d_goals, field=fld, lib_=L, r_max2=r_max * r_max))
            nv = v["n_visible"].cpu().numpy()
            res[key].update(r_max2=r_max * r_max, goals_with_a_view=int((nv > 0).sum()), visible_cells=int(nv.sum()))
            views[key] = v
    for minc in (0, 42):
        old, res["route_min_clearance_%d" % minc] = timed(lambda: _lib.nav_route(d_m, starts[0], d_goals, lib_=L, min_clearance=minc))
        new, res["view_route_3m_min_clearance_%d" % minc] = timed(
            lambda: _lib.nav_view_route(d_m, d_blk, starts[0], d_goals, lib_=L, min_clearance=minc, r_max2=100 * 100))
        res["route_min_clearance_%d" % minc].update(path_cells=int(len(old["path_rc"])), reached=int((old["goal_dist"].cpu().numpy() != RR.UNREACHED).sum()))
        oc, nc = old["goal_cell"].cpu().numpy(), new["goal_cell"].cpu().numpy()
        res["view_route_3m_min_clearance_%d" % minc].update(
            path_cells=int(len(new["path_rc"])), with_a_view=int((new["goal_dist"].cpu().numpy() != RR.UNREACHED).sum()),
            goals_moved=int((oc != nc).any(axis=1).sum()), over_route=res["view_route_3m_min_clearance_%d" % minc]["ms_median"] /
            res["route_min_clearance_%d" % minc]["ms_median"])
    for k, v in res.items():
        if isinstance(v, dict) and "ms_median" in v:
            print("%-34s %8.3f ms median (%.3f .. %.3f)" % (k, v["ms_median"], v["ms_best"], v["ms_worst"]), flush=True)
    if not a.no_reference:
        k, h_f = min(a.ref_goals, a.goals), f0.cpu().numpy()
        ref = {}
        for name, r_max in (("3m", 100), ("limit", 255)):
            t0 = time.perf_counter()
            r = VR.viewpoints(blk, m, goals[:k], 0, r_max * r_max, h_f, 0)
            ms = (time.perf_counter() - t0) * 1e3
            got = views["viewpoints_%s_field" % name]
            same = all(bool(np.array_equal(got[q].cpu().numpy()[:k], r[q])) for q in ("view_rc", "view_d2", "view_dist", "n_visible"))
            ref[name] = dict(goals=k, ms=ms, ms_scaled_to_all_goals=ms * a.goals / max(k, 1), equal=same)
            print("reference %s: %d goals %.0f ms (%.0f ms for %d), equal: %s" % (name, k, ms, ms * a.goals / max(k, 1), a.goals, same), flush=True)
        res["reference"] = dict(what="tests/navview_reference.py: numpy over the candidates, one array step per line index, goal by goal", **ref)
        if not all(v["equal"] for v in ref.values()):
            raise SystemExit("the library's viewpoints differ from the reference's")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
