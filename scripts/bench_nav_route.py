"""Timing of the routing calls (include/hmsg.h, N7) on one storey of 700 x 500 cells against scipy's Dijkstra on the same map on the
same host (tests/navroute_reference.py, never the code under test).  To be run on the MI355X, outside the test suite:

    python scripts/bench_nav_route.py [--reps 10] [--goals 1000] [--no-reference] [--out profiles/nav_route.json]

Map: the rooms-and-doors generator of tests/navroute_cases.py at 500 rows x 700 columns (walls every 37 cells, 4-cell doors, 3 %
clutter).  Each of the four calls and the composition is timed with device tensors in and out: hmsg_nav_clearance;
hmsg_nav_distance_fields with 1, 8 and 64 starts in one call; hmsg_nav_snap_cells and hmsg_nav_paths with --goals goals;
hmsg_nav_route with --goals goals at min_clearance 0 and 42 (0.25 m).  A call returns when its outputs are complete (it ends in a
stream synchronise), so a sample is the host clock around one call; after two warm-up calls the best, the median and the worst of
--reps samples are reported.  Beside them: the relaxation rounds and host round trips of a field on this map and on the 130 x 130
serpentine, and -- unless --no-reference -- scipy's time for one field and whether it equals the library's.  Writes
profiles/nav_route.json.
"""
from __future__ import annotations

import argparse
import ctypes as C
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
    ap.add_argument("--no-reference", action="store_true")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "nav_route.json"))
    a = ap.parse_args()
    import torch
    from holoagent_amd import _lib
    from tests import navroute_cases as NC
    from tests import navroute_reference as RR
    if not torch.cuda.is_available():
        raise SystemExit("bench_nav_route.py measures on the GPU: none found")
    L = _lib.HmsgLib()
    m = np.array(NC.rooms_map(500, 700, 6), order="C")                               # (a copy: the shared map is read-only)
    rng = np.random.default_rng(1)
    free = np.argwhere(m != 0)
    starts = free[rng.integers(0, len(free), 64)].astype(np.int32)
    goals = np.c_[rng.integers(0, 500, a.goals), rng.integers(0, 700, a.goals)].astype(np.int32)
    d_m, d_goals = torch.from_numpy(m).cuda(), torch.from_numpy(goals).cuda()

    def last():
        r, t = C.c_int32(0), C.c_int32(0)
        L.c.hmsg_test_nav_route_last(C.byref(r), C.byref(t))
        return dict(rounds=r.value, host_round_trips=t.value)

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
    _, res["clearance"] = timed(lambda: _lib.nav_clearance(d_m, lib_=L))
    res["clearance"].update(last())
    fields = None
    for n in (1, 8, 64):
        (fields, _), res["distance_fields_%d" % n] = timed(lambda: _lib.nav_distance_fields(d_m, [starts[k:k + 1] for k in range(n)], lib_=L))
        res["distance_fields_%d" % n].update(last())
    f0 = _lib.nav_distance_fields(d_m, [starts[:1]], lib_=L)[0][0]
    res["field_rooms"] = last()
    (cells, _), res["snap_cells"] = timed(lambda: _lib.nav_snap_cells(d_m, d_goals, f0, lib_=L))
    (off, _), res["paths"] = timed(lambda: _lib.nav_paths(d_m, f0, cells, lib_=L))
    res["paths"]["path_cells"] = int(off[-1])
    for minc in (0, 42):
        r, res["route_min_clearance_%d" % minc] = timed(lambda: _lib.nav_route(d_m, starts[0], d_goals, lib_=L, min_clearance=minc))
        res["route_min_clearance_%d" % minc].update(path_cells=int(len(r["path_rc"])), reached=int((r["goal_dist"].cpu().numpy() != RR.UNREACHED).sum()))
    s = np.array(NC.serpentine_map(), order="C")
    fs, res["field_serpentine"] = timed(lambda: _lib.nav_distance_fields(torch.from_numpy(s).cuda(), [[(0, 0)]], lib_=L))
    res["field_serpentine"].update(last())
    for k, v in res.items():
        if isinstance(v, dict) and "ms_median" in v:
            print("%-24s %8.3f ms median (%.3f .. %.3f) %s" % (k, v["ms_median"], v["ms_best"], v["ms_worst"],
                                                               {q: v[q] for q in ("rounds", "host_round_trips") if q in v}), flush=True)
    if not a.no_reference:
        t0 = time.perf_counter()
        g = RR.grid_graph(m)
        t1 = time.perf_counter()
        ref, _ = RR.field(m, starts[:1], graph=g)
        t2 = time.perf_counter()
        same = bool(np.array_equal(f0.cpu().numpy(), ref)) and bool(np.array_equal(fs[0][0].cpu().numpy(), RR.field(s, [(0, 0)])[0]))
        res["reference"] = dict(what="tests/navroute_reference.py: scipy.sparse.csgraph.dijkstra(min_only=True) on the grid graph, one field",
                                graph_build_ms=(t1 - t0) * 1e3, dijkstra_ms=(t2 - t1) * 1e3, fields_equal=same)
        print("reference: graph %.0f ms, dijkstra %.0f ms, equal: %s" % ((t1 - t0) * 1e3, (t2 - t1) * 1e3, same), flush=True)
        if not same:
            raise SystemExit("the library's field differs from the reference's")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
