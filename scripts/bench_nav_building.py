"""Timing of the calls that route across storeys (include/hmsg.h, N9) on buildings of two and three storeys of 500 x 700 cells
against the single-storey fields of hmsg_nav_distance_fields on the same storeys (the floor: it ignores the links) and scipy's
Dijkstra on the layered graph on the same host (tests/navbuilding_reference.py, never the code under test).  To be run on the
MI355X, outside the test suite:

    python scripts/bench_nav_building.py [--reps 10] [--goals 1000] [--no-reference] [--kernel-stats a_kernel_stats.csv]
                                         [--out profiles/nav_building.json]

Storeys: the rooms-and-doors generator of tests/navroute_cases.py at 500 rows x 700 columns with seeds 6, 7, 8.  Links: 1, 4 or 16
per pair of consecutive storeys, between free cells drawn at random, cost 60.  (a) hmsg_nav_building_fields for 1 and 64 starts
with device tensors in and out, beside the sum of hmsg_nav_distance_fields on each storey alone for as many starts and, for one
start, scipy's Dijkstra; (b) the rounds and host round trips of every such call from hmsg_test_nav_building_last, beside
hmsg_test_nav_route_last's for the single storeys; 64 starts in one call beside 64 calls of one start; (c)
hmsg_nav_building_route to --goals goals spread over the storeys.  A call returns when its outputs are complete (it ends in a stream
synchronise), so a sample is the host clock around one call; after two warm-up calls the best, the median and the worst of --reps
samples are reported.  --kernel-stats folds the csv of a separate `rocprofv3 --kernel-trace --stats` run of this script in (a run
of its own: no counters beside the trace).  Writes profiles/nav_building.json.
"""
from __future__ import annotations

import argparse
import csv
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
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "nav_building.json"))
    a = ap.parse_args()
    import torch
    from holoagent_amd import _lib
    from tests import navbuilding_reference as RB
    from tests import navroute_cases as NC
    if not torch.cuda.is_available():
        raise SystemExit("bench_nav_building.py measures on the GPU: none found")
    L = _lib.HmsgLib()
    maps = [np.array(NC.rooms_map(500, 700, seed), order="C") for seed in (6, 7, 8)]
    d_maps = [torch.from_numpy(m).cuda() for m in maps]
    free = [np.argwhere(m != 0) for m in maps]
    rng = np.random.default_rng(1)

    def links_of(n_storeys, per_pair):
        r = np.random.default_rng(100 + per_pair)
        out = []
        for l in range(n_storeys - 1):
            for _ in range(per_pair):
                out.append((l,) + tuple(free[l][r.integers(0, len(free[l]))]) + (l + 1,) + tuple(free[l + 1][r.integers(0, len(free[l + 1]))]) + (60,))
        return np.array(out, np.int32)

    def last(fn):
        r, t = C.c_int32(0), C.c_int32(0)
        getattr(L.c, fn)(C.byref(r), C.byref(t))
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

    res = dict(rows=500, cols=700, passable_cells=[int((m != 0).sum()) for m in maps], goals=a.goals, link_cost=60,
               device=torch.cuda.get_device_name(0),
               timing="host clock around one call with device tensors in and out; every call ends in a stream synchronise; two warm-up calls")
    starts = np.c_[np.zeros(64, np.int64), free[0][rng.integers(0, len(free[0]), 64)]].astype(np.int32)
    # the floor: every storey alone, the links ignored (for the storeys above the start: a start of their own)
    res["single_storeys"] = {}
    for n in (1, 64):
        total, rounds = 0.0, []
        for l in range(3):
            own = free[l][rng.integers(0, len(free[l]), n)].astype(np.int32) if l else starts[:n, 1:]
            _, t = timed(lambda: _lib.nav_distance_fields(d_maps[l], [own[k:k + 1] for k in range(n)], lib_=L))
            t.update(last("hmsg_test_nav_route_last"))
            res["single_storeys"]["storey_%d_starts_%d" % (l, n)] = t
    for ns in (2, 3):
        for per_pair in (1, 4, 16):
            links = links_of(ns, per_pair)
            key = "storeys_%d_links_%d" % (ns, len(links))
            entry = dict(n_links=int(len(links)))
            for n in (1, 64):
                (fields, reached), t = timed(lambda: _lib.nav_building_fields(d_maps[:ns], links, starts[:n], lib_=L))
                t.update(last("hmsg_test_nav_building_last"))
                t["floor_ms_median"] = sum(res["single_storeys"]["storey_%d_starts_%d" % (l, n)]["ms_median"] for l in range(ns))
                t["reached_cells_start_0"] = [int(v) for v in reached[0].cpu().numpy()]
                entry["fields_starts_%d" % n] = t
                print("%-24s starts %2d %9.3f ms median (%.3f .. %.3f) rounds %d trips %d floor %.3f ms" %
                      (key, n, t["ms_median"], t["ms_best"], t["ms_worst"], t["rounds"], t["host_round_trips"], t["floor_ms_median"]), flush=True)
            if ns == 3 and per_pair == 4:
                t0 = time.perf_counter()
                for k in range(64):
                    _lib.nav_building_fields(d_maps[:ns], links, starts[k:k + 1], lib_=L)
                entry["sixty_four_single_calls_ms"] = (time.perf_counter() - t0) * 1e3
                goals = np.c_[rng.integers(0, ns, a.goals), rng.integers(0, 500, a.goals), rng.integers(0, 700, a.goals)].astype(np.int32)
                for minc in (0, 42):
                    r, t = timed(lambda: _lib.nav_building_route(d_maps[:ns], links, starts[0], goals, lib_=L, min_clearance=minc))
                    t.update(last("hmsg_test_nav_building_last"))
                    t.update(path_cells=int(len(r["path_src"])), reached=int((r["goal_dist"].cpu().numpy() != RB.UNREACHED).sum()))
                    entry["route_min_clearance_%d" % minc] = t
                    print("%-24s route minc %2d %9.3f ms median, %d path cells, %d of %d goals reached" %
                          (key, minc, t["ms_median"], t["path_cells"], t["reached"], a.goals), flush=True)
                if not a.no_reference:
                    t0 = time.perf_counter()
                    B = RB.Building(maps[:ns], links)
                    t1 = time.perf_counter()
                    ref, _ = B.fields(starts[0])
                    t2 = time.perf_counter()
                    got, _ = _lib.nav_building_fields(d_maps[:ns], links, starts[:1], lib_=L)
                    same = all(np.array_equal(g[0].cpu().numpy(), f) for g, f in zip(got, ref))
                    entry["reference"] = dict(what="tests/navbuilding_reference.py: scipy.sparse.csgraph.dijkstra on the layered graph, one start",
                                              graph_build_ms=(t1 - t0) * 1e3, dijkstra_ms=(t2 - t1) * 1e3, fields_equal=bool(same))
                    print("reference: graph %.0f ms, dijkstra %.0f ms, equal: %s" % ((t1 - t0) * 1e3, (t2 - t1) * 1e3, same), flush=True)
                    if not same:
                        raise SystemExit("the library's fields differ from the reference's")
            res[key] = entry
    if a.kernel_stats:
        with open(a.kernel_stats) as f:
            rows = [r for r in csv.DictReader(f) if "navb" in r.get("Name", "") or "navr" in r.get("Name", "")]
        res["kernels"] = {r["Name"].split("(")[0]: dict(calls=int(r["Calls"]), total_us=float(r["TotalDurationNs"]) / 1e3,
                                                        mean_us=float(r["AverageNs"]) / 1e3, min_us=float(r["MinNs"]) / 1e3,
                                                        max_us=float(r["MaxNs"]) / 1e3) for r in rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res)[:400])


if __name__ == "__main__":
    main()
