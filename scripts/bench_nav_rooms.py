"""Timing of N11 (include/hmsg.h: hmsg_nav_room_labels, hmsg_nav_doors, hmsg_nav_room_doors) beside the only way the library had to
the same labels before: hmsg_nav_distance_fields with one field per room, then an argmin in torch.  To be run on the MI355X, outside
the test suite:

    python scripts/bench_nav_rooms.py [--reps 10] [--kernel-stats <rocprofv3 kernel_stats.csv>] [--out profiles/nav_rooms.json]

The map is the 500 x 700 rooms map of tests/navroute_cases.py (rooms_map(500, 700, 6)), device tensors in and out.  Two seed lists:
24 rooms (4 x 6 blocks of 125 x 117 cells, a seed at every third cell that is free) and 234 rooms (the first 234 of its 37-cell
rooms in row-major order, their centre cells).  Per list, in the same run and on the same inputs, alternating: hmsg_nav_room_labels; the per-room way (one field
per room in one hmsg_nav_distance_fields call, torch.min over the rooms, -1 where nothing reaches); one hmsg_nav_distance_fields
call with the union of the seeds as a single field; hmsg_nav_doors on the labels; hmsg_nav_room_doors, the composition.  A sample
is the host clock around one call, which ends in a stream synchronise; two warm-up calls; the best, the median and the worst of
--reps samples.  The labels of the two ways are compared before anything is timed.  Rounds and round trips come from
hmsg_test_nav_rooms_last and hmsg_test_nav_route_last.  Kernel times come from a run of their own under `rocprofv3 --kernel-trace
--stats -- python scripts/bench_nav_rooms.py`, whose csv a second call folds in with --kernel-stats.  Writes
profiles/nav_rooms.json.
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


def seed_lists(m):
    """24 rooms: 4 x 6 blocks of 125 x 117 cells, every third free cell; 234 rooms: the 37-cell rooms between the walls, their centre cells"""
    H, W = m.shape
    big = []
    for r0 in range(0, H, 125):
        for c0 in range(0, W, 117):
            rr, cc = np.mgrid[r0:min(r0 + 125, H):3, c0:min(c0 + 117, W):3]
            rc = np.c_[rr.ravel(), cc.ravel()]
            big.append(rc[m[rc[:, 0], rc[:, 1]] != 0])
    rows = list(zip([0] + [r + 1 for r in range(37, H, 37)], list(range(37, H, 37)) + [H]))
    cols = list(zip([0] + [c + 1 for c in range(37, W, 37)], list(range(37, W, 37)) + [W]))
    small = [np.array([((a + b) // 2, (c + d) // 2)]) for a, b in rows for c, d in cols][:234]
    return {"24": big, "234": small}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "nav_rooms.json"))
    a = ap.parse_args()
    if a.kernel_stats:                                                                # fold a profiler run into the existing file
        res = json.load(open(a.out))
        rows = [r for r in csv.DictReader(open(a.kernel_stats)) if "k_nav" in r["Name"] or "k_sort" in r["Name"] or "scan" in r["Name"]]
        res["kernels"] = {r["Name"].split("(")[0]: dict(calls=int(r["Calls"]), total_us=int(r["TotalDurationNs"]) / 1e3,
                                                         mean_us=float(r["AverageNs"]) / 1e3) for r in rows}
        res["kernels_note"] = "rocprofv3 --kernel-trace --stats over a run of its own; totals are over all its calls"
        json.dump(res, open(a.out, "w"), indent=1)
        print(json.dumps(res["kernels"]))
        return
    import ctypes as C
    import torch
    from holoagent_amd import _lib
    from tests import navroute_cases as NC
    if not torch.cuda.is_available():
        raise SystemExit("bench_nav_rooms.py measures on the GPU: none found")
    L = _lib.HmsgLib()
    m = np.array(NC.rooms_map(500, 700, 6), order="C")
    d_m = torch.from_numpy(m).cuda()
    res = dict(device=torch.cuda.get_device_name(0), rows=500, cols=700,
               timing="host clock around one call with device tensors in and out; every call ends in a stream synchronise; two warm-up calls; "
                      "the calls of one seed list alternate within a repetition")

    def last(fn):
        x, y = C.c_int32(0), C.c_int32(0)
        fn(C.byref(x), C.byref(y))
        return dict(rounds=x.value, round_trips=y.value)

    def stats(ts):
        return dict(ms_best=min(ts), ms_median=float(np.median(ts)), ms_worst=max(ts), samples=len(ts))

    for name, seeds in seed_lists(m).items():
        n = len(seeds)
        union = np.concatenate(seeds)
        unreached = _lib.NAV_UNREACHED

        def per_room():
            f, _ = _lib.nav_distance_fields(d_m, seeds, lib_=L)
            d, lab = torch.min(f, dim=0)                                              # (of equal values torch returns some index, see below)
            return torch.where(d == unreached, torch.full_like(lab, -1), lab), d, f

        calls = dict(room_labels=lambda: _lib.nav_room_labels(d_m, seeds, lib_=L, want_dist=True),
                     per_room_fields_and_argmin=per_room,
                     union_field=lambda: _lib.nav_distance_fields(d_m, [union], lib_=L),
                     room_doors=lambda: _lib.nav_room_doors(d_m, seeds, lib_=L))
        lab, cells, dist = calls["room_labels"]()
        counts = last(L.c.hmsg_test_nav_rooms_last)
        old_lab, old_d, f = per_room()
        # torch.min's index among equal values is not specified: the least room with the minimal field, spelt out, is the reference
        first = torch.argmax((f == old_d.unsqueeze(0)).to(torch.uint8), dim=0)
        first = torch.where(old_d == unreached, torch.full_like(first, -1), first)
        same = bool(torch.equal(first.to(torch.int32), lab)) and bool(torch.equal(old_d, dist))
        if not same:
            raise SystemExit("hmsg_nav_room_labels differs from the per-room fields at %s rooms" % name)
        del f, old_d, old_lab, first
        calls["union_field"]()
        union_counts = last(L.c.hmsg_test_nav_route_last)
        calls["doors"] = lambda: _lib.nav_doors(d_m, lab, n, lib_=L)
        table = calls["doors"]()
        for fn in calls.values():
            for _ in range(2):
                fn()
        ts = {k: [] for k in calls}
        for _ in range(a.reps):
            for k, fn in calls.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                ts[k].append((time.perf_counter() - t0) * 1e3)
        r = {k: stats(v) for k, v in ts.items()}
        r.update(n_rooms=n, n_seeds=int(len(union)), labels_in_use=int(len(torch.unique(lab[lab >= 0]))), n_doors=int(table["n_doors"]),
                 n_door_cells=int(table["n_door_cells"]), equal_to_per_room_fields=same, room_labels_counts=counts, union_field_counts=union_counts,
                 per_room_over_room_labels=r["per_room_fields_and_argmin"]["ms_median"] / r["room_labels"]["ms_median"],
                 room_labels_over_union_field=r["room_labels"]["ms_median"] / r["union_field"]["ms_median"])
        res["rooms_%s" % name] = r
        for k in calls:
            print("%4s rooms  %-28s %8.3f ms median (%.3f .. %.3f)" % (name, k, r[k]["ms_median"], r[k]["ms_best"], r[k]["ms_worst"]), flush=True)
        print("%4s rooms  rounds and trips: labels %s, union field %s; doors %d, cells %d; per-room / labels x%.2f, labels / union field x%.2f" %
              (name, counts, union_counts, r["n_doors"], r["n_door_cells"], r["per_room_over_room_labels"], r["room_labels_over_union_field"]),
              flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
