"""Cross-scene retrieval over 8 scenes on one GPU: the sharded query (include/hmsg.h: hmsg_graphs_query -- tables stay with their graph)
against the all-gather form (ONE concatenated index + hmsg_query_hier), once with the index build counted and once with it resident.

Scenes: 8 saved graphs of configs[1]'s shape -- one storey, 4 x 2 rooms, 8 objects a room, 24 view embeddings a room, D = 512,
seeded unit vectors -- written to a temporary directory and loaded with hmsg_load (float64 tables in HBM).  Queries: Q = 1000, k = 5,
label mode, negatives on, three text rows each, query q on storey q % 8.  Warm-up, then `--repeats` timed calls per path, each ended by
the call's own device synchronise; median, min and max.  The answers of the two paths are compared bit for bit first.

  python scripts/bench_query_sharded.py [--repeats 30] [--out FILE]
prints one JSON line."""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_SCENES, ROOMS_X, ROOMS_Z, OBJ_PER_ROOM, VIEWS, D = 8, 4, 2, 8, 24, 512
Q, K, C = 1000, 5, 3


def write_scene(L, directory, seed):
    from holoagent_amd._lib import write_ply
    rng = np.random.Generator(np.random.PCG64(seed))
    unit = lambda a: a / np.linalg.norm(a, axis=-1, keepdims=True)
    for sub in ("floors", "rooms", "objects", "views"):
        os.makedirs(os.path.join(directory, sub), exist_ok=True)
    pts = rng.standard_normal((8, 3))
    write_ply(os.path.join(directory, "floors", "0.ply"), pts, lib_=L)
    json.dump(dict(name="floor_0", floor_height=3.0, floor_zero_level=0.0), open(os.path.join(directory, "floors", "0.json"), "w"))
    for r in range(ROOMS_X * ROOMS_Z):
        rid = "0_%d" % r
        write_ply(os.path.join(directory, "rooms", rid + ".ply"), pts, lib_=L)
        json.dump(dict(name="room_" + rid, embeddings=unit(rng.standard_normal((VIEWS, D))).tolist()), open(os.path.join(directory, "rooms", rid + ".json"), "w"))
        for o in range(OBJ_PER_ROOM):
            oid = "%s_%d" % (rid, o)
            write_ply(os.path.join(directory, "objects", oid + ".ply"), pts, lib_=L)
            json.dump(dict(name="object_" + oid, embedding=unit(rng.standard_normal(D)).tolist()), open(os.path.join(directory, "objects", oid + ".json"), "w"))


def tables(directory, g):
    rooms, objs = g.rooms(), g.objects()
    emb = np.asarray([json.load(open(os.path.join(directory, "objects", o["object_id"] + ".json")))["embedding"] for o in objs], np.float64)
    views = [np.asarray(json.load(open(os.path.join(directory, "rooms", r["room_id"] + ".json")))["embeddings"], np.float64) for r in rooms]
    return dict(emb=emb, room=np.array([o["room"] for o in objs], np.int32), views=views, keys=[int(r["room_id"].split("_")[-1]) for r in rooms],
                floors=[[i for i, r in enumerate(rooms) if r["floor"] == f] for f in range(g.counts()["floors"])])


def stats(ts):
    ts = sorted(ts)
    return dict(median_ms=round(1e3 * ts[len(ts) // 2], 4), min_ms=round(1e3 * ts[0], 4), max_ms=round(1e3 * ts[-1], 4), n=len(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    import torch  # noqa: F401  (one HIP runtime for torch and the library, as bench.py loads them)
    from holoagent_amd._lib import HmsgLib, NodeIndex, SceneGraph, query_graphs, sharded_query_bytes
    L = HmsgLib()
    tmp = tempfile.mkdtemp(prefix="hmsg_qs_")
    dirs = [os.path.join(tmp, "s%d" % i) for i in range(N_SCENES)]
    for i, d in enumerate(dirs):
        write_scene(L, d, 1000 + i)
    gs = [SceneGraph.load(d, lib_=L) for d in dirs]
    tabs = [tables(d, g) for d, g in zip(dirs, gs)]
    R = ROOMS_X * ROOMS_Z
    rng = np.random.Generator(np.random.PCG64(5))
    names = [rng.standard_normal((R, D)) for _ in range(N_SCENES)]
    names = [n / np.linalg.norm(n, axis=1, keepdims=True) for n in names]
    all_emb = np.concatenate([t["emb"] for t in tabs])
    T = rng.standard_normal((Q, C, D))
    T[:, 0] += 3.0 * all_emb[rng.integers(0, len(all_emb), Q)]
    T = (T / np.linalg.norm(T, axis=2, keepdims=True)).astype(np.float32)
    Tr = rng.standard_normal((Q, D))
    Tr = (Tr / np.linalg.norm(Tr, axis=1, keepdims=True)).astype(np.float32)
    qid = np.zeros(Q, np.int32)
    fl = (np.arange(Q) % N_SCENES).astype(np.int32)
    mode = np.ones(Q, np.int32)
    RM = N_SCENES * R

    def sharded():
        return query_graphs(gs, names, T, qid, Tr, fl, mode, K, max_rooms=RM)

    roff = np.concatenate([[0], np.cumsum([len(t["keys"]) for t in tabs])])
    cat_emb = np.ascontiguousarray(all_emb)
    cat_room = np.concatenate([t["room"] + roff[s] for s, t in enumerate(tabs)]).astype(np.int32)
    cat_floors = [[int(roff[s] + r) for r in fl_] for s, t in enumerate(tabs) for fl_ in t["floors"]]
    cat_views = [v for t in tabs for v in t["views"]]
    cat_keys = [k for t in tabs for k in t["keys"]]
    cat_names = np.concatenate(names)

    def build_index():
        ix = NodeIndex(cat_emb, cat_room, lib_=L)
        ix.set_hierarchy(cat_floors, cat_names, cat_views, cat_keys)
        return ix

    resident = build_index()

    def gathered_resident():
        return resident.query_hier(T, qid, Tr, fl, mode, K, max_rooms=RM)

    def gathered_with_build():
        ix = build_index()
        out = ix.query_hier(T, qid, Tr, fl, mode, K, max_rooms=RM)
        ix.close()
        return out

    a, b = sharded(), gathered_resident()
    same = a[0] == b[0] and all(np.array_equal(x, y) for x, y in zip(a[1:3], b[1:3])) and np.array_equal(a[3].view(np.int64), b[3].view(np.int64))
    assert same, "the sharded answer differs from the concatenated index"

    res = {}
    for name, fn in (("sharded", sharded), ("allgather_resident", gathered_resident), ("allgather_with_index_build", gathered_with_build)):
        for _ in range(args.warmup):
            fn()
    for name, fn in (("sharded", sharded), ("allgather_resident", gathered_resident), ("allgather_with_index_build", gathered_with_build)):
        res[name] = []
    for _ in range(args.repeats):                       # (the three paths alternate: drift on the host hits all of them alike)
        for name, fn in (("sharded", sharded), ("allgather_resident", gathered_resident), ("allgather_with_index_build", gathered_with_build)):
            t0 = time.perf_counter()
            fn()
            res[name].append(time.perf_counter() - t0)
    out = {k: stats(v) for k, v in res.items()}
    for k in out:
        out[k]["queries_per_s"] = round(Q / (out[k]["median_ms"] / 1e3), 1)
    n_nodes = len(cat_emb)
    n_views = sum(len(v) for v in cat_views)
    rec = dict(metric="query_sharded_8_scenes", scenes=N_SCENES, nodes_per_scene=n_nodes // N_SCENES, rooms_per_scene=R, views_per_room=VIEWS, D=D,
               Q=Q, k=K, C=C, room_mode="label", answers_bit_identical=bool(same), **out,
               bytes_per_call_sharded_8_ranks=sharded_query_bytes(N_SCENES, Q, K, R, 1, R, label=True),
               bytes_per_rank_tables_allgather=int(N_SCENES * ((n_nodes // N_SCENES) * D * 8 + R * D * 8 + (n_views // N_SCENES) * D * 8)),
               note="hmsg_graphs_query on one GPU (no wire); bytes_per_call_sharded_8_ranks = what hmsg_graph_query_sharded would move over 8 "
                    "ranks per call (include/hmsg.h); bytes_per_rank_tables_allgather = the float64 node, room-name and view tables an "
                    "all-gathered index holds on every rank")
    line = json.dumps(rec)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(line + "\n")
    for g in gs:
        g.close()
    resident.close()
    shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
