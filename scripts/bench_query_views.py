"""The view level of the slow path on a BUILT graph of configs[1]'s shape (1000 frames of 640x480, 32 masks, D = 512; the scene of
bench.py): time per call of

  hmsg_graph_goal_views        Q = 1000 object texts, every room, k = 24
  hmsg_graph_rematch_in_views  Q = 1000 (text, view) pairs -- the view of each query's best goal image -- with the distance of the
                               chosen object in that view's camera
  hmsg_graph_object_view_depths  the Q fast-path hits in their own best views

and, for comparison, what the mirror did before these calls existed: Graph.rank_goal_views called once per query, 1000 times (a
throw-away index per call, numpy's ordering).  Every call ends with its own device synchronise, so a call is timed on the host clock
around it; warm-up calls first, then `--repeats` timed calls, the paths alternating; median, min, max.  The first call of each path
(which makes the resident table / the view lists on the index) is timed separately as `first_call_ms`.

  python scripts/bench_query_views.py [--repeats 20] [--frames 1000] [--out profiles/query_views.json]
prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

Q, K_TOP = 1000, 24


def stats(ts):
    ts = sorted(ts)
    return dict(median_ms=round(1e3 * ts[len(ts) // 2], 4), min_ms=round(1e3 * ts[0], 4), max_ms=round(1e3 * ts[-1], 4), n=len(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--mirror-repeats", type=int, default=3)
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--feat-dim", type=int, default=512)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    import torch
    import bench
    from holoagent_amd._lib import HmsgLib, Scene, SceneGraph
    from holoagent_amd.graph import Graph
    from holoagent_amd.synth import SceneSpec
    L = HmsgLib()
    device = torch.device("cuda", 0)
    F, D = args.frames, args.feat_dim
    spec = SceneSpec(seed=1234, n_frames=F, feat_dim=D, n_masks=32, width=args.width, height=args.height)
    inp = bench.build_scene_inputs(L, spec, device, torch)
    sc = Scene(lib_=L, device_id=0, height=spec.height, width=spec.width, max_frames=F, max_masks=32, feat_dim=D)
    sc.add_frames(inp["rgb"], inp["depth"], inp["pose"], inp["K"])
    sc.finalize_map()
    poses = np.ascontiguousarray(np.asarray(inp["pose"], np.float64).reshape(F, 4, 4))
    inv = np.linalg.inv(poses)
    fg = inp["f_g"].cpu().numpy()
    cg = SceneGraph.begin(sc, poses, fg, poses_inv=inv)
    sc.add_frame_features(0, inp["masks"], inp["f_g"], inp["f_masked"], inp["f_crop"])
    sc.fuse_frames()
    sc.merge_instances()
    sc.pool_instances()
    cg.finish(None, None)
    cnt = cg.counts()
    d = cg.to_dict()
    K = np.asarray(inp["K"], np.float64).reshape(3, 3)
    wh = [spec.width, spec.height]
    rng = np.random.Generator(np.random.PCG64(11))
    T = rng.standard_normal((Q, D)).astype(np.float32)
    T /= np.linalg.norm(T, axis=1, keepdims=True)
    floor = np.full(Q, -1, np.int32)
    zero = np.zeros(Q, np.int32)

    first = {}
    t0 = time.perf_counter()
    img, room, score, n = cg.goal_views(T, floor, k=K_TOP)
    first["goal_views"] = time.perf_counter() - t0
    assert (n > 0).all()
    views = np.array([cg.find_view(img_id=int(i)) for i in img[:, 0]], np.int32)
    assert (views >= 0).all()
    cams = np.ascontiguousarray(inv[img[:, 0]])
    t0 = time.perf_counter()
    obj, sc_re, dist = cg.rematch_in_views(T, views, pose_inv=cams, wh=wh, K=K)
    first["rematch_in_views"] = time.perf_counter() - t0
    _, hit, _, _ = cg.query(T[:, None, :], zero, None, floor, zero, 1, use_negatives=False)
    hit = np.ascontiguousarray(hit[:, 0])
    bv, bimg = cg.object_best_views(hit)
    have = np.nonzero(bv >= 0)[0]
    hit_cams = np.ascontiguousarray(inv[bimg[have]])

    # the mirror's rooms for rank_goal_views: sample_images / clip_embeddings as the built graph holds them
    class R:
        pass
    mg = Graph(dict(main=dict(), models=dict(clip=dict(feat_dim=D))), lib=L)
    mg.get_text_feats_multiple_templates = lambda words: np.stack([T[int(w)] for w in words])
    rooms_list = []
    for r in d["rooms"]:
        o = R()
        o.sample_images, o.clip_embeddings = r["sample_images"], [fg[i] for i in r["sample_images"]]
        rooms_list.append(o)

    def mirror():
        return [mg.rank_goal_views(str(q), rooms_list, top_k=K_TOP)[0] for q in range(Q)]

    best = mirror()
    agree = int(sum(int(b == i) for b, i in zip(best, img[:, 0])))
    paths = (("goal_views", lambda: cg.goal_views(T, floor, k=K_TOP)),
             ("rematch_in_views", lambda: cg.rematch_in_views(T, views, pose_inv=cams, wh=wh, K=K)),
             ("rematch_in_views_no_distance", lambda: cg.rematch_in_views(T, views)),
             ("object_view_depths", lambda: cg.object_view_depths(hit[have], hit_cams, wh, K)))
    res = {name: [] for name, _ in paths}
    for _ in range(args.warmup):
        for _, fn in paths:
            fn()
    for _ in range(args.repeats):                       # (the paths alternate: drift on the host hits all of them alike)
        for name, fn in paths:
            t0 = time.perf_counter()
            fn()
            res[name].append(time.perf_counter() - t0)
    res["mirror_rank_goal_views_x1000"] = []
    for _ in range(args.mirror_repeats):
        t0 = time.perf_counter()
        mirror()
        res["mirror_rank_goal_views_x1000"].append(time.perf_counter() - t0)
    out = {k: stats(v) for k, v in res.items()}
    n_img = int(sum(len(r["sample_images"]) for r in d["rooms"]))
    vo = [v["n_objects"] for v in cg.views()]
    pts = sc.instance_sizes()
    objs = cg.objects()
    rec = dict(metric="query_views", graph="built, configs[1] shape", frames=F, D=D, Q=Q, k=K_TOP, rooms=cnt["rooms"], views=cnt["views"], objects=cnt["objects"],
               sampled_images=n_img, objects_per_view_mean=round(float(np.mean(vo)), 1), objects_per_view_max=int(max(vo)),
               points_per_object_mean=round(float(np.mean(pts)), 1), points_of_rematched_objects=int(sum(pts[objs[o]["instance"]] for o in obj if o >= 0)),
               first_call_ms={k: round(1e3 * v, 3) for k, v in first.items()}, mirror_argmax_agrees=agree, **out,
               note="host clock around each call (every call ends with its own stream synchronise); goal_views = text upload + f64 MFMA GEMM "
                    "[Q x images x D] + one top-k workgroup per query + read-back; rematch = text upload + one workgroup per query (+ two distance "
                    "kernels over the chosen objects' clouds)")
    line = json.dumps(rec)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(line + "\n")
    cg.close()
    sc.close()


if __name__ == "__main__":
    main()
