"""Resume against rebuild on configs[1]'s scene (1000 frames of 640 x 480, 32 masks a frame, D = 512) on one MI355X:

  rebuild   hmsg_reset, A1..A7 on the frames (already in HBM, as bench.py has them) and the graph object (hmsg_graph_begin after the
            map, hmsg_graph_finish after the pooling) -- the step bench.py times, without its queries;
  resume    hmsg_reset, hmsg_restore_stage of the artefacts of that scene (map points + colours + features, instance pool, pooled
            features: host arrays, as a caller that read them from disk holds them; and once more as device arrays), hmsg_build_graph.

Both graphs are checked equal (counts, edges) before anything is timed.  Also the bounds pass of the restore (k_stage_bounds, HIP
events) against the bytes it reads.  Medians of --steps runs after --warmup.  -> one JSON line, and --out FILE.

    python scripts/bench_restore.py [--frames 1000] [--steps 3] [--warmup 1] [--out profiles/restore_stage.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--feat-dim", type=int, default=512)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import bench
    from holoagent_amd._lib import HmsgLib, Scene, SceneGraph
    from holoagent_amd.synth import SceneSpec
    emu = os.environ.get("HMSG_BENCH_EMU")                      # (the script against the kernel simulator: never a measurement)
    L = HmsgLib(emu) if emu else HmsgLib()
    device = torch.device("cpu") if emu else torch.device("cuda", 0)
    sync = (lambda: None) if emu else torch.cuda.synchronize
    F, D = a.frames, a.feat_dim
    spec = SceneSpec(seed=1234, n_frames=F, feat_dim=D, n_masks=32, width=a.width, height=a.height)
    inp = bench.build_scene_inputs(L, spec, device, torch)
    poses = np.ascontiguousarray(np.asarray(inp["pose"], np.float64).reshape(F, 4, 4))
    pinv = np.ascontiguousarray(np.linalg.inv(poses))
    fg = inp["f_g"].cpu().numpy()
    rng = np.random.Generator(np.random.PCG64(99))
    label_feats = rng.standard_normal((205, D)).astype(np.float32)
    label_feats /= np.linalg.norm(label_feats, axis=1, keepdims=True)
    label_names = ["label%d" % i for i in range(205)]
    sc = Scene(lib_=L, device_id=0, height=spec.height, width=spec.width, max_frames=F, max_masks=32, feat_dim=D)
    art = {}

    def rebuild(keep=False):
        sc.reset()
        sc.add_frames(inp["rgb"], inp["depth"], inp["pose"], inp["K"])
        sc.finalize_map()
        g = SceneGraph.begin(sc, poses, fg, poses_inv=pinv)
        sc.add_frame_features(0, inp["masks"], inp["f_g"], inp["f_masked"], inp["f_crop"])
        sc.fuse_frames()
        sc.merge_instances()
        sc.pool_instances()
        if keep:                                                # the artefacts, before the object level denoises the clouds
            xyz, rgb = sc.map_points(colors=True)
            sizes = sc.instance_sizes()
            off = np.zeros(len(sizes) + 1, np.int64)
            off[1:] = np.cumsum(sizes)
            flat = np.empty((int(off[-1]), 3), np.float64)
            sc.instance_points_into(flat)
            art.update(xyz=xyz, rgb=rgb, mf=sc.map_feats(), off=off, flat=flat, feats=sc.instance_feats())
        g.finish(label_feats, label_names)
        return g
    sc2 = Scene(lib_=L, device_id=0, height=spec.height, width=spec.width, max_frames=1, max_masks=32, feat_dim=D)
    laps = {}

    def resume(src):
        sc2.reset()
        t0 = time.perf_counter()
        sc2.restore_stage(src["xyz"], (art["off"], src["flat"]), src["feats"], inp["K"], map_colors=src["rgb"], map_feats=src["mf"])
        laps["restore"] = time.perf_counter() - t0
        return SceneGraph.build(sc2, poses, fg, label_feats, label_names, poses_inv=pinv)
    ga = rebuild(keep=True)
    gb = resume(art)
    ca, cb = ga.counts(), gb.counts()
    same = all(ca[k] == cb[k] for k in ("floors", "rooms", "views", "objects", "edges", "view_object_links")) and np.array_equal(ga.edges(), gb.edges())
    assert same, "the resumed graph differs from the rebuilt one"
    ga.close()
    gb.close()
    dev = art if emu else {k: torch.from_numpy(v).to(device) for k, v in art.items() if k != "off"}

    def timed(fn, *args):
        out, rest = [], []
        for i in range(a.warmup + a.steps):
            sync()
            t0 = time.perf_counter()
            g = fn(*args)
            sync()
            if i >= a.warmup:
                out.append(time.perf_counter() - t0)
                rest.append(laps.get("restore", 0.0))
            g.close()
        return float(np.median(out)) * 1e3, float(np.median(rest)) * 1e3
    t_rebuild, _ = timed(rebuild)
    t_host, t_host_restore = timed(resume, art)
    t_dev, t_dev_restore = timed(resume, dev)
    sc2.reset()
    sc2.set_profiling(True)
    resume(dev).close()
    n, ms, work = sc2.profile().get("k_stage_bounds", (0, 0.0, 0.0))
    res = dict(scene="%d frames of %d x %d, 32 masks a frame, D = %d" % (F, spec.width, spec.height, D), emulated=bool(emu),
               map_points=int(len(art["xyz"])), instances=int(len(art["off"]) - 1), instance_points=int(art["off"][-1]),
               artefact_bytes=int(sum(v.nbytes for v in art.values())), graph=dict((k, int(ca[k])) for k in ("floors", "rooms", "views", "objects")),
               rebuild_ms=t_rebuild, resume_host_arrays_ms=t_host, resume_host_arrays_restore_ms=t_host_restore,
               resume_device_arrays_ms=t_dev, resume_device_arrays_restore_ms=t_dev_restore,
               bounds_pass=dict(ms=float(ms), bytes_read=float(work), gb_per_s=(float(work) / (ms * 1e-3) / 1e9) if ms > 0 else None),
               steps=a.steps, warmup=a.warmup)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
