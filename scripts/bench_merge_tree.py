"""The hierarchical merge pair by pair against a level of its tree per batch (hmsg_set_merge_tree_batch), on the scene bench.py
renders for BASELINE.json configs[1]: 1000 frames of 640 x 480, 32 masks a frame (--hd: 1280 x 720), merge_type hierarchical.

Every figure is hmsg_merge_instances alone, on inputs that are resident and fused: wall time (median of --runs runs after
--warmup warm-ups), DBSCAN batches and bracketed kernel launches (hmsg_set_profiling, in one run of its own), the host's phase
times (HMSG_DEBUG_TIMING, in one run of its own: every lap drains the stream), and the device memory the merge took (free
memory before and after, the allocator's cache emptied first).  Settings: 0 (the pair-by-pair tree: the yardstick, same run),
-1, one bounded value, and -1 with the candidate pairs enumerated by the host (HMSG_DEBUG_TREE_HOST_PAIRS=1).

    python scripts/bench_merge_tree.py [--frames 1000] [--hd] [--runs 5] [--warmup 2] [--bound 2000000] [--out profiles/merge_tree_level_batch.json]
"""
import argparse
import json
import os
import re
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--hd", action="store_true")
    ap.add_argument("--feat-dim", type=int, default=512)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--bound", type=int, default=2000000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "merge_tree_level_batch.json"))
    args = ap.parse_args()
    assert args.runs >= 5 and args.warmup >= 2, "medians of at least 5 runs after 2 warm-ups"
    import torch
    import bench
    from holoagent_amd._lib import HmsgLib, Scene
    from holoagent_amd.synth import SceneSpec
    L = HmsgLib()
    device = torch.device("cuda:0")
    W, H = (1280, 720) if args.hd else (640, 480)
    F, D = args.frames, args.feat_dim
    spec = SceneSpec(seed=1234, n_frames=F, feat_dim=D, n_masks=32, width=W, height=H)
    inp = bench.build_scene_inputs(L, spec, device, torch)
    sc = Scene(lib_=L, device_id=0, height=H, width=W, max_frames=F, max_masks=32, feat_dim=D, merge_type=1)

    def fused():
        sc.reset()
        sc.add_frames(inp["rgb"], inp["depth"], inp["pose"], inp["K"])
        sc.finalize_map()
        sc.add_frame_features(0, inp["masks"], inp["f_g"], inp["f_masked"], inp["f_crop"])
        sc.fuse_frames()
        torch.cuda.synchronize()

    def merge(batch):
        sc.set_merge_tree_batch(batch)
        t = time.perf_counter()
        sc.merge_instances()
        return (time.perf_counter() - t) * 1e3

    def digest():
        return [int(sc.num_instances()), int(sc.instance_sizes().sum()), float(np.concatenate(sc.instances()).sum())]

    settings = [("pair_by_pair", 0, {}), ("level", -1, {}), ("bounded_%d" % args.bound, args.bound, {}),
                ("level_host_pairs", -1, {"HMSG_DEBUG_TREE_HOST_PAIRS": "1"})]
    out = {"scene": "bench.py configs[1] scene: %d frames of %d x %d, 32 masks a frame, %d-d, merge_type hierarchical" % (F, W, H, D),
           "what": ("hmsg_merge_instances on resident fused inputs; ms are medians of %d runs after %d warm-ups.  host_phase_ms is the "
                    "library's HMSG_DEBUG_TIMING line of one extra run: with level batches its 'pairs' phase holds the two passes of "
                    "k_gp_pairs, their scan and the wait for the list, not host work alone (level_host_pairs: the host's loop).  "
                    "bracketed_launches counts profiling brackets (hmsg_set_profiling), not kernel launches: one k_gp_pairs bracket is "
                    "count pass + scan + fill pass, one k_db_union/scan bracket one DBSCAN batch" % (args.runs, args.warmup)),
           "settings": {}}
    ref = None
    for name, batch, env in settings:
        for k in ("HMSG_DEBUG_TIMING", "HMSG_DEBUG_TREE_HOST_PAIRS"):
            os.environ.pop(k, None)
        os.environ.update(env)
        times = []
        for r in range(args.warmup + args.runs):
            fused()
            ms = merge(batch)
            if r >= args.warmup:
                times.append(ms)
        d = digest()
        ref = ref or d
        assert d == ref, (name, d, ref)                     # (the tests compare bit for bit; this guards the run)
        # launches: one profiled run
        fused()
        sc.set_profiling(True)
        merge(batch)
        prof = sc.profile()
        sc.set_profiling(False)
        # device memory: the allocator's cache emptied, then what one merge takes from the device (its parked blocks included)
        fused()
        L.c.hmsg_release_cached_memory()
        torch.cuda.synchronize()
        free0 = torch.cuda.mem_get_info(0)[0]
        merge(batch)
        free1 = torch.cuda.mem_get_info(0)[0]
        # the host's phases: stderr of one run with HMSG_DEBUG_TIMING
        fused()
        os.environ["HMSG_DEBUG_TIMING"] = "1"
        sys.stderr.flush()
        with tempfile.TemporaryFile() as tf:
            keep = os.dup(2)
            os.dup2(tf.fileno(), 2)
            try:
                merge(batch)
            finally:
                os.dup2(keep, 2)
                os.close(keep)
            tf.seek(0)
            log = tf.read().decode(errors="replace")
        os.environ.pop("HMSG_DEBUG_TIMING", None)
        m = re.search(r"\[hmsg merge\] index ([\d.]+)\s+pairs\(host\) ([\d.]+)\s+overlap ([\d.]+)\s+components\+concat ([\d.]+)\s+dbscan ([\d.]+)\s+bookkeeping ([\d.]+)", log)
        phases = dict(zip(("index", "pairs", "overlap", "components_concat", "dbscan", "bookkeeping"), map(float, m.groups()))) if m else None
        out["settings"][name] = {
            "max_batch_points": batch, "env": env, "merge_ms_median": float(np.median(times)), "merge_ms_runs": [round(t, 2) for t in times],
            "dbscan_batches": prof.get("k_db_union/scan", (0,))[0], "bracketed_launches": int(sum(v[0] for v in prof.values())),
            "pair_kernel_passes": prof.get("k_gp_pairs", (0,))[0], "host_phase_ms": phases,
            "device_memory_taken_gb": round((free0 - free1) / 2 ** 30, 3)}
        print(name, json.dumps(out["settings"][name]), flush=True)
    base = out["settings"]["pair_by_pair"]["merge_ms_median"]
    for name, v in out["settings"].items():
        v["speedup_vs_pair_by_pair"] = round(base / v["merge_ms_median"], 3)
    out["instances"] = ref[0]
    out["against_60_ms_wish"] = "VERDICT.md wishes <= 60 ms for 1000 frames at 640 x 480 (not a gate): level batches take %.1f ms, pair by pair %.1f ms" % (
        out["settings"]["level"]["merge_ms_median"], base)
    lv, hp = out["settings"]["level"], out["settings"]["level_host_pairs"]
    out["pair_kernels"] = "pairs on the device %.1f ms, by the host's loop %.1f ms (whole levels): %s" % (
        lv["merge_ms_median"], hp["merge_ms_median"],
        "the kernels are not slower and stay the batched path's default" if lv["merge_ms_median"] <= hp["merge_ms_median"] * 1.02
        else "the host enumeration is faster at this size")
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)
    sc.close()


if __name__ == "__main__":
    main()
