"""A frame's masks handed over dense (hmsg_add_frame_features, u8 [M][H][W]) and as SAM's uncompressed run-length records
(hmsg_add_frame_features_rle) on cuda:0, at 640x480 / M = 32 and 1280x720 / M = 32, on device-rendered frames (bench.py's renderer)
whose masks are read back and encoded ONCE, outside every timed region.  Per shape, 5 warm-up frames and 50 timed ones:
  (a) wall time per frame of the hand-over FROM HOST MEMORY (numpy arrays: masks or records, and the same F tables), the two calls
      alternating frame by frame on two handles in one process; a host clock around a call that ends in the stream's synchronise.
      With the bytes that crossed and the counts per mask.
  (b) device time (hmsg_set_profiling: HIP events around the launches) of k_rle_scan + k_rle_bitset against k_bitset with every
      input already in HBM (torch device tensors), and each kernel's algorithmic bytes over that time.
  (c) by arithmetic: the mask bytes of Graph.create_feature_map's batch of 32 frames at 1280x720 / M = 100, dense against records.
Writes profiles/rle_masks.json (or the path given) and prints it.
    python scripts/bench_mask_handover.py [out.json]"""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from bench import build_scene_inputs  # noqa: E402
from holoagent_amd import rle  # noqa: E402
from holoagent_amd._lib import Scene, lib  # noqa: E402
from holoagent_amd.synth import SceneSpec  # noqa: E402

WARM, TIMED, M, D = 5, 50, 32, 512


def _stats(v):
    q = statistics.quantiles(v, n=10)
    return {"median_ms": round(statistics.median(v) * 1e3, 4), "p10_ms": round(q[0] * 1e3, 4), "p90_ms": round(q[-1] * 1e3, 4),
            "min_ms": round(min(v) * 1e3, 4), "max_ms": round(max(v) * 1e3, 4), "n": len(v)}


def _scene(L, inp, H, W, F):
    sc = Scene(lib_=L, height=H, width=W, max_frames=F, max_masks=M, feat_dim=D)
    sc.add_frames(inp["rgb"], inp["depth"], inp["pose"], inp["K"])
    return sc


def bench_shape(L, H, W):
    dev = torch.device("cuda:0")
    F = WARM + TIMED
    spec = SceneSpec(seed=1234, n_frames=F, feat_dim=D, n_masks=M, width=W, height=H)
    inp = build_scene_inputs(L, spec, dev, torch)
    # ---- outside every timed region: the masks to the host, encoded once; the F tables to the host
    masks_h = inp["masks"].cpu().numpy()                                     # [F][M][H][W]
    recs = [rle.pack([[rle.encode(m) for m in masks_h[f]]]) for f in range(F)]
    for f in (0, F - 1):                                                     # the records are these masks
        assert all(np.array_equal(rle.decode(recs[f][0][recs[f][1][i]:recs[f][1][i + 1]], H, W), masks_h[f, i] != 0) for i in range(M))
    fg_h, fm_h, fc_h = (inp[k].cpu().numpy() for k in ("f_g", "f_masked", "f_crop"))
    per_mask = np.concatenate([np.diff(r[1]) for r in recs])
    f_bytes = (2 * M + 1) * D * 4
    dense_bytes = M * H * W
    rle_bytes = [int(r[0].nbytes + r[1].nbytes + r[2].nbytes) for r in recs]
    # ---- (a) from host memory, alternating
    sc_d, sc_r = _scene(L, inp, H, W, F), _scene(L, inp, H, W, F)
    t_d, t_r = [], []
    for f in range(F):
        def dense():
            sc_d.add_frame_features(f, masks_h[f:f + 1], fg_h[f:f + 1], fm_h[f:f + 1], fc_h[f:f + 1])

        def runlen():
            sc_r.add_frame_features_rle(f, recs[f], fg_h[f:f + 1], fm_h[f:f + 1], fc_h[f:f + 1])
        for fn, acc in ((dense, t_d), (runlen, t_r)) if f % 2 == 0 else ((runlen, t_r), (dense, t_d)):
            t0 = time.perf_counter()
            fn()                                                             # (returns after its stream's synchronise)
            acc.append(time.perf_counter() - t0)
    sc_d.close()
    sc_r.close()
    t_d, t_r = t_d[WARM:], t_r[WARM:]
    sd, sr = _stats(t_d), _stats(t_r)
    # ---- (b) device time, inputs in HBM
    d_recs = [tuple(torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to(dev) for a in r) for r in recs]
    sc_d, sc_r = _scene(L, inp, H, W, F), _scene(L, inp, H, W, F)
    for f in range(F):
        if f == WARM:
            sc_d.set_profiling(True)
            sc_r.set_profiling(True)
        sc_d.add_frame_features(f, inp["masks"][f:f + 1], inp["f_g"][f:f + 1], inp["f_masked"][f:f + 1], inp["f_crop"][f:f + 1])
        sc_r.add_frame_features_rle(f, d_recs[f], inp["f_g"][f:f + 1], inp["f_masked"][f:f + 1], inp["f_crop"][f:f + 1])
    prof = {}
    for sc in (sc_d, sc_r):
        for k, (n, ms, work) in sc.profile().items():
            if k in ("k_bitset", "k_rle_scan", "k_rle_bitset"):
                prof[k] = {"launches": n, "mean_us": round(ms / n * 1e3, 3), "algorithmic_bytes_per_launch": round(work / n),
                           "gb_per_s": round(work / (ms * 1e-3) / 1e9, 2)}
        sc.close()
    rle_dev_us = prof["k_rle_scan"]["mean_us"] + prof["k_rle_bitset"]["mean_us"]
    return {"frame": f"{W}x{H}", "masks": M, "feat_dim": D, "warmup_frames": WARM, "timed_frames": TIMED,
            "counts_per_mask": {"mean": round(float(per_mask.mean()), 1), "median": int(np.median(per_mask)), "max": int(per_mask.max())},
            "counts_per_frame_mean": round(float(per_mask.sum()) / F, 1),
            "bytes_per_frame": {"dense_masks": dense_bytes, "rle_records_mean": round(float(np.mean(rle_bytes))), "rle_records_max": max(rle_bytes),
                                "f_tables_either_way": f_bytes, "dense_over_rle": round(dense_bytes / float(np.mean(rle_bytes)), 1)},
            "a_wall_per_frame_from_host": {"dense": sd, "rle": sr,
                                           "dense_spread_p90_minus_p10_ms": round(sd["p90_ms"] - sd["p10_ms"], 4),
                                           "dense_spread_max_minus_min_ms": round(sd["max_ms"] - sd["min_ms"], 4),
                                           "rle_faster_by_more_than_dense_p10_p90_spread": bool(sd["median_ms"] - sr["median_ms"] > sd["p90_ms"] - sd["p10_ms"]),
                                           "rle_faster_by_more_than_dense_min_max_spread": bool(sd["median_ms"] - sr["median_ms"] > sd["max_ms"] - sd["min_ms"]),
                                           "slowest_rle_under_fastest_dense": bool(sr["max_ms"] < sd["min_ms"])},
            "b_device_time_inputs_in_hbm": dict(prof, rle_scan_plus_bitset_mean_us=round(rle_dev_us, 3),
                                                rle_not_slower_than_k_bitset=bool(rle_dev_us <= prof["k_bitset"]["mean_us"]))}


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "rle_masks.json")
    L = lib()
    shapes = [bench_shape(L, 480, 640), bench_shape(L, 720, 1280)]
    # (c) create_feature_map's batch: 32 frames, 1280x720, M = 100 -- the dense [32][M][H][W] array against the records, whose size is
    # the counts per mask measured above at 1280x720 (the synthetic masks; SAM's are raggeder: SURVEY's fixtures give 98 counts per mask
    # at 160x120, and counts grow with the outline, i.e. with the side, not the area)
    cpm = shapes[1]["counts_per_mask"]["mean"]
    dense_c = 32 * 100 * 720 * 1280
    rle_c = 32 * (100 * cpm * 4 + 101 * 8 + 4)
    res = {"benchmark": "rle_masks", "device": torch.cuda.get_device_name(0),
           "note": "(a) host clock around one hand-over call per frame, numpy arrays in pageable host memory, the two calls alternating; "
                   "(b) HIP events around the launches, algorithmic bytes (k_bitset: M + 8 NW per pixel; k_rle_scan: 8 per count; "
                   "k_rle_bitset: 4 per count + 8 NW per pixel) over that time -- not a share of peak",
           "shapes": shapes,
           "c_create_feature_map_batch_720p_M100_by_arithmetic": {"dense_array_bytes": dense_c, "rle_bytes_at_measured_counts_per_mask": round(rle_c),
                                                                  "counts_per_mask_used": cpm, "ratio": round(dense_c / rle_c, 1)}}
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
