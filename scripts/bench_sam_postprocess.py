"""SAM's mask post-processing of one frame (N = 432 logit images: 144 prompts x 3) on cuda:0 at 640x480 and 1280x720,
min_mask_region_area = 100, two routes timed in turn in one process on seeded inputs (tests/sam_post_cases.py: ellipses with
sharp or soft edges, holes, specks, near-duplicates), logits and iou_preds resident in HBM before:
  (a) what the wrapped SamAutomaticMaskGenerator does today behind predict_torch, restated with torch ops on the same device
      (segment_anything is not installed): the filters, calculate_stability_score, batched_mask_to_box, an NMS (torchvision is not
      installed: the boxes go to the host, one vectorised IoU row per kept box), mask_to_rle_pytorch with its Python loop per mask
      and .tolist(), and postprocess_small_regions on the host -- rle_to_mask, remove_small_regions twice, re-encoding, the second
      NMS -- with scipy.ndimage.label STANDING IN FOR cv2.connectedComponentsWithStats, which is not installed either.
  (b) hmsg_sam_postprocess with device tensors in and out: wall time and device_ms (HIP events, first launch to last).
Each timing is a host clock around work that ends with the results complete; the routes alternate ROUNDS times after a warm-up
of each.  Also reported: the statistics kernel's bytes over its time as a share of the HBM peak DESIGN.md quotes (the time is
hmsg_test_sam_post_last's: HIP events around the launch), the labelling rounds,
and that both routes return the same records.  Writes profiles/sam_postprocess.json (or the path given) and prints it.
    python scripts/bench_sam_postprocess.py [out.json]"""
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from holoagent_amd import rle  # noqa: E402
from holoagent_amd._lib import lib, sam_post_params, sam_postprocess  # noqa: E402
from tests import sam_post_cases as CS  # noqa: E402
from tests import sam_post_oracle as O  # noqa: E402

ROUNDS, N, AREA = 5, 432, 100
HBM_PEAK = 8.0e12          # bytes / s, the data-sheet figure DESIGN.md section 4 measures against
PRM = dict(O.DEFAULTS, min_mask_region_area=AREA)


def _stats(v):
    q = np.percentile(v, [10, 50, 90])
    return {"median_ms": round(float(q[1]) * 1e3, 3), "p10_ms": round(float(q[0]) * 1e3, 3), "p90_ms": round(float(q[2]) * 1e3, 3),
            "min_ms": round(min(v) * 1e3, 3), "max_ms": round(max(v) * 1e3, 3), "n": len(v)}


def _nms_host(boxes, scores, thr):
    """torchvision.ops.nms' result (float32, stable order among ties), one vectorised row per kept box"""
    b = np.asarray(boxes, np.float32).reshape(-1, 4)
    order = np.argsort(-np.asarray(scores, np.float64), kind="stable")
    b = b[order]
    area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    dead = np.zeros(len(b), bool)
    keep = []
    for i in range(len(b)):
        if dead[i]:
            continue
        keep.append(int(order[i]))
        w = np.maximum(np.float32(0), np.minimum(b[i, 2], b[i + 1:, 2]) - np.maximum(b[i, 0], b[i + 1:, 0]))
        h = np.maximum(np.float32(0), np.minimum(b[i, 3], b[i + 1:, 3]) - np.maximum(b[i, 1], b[i + 1:, 1]))
        inter = w * h
        with np.errstate(invalid="ignore", divide="ignore"):
            dead[i + 1:] |= inter / (area[i] + area[i + 1:] - inter) > np.float32(thr)
    return keep


def _boxes(masks):
    """batched_mask_to_box for [B, H, W] bool on the device -> float32 XYXY"""
    B, H, W = masks.shape
    in_h, in_w = masks.any(dim=2), masks.any(dim=1)
    ys, xs = torch.arange(H, device=masks.device), torch.arange(W, device=masks.device)
    bottom, right = (in_h * ys).max(dim=1).values, (in_w * xs).max(dim=1).values
    top = (in_h * ys + H * (~in_h)).min(dim=1).values
    left = (in_w * xs + W * (~in_w)).min(dim=1).values
    out = torch.stack([left, top, right, bottom], dim=1)
    return (out * ~((right < left) | (bottom < top)).unsqueeze(1)).float()


def _rle_torch(masks):
    """mask_to_rle_pytorch (utils/amg.py): the change positions on the device, one Python loop trip and one .tolist() per mask"""
    b, h, w = masks.shape
    t = masks.permute(0, 2, 1).flatten(1)
    change = (t[:, 1:] ^ t[:, :-1]).nonzero()
    out = []
    for i in range(b):
        cur = change[change[:, 0] == i, 1]
        cur = torch.cat([torch.tensor([0], dtype=cur.dtype, device=cur.device), cur + 1,
                         torch.tensor([h * w], dtype=cur.dtype, device=cur.device)])
        counts = [] if t[i, 0] == 0 else [0]
        counts.extend((cur[1:] - cur[:-1]).detach().cpu().tolist())
        out.append(counts)
    return out


def route_a(logits, iou):
    H, W = logits.shape[-2:]
    keep = iou > PRM["pred_iou_thresh"]
    lg, sc = logits[keep], iou[keep]
    idx = keep.nonzero().flatten()
    hi, lo = PRM["mask_threshold"] + PRM["stability_score_offset"], PRM["mask_threshold"] - PRM["stability_score_offset"]
    stab = (lg > hi).sum(-1, dtype=torch.int16).sum(-1, dtype=torch.int32) / (lg > lo).sum(-1, dtype=torch.int16).sum(-1, dtype=torch.int32)
    keep = stab >= PRM["stability_score_thresh"]
    lg, sc, idx = lg[keep], sc[keep], idx[keep]
    masks = lg > PRM["mask_threshold"]
    boxes = _boxes(masks)
    k = _nms_host(boxes.cpu().numpy(), sc.cpu().numpy(), PRM["box_nms_thresh"])
    kt = torch.as_tensor(k, device=logits.device, dtype=torch.long)
    rles, boxes, idx = _rle_torch(masks[kt]), boxes[kt].cpu().numpy(), idx[kt].cpu().numpy()
    new_boxes, scores, new_masks = [], [], []
    for c in rles:                                           # postprocess_small_regions, on the host as in SAM
        m = rle.decode(c, H, W)
        m2, c1 = O.remove_small_regions(m, AREA, "holes")
        m2, c2 = O.remove_small_regions(m2, AREA, "islands")
        new_masks.append(m2)
        new_boxes.append(O.mask_box(m2))
        scores.append(0.0 if (c1 or c2) else 1.0)
    k2 = _nms_host(new_boxes, scores, PRM["box_nms_thresh"])
    for j in k2:
        if scores[j] == 0.0:
            rles[j] = _rle_torch(torch.as_tensor(new_masks[j]).unsqueeze(0))[0]
            boxes[j] = new_boxes[j]
    return [rles[j] for j in k2], [idx[j] for j in k2]


def bench_shape(L, H, W):
    dev = torch.device("cuda:0")
    logits_h, iou_h = CS.seeded_logits(7, N, H, W)
    logits, iou = torch.from_numpy(logits_h).to(dev), torch.from_numpy(iou_h).to(dev)
    del logits_h
    prm = sam_post_params(L, min_mask_region_area=AREA)
    last = {}

    def route_b():
        r = sam_postprocess(logits, iou, params=prm, return_masks=False, lib_=L)
        h, i, ms = C.c_int32(0), C.c_int32(0), C.c_double(0)
        L.c.hmsg_test_sam_post_last(C.byref(h), C.byref(i), C.byref(ms))
        last.update(rounds_holes=h.value, rounds_islands=i.value, stats_ms=ms.value, device_ms=r["device_ms"])
        return r

    def timed_a():
        out = route_a(logits, iou)
        torch.cuda.synchronize()
        return out
    routes = {"a_torch_ops_and_host_scipy": timed_a, "b_hmsg_sam_postprocess": route_b}
    for fn in routes.values():
        fn()
    ra, ia = timed_a()
    rb = route_b()
    cb, ob = rb["counts"].cpu().numpy().view(np.uint32), rb["run_off"].cpu().numpy()
    same = ia == rb["keep_idx"].cpu().numpy().tolist() and all(ra[j] == cb[ob[j]:ob[j + 1]].tolist() for j in range(rb["n"]))
    wall = {k: [] for k in routes}
    dev_ms, stats_ms = [], []
    for _ in range(ROUNDS):
        for k, fn in routes.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            wall[k].append(time.perf_counter() - t0)
            if k.startswith("b_"):
                dev_ms.append(last["device_ms"] * 1e-3)
                stats_ms.append(last["stats_ms"] * 1e-3)
    rows_read = int((iou > PRM["pred_iou_thresh"]).sum())
    nbytes = rows_read * H * W * 4
    return {"frame": f"{W}x{H}", "logit_images": N, "logits_MB": round(N * H * W * 4 / 1e6, 1), "min_mask_region_area": AREA,
            "masks_out": rb["n"], "counts_out": int(ob[-1]), "rows_the_iou_filter_keeps": rows_read,
            "wall_per_frame": {k: _stats(v) for k, v in wall.items()}, "b_device_ms": _stats(dev_ms),
            "b_statistics_kernel": dict(_stats(stats_ms), bytes_read=nbytes,
                                        share_of_hbm_peak=round(nbytes / statistics.median(stats_ms) / HBM_PEAK, 4)),
            "b_labelling_rounds": {"holes": last["rounds_holes"], "islands": last["rounds_islands"]},
            "a_and_b_return_the_same_records": bool(same)}


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "sam_postprocess.json")
    L = lib()
    res = {"benchmark": "sam_postprocess", "device": torch.cuda.get_device_name(0), "rounds": ROUNDS, "hbm_peak_bytes_per_s": HBM_PEAK,
           "note": "route (a) labels with scipy.ndimage.label in place of cv2.connectedComponentsWithStats and runs its NMS on the host "
                   "(neither cv2 nor torchvision is installed); share_of_hbm_peak = bytes of the rows the IoU filter keeps over the "
                   "HIP-event time around the statistics launch",
           "shapes": [bench_shape(L, 480, 640), bench_shape(L, 720, 1280)]}
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
