"""What hmsg_sam_postprocess returns (holoagent_amd._lib.sam_postprocess) as the records SamAutomaticMaskGenerator.generate
returns in output_mode="uncompressed_rle" (segment_anything/automatic_mask_generator.py generate, the `curr_anns` loop): for a
caller that keeps the reference's list-of-dicts interface.  The device path does not need it -- encoder_handoff.handoff_frame_logits
hands the device arrays on as they are."""
import numpy as np


def _host(a):
    return a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)


def to_sam_records(result, H, W, iou_preds, points=None):
    """result: the dict of sam_postprocess (numpy arrays or device tensors); iou_preds [N] (or [P, 3]) as given to it; points
    (optional) [N, 2] (or [P, 2] with three masks per prompt): the prompt of every logit image.  -> list of dicts with
    segmentation {"size": [H, W], "counts": [...]}, area, bbox (XYWH), predicted_iou, stability_score, crop_box (the whole image,
    XYWH) and, with points, point_coords -- rle.from_sam takes every one of them unchanged."""
    counts = _host(result["counts"]).view(np.uint32)
    run_off, keep = _host(result["run_off"]), _host(result["keep_idx"])
    bbox, area, stab = _host(result["bbox"]), _host(result["area"]), _host(result["stability_score"])
    iou = _host(iou_preds).reshape(-1)
    if points is not None:
        points = _host(points).reshape(-1, 2)
        per = max(iou.size // max(len(points), 1), 1)             # masks per prompt (3 with multimask_output)
    recs = []
    for j in range(int(result["n"])):
        i = int(keep[j])
        r = {"segmentation": {"size": [int(H), int(W)], "counts": [int(c) for c in counts[run_off[j]:run_off[j + 1]]]},
             "area": int(area[j]), "bbox": [float(v) for v in bbox[j]], "predicted_iou": float(iou[i]),
             "stability_score": float(stab[j]), "crop_box": [0, 0, int(W), int(H)]}
        if points is not None:
            r["point_coords"] = [[float(v) for v in points[i // per]]]
        recs.append(r)
    return recs
