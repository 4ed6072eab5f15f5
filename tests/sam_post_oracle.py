"""numpy + scipy.ndimage.label restatement of hmsg_sam_postprocess (include/hmsg.h, the numbered steps there): what
SamAutomaticMaskGenerator.generate does behind predict_torch for crop_n_layers = 0 -- segment_anything/automatic_mask_generator.py
_process_batch / postprocess_small_regions, utils/amg.py calculate_stability_score / batched_mask_to_box / remove_small_regions /
mask_to_rle_pytorch / box_xyxy_to_xywh, torchvision.ops.nms.  The labelling structure is all ones (8-connectivity), components
are numbered as scipy numbers them (by their first pixel in row-major order).  Every float operation is one float32 operation."""
import numpy as np

from holoagent_amd import rle

F = np.float32
DEFAULTS = dict(pred_iou_thresh=0.88, stability_score_thresh=0.95, stability_score_offset=1.0, mask_threshold=0.0, box_nms_thresh=0.7,
                min_mask_region_area=0)


def have_scipy():
    try:
        import scipy.ndimage  # noqa: F401
        return True
    except Exception:
        return False


def stability_score(logit, mask_threshold, offset):
    hi, lo = F(mask_threshold) + F(offset), F(mask_threshold) - F(offset)
    with np.errstate(invalid="ignore", divide="ignore"):
        return F(np.count_nonzero(logit > hi)) / F(np.count_nonzero(logit > lo))


def mask_box(mask):
    """batched_mask_to_box of one mask: XYXY float32, inclusive indices; empty -> zeros"""
    ys, xs = np.nonzero(mask)
    if ys.size == 0:
        return np.zeros(4, F)
    return np.array([xs.min(), ys.min(), xs.max(), ys.max()], F)


def nms(boxes, scores, thresh):
    """torchvision.ops.nms in float32; ties by position (stable)"""
    boxes = np.asarray(boxes, F).reshape(-1, 4)
    scores = np.asarray(scores, F)
    thresh = F(thresh)
    order = np.argsort(-scores.astype(np.float64), kind="stable")
    areas = (boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])
    dead = np.zeros(len(boxes), bool)
    keep = []
    for a, i in enumerate(order):
        if dead[i]:
            continue
        keep.append(int(i))
        for j in order[a + 1:]:
            if dead[j]:
                continue
            w = max(F(0), min(boxes[i, 2], boxes[j, 2]) - max(boxes[i, 0], boxes[j, 0]))
            h = max(F(0), min(boxes[i, 3], boxes[j, 3]) - max(boxes[i, 1], boxes[j, 1]))
            inter = F(w) * F(h)
            with np.errstate(invalid="ignore", divide="ignore"):
                if inter / (areas[i] + areas[j] - inter) > thresh:
                    dead[j] = True
    return keep


def remove_small_regions(mask, area, mode):
    """utils/amg.py remove_small_regions with scipy's labelling in place of cv2.connectedComponentsWithStats -> (mask, changed)"""
    from scipy import ndimage
    holes = mode == "holes"
    working = mask ^ holes
    regions, n = ndimage.label(working, structure=np.ones((3, 3), int))
    sizes = np.bincount(regions.reshape(-1), minlength=n + 1)[1:]
    small = [i + 1 for i, s in enumerate(sizes) if s < area]
    if not small:
        return mask, False
    fill = [0] + small
    if not holes:
        fill = [i for i in range(n + 1) if i not in fill]
        if not fill:
            fill = [int(np.argmax(sizes)) + 1]           # (argmax: the first of equally large ones)
    return np.isin(regions, fill), True


def postprocess(logits, iou_preds, **params):
    """-> dict(n, keep_idx, counts, run_off, bbox, area, stability_score, masks, stage=...)"""
    p = dict(DEFAULTS, **params)
    logits = np.asarray(logits, F)
    H, W = logits.shape[-2:]
    logits = logits.reshape(-1, H, W)
    iou = np.asarray(iou_preds, F).reshape(-1)
    rows = [i for i in range(len(iou)) if not F(p["pred_iou_thresh"]) > 0 or iou[i] > F(p["pred_iou_thresh"])]
    stab = {i: stability_score(logits[i], p["mask_threshold"], p["stability_score_offset"]) for i in rows}
    if F(p["stability_score_thresh"]) > 0:
        rows = [i for i in rows if stab[i] >= F(p["stability_score_thresh"])]
    masks = [logits[i] > F(p["mask_threshold"]) for i in rows]
    boxes = [mask_box(m) for m in masks]
    keep = nms(boxes, iou[rows], p["box_nms_thresh"])
    rows, masks, boxes = [rows[k] for k in keep], [masks[k] for k in keep], [boxes[k] for k in keep]
    stage = dict(after_first_nms=len(rows))
    area = int(p["min_mask_region_area"])
    if area > 0 and rows:
        new, scores = [], []
        for m in masks:
            m2, c1 = remove_small_regions(m, area, "holes")
            m2, c2 = remove_small_regions(m2, area, "islands")
            new.append(m2)
            scores.append(0.0 if (c1 or c2) else 1.0)
        keep = nms([mask_box(m) for m in new], scores, p["box_nms_thresh"])
        stage.update(changed_kept=sum(1 for k in keep if scores[k] == 0.0), unchanged_kept=sum(1 for k in keep if scores[k] == 1.0))
        for k in keep:
            if scores[k] == 0.0:
                masks[k], boxes[k] = new[k], mask_box(new[k])
        rows, masks, boxes = [rows[k] for k in keep], [masks[k] for k in keep], [boxes[k] for k in keep]
    stage["after_second_nms"] = len(rows)
    recs = [rle.encode(m) for m in masks]
    counts, run_off, _ = rle.pack([recs])
    bbox = np.array([[b[0], b[1], b[2] - b[0], b[3] - b[1]] for b in boxes], np.float64).reshape(-1, 4)
    return dict(n=len(rows), keep_idx=np.array(rows, np.int32), counts=counts, run_off=run_off, bbox=bbox,
                area=np.array([int(c[1::2].sum()) for c in recs], np.int32), stability_score=np.array([stab[i] for i in rows], F),
                masks=np.array(masks, np.uint8).reshape(-1, H, W), stage=stage)
