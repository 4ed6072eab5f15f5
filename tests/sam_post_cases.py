"""Inputs of the hmsg_sam_postprocess tests: seeded generators (ellipses with sharp or soft edges, with small holes, with far-away
specks, specks only, near-duplicates: what a SAM decoder's batch looks like to the post-processing) and hand-made masks, each
there because a kernel can go wrong on it.  37 x 53: neither side a multiple of 4 or 64, H * W odd (every second mask of the batch
starts off a 16-byte boundary).  Everything is re-made from seeds; tests/golden/sam_postprocess.npz holds the expected outputs."""
import numpy as np

H0, W0 = 37, 53


def seeded_logits(seed, N, H, W):
    """-> logits f32 [N, H, W], iou_preds f32 [N].  Kinds in turn: sharp ellipse, sharp with holes, sharp with specks, soft
    (dropped by the stability filter), specks only, near-duplicate of the mask three places before."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    s = min(H, W) / 37.0
    logits = np.empty((N, H, W), np.float32)
    iou = rng.uniform(0.84, 0.99, N).astype(np.float32)
    shapes = []
    for i in range(N):
        kind = i % 6
        if kind == 5 and i >= 3:
            cy, cx, ry, rx = shapes[i - 3]
            cy = cy + rng.integers(-1, 2)
        else:
            ry, rx = rng.uniform(4, 11, 2) * s
            cy, cx = rng.uniform(2, H - 2), rng.uniform(2, W - 2)
        shapes.append((cy, cx, ry, rx))
        d = np.sqrt(((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2)
        lg = (1.0 - d) * (3.0 if kind == 3 else 200.0)
        if kind == 4:
            lg[:] = -9.0
        if kind == 1:                                   # holes of 1 .. 5 x 1 .. 5 pixels inside
            for _ in range(4):
                hy, hx = int(cy + rng.uniform(-0.5, 0.5) * ry), int(cx + rng.uniform(-0.5, 0.5) * rx)
                h, w = rng.integers(1, 6, 2)
                lg[max(hy, 0):max(hy, 0) + h, max(hx, 0):max(hx, 0) + w] = -7.0
        if kind in (2, 4):                              # specks of 1 .. 4 x 1 .. 4 pixels anywhere
            for _ in range(5):
                py, px = rng.integers(0, H), rng.integers(0, W)
                h, w = rng.integers(1, 5, 2)
                lg[py:py + h, px:px + w] = 6.0
        logits[i] = lg
    return logits, iou


def _lg(mask):
    return np.where(mask, np.float32(5.0), np.float32(-5.0)).astype(np.float32)


def hand_rle(H=H0, W=W0):
    """run-length edge cases (no small-region pass)"""
    m = np.zeros((7, H, W), bool)
    m[0, 0:5, 0:4] = True                               # pixel (0, 0) set: a leading 0
    m[1] = True                                         # the full image: [0, H * W]
    #   2: empty after thresholding (survives with stability threshold 0)
    m[3, H - 8:, 10:12] = True                          # a run that goes on across a column end ...
    m[3, :6, 11:13] = True
    m[4, H - 4:, 20] = True                             # ... one that ends exactly there, one that starts at a column's top
    m[4, :4, 30] = True
    m[5, H - 3:, W - 2:] = True                         # the last pixel set: no closing run of zeros
    m[5, 10, 5] = True
    m[6, 3:30, 7] = True                                # zero-width boxes: 0 / 0 in the NMS (7 and its copy below)
    masks = np.concatenate([m, m[6:7]])
    iou = np.array([0.95, 0.94, 0.93, 0.92, 0.92, 0.92, 0.9, 0.9], np.float32)      # equal scores: stable order
    return _lg(masks), iou


def hand_cc(H=H0, W=W0, A=6):
    """labelling cases for min_mask_region_area = A (the comparison is a strict <)"""
    m = np.zeros((8, H, W), bool)
    m[0, 5:7, 5:7] = True                               # two 2 x 2 blocks joined by a diagonal only: one component of 8 >= A
    m[0, 7:9, 7:9] = True
    m[1, 2:30, 2:40] = True                             # ... and the same as holes: one hole of 8, not filled
    m[1, 10:12, 10:12] = False
    m[1, 12:14, 12:14] = False
    for r in range(1, H - 1, 2):                        # a serpentine through the whole image (its complement is one too)
        m[2, r, 1:W - 1] = True
        if r + 2 < H - 1:
            m[2, r + 1, (W - 2) if (r // 2) % 2 == 0 else 1] = True
    m[3, 2:20, 2:30] = True                             # holes of exactly A (stays) and A - 1 (filled)
    m[3, 5:7, 5:8] = False
    m[3, 10, 5:5 + A - 1] = False
    m[3, 25:27, 40:43] = True                           # islands of exactly A (stays) and A - 1 (goes)
    m[3, 30, 40:40 + A - 1] = True
    m[4, 10:12, 40:42] = True                           # two equally large small components and nothing else: the one whose
    m[4, 12:14, 5:7] = True                             # first pixel comes first in ROW-major order stays
    m[5, 0:6, 20:30] = True                             # a hole on the image's border (not exempt) and a lone pixel
    m[5, 0, 22:25] = False
    m[5, 2, 50] = True
    m[6, 3:30, 7] = True                                # zero-width boxes again, now through both NMS passes
    m[7, 15:19, 30:50] = True                           # nothing to do: keeps score 1.0
    masks = np.concatenate([m, m[6:7]])
    iou = np.array([0.95, 0.94, 0.93, 0.92, 0.92, 0.92, 0.9, 0.89, 0.9], np.float32)
    return _lg(masks), iou


def many(H=H0, W=W0):
    """more than 64 survivors: 3 x 3 blocks on a grid (and as many rows the IoU filter drops, which are never read)"""
    masks = []
    for r in range(1, H - 3, 5):
        for c in range(1, W - 3, 4):
            m = np.zeros((H, W), bool)
            m[r:r + 3, c:c + 3] = True
            masks.append(m)
    masks = np.array(masks)
    n = len(masks)
    lg = np.concatenate([_lg(masks), np.full((n, H, W), np.float32(np.nan))])
    iou = np.concatenate([np.linspace(0.99, 0.9, n), np.full(n, 0.1)]).astype(np.float32)
    order = np.random.default_rng(5).permutation(2 * n)
    return lg[order], iou[order]


HAND = dict(pred_iou_thresh=0.5, stability_score_thresh=0.0, box_nms_thresh=0.95)


def cases():
    """-> list of (name, logits, iou_preds, params)"""
    seeded = seeded_logits(11, 100, H0, W0)
    soft = seeded_logits(12, 70, H0, W0)
    out = [("seeded_area12", *seeded, dict(min_mask_region_area=12)),
           ("seeded_area0", *seeded, dict()),
           ("seeded_mask_threshold", *seeded, dict(min_mask_region_area=12, mask_threshold=0.5, stability_score_offset=0.75)),
           ("hand_rle", *hand_rle(), dict(HAND)),
           ("hand_cc", *hand_cc(), dict(HAND, min_mask_region_area=6)),
           ("hand_cc_off", *hand_cc(), dict(HAND)),
           ("many", *many(), dict(pred_iou_thresh=0.5, min_mask_region_area=4)),
           ("all_filtered_by_iou", seeded[0][:70], np.full(70, 0.5, np.float32), dict(min_mask_region_area=12)),
           ("all_filtered_by_stability", soft[0][3::6], np.full(len(soft[0][3::6]), 0.95, np.float32), dict(min_mask_region_area=12)),
           ("n0", np.zeros((0, H0, W0), np.float32), np.zeros(0, np.float32), dict(min_mask_region_area=12))]
    return [(n, np.ascontiguousarray(l), np.ascontiguousarray(i), p) for n, l, i, p in out]


RESULT_KEYS = ("keep_idx", "counts", "run_off", "bbox", "area", "stability_score", "masks")
