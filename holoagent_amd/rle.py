"""SAM's uncompressed run-length masks (SamAutomaticMaskGenerator with output_mode="uncompressed_rle") in numpy: the form
include/hmsg.h's hmsg_add_frame_features_rle takes.

One mask of an H x W image is a list of counts whose sum is H * W.  The image is read in COLUMN-major order (position
t = x * H + y); even runs are zeros, odd runs are ones, so a mask that starts with a one has counts[0] == 0.  SAM's record is
{"size": [H, W], "counts": [...]}.  COCO's compressed string form (output_mode="coco_rle") is not handled."""
import numpy as np


def encode(mask):
    """bool / 0-1 array [H, W] -> counts uint32 [k]."""
    m = np.asarray(mask)
    assert m.ndim == 2, "mask: [H, W]"
    flat = (m != 0).T.reshape(-1)                            # column-major
    if flat.size == 0:
        return np.zeros(1, np.uint32)
    change = np.flatnonzero(flat[1:] != flat[:-1]) + 1       # first position of every run but the first
    edges = np.concatenate([[0], change, [flat.size]])
    counts = np.diff(edges)
    if flat[0]:
        counts = np.concatenate([[0], counts])
    return counts.astype(np.uint32)


def decode(counts, H, W):
    """counts -> bool [H, W]; raises ValueError unless they sum to H * W."""
    c = np.asarray(counts, dtype=np.int64).reshape(-1)
    if c.size == 0 or (c < 0).any() or int(c.sum()) != H * W:
        raise ValueError("run-length mask: %d counts summing to %d, H * W = %d" % (c.size, int(c.sum()), H * W))
    ones = np.zeros(c.size, bool)
    ones[1::2] = True
    return np.repeat(ones, c).reshape(W, H).T.copy()


def from_sam(seg, H=None, W=None):
    """SAM's {"size": [H, W], "counts": [...]} record (or an annotation dict that holds it under "segmentation") -> counts uint32.
    With H and W given, a record of another size raises ValueError."""
    if "counts" not in seg and "segmentation" in seg:
        seg = seg["segmentation"]
    if isinstance(seg["counts"], (str, bytes)):
        raise ValueError("COCO's compressed RLE string (output_mode='coco_rle') is not supported: use 'uncompressed_rle'")
    h, w = (int(v) for v in seg["size"])
    if H is not None and (h, w) != (int(H), int(W)):
        raise ValueError("run-length mask of size %s for a %d x %d frame" % (list(seg["size"]), H, W))
    c = np.asarray(seg["counts"], dtype=np.int64).reshape(-1)
    if c.size == 0 or (c < 0).any() or (c > 0xffffffff).any() or int(c.sum()) != h * w:
        raise ValueError("run-length mask: %d counts summing to %d, size %s" % (c.size, int(c.sum()), list(seg["size"])))
    return c.astype(np.uint32)


def pack(frames):
    """list (frames) of lists (masks) of counts -> (counts uint32 [sum k], run_off int64 [T + 1], n_masks int32 [n]): the three
    arrays of hmsg_add_frame_features_rle, masks in hand-over order."""
    per_mask = [np.asarray(c, dtype=np.uint32).reshape(-1) for fr in frames for c in fr]
    run_off = np.zeros(len(per_mask) + 1, np.int64)
    if per_mask:
        run_off[1:] = np.cumsum([c.size for c in per_mask])
    counts = np.ascontiguousarray(np.concatenate(per_mask)) if per_mask else np.zeros(0, np.uint32)
    return counts, run_off, np.array([len(fr) for fr in frames], np.int32)


def is_rle_records(masks):
    """whether an encoder output's `masks` is a list of run-length records (dicts with "counts") rather than an array"""
    if not isinstance(masks, (list, tuple)):
        return False
    if len(masks) == 0:
        return True
    rec = masks[0]
    return isinstance(rec, dict) and ("counts" in rec or (isinstance(rec.get("segmentation"), dict) and "counts" in rec["segmentation"]))
