"""open_clip's inference `preprocess` restated in numpy: torchvision's Resize(S) / CenterCrop(S) size rules, Pillow's 8-bit
BICUBIC resample (src/libImaging/Resample.c: precompute_coeffs, normalize_coeffs_8bpc, ImagingResampleHorizontal_8bpc /
Vertical_8bpc), ToTensor and Normalize.  The oracle of the device path is Pillow itself (tests/golden/clip_preprocess.npz, or
the installed Pillow); this restatement stands in only where Pillow cannot be imported, and states the integer tables that
holoagent_amd/csrc/hmsg_resample_coef.h must reproduce (tests/test_resample_coef.py)."""
import math

import numpy as np

PRECISION_BITS = 22
MEAN = (0.48145466, 0.4578275, 0.40821073)          # open_clip's OPENAI_DATASET_MEAN / _STD
STD = (0.26862954, 0.26130258, 0.27577711)


def resize_dims(H, W, S):
    """torchvision Resize(S) on a PIL image -> (w', h')"""
    if W <= H:
        return S, int(S * H / W)
    return int(S * W / H), S


def center_crop_offset(n, S):
    return int(round((n - S) / 2.0))                # Python's round: halves to even


def bicubic(x, a=-0.5):
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def coefficients(in_size, out_size):
    """-> (bounds int64 [out, 2] = (xmin, taps), kk int64 [out, ksize])"""
    scale = filterscale = in_size / out_size
    if filterscale < 1.0:
        filterscale = 1.0
    support = 2.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((out_size, 2), np.int64)
    kk = np.zeros((out_size, ksize), np.int64)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        ss = 1.0 / filterscale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = [bicubic((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        for x, v in enumerate(w):
            kk[xx, x] = int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS))
        bounds[xx] = (xmin, xmax)
    return bounds, kk


def _pass(a, out_size):
    """resample axis 1 of a uint8 [R, C, 3]; equal lengths: no pass"""
    if a.shape[1] == out_size:
        return a
    bounds, kk = coefficients(a.shape[1], out_size)
    out = np.empty((a.shape[0], out_size, a.shape[2]), np.uint8)
    ai = a.astype(np.int64)
    for xx in range(out_size):
        x0, n = bounds[xx]
        ss = (1 << (PRECISION_BITS - 1)) + (ai[:, x0:x0 + n, :] * kk[xx, :n, None]).sum(axis=1)
        out[:, xx, :] = np.clip(ss >> PRECISION_BITS, 0, 255)
    return out


def resize_bicubic_u8(img, w, h):
    """Image.fromarray(img).resize((w, h), Image.BICUBIC) as an array"""
    t = _pass(img, w)                                                     # horizontal, then a uint8 image, then vertical
    return np.ascontiguousarray(_pass(t.transpose(1, 0, 2), h).transpose(1, 0, 2))


def resize_center_crop_u8(img, S=224, resize=resize_bicubic_u8):
    """np.asarray(CenterCrop(S)(Resize(S, BICUBIC)(Image.fromarray(img)))) -> uint8 [S, S, 3]"""
    H, W = img.shape[:2]
    w2, h2 = resize_dims(H, W, S)
    r = img if (w2, h2) == (W, H) else resize(img, w2, h2)
    top, left = center_crop_offset(h2, S), center_crop_offset(w2, S)
    return np.ascontiguousarray(r[top:top + S, left:left + S])


def pil_resize(img, w, h):
    from PIL import Image
    return np.asarray(Image.fromarray(img).resize((w, h), Image.BICUBIC))


def normalize_table(mean=MEAN, std=STD):
    """float32 [3, 256]: ToTensor + Normalize of every byte value per channel"""
    v = np.arange(256, dtype=np.float32) / np.float32(255.0)
    m, s = np.asarray(mean, np.float32), np.asarray(std, np.float32)
    return ((v[None, :] - m[:, None]) / s[:, None]).astype(np.float32)


def to_tensor_normalize(u8, mean=MEAN, std=STD):
    """uint8 [.., S, S, 3] -> float32 [.., 3, S, S]"""
    x = u8.astype(np.float32) / np.float32(255.0)
    x = (x - np.asarray(mean, np.float32)) / np.asarray(std, np.float32)
    return np.ascontiguousarray(np.moveaxis(x.astype(np.float32), -1, -3))


# ---- the cases of tests/test_clip_preprocess.py and scripts/gen_golden_clip_preprocess.py: (name, B, H, W, S)
CASES = [
    ("crop512", 3, 512, 512, 224),        # the crop case, ksize 11
    ("landscape", 1, 480, 640, 224),      # left = 37
    ("halfeven", 1, 480, 641, 224),       # left = 37.5 -> 38
    ("portrait", 1, 640, 480, 224),       # crop along y
    ("upscale", 1, 100, 37, 224),         # filterscale = 1, top = 190.5 -> 190
    ("identity", 1, 224, 224, 224),       # nothing resampled, nothing cropped
    ("cropx", 1, 224, 500, 224),          # the shorter side is S already: nothing resampled, crop along x
    ("cropy", 1, 300, 224, 224),          # the same, crop along y
    ("pixel", 2, 1, 1, 224),              # a single pixel
    ("s336", 1, 512, 512, 336),           # another tile shape
    ("s30", 1, 512, 512, 30),             # a ragged last tile, large scale
    ("fewrows", 1, 1500, 1500, 224),      # the source rows of 16 output rows exceed the LDS budget: fewer rows per tile
]
KINDS = ("bytes", "binary")               # random bytes | 0 / 255 noise (overshoot: the clamp at both ends)


def case_seed(name, kind):
    return 1000 + 2 * [c[0] for c in CASES].index(name) + KINDS.index(kind)


def make_input(name, kind):
    """uint8 [B, H, W, 3] of a case"""
    _, B, H, W, _ = next(c for c in CASES if c[0] == name)
    rng = np.random.default_rng(case_seed(name, kind))
    if kind == "bytes":
        return rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    return np.where(rng.random((B, H, W, 3)) < 0.5, 0, 255).astype(np.uint8)


def subsample(u8, i):
    """the strided sub-sample of image i of a batch that the golden file keeps (the scheme of tests/golden/crops.npz)"""
    return u8[(i % 8)::8, ((3 * i) % 8)::8]
