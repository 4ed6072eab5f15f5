"""Writes tests/golden/clip_preprocess.npz with Pillow: for every case of tests/clip_preprocess_oracle.py (CASES x KINDS) the
seed, the shape, a strided sub-sample and the SHA-1 of np.asarray(CenterCrop(S)(Resize(S, BICUBIC)(Image.fromarray(img)))) --
Pillow's own resample; the size rules of torchvision's Resize / CenterCrop as the oracle module states them.
    python scripts/gen_golden_clip_preprocess.py [out.npz]"""
import hashlib
import os
import sys

import numpy as np
import PIL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import clip_preprocess_oracle as O  # noqa: E402


def main(path):
    out = {"pillow_version": np.array(PIL.__version__)}
    for name, B, H, W, S in O.CASES:
        for kind in O.KINDS:
            imgs = O.make_input(name, kind)
            res = [O.resize_center_crop_u8(im, S, O.pil_resize) for im in imgs]
            key = f"{name}_{kind}"
            out[key + "_seed"] = np.array(O.case_seed(name, kind), np.int64)
            out[key + "_shape"] = np.array([B, H, W, S], np.int64)
            out[key + "_sub"] = np.stack([O.subsample(r, i) for i, r in enumerate(res)])
            out[key + "_sha1"] = np.array([hashlib.sha1(np.ascontiguousarray(r).tobytes()).hexdigest() for r in res])
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes, Pillow", PIL.__version__)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "clip_preprocess.npz"))
