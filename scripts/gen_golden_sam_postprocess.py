"""Writes tests/golden/sam_postprocess.npz: the expected outputs of hmsg_sam_postprocess for the cases of tests/sam_post_cases.py,
made with the numpy + scipy restatement tests/sam_post_oracle.py.  Outputs only -- the inputs are re-made from their seeds by the
tests, which so hold where scipy is missing and compare against the live restatement where it is there.

    python scripts/gen_golden_sam_postprocess.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import sam_post_cases as CS  # noqa: E402
from tests import sam_post_oracle as O  # noqa: E402


def main():
    out = {}
    for name, logits, iou, prm in CS.cases():
        r = O.postprocess(logits, iou, **prm)
        for k in CS.RESULT_KEYS:
            out[name + "/" + k] = np.packbits(r[k]) if k == "masks" else (r[k].view(np.uint32) if k == "stability_score" else r[k])
        print("%-28s N = %3d -> %3d masks, %5d counts  %s" % (name, len(iou), r["n"], len(r["counts"]), r["stage"]))
    path = os.path.join(ROOT, "tests", "golden", "sam_postprocess.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
