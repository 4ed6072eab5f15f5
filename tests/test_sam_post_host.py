"""The host decisions of hmsg_sam_postprocess (holoagent_amd/csrc/hmsg_sam_post_host.h: the predicted-IoU and stability filters,
the boxes, both NMS passes, the statistics kernel's launch plan) against the numpy restatement tests/sam_post_oracle.py, exactly.
tests/host_cpp/sam_post_host.cpp, a stand-alone program with its own main that includes nothing but that header, is built and run
here twice -- plain, and with the address and undefined-behaviour sanitizers of the host compiler.  Nothing of it is loaded into
Python and no GPU is involved."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import sam_post_cases as CS
from tests import sam_post_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host_cpp", "sam_post_host.cpp")
INC = os.path.join(ROOT, "holoagent_amd", "csrc")
F = np.float32


def _bits(v):
    return int(np.asarray(v, F).reshape(1).view(np.uint32)[0])


def _stats(logits, prm):
    """the seven integers per mask the device leaves (SpStats)"""
    p = dict(O.DEFAULTS, **prm)
    t, off = F(p["mask_threshold"]), F(p["stability_score_offset"])
    rows = []
    for lg in logits:
        m = lg > t
        b = O.mask_box(m).astype(int) if m.any() else (0x7fffffff, 0x7fffffff, -1, -1)
        rows.append((int((lg > t + off).sum()), int(m.sum()), int((lg > t - off).sum())) + tuple(int(v) for v in b))
    return rows


def _second_tables():
    """random tables for the second NMS: boxes that overlap heavily, zero-width ones, an empty mask, all ties within a score"""
    rng = np.random.default_rng(3)
    tables = []
    for K in (0, 1, 2, 17, 70):
        x0, y0 = rng.integers(0, 20, K), rng.integers(0, 20, K)
        x1, y1 = x0 + rng.integers(0, 12, K), y0 + rng.integers(0, 12, K)
        if K >= 17:
            x0[3:6], y0[3:6], x1[3:6], y1[3:6] = x0[0], y0[0], x1[0], y1[0]      # copies of box 0
            x1[7] = x0[7]                                                           # zero width, twice
            x0[8], y0[8], x1[8], y1[8] = x0[7], y0[7], x1[7], y1[7]
        n_mid = rng.integers(1, 50, K)
        if K >= 2:
            n_mid[1] = 0                                                            # an empty mask: box [0, 0, 0, 0]
        for thr in (0.7, 0.3):
            tables.append((K, thr, rng.integers(0, 2, K), n_mid, x0, y0, x1, y1))
    return tables


def _run(tmp_path, name, flags):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ is needed to build tests/host_cpp/sam_post_host.cpp")
    exe = str(tmp_path / name)
    r = subprocess.run([cxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-I", INC, SRC, "-o", exe] + flags,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    req, first = [], []
    for cname, logits, iou, prm in CS.cases():
        p = dict(O.DEFAULTS, **prm)
        st = _stats(logits, prm)
        req.append("F %d %d %d %d" % (len(iou), _bits(p["pred_iou_thresh"]), _bits(p["stability_score_thresh"]), _bits(p["box_nms_thresh"])))
        req += ["%d %d %d %d %d %d %d %d" % ((_bits(iou[i]),) + st[i]) for i in range(len(iou))]
        first.append((cname, logits, iou, p))
    second = _second_tables()
    for K, thr, ch, n_mid, x0, y0, x1, y1 in second:
        req.append("S %d %d" % (K, _bits(thr)))
        req += ["%d %d %d %d %d %d" % (ch[k], n_mid[k], x0[k], y0[k], x1[k], y1[k]) for k in range(K)]
    sizes = [1, 37 * 53, 4096, 4097, 640 * 480, 1280 * 720, (1 << 24) - 1]
    req += ["B %d" % s for s in sizes]
    n_req = len(first) + len(second) + len(sizes)
    r = subprocess.run([exe], input="\n".join(req) + "\n", capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.splitlines()
    assert lines[-1] == "sam_post_host ok %d" % n_req
    it = iter(lines)
    n_kept = 0
    for cname, logits, iou, p in first:
        head, rows, keep, stab = _split(next(it))
        assert head == "F", cname
        thr = F(p["pred_iou_thresh"])
        assert rows == [i for i in range(len(iou)) if not thr > 0 or iou[i] > thr], cname
        want = O.postprocess(logits, iou, **dict(p, min_mask_region_area=0))          # (area 0: the first NMS' order is the output's)
        assert keep == want["keep_idx"].tolist(), cname
        assert stab == want["stability_score"].view(np.uint32).tolist(), cname
        n_kept += len(keep)
    for K, thr, ch, n_mid, x0, y0, x1, y1 in second:
        head, keep = _split(next(it))[:2]
        boxes = [[x0[k], y0[k], x1[k], y1[k]] if n_mid[k] > 0 else [0, 0, 0, 0] for k in range(K)]
        assert head == "S" and keep == O.nms(boxes, [0.0 if ch[k] else 1.0 for k in range(K)], thr), (K, thr)
    for s in sizes:
        blocks = int(next(it).split()[1])
        assert 1 <= blocks <= 1024 and (blocks == 1024 or (blocks - 1) * 16384 < s <= blocks * 16384)     # four trips of 4096 elements
    return n_kept


def _split(line):
    """'F 1 2 | 2 1 | 9 9' -> ('F', [1, 2], [2, 1], [9, 9])"""
    parts = line[1:].split("|")
    return (line[0],) + tuple([int(v) for v in p.split()] for p in parts)


def test_host_decisions_equal_the_restatement(tmp_path):
    assert _run(tmp_path, "sam_post_host", ["-O2"]) > 100


def test_header_under_the_host_sanitizers(tmp_path):
    _run(tmp_path, "sam_post_host_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"])
