"""The host arithmetic of the CLIP preprocess (holoagent_amd/csrc/hmsg_resample_coef.h: Pillow's BICUBIC coefficient tables in
int32, torchvision's Resize / CenterCrop size rules, the ToTensor + Normalize table, float32 -> float16) against the numpy
restatement (tests/clip_preprocess_oracle.py), integer for integer.  tests/host_cpp/resample_coef.cpp, a stand-alone program
with its own main that includes nothing but that header, is built and run here twice -- plain, and with the address and
undefined-behaviour sanitizers of the host compiler.  Nothing of it is loaded into Python and no GPU is involved."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import clip_preprocess_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host_cpp", "resample_coef.cpp")
INC = os.path.join(ROOT, "holoagent_amd", "csrc")


def _pairs():
    """about 200 (inSize, outSize): the axes of the device test's cases, small sizes against each other, 4000 -> 224"""
    p = []
    for _, _, H, W, S in O.CASES:
        w2, h2 = O.resize_dims(H, W, S)
        p += [(W, w2), (H, h2)]
    p += [(720, 224), (1280, 398), (4000, 224), (16384, 224), (7, 224), (9, 288), (224, 1024)]
    p += [(a, b) for a in range(1, 13) for b in range(1, 13)]
    p += [(a, b) for a in range(13, 41, 3) for b in (1, 7, 19, 40)] + [(b, a) for a in range(13, 41, 3) for b in (1, 7, 19, 40)]
    return sorted(set(p))


def _shapes():
    s = [(H, W, S) for _, _, H, W, S in O.CASES]
    s += [(480, 641, 224), (641, 480, 224), (100, 37, 224), (720, 1280, 224), (1080, 1920, 336), (7, 9, 224), (3, 1000, 5), (225, 224, 224),
          (226, 224, 224), (227, 224, 224), (224, 229, 224)]
    return s + [(h, w, s_) for h in (1, 2, 3, 5, 8) for w in (1, 2, 3, 5, 8) for s_ in (1, 2, 7)]


def _run(tmp_path, name, flags):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ is needed to build tests/host_cpp/resample_coef.cpp")
    exe = str(tmp_path / name)
    r = subprocess.run([cxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-I", INC, SRC, "-o", exe] + flags,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    pairs, shapes = _pairs(), _shapes()
    rng = np.random.default_rng(7)
    halves = np.concatenate([rng.integers(0, 2 ** 32, 2000, dtype=np.uint64).astype(np.uint32),
                             np.array([0, 0x80000000, 0x33000000, 0x33000001, 0x387fc000, 0x387fe000, 0x38800000, 0x477fe000, 0x477ff000,
                                       0x7f800000, 0x3f801000, 0x3f803000, 0x3f802000, 0x3f802001], np.uint32)])
    halves = halves[np.isfinite(halves.view(np.float32))]
    req = [f"C {a} {b}" for a, b in pairs] + ["W 512 224 0 224", "W 640 298 37 224", "W 100 605 190 224", "W 5 3 3 0"]
    req += [f"R {h} {w} {s}" for h, w, s in shapes] + ["L"] + [f"H {int(v)}" for v in halves]
    r = subprocess.run([exe], input="\n".join(req) + "\n", capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.splitlines()
    assert lines[-1] == "resample_coef ok %d" % len(req)
    it = iter(lines)
    n_coef = 0
    for a, b in pairs:
        bounds, kk = O.coefficients(a, b)
        assert next(it) == f"C {a} {b} {kk.shape[1]}", (a, b)
        for i in range(b):
            got = [int(v) for v in next(it).split()]
            assert got == [int(bounds[i, 0]), int(bounds[i, 1])] + [int(v) for v in kk[i]], (a, b, i)
            n_coef += kk.shape[1]
    for a, b, first, count in ((512, 224, 0, 224), (640, 298, 37, 224), (100, 605, 190, 224), (5, 3, 3, 0)):
        bounds, kk = O.coefficients(a, b)
        assert next(it) == f"W {a} {b} {kk.shape[1]}"
        for i in range(first, first + count):
            assert [int(v) for v in next(it).split()] == [int(bounds[i, 0]), int(bounds[i, 1])] + [int(v) for v in kk[i]], (a, b, i)
    for h, w, s in shapes:
        w2, h2 = O.resize_dims(h, w, s)
        assert next(it) == f"R {h} {w} {s} {w2} {h2} {O.center_crop_offset(w2, s)} {O.center_crop_offset(h2, s)}"
    assert next(it) == "L"
    lut = O.normalize_table().reshape(-1)
    for i in range(768):
        assert next(it) == f"{int(lut[i].view(np.uint32))} {int(lut[i].astype(np.float16).view(np.uint16))}", i
    with np.errstate(over="ignore"):
        want = halves.view(np.float32).astype(np.float16).view(np.uint16)
    for v, wv in zip(halves, want):
        assert next(it) == f"H {int(wv)}", hex(int(v))
    return len(pairs), n_coef


def test_header_tables_equal_the_restatement(tmp_path):
    n_pairs, n_coef = _run(tmp_path, "resample_coef", ["-O2"])
    assert n_pairs >= 200 and n_coef > 20000


def test_header_under_the_host_sanitizers(tmp_path):
    _run(tmp_path, "resample_coef_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"])
