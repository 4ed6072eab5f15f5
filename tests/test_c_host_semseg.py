"""The semantic segmentation score from C (tests/host_c/hmsg_host_semseg.c, strict C99 against include/hmsg.h ALONE): the host builds
a small scene as tests/host_c/hmsg_host.c does, calls hmsg_evaluate_semseg and prints the scores; they -- and the per-class IoU and the
confusion matrix it writes -- equal the same calls made through the Python binding.  CPU: the kernel simulator; -m gpu: libhmsg.so."""
import os
import subprocess

import numpy as np
import pytest

from tests import parity_common as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host_c", "hmsg_host_semseg.c")
INC = os.path.join(ROOT, "include")
LIB = os.path.join(ROOT, "holoagent_amd", "libhmsg.so")


def _compile(lib_path, out):
    cmd = ["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-O1", "-I", INC, SRC, "-o", out, lib_path,
           "-Wl,-rpath," + os.path.dirname(lib_path), "-Wl,-rpath,/opt/rocm/lib", "-Wl,--allow-shlib-undefined"]
    subprocess.run(cmd, check=True, capture_output=True)
    return out


def _run(lib_path, tmp_path):
    from holoagent_amd._lib import HmsgLib
    from holoagent_amd.synth import SceneSpec, SynthScene
    spec = SceneSpec(seed=40, rooms_x=1, rooms_z=1, room_size=(3.2, 2.6, 3.0), objects_per_room=3, width=96, height=72,
                     n_frames=6, n_masks=5, feat_dim=16, yaw_step_deg=60.0)
    scn = SynthScene(spec)
    frames = [scn.frame(i) for i in range(spec.n_frames)]
    text = np.ascontiguousarray(np.asarray(scn.text_table(5)[0], np.float32).reshape(5, -1, spec.feat_dim)[:, 0, :])
    S = PC.stack_frames(frames)
    F, (H, W), M, D, Cn, k = len(frames), frames[0]["depth"].shape, S["masks"].shape[1], spec.feat_dim, text.shape[0], 5
    over = dict(feat_dim=D, outlier_nb_points=40, feat_dbscan_min=8, outlier_radius=0.5)
    # the same scene through the binding first: the ground truth is drawn around its instance points
    L = HmsgLib(lib_path)
    sc = PC.make_scene(L, frames, over)
    sc.add_frames(S["rgb"], S["depth"], S["pose"], S["K"])
    sc.finalize_map()
    sc.add_frame_features(0, S["masks"], S["f_g"], S["f_masked"], S["f_crop"], S["n_masks"])
    sc.fuse_frames()
    sc.merge_instances()
    sc.pool_instances()
    pts = np.concatenate(sc.instances())
    rng = np.random.default_rng(23)
    m = 600
    near = pts[rng.integers(0, len(pts), 500)] + 0.03 * rng.standard_normal((500, 3))
    lo, hi = pts.min(0) - 1.0, pts.max(0) + 1.0
    gt_pts = np.ascontiguousarray(np.concatenate([near, lo + (hi - lo) * rng.random((m - 500, 3))]))
    Ln = Cn + 1                                                # class ids 0 .. C - 1 carry a text row, C is ground truth only
    gt_lab = rng.integers(0, Ln, m).astype(np.int32)
    gt_lab[0] = Cn
    ignore = np.array([0], np.int32)
    want = sc.evaluate_semseg(text, np.arange(Cn), gt_pts, gt_lab, k=k, ignore=ignore.tolist())
    assert len(want["classes"]) == Ln
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        np.array([F, H, W, M, D, Cn, k, Ln, len(ignore), over["outlier_nb_points"], over["feat_dbscan_min"],
                  int(round(over["outlier_radius"] * 1000))], np.int32).tofile(f)
        np.array([m], np.int64).tofile(f)
        for a, t in ((S["K"], np.float64), (S["rgb"], np.uint8), (S["depth"], np.uint16), (S["pose"], np.float64),
                     (S["masks"], np.uint8), (S["n_masks"], np.int32), (S["f_g"], np.float32), (S["f_masked"], np.float32),
                     (S["f_crop"], np.float32), (text, np.float32), (np.arange(Cn), np.int32), (gt_pts, np.float64), (gt_lab, np.int32),
                     (ignore, np.int32)):
            np.ascontiguousarray(a, t).tofile(f)
    exe = _compile(lib_path, str(tmp_path / "hmsg_host_semseg"))
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout + r.stderr
    words = r.stdout.split()
    printed = {words[i]: float(words[i + 1]) for i in range(0, 8, 2)}
    for key in ("miou", "fmiou", "acc", "macc"):
        assert np.array_equal(printed[key], want[key], equal_nan=True), (key, printed[key], want[key])
    assert int(words[9]) == sc.num_instances() >= 2
    raw = open(fout, "rb").read()
    scores = np.frombuffer(raw, np.float64, 4)
    per_class = np.frombuffer(raw, np.float64, Ln, 32)
    conf = np.frombuffer(raw, np.int64, Ln * Ln, 32 + 8 * Ln).reshape(Ln, Ln)
    assert len(raw) == 32 + 8 * Ln + 8 * Ln * Ln
    assert np.array_equal(scores, [want["miou"], want["fmiou"], want["acc"], want["macc"]], equal_nan=True)
    assert np.array_equal(per_class, [want["per_class_iou"][c] for c in range(Ln)], equal_nan=True)
    assert np.array_equal(conf, want["confusion"]) and conf.sum() == m
    sc.close()


@pytest.mark.skipif(not os.path.exists(PC.EMU_PATH), reason="kernel simulator not built")
def test_c_host_semseg_on_the_simulator(tmp_path):
    _run(PC.EMU_PATH, tmp_path)


@pytest.mark.gpu
def test_c_host_semseg_gpu(tmp_path):
    _run(LIB, tmp_path)
