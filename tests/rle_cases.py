"""Shared cases of the run-length mask tests (tests/test_rle_masks.py on the kernel simulator, tests/test_rle_masks_gpu.py on the
MI355X): edge-case masks, a numpy reference of the membership bitsets that is independent of k_bitset, a small ragged scene, a
Scene whose dense hand-over goes through the run-length call, and the strict-C host."""
import os
import subprocess

import numpy as np

from holoagent_amd import rle
from tests import parity_common as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H0, W0 = 37, 50              # H * W = 1850 is no multiple of 16; neither side is a multiple of the 64-column tile or its rows
M_CASES = (1, 64, 65, 130, 256)
SAME_PIXEL = (11, 23)        # (y, x) every mask of the "full word" frame covers


def numpy_bitsets(masks, M=None):
    """bool [M, H, W] -> uint64 [H * W, NW], NW = ceil(max(M, 1) / 64): bit i & 63 of word i >> 6 of pixel y * W + x = masks[i, y, x]"""
    masks = np.asarray(masks).astype(bool)
    M = masks.shape[0] if M is None else M
    HW = masks.shape[1] * masks.shape[2]
    out = np.zeros((HW, (max(M, 1) + 63) // 64), np.uint64)
    for i in range(masks.shape[0]):
        out[:, i >> 6] |= masks[i].reshape(-1).astype(np.uint64) << np.uint64(i & 63)
    return out


def _with_zero_counts(counts):
    """the same mask with empty runs put in: two in front (an empty zero-run and an empty one-run), and the longest run split in
    two around an empty run of the other kind"""
    c = [int(v) for v in counts]
    j = int(np.argmax(c))
    a = c[j] // 2
    c = c[:j] + [a, 0, c[j] - a] + c[j + 1:]
    return np.array([0, 0] + c, np.uint32)


def edge_masks(H=H0, W=W0):
    """[(name, counts, dense bool [H, W])]: the masks a decoder can get wrong"""
    z = lambda: np.zeros((H, W), bool)
    out = []
    out.append(("empty", z()))
    out.append(("full", ~z()))
    m = z(); m[:5, 0] = True; m[20:, 7] = True
    out.append(("starts with a one", m))
    m = z(); m[0, 0] = True
    out.append(("pixel (0, 0)", m))
    m = z(); m[H - 1, W - 1] = True
    out.append(("pixel (H-1, W-1)", m))
    m = z(); m[H - 9:, 12] = True                      # ... ends with column 12, column 13 starts with a zero
    out.append(("run ends on a column boundary", m))
    m = z(); m[30:, 3] = True; m[:, 4:9] = True; m[:6, 9] = True
    out.append(("run spans whole columns", m))
    yy, xx = np.mgrid[:H, :W]
    out.append(("checkerboard", ((yy + xx) & 1) == 0))           # (starts with a one: a leading 0, then H * W ones)
    cases = [(n, rle.encode(m), m) for n, m in out]
    assert len(cases[7][1]) == H * W + 1               # 1 851 counts at 37 x 50: the most a mask of this size can have
    m = z(); m[3:30, 10:40] = True; m[10:12, 20:25] = False
    cases.append(("zero counts in the middle", _with_zero_counts(rle.encode(m)), m))
    assert (cases[-1][1][2:] == 0).any() and np.array_equal(rle.decode(cases[-1][1], H, W), m)
    return cases


def frames_for(M, H=H0, W=W0, seed=0):
    """[(name, [counts] * M, dense bool [M, H, W])]: the frames checked for one M.  M = 1: every edge mask as a frame of its own;
    otherwise one frame that starts with the edge masks and goes on with random blobs, and one frame whose masks all cover
    SAME_PIXEL (full 64-bit words, and a partial last one)."""
    edges = edge_masks(H, W)
    if M == 1:
        return [(n, [c], m[None]) for n, c, m in edges]
    rng = np.random.Generator(np.random.PCG64(seed + M))

    def blob():
        m = np.zeros((H, W), bool)
        h, w = int(rng.integers(1, H)), int(rng.integers(1, W))
        y, x = int(rng.integers(0, H - h + 1)), int(rng.integers(0, W - w + 1))
        m[y:y + h, x:x + w] = rng.random((h, w)) < 0.8
        return m
    a_counts = [c for _, c, _ in edges]
    a_dense = [m for _, _, m in edges]
    while len(a_dense) < M:
        a_dense.append(blob())
        a_counts.append(rle.encode(a_dense[-1]))
    b_dense = []
    for _ in range(M):
        m = blob()
        m[SAME_PIXEL] = True
        b_dense.append(m)
    return [("edge masks first", a_counts, np.stack(a_dense)), ("every mask covers one pixel", [rle.encode(m) for m in b_dense], np.stack(b_dense))]


# ---------------------------------------------------------------------------------------------------------- a small ragged scene
SCENE_OVER = dict(voxel_size=0.1, outlier_nb_points=60, feat_dbscan_min=8)      # (coarse voxels: a build takes seconds on the simulator)


def small_scene():
    """SceneSpec 64 x 48, 6 frames, ragged mask counts with a frame of 0 masks between frames that have some"""
    from holoagent_amd.synth import SceneSpec, SynthScene
    spec = SceneSpec(seed=3, rooms_x=1, rooms_z=1, room_size=(3.6, 2.5, 3.2), objects_per_room=4, width=64, height=48, n_frames=6,
                     n_masks=6, feat_dim=32)
    scn = SynthScene(spec)
    frames = [scn.frame(i) for i in range(spec.n_frames)]
    for f, keep in zip(frames, (3, 6, 0, 5, 1, 4)):
        f["masks"], f["f_masked"], f["f_crop"] = f["masks"][:keep], f["f_masked"][:keep], f["f_crop"][:keep]
    return frames


def frame_rles(frames):
    return [[rle.encode(m) for m in f["masks"]] for f in frames]


def build(L, frames, hand_over, over=None):
    """scene with the frames' geometry and a final map; hand_over(sc, S) gives it the encoder outputs; then fuse, merge, pool.
    Returns every getter the dense and the run-length build are compared at."""
    over = dict(SCENE_OVER if over is None else over, feat_dim=frames[0]["f_g"].reshape(-1).shape[0])
    sc = PC.make_scene(L, frames, over)
    S = PC.stack_frames(frames)
    sc.add_frames(S["rgb"], S["depth"], S["pose"], S["K"])
    sc.finalize_map()
    hand_over(sc, S)
    sc.fuse_frames()
    out = dict(fp=[sc.frame_fp(i) for i in range(len(frames))], masks3d=[sc.frame_masks3d(i) for i in range(len(frames))],
               map_feats=sc.map_feats(counter=True))
    sc.merge_instances()
    sc.pool_instances()
    out["instances"] = sc.instances()
    out["pooled"] = sc.instance_feats()
    sc.close()
    return out


def assert_same_build(a, b):
    for x, y in zip(a["fp"], b["fp"]):
        assert np.array_equal(x, y)
    for fa, fb in zip(a["masks3d"], b["masks3d"]):
        assert len(fa) == len(fb)
        for x, y in zip(fa, fb):
            assert np.array_equal(x, y)
    assert np.array_equal(a["map_feats"][0], b["map_feats"][0]) and np.array_equal(a["map_feats"][1], b["map_feats"][1])
    assert len(a["instances"]) == len(b["instances"])
    for x, y in zip(a["instances"], b["instances"]):
        assert np.array_equal(x, y)
    assert np.array_equal(a["pooled"], b["pooled"])


def dense_hand_over(sc, S):
    sc.add_frame_features(0, S["masks"], S["f_g"], S["f_masked"], S["f_crop"], S["n_masks"])


def rle_of_stack(masks, n_masks):
    """the dense hand-over layout u8 [n, M, H, W] + n_masks -> (counts, run_off, n_masks)"""
    return rle.pack([[rle.encode(masks[f, i]) for i in range(int(n_masks[f]))] for f in range(masks.shape[0])])


def rle_scene_class():
    """a Scene whose add_frame_features encodes the dense masks and hands them over run-length coded: tests/parity_common.py's
    checks, which call add_frame_features themselves, then check the run-length path"""
    from holoagent_amd._lib import Scene

    class RleScene(Scene):
        def add_frame_features(self, first, masks, f_g, f_masked, f_crop, n_masks=None):
            masks = np.asarray(masks)
            nm = np.full(masks.shape[0], masks.shape[1], np.int32) if n_masks is None else np.asarray(n_masks, np.int32)
            self.add_frame_features_rle(first, rle_of_stack(masks, nm), f_g, f_masked, f_crop)
    return RleScene


# ---------------------------------------------------------------------------------------------------------- the strict-C host
def c_host_instances(lib_path, tmp_path, frames, over):
    """tests/host_c/hmsg_host_rle.c on `frames`: the instance sizes it prints"""
    src = os.path.join(ROOT, "tests", "host_c", "hmsg_host_rle.c")
    exe = str(tmp_path / "hmsg_host_rle")
    d = os.path.dirname(lib_path)
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-O1", "-I", os.path.join(ROOT, "include"), src, "-o", exe,
                    lib_path, "-Wl,-rpath," + d, "-Wl,-rpath,/opt/rocm/lib", "-Wl,--allow-shlib-undefined"], check=True, capture_output=True)
    S = PC.stack_frames(frames)
    counts, run_off, n_masks = rle_of_stack(S["masks"], S["n_masks"])
    F, (H, W), M, D = len(frames), frames[0]["depth"].shape, S["masks"].shape[1], S["f_g"].shape[1]
    fin = str(tmp_path / "in.bin")
    with open(fin, "wb") as f:
        np.array([F, H, W, M, D, over["outlier_nb_points"], over["feat_dbscan_min"], int(round(over.get("outlier_radius", 1.0) * 1000)),
                  int(round(over.get("voxel_size", 0.05) * 1000)), 0], np.int32).tofile(f)
        np.array([len(run_off) - 1, len(counts)], np.int64).tofile(f)
        for a, t in ((S["K"], np.float64), (S["rgb"], np.uint8), (S["depth"], np.uint16), (S["pose"], np.float64), (n_masks, np.int32),
                     (run_off, np.int64), (counts, np.uint32), (S["f_g"], np.float32), (S["f_masked"], np.float32), (S["f_crop"], np.float32)):
            np.ascontiguousarray(a, t).tofile(f)
    r = subprocess.run([exe, fin], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.split("\n")
    n = int([l for l in lines if l.startswith("instances ")][0].split()[1])
    sizes = [int(l.split()[1]) for l in lines if l.startswith("size ")]
    assert len(sizes) == n
    return sizes
