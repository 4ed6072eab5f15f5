"""The map's colour sums ride with the ordered voxel sums (k_accum_ordered, hmsg_map.hip): every voxel's colour is the exact
integer sum of its pixels' bytes, taken by the wave that replays the voxel's runs, and its count is the sum of its run lengths.

Small numpy-made scenes aimed at the places where runs are cut and packed, each built by both routes of the kernel (the default,
and HMSG_DEBUG_ACCUM_WAVES=1) in a child process of its own -- the switch is read once per process.  Expected values come from
the oracle (`PC.check_map`: voxel set and order, centroids bit for bit, colours to 1e-9), never from the library; the two routes
must hand out equal arrays.  What a scene is meant to contain (runs of one pixel, a full 64-pixel run, a voxel of thousands of
pixels ...) is asserted on the oracle's voxel keys before anything is built."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import hmsg_oracle as O
from tests import parity_common as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D = 8                      # feature width of the handles (no features are added)
RUN_CHUNK = 4096           # pixels per workgroup of k_slots / k_emit_runs


def _frame(rgb, depth, t, K):
    H, W = depth.shape
    pose = np.eye(4)
    pose[:3, 3] = t
    return dict(rgb=np.ascontiguousarray(rgb, dtype=np.uint8), depth=np.ascontiguousarray(depth, dtype=np.uint16), pose=pose,
                K=np.array(K, np.float64), masks=np.zeros((0, H, W), bool), f_g=np.zeros(D, np.float32),
                f_masked=np.zeros((0, D), np.float32), f_crop=np.zeros((0, D), np.float32))


def _K(f, W, H):
    return [[f, 0, W / 2.0], [0, f, H / 2.0], [0, 0, 1]]


def _rgb(rng, H, W):
    return rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)


def scenes():
    """name -> (frames, cfg of the oracle, configuration overrides of the handle)"""
    out = {}
    cfg = lambda vs: dict(voxel_size=vs, outlier_nb=2, outlier_radius=4.0 * vs)
    over = lambda vs: dict(feat_dim=D, voxel_size=vs, outlier_nb_points=2, outlier_radius=4.0 * vs)

    # slice and row edges: 72 columns (rows begin at every eighth lane of a 64-lane slice); frame 0 alternates two depths
    # column by column (runs of one pixel), frame 1 is a near wall inside one large voxel (row 8 begins a slice: a 64-pixel run),
    # frame 2 a sloped wall (runs of a few pixels, cut by row ends and slice edges)
    rng = np.random.Generator(np.random.PCG64(11))
    H, W = 40, 72
    K = _K(60.0, W, H)
    x = np.arange(W)[None, :].repeat(H, 0)
    y = np.arange(H)[:, None].repeat(W, 1)
    fr = [_frame(_rgb(rng, H, W), np.where(x % 2 == 0, 900, 2100), (0, 0, 0), K),
          _frame(_rgb(rng, H, W), np.full((H, W), 100), (0.2, 0.3, 0.7), K),
          _frame(_rgb(rng, H, W), 800 + 9 * x + 3 * y, (0.1, 0, 0), K)]
    out["edges"] = (fr, cfg(0.5), over(0.5))

    # frames smaller than a chunk: 48 x 40 = 1920 pixels, three frames in the first chunk, chunk boundaries in the middle of a row
    rng = np.random.Generator(np.random.PCG64(12))
    H, W = 40, 48
    K = _K(50.0, W, H)
    x = np.arange(W)[None, :].repeat(H, 0)
    y = np.arange(H)[:, None].repeat(W, 1)
    fr = [_frame(_rgb(rng, H, W), 700 + 40 * i + 5 * x + 2 * y, (0.03 * i, 0, 0), K) for i in range(6)]
    out["small_frames"] = (fr, cfg(0.05), over(0.05))

    # invalid pixels: depth 0 inside runs, and a frame without a valid pixel between two that have some
    rng = np.random.Generator(np.random.PCG64(13))
    H, W = 40, 72
    K = _K(60.0, W, H)
    x = np.arange(W)[None, :].repeat(H, 0)
    fr = []
    for i in range(3):
        d = 600 + 2 * x + 30 * i
        d[rng.random((H, W)) < 0.15] = 0
        fr.append(_frame(_rgb(rng, H, W), d if i != 1 else np.zeros((H, W)), (0, 0.01 * i, 0), K))
    out["invalid"] = (fr, cfg(0.05), over(0.05))

    # a heavy voxel: six frames 15 cm in front of a white wall, 1.25 mm between pixels -- a voxel holds thousands of pixels
    H, W = 40, 72
    K = _K(120.0, W, H)
    fr = [_frame(np.full((H, W, 3), 255), np.full((H, W), 150), (0.0005 * i, 0, 0), K) for i in range(6)]
    out["heavy"] = (fr, cfg(0.05), over(0.05))
    return out


def _runs(frames, vs):
    """(run lengths, pixels per voxel, runs per voxel, slot per pixel) by the rule of hmsg_map.hip, on the oracle's voxel keys: a
    run ends where the voxel changes, at column 0 and at the edge of a 64-pixel slice of the scene's pixel order."""
    H, W = frames[0]["depth"].shape
    pts, valid = [], []
    for f in frames:
        p, _, m = O.create_pcd(f["rgb"], f["depth"], f["pose"], f["K"])
        pts.append(p)
        valid.append(m.reshape(-1))
    valid = np.concatenate(valid)
    idx, _ = O.o3d_voxel_keys(np.concatenate(pts), vs)
    _, inv = np.unique(idx, axis=0, return_inverse=True)
    slot = np.full(valid.size, -1, np.int64)
    slot[valid] = inv.reshape(-1)
    i = np.arange(valid.size)
    head = np.ones(valid.size, bool)
    head[1:] = slot[1:] != slot[:-1]
    head |= (i % W == 0) | (i % 64 == 0)
    run_id = np.cumsum(head) - 1
    ok = slot >= 0
    lens = np.bincount(run_id[ok], minlength=run_id[-1] + 1)
    lens = lens[lens > 0]
    px = np.bincount(slot[ok])
    runs_per_voxel = np.bincount(slot[head & ok])
    return lens, px, runs_per_voxel, slot


def test_scenes_hold_what_they_are_for():
    S = scenes()
    lens, _, _, _ = _runs(S["edges"][0], 0.5)
    assert lens.min() == 1 and lens.max() == 64 and (lens == 1).sum() > 1000
    assert 1 < np.median(lens[(lens > 1) & (lens < 64)]) < 64
    fr = S["small_frames"][0]
    H, W = fr[0]["depth"].shape
    assert 3 * H * W > RUN_CHUNK > 2 * H * W and RUN_CHUNK % (H * W) % W != 0       # three frames in a chunk, boundary inside a row
    H, W = S["edges"][0][0]["depth"].shape
    assert RUN_CHUNK % (H * W) % W != 0 and W % 64 != 0
    fr = S["invalid"][0]
    assert not fr[1]["depth"].any() and fr[0]["depth"].any() and fr[2]["depth"].any()
    d = fr[0]["depth"]
    assert ((d[:, 1:-1] == 0) & (d[:, :-2] > 0) & (d[:, 2:] > 0)).sum() > 50        # holes with valid pixels on both sides
    lens, px, rpv, _ = _runs(S["heavy"][0], 0.05)
    v = int(np.argmax(px))
    assert px[v] > 4000 and rpv[v] > 64 and 255 * px[v] > 2 ** 20 and 255 * (px[v] // 64) > 2 ** 14


_CHILD = """
import sys
sys.path.insert(0, {root!r})
import numpy as np
from tests import parity_common as PC
from tests.test_map_colour_sums import scenes
from holoagent_amd._lib import HmsgLib
L = HmsgLib({lib})
out = {{}}
for name, (frames, cfg, over) in scenes().items():
    sc = PC.make_scene(L, frames, over)
    PC.check_map(sc, frames, cfg)
    pts, cols = sc.map_points(colors=True)
    assert pts.shape[0] > 0, name
    out[name + "_pts"], out[name + "_cols"] = pts, cols
    sc.close()
np.savez({dst!r}, **out)
print("CHILD OK")
"""


def _both_routes(lib, tmp_path):
    got = []
    for tag, env_over in (("lds", {}), ("waves", {"HMSG_DEBUG_ACCUM_WAVES": "1"})):
        env = dict(os.environ)
        env.pop("HMSG_DEBUG_ACCUM_WAVES", None)
        env.update(env_over)
        dst = str(tmp_path / (tag + ".npz"))
        r = subprocess.run([sys.executable, "-c", _CHILD.format(root=ROOT, lib=lib, dst=dst)], env=env, capture_output=True,
                           text=True, timeout=900)
        assert r.returncode == 0 and "CHILD OK" in r.stdout, tag + "\n" + r.stdout + r.stderr       # (check_map passed for each scene)
        got.append(np.load(dst))
    assert sorted(got[0].files) == sorted(got[1].files) and len(got[0].files) == 2 * len(scenes())
    for k in got[0].files:
        assert np.array_equal(got[0][k], got[1][k]), k


@pytest.mark.skipif(not os.path.exists(PC.EMU_PATH), reason="kernel simulator not built")
def test_colour_sums_two_routes_simulator(tmp_path):
    _both_routes(repr(PC.EMU_PATH), tmp_path)


@pytest.mark.gpu
def test_colour_sums_two_routes_gpu(tmp_path):
    _both_routes("", tmp_path)
