"""The navigation maps from C (tests/host_c/hmsg_host_nav.c, strict C99 against include/hmsg.h ALONE): the host builds a small scene
and its graph, sizes the maps with hmsg_graph_nav_grid, is told by the first hmsg_graph_nav_floor_maps how long the boundary list
has to be and repeats the call; what it writes equals the same calls made through the Python binding.  CPU: the kernel simulator;
-m gpu: libhmsg.so."""
import os
import subprocess

import numpy as np
import pytest

from tests import parity_common as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host_c", "hmsg_host_nav.c")
INC = os.path.join(ROOT, "include")
LIB = os.path.join(ROOT, "holoagent_amd", "libhmsg.so")


def _compile(lib_path, out):
    cmd = ["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-O1", "-I", INC, SRC, "-o", out, lib_path,
           "-Wl,-rpath," + os.path.dirname(lib_path), "-Wl,-rpath,/opt/rocm/lib", "-Wl,--allow-shlib-undefined"]
    subprocess.run(cmd, check=True, capture_output=True)
    return out


def _run(lib_path, tmp_path):
    from holoagent_amd._lib import HmsgLib, SceneGraph
    from holoagent_amd.synth import SceneSpec, SynthScene
    D, cell_mm = 16, 50
    spec = SceneSpec(seed=31, rooms_x=1, rooms_z=1, room_size=(3.6, 2.5, 3.2), objects_per_room=4, width=64, height=48, n_frames=6, n_masks=8,
                     feat_dim=D, yaw_step_deg=25.0)
    scn = SynthScene(spec)
    frames = [scn.frame(i) for i in range(spec.n_frames)]
    S = PC.stack_frames(frames)
    F, (H, W), M = len(frames), frames[0]["depth"].shape, S["masks"].shape[1]
    over = dict(feat_dim=D, outlier_nb_points=20, outlier_radius=0.3, feat_dbscan_min=8)
    L = HmsgLib(lib_path)
    sc = PC.make_scene(L, frames, over)
    sc.add_frames(S["rgb"], S["depth"], S["pose"], S["K"])
    sc.finalize_map()
    sc.add_frame_features(0, S["masks"], S["f_g"], S["f_masked"], S["f_crop"], S["n_masks"])
    sc.fuse_frames()
    sc.merge_instances()
    sc.pool_instances()
    g = SceneGraph.build(sc, S["pose"], S["f_g"], num_views=3, host_threads=1)
    track = np.array(S["pose"], np.float64).reshape(-1, 4, 4).copy()
    track[:, 1, 3] = sc.segment_floors()[0]["zero_level"] + 0.8
    want = g.nav_floor_maps(0, track, cell_size=cell_mm / 1000.0)
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        np.array([F, H, W, M, D, len(track), over["outlier_nb_points"], over["feat_dbscan_min"], int(round(over["outlier_radius"] * 1000)),
                  cell_mm], np.int32).tofile(f)
        for a, t in ((S["K"], np.float64), (S["rgb"], np.uint8), (S["depth"], np.uint16), (S["pose"], np.float64), (S["masks"], np.uint8),
                     (S["n_masks"], np.int32), (S["f_g"], np.float32), (S["f_masked"], np.float32), (S["f_crop"], np.float32),
                     (track, np.float64)):
            np.ascontiguousarray(a, t).tofile(f)
    exe = _compile(lib_path, str(tmp_path / "hmsg_host_nav"))
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout + r.stderr
    raw = open(fout, "rb").read()
    gw, gh, n_regions, main_label = np.frombuffer(raw, np.int32, 4)
    main_area, n_boundary = np.frombuffer(raw, np.int64, 2, 16)
    o = 32
    mn = np.frombuffer(raw, np.float64, 3, o); o += 24
    mx = np.frombuffer(raw, np.float64, 3, o); o += 24
    cells = int(gw) * int(gh)
    obst = np.frombuffer(raw, np.float32, cells, o).reshape(gh, gw); o += 4 * cells
    free = np.frombuffer(raw, np.uint8, cells, o).reshape(gh, gw); o += cells
    main = np.frombuffer(raw, np.uint8, cells, o).reshape(gh, gw); o += cells
    bgr = np.frombuffer(raw, np.uint8, cells * 3, o).reshape(gh, gw, 3); o += cells * 3
    rc = np.frombuffer(raw, np.int32, int(n_boundary) * 2, o).reshape(-1, 2); o += 8 * int(n_boundary)
    assert o == len(raw)
    assert (gw, gh) == want["grid"] and (n_regions, main_label, main_area) == (want["n_regions"], want["main_label"], want["main_area"])
    assert n_boundary == len(want["boundary_rc"]) > 1                     # (the host's first list of one cell was too short)
    assert np.array_equal(mn, want["pcd_min"]) and np.array_equal(mx, want["pcd_max"])
    assert np.array_equal(obst, want["obstacle_map"]) and np.array_equal(free, want["free_map"]) and np.array_equal(main, want["main_free_map"])
    assert np.array_equal(bgr, want["top_down_bgr"]) and np.array_equal(rc, want["boundary_rc"])
    assert main.any() and bgr.any()
    assert "boundary %d" % n_boundary in r.stdout
    g.close()
    sc.close()


@pytest.mark.skipif(not os.path.exists(PC.EMU_PATH), reason="kernel simulator not built")
def test_c_host_nav_on_the_simulator(tmp_path):
    _run(PC.EMU_PATH, tmp_path)


@pytest.mark.gpu
def test_c_host_nav_gpu(tmp_path):
    _run(LIB, tmp_path)
