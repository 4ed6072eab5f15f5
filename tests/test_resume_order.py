"""The resume order of the reference's build applications (semantic_scene_reconstruction.py:114-127) on the mirror Graph and from C:

    create_feature_map, save_masked_pcds, save_full_pcd, save_full_pcd_feats, build_hier_multimodal_scene_graph(dir_a)
    -- a fresh Graph --  load_full_pcd, load_full_pcd_feats, load_masked_pcds_new, build_hier_multimodal_scene_graph(dir_b)

dir_b/graph is dir_a/graph byte for byte: the loaders' arrays go back into HBM (Graph.restore_scene -> hmsg_restore_stage) and the
graph level runs on the device as it does right after create_feature_map.  (Before, the second build made floors and nothing below
them.)  tests/host_c/hmsg_host_resume.c does the same from the files through include/hmsg.h alone.
The scene is the one of tests/test_scene_graph_cabi.py; as there, both sides take the library's rule for a two-member KMeans cluster
and five representative views, so that directories can be compared byte for byte.  CPU: the kernel simulator; -m gpu: libhmsg.so."""
import contextlib
import os
import subprocess

import numpy as np
import pytest

from tests import parity_common as PC
from tests.test_scene_graph_cabi import _build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host_c", "hmsg_host_resume.c")
INC = os.path.join(ROOT, "include")
LIB = os.path.join(ROOT, "holoagent_amd", "libhmsg.so")
needs_emu = pytest.mark.skipif(not os.path.exists(PC.EMU_PATH), reason="kernel simulator not built")


@contextlib.contextmanager
def _byte_comparable():
    import holoagent_amd.graph as G
    orig, orig_pick = G.compute_room_embeddings, G._closest_member
    G.compute_room_embeddings = lambda *a, **k: orig(a[0], a[1], a[2], a[3], a[4], 5, *a[6:], **k)
    G._closest_member = lambda cluster, centre: int(np.argmax(np.asarray(cluster, np.float64) @ np.asarray(centre, np.float64)))
    try:
        yield
    finally:
        G.compute_room_embeddings, G._closest_member = orig, orig_pick


class _Frames:
    """dataset double over the synthetic scene's frames: (rgb, depth, pose, _, K) per index, as the reference's datasets"""

    def __init__(self, inp, F):
        self.rgb, self.depth = inp["rgb"].cpu().numpy(), inp["depth"].cpu().numpy()
        self.poses = [np.asarray(inp["pose"][i], np.float64).reshape(4, 4) for i in range(F)]
        self.K = np.asarray(inp["K"], np.float64).reshape(3, 3)
        self.frameId2imgPath = ["img/%05d.png" % i for i in range(F)]

    def __len__(self):
        return len(self.poses)

    def __getitem__(self, i):
        return self.rgb[i], self.depth[i], self.poses[i], None, self.K

    def get_camera_intrinsics(self):
        return self.K


class _Encoders:
    """encoder double: the scene's masks and features of the frame an image belongs to; counts its calls"""

    def __init__(self, inp, ds):
        self.index = {ds.rgb[i].tobytes(): i for i in range(len(ds))}
        assert len(self.index) == len(ds)
        self.masks, self.fg = inp["masks"].cpu().numpy(), inp["f_g"].cpu().numpy()
        self.fm, self.fc = inp["f_masked"].cpu().numpy(), inp["f_crop"].cpu().numpy()
        self.calls = 0

    def extract(self, rgb):
        i = self.index[np.ascontiguousarray(rgb).tobytes()]
        self.calls += 1
        return dict(masks=self.masks[i], f_g=self.fg[i], f_masked=self.fm[i], f_crop=self.fc[i])


def _same_dirs(a, b):
    for sub in ("floors", "rooms", "objects", "views"):
        fa, fb = sorted(os.listdir(os.path.join(a, sub))), sorted(os.listdir(os.path.join(b, sub)))
        assert fa == fb and len(fa) > 0, sub
        for f in fa:
            assert open(os.path.join(a, sub, f), "rb").read() == open(os.path.join(b, sub, f), "rb").read(), (sub, f)


_STAGE = {}      # library path -> the direct build and its artefacts on disk (minutes on the simulator: made once per session)


def _stage(lib_path, device, tmp_path_factory):
    if lib_path in _STAGE:
        return _STAGE[lib_path]
    from holoagent_amd._lib import HmsgLib
    from holoagent_amd.graph import Graph
    L = HmsgLib(lib_path)
    spec, inp, sc = _build(L, device)
    sc.close()                                                  # (only the frames are wanted: the Graph builds its own scene)
    ds = _Frames(inp, spec.n_frames)
    enc = _Encoders(inp, ds)
    cfg = dict(main=dict(device_id=0), models=dict(clip=dict(feat_dim=spec.feat_dim)),
               pipeline=dict(grid_resolution=0.05, skip_frames=1, views_on_device=True, max_masks=32))
    root = tmp_path_factory.mktemp("resume")
    art, dir_a = str(root / "artefacts"), str(root / "a")
    g = Graph(cfg, dataset=ds, encoders=enc, lib=L)
    with _byte_comparable():
        g.create_feature_map()
        g.save_masked_pcds(art)
        g.save_full_pcd(art)
        g.save_full_pcd_feats(art)
        g.build_hier_multimodal_scene_graph(dir_a)
    topo = _topology(g)
    assert len(g.rooms) >= 1 and len(g.objects) >= 3 and sum(len(v.object_ids) for v in g.views) >= 3
    g.scene.close()
    _STAGE[lib_path] = dict(L=L, spec=spec, inp=inp, ds=ds, cfg=cfg, art=art, dir_a=dir_a, topo=topo)
    return _STAGE[lib_path]


def _topology(g):
    return dict(floors=[(f.floor_id, [r.room_id for r in f.rooms]) for f in g.floors],
                rooms=[(r.room_id, [o.object_id for o in r.objects], [v.view_id for v in r.views], list(r.sample_images)) for r in g.rooms],
                objects=[(o.object_id, o.room_id, o.name, list(o.view_ids), o.best_view_id) for o in g.objects],
                views=[(v.view_id, v.room_id, v.img_id, list(v.object_ids)) for v in g.views])


def check_resume_order(lib_path, device, tmp_path, tmp_path_factory):
    import torch
    from holoagent_amd.graph import Graph, _LazyFn, _Pcd
    st = _stage(lib_path, device, tmp_path_factory)
    L, ds, cfg, art, F = st["L"], st["ds"], st["cfg"], st["art"], st["spec"].n_frames

    def loaded(enc, normalize):
        g = Graph(cfg, dataset=ds, encoders=enc, lib=L)
        assert g.load_full_pcd(art) is not None
        assert g.load_full_pcd_feats(art, normalize=normalize) is not None
        assert g.load_masked_pcds_new(art) is not None
        return g
    # ---- the reference's order, nothing else said: the encoders are asked once per processed frame
    enc = _Encoders(st["inp"], ds)
    gb = loaded(enc, False)
    with _byte_comparable():
        gb.build_hier_multimodal_scene_graph(str(tmp_path / "b"))
    assert enc.calls == F
    assert gb.scene is not None and isinstance(gb.full_pcd, _LazyFn)
    assert len(gb.rooms) >= 1 and len(gb.objects) >= 3 and sum(len(v.object_ids) for v in gb.views) >= 3
    assert _topology(gb) == st["topo"]
    _same_dirs(os.path.join(st["dir_a"], "graph"), str(tmp_path / "b" / "graph"))
    gb.scene.close()
    # ---- load_full_pcd_feats' default normalize=True (the reference's): same ids and topology, embeddings = the normalised rows;
    #      view features handed in: no encoder is needed
    saved = torch.load(os.path.join(art, "mask_feats.pt")).float()
    want = torch.nn.functional.normalize(saved, p=2, dim=-1).numpy()
    gc = loaded(None, True)
    gc.set_view_feats(st["inp"]["f_g"].cpu().numpy())
    sc = gc.restore_scene()                                     # (the explicit form)
    assert gc.scene is sc and np.array_equal(sc.instance_feats(), want)
    with _byte_comparable():
        gc.build_hier_multimodal_scene_graph(None)
    assert _topology(gc) == st["topo"]
    assert all(np.array_equal(np.asarray(o.embedding), want[o._instance]) for o in gc.objects)
    sc.close()
    # ---- neither view features nor encoders: refused before a scene is made, the message says what to call
    gd = loaded(None, False)
    with pytest.raises(RuntimeError, match="set_view_feats"):
        gd.build_hier_multimodal_scene_graph(None)
    assert gd.scene is None
    # ---- a cloud somebody set by hand is not the loaders': as before (host floors, no rooms, no scene)
    ge = loaded(None, False)
    ge.full_pcd = _Pcd(np.asarray(ge.full_pcd.points))
    ge.build_hier_multimodal_scene_graph(None)
    assert ge.scene is None and len(ge.floors) >= 1 and len(ge.rooms) == 0 and len(ge.objects) == 0


@needs_emu
def test_resume_order_on_the_simulator(tmp_path, tmp_path_factory):
    import torch
    check_resume_order(PC.EMU_PATH, torch.device("cpu"), tmp_path, tmp_path_factory)


@pytest.mark.gpu
def test_resume_order_gpu(tmp_path, tmp_path_factory):
    import torch
    check_resume_order(LIB, torch.device("cuda", 0), tmp_path, tmp_path_factory)


# ------------------------------------------------------------------------------------------------ the same from C
def _compile(lib_path, out):
    cmd = ["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-O1", "-I", INC, SRC, "-o", out, lib_path,
           "-Wl,-rpath," + os.path.dirname(lib_path), "-Wl,-rpath,/opt/rocm/lib", "-Wl,--allow-shlib-undefined"]
    subprocess.run(cmd, check=True, capture_output=True)
    return out


def check_c_host_resume(lib_path, device, tmp_path, tmp_path_factory):
    import torch
    st = _stage(lib_path, device, tmp_path_factory)
    spec, ds = st["spec"], st["ds"]
    feats = torch.load(os.path.join(st["art"], "mask_feats.pt")).float().numpy()     # (a C host cannot read .pt: raw f32 instead)
    N, D, F = feats.shape[0], spec.feat_dim, spec.n_frames
    assert N == len(os.listdir(os.path.join(st["art"], "objects")))
    poses = np.stack(ds.poses)
    fin = tmp_path / "in.bin"
    with open(fin, "wb") as f:
        np.array([D, N, F, spec.width, spec.height, 5], np.int32).tofile(f)
        np.array([0.05], np.float64).tofile(f)
        np.ascontiguousarray(ds.K, np.float64).tofile(f)
        np.ascontiguousarray(feats, np.float32).tofile(f)
        np.ascontiguousarray(poses, np.float64).tofile(f)
        np.ascontiguousarray(np.stack([np.linalg.inv(p) for p in ds.poses]), np.float64).tofile(f)
        np.ascontiguousarray(st["inp"]["f_g"].cpu().numpy(), np.float32).tofile(f)
        for p in ds.frameId2imgPath:
            np.array([len(p.encode())], np.int32).tofile(f)
            f.write(p.encode())
    exe = _compile(lib_path, str(tmp_path / "hmsg_host_resume"))
    out = tmp_path / "c"
    r = subprocess.run([exe, st["art"], str(fin), str(out)], capture_output=True, text=True, timeout=1800)
    assert r.returncode == 0, r.stderr
    t = st["topo"]
    assert "hmsg_host_resume ok: %d floors, %d rooms, %d views, %d objects," % (len(t["floors"]), len(t["rooms"]), len(t["views"]), len(t["objects"])) in r.stdout
    assert "%d instances" % N in r.stdout
    _same_dirs(os.path.join(st["dir_a"], "graph"), str(out))


@needs_emu
def test_c_host_resume_on_the_simulator(tmp_path, tmp_path_factory):
    import torch
    check_c_host_resume(PC.EMU_PATH, torch.device("cpu"), tmp_path, tmp_path_factory)


@pytest.mark.gpu
def test_c_host_resume_gpu(tmp_path, tmp_path_factory):
    import torch
    check_c_host_resume(LIB, torch.device("cuda", 0), tmp_path, tmp_path_factory)
