"""hmsg_restore_stage (include/hmsg.h, holoagent_amd/csrc/hmsg_restore.hip): map, instance pool and pooled features from stage artefacts
back into a handle, which the graph level cannot tell from one that went through A1..A7.

  * round trip: the arrays read out after hmsg_pool_instances, restored into a second handle, give the same graph -- saved directories
    byte for byte, JSON, edges in order, answers of the resident index;
  * the bounds pass at its edges: boxes bit-equal to numpy.min / max per instance (empty instances, one point, the wave and chunk
    sizes +-1, -0.0, repeated points, a 1e6 offset), not-finite coordinates and bad offsets refused with the handle left fresh;
  * the calls that need the frame store or the voxel bitmap refuse on a restored handle; hmsg_reset makes it an ordinary one again.
Every check runs on the kernel simulator (CPU suite) and on the MI355X (-m gpu)."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import parity_common as PC
from tests.test_scene_graph_cabi import _build, _rest

needs_emu = pytest.mark.skipif(not os.path.exists(PC.EMU_PATH), reason="kernel simulator not built")


def _emu():
    import torch
    from holoagent_amd._lib import HmsgLib
    return HmsgLib(PC.EMU_PATH), torch.device("cpu")


def _gpu():
    import torch
    from holoagent_amd._lib import HmsgLib
    return HmsgLib(), torch.device("cuda", 0)


def _fresh(L, spec, max_frames=None):
    from holoagent_amd._lib import Scene
    return Scene(lib_=L, device_id=0, height=spec.height, width=spec.width, max_frames=max_frames or spec.n_frames, max_masks=32, feat_dim=spec.feat_dim)


def _artefacts(sc):
    """what save_full_pcd / save_full_pcd_feats / save_masked_pcds write, as arrays -- read BEFORE any graph call (the per-object
    denoise of the object level changes the instance clouds)"""
    xyz, rgb = sc.map_points(colors=True)
    sizes = sc.instance_sizes()
    off = np.zeros(len(sizes) + 1, np.int64)
    off[1:] = np.cumsum(sizes)
    flat = np.empty((int(off[-1]), 3), np.float64)
    sc.instance_points_into(flat)
    return dict(xyz=xyz, rgb=rgb, mf=sc.map_feats(), off=off, flat=flat, feats=sc.instance_feats())


_BUILT = {}      # library path -> (spec, inputs, artefacts, instances) of the test scene after A1..A7: minutes on the simulator, made once


def _built(L, device):
    if L.path not in _BUILT:
        spec, inp, sc = _build(L, device)
        _rest(sc, inp)
        _BUILT[L.path] = (spec, inp, _artefacts(sc), sc.instances())
        sc.close()
    return _BUILT[L.path]


def _same_dirs(a, b):
    for sub in ("floors", "rooms", "objects", "views"):
        fa, fb = sorted(os.listdir(a / sub)), sorted(os.listdir(b / sub))
        assert fa == fb and len(fa) > 0, sub
        for f in fa:
            assert open(a / sub / f, "rb").read() == open(b / sub / f, "rb").read(), (sub, f)


def _graph_json(g):
    n = C.c_int64(0)
    g._ck(g.L.c.hmsg_graph_to_json(g.g, None, 0, C.byref(n)))
    buf = C.create_string_buffer(n.value)
    g._ck(g.L.c.hmsg_graph_to_json(g.g, buf, n.value, C.byref(n)))
    return buf.value


def check_round_trip(L, device, tmp_path, merge=False, device_arrays=False):
    from holoagent_amd._lib import SceneGraph, _ptr
    spec, inp, sc = _build(L, device)
    _rest(sc, inp)
    art = _artefacts(sc)
    _BUILT.setdefault(L.path, (spec, inp, art, sc.instances()))
    F, D = spec.n_frames, spec.feat_dim
    poses = np.stack([np.asarray(inp["pose"][i], np.float64).reshape(4, 4) for i in range(F)])
    pinv = np.stack([np.linalg.inv(p) for p in poses])
    fg = inp["f_g"].cpu().numpy()
    rng = np.random.Generator(np.random.PCG64(99))
    label_feats = rng.standard_normal((9, D)).astype(np.float32)
    label_feats /= np.linalg.norm(label_feats, axis=1, keepdims=True)
    label_names = ["label%d" % i for i in range(8)] + ["café \"table\""]
    if merge:                                                   # (the one-name vocabulary of test_scene_graph_cabi's merge=True case)
        label_feats, label_names = label_feats[:1], ["thing"]
    paths = ["img/%05d.png" % i for i in range(F)]
    kw = dict(poses_inv=pinv, img_paths=paths, num_views=5, host_threads=2, merge_objects_graph=1 if merge else 0)
    ga = SceneGraph.build(sc, poses, fg, label_feats, label_names, **kw)
    sc2 = _fresh(L, spec)
    K = np.ascontiguousarray(np.asarray(inp["K"], np.float64).reshape(9))
    if device_arrays:
        import torch
        dev = {k: torch.from_numpy(v).to(device) for k, v in art.items()}
        dK = torch.from_numpy(K).to(device)
        sc2._ck(L.c.hmsg_restore_stage(sc2.h, len(art["xyz"]), _ptr(dev["xyz"]), _ptr(dev["rgb"]), _ptr(dev["mf"]), len(art["off"]) - 1,
                                       _ptr(dev["off"]), _ptr(dev["flat"]), _ptr(dev["feats"]), _ptr(dK)))
    else:
        sc2.restore_stage(art["xyz"], (art["off"], art["flat"]), art["feats"], K, map_colors=art["rgb"], map_feats=art["mf"])
    # the restored handle hands back what went in
    back = _artefacts(sc2)
    for k in art:
        assert np.array_equal(art[k], back[k]), k
    gb = SceneGraph.build(sc2, poses, fg, label_feats, label_names, **kw)
    ca, cb = ga.counts(), gb.counts()
    for k in ("floors", "rooms", "views", "objects", "edges", "view_object_links"):
        assert ca[k] == cb[k], k
    assert ca["rooms"] >= 1 and ca["objects"] >= 3 and ca["view_object_links"] >= 3
    assert _graph_json(ga) == _graph_json(gb)
    assert np.array_equal(ga.edges(), gb.edges())
    ga.save(tmp_path / "a")
    gb.save(tmp_path / "b")
    _same_dirs(tmp_path / "a", tmp_path / "b")
    Q = 6
    rng = np.random.default_rng(5)
    T = rng.standard_normal((Q, 2, D)).astype(np.float32)
    T /= np.linalg.norm(T, axis=-1, keepdims=True)
    room_names = rng.standard_normal((ca["rooms"], D))
    room_names /= np.linalg.norm(room_names, axis=1, keepdims=True)
    Tr = np.ascontiguousarray(room_names[rng.integers(0, ca["rooms"], Q)], np.float32)
    zero = np.zeros(Q, np.int32)
    hits = 0
    for mode in (0, 1, 2):
        sa, ia, ra, xa = ga.query(T, zero, Tr, zero - 1, zero + mode, 3, room_name_emb=room_names)
        sb, ib, rb, xb = gb.query(T, zero, Tr, zero - 1, zero + mode, 3, room_name_emb=room_names)
        assert sa == sb and np.array_equal(ia, ib) and np.array_equal(ra, rb), mode
        assert np.array_equal(xa.view(np.uint64)[ia >= 0], xb.view(np.uint64)[ib >= 0]), mode
        hits += int((ia >= 0).sum())
    assert hits > 0
    for o in (ga, gb, sc, sc2):
        o.close()


@needs_emu
@pytest.mark.parametrize("merge", [False, True], ids=["plain", "merge_objects"])
def test_round_trip_on_the_simulator(tmp_path, merge):
    check_round_trip(*_emu(), tmp_path, merge=merge)


@pytest.mark.gpu
@pytest.mark.parametrize("merge,device_arrays", [(False, False), (True, False), (False, True)], ids=["plain", "merge_objects", "device_pointers"])
def test_round_trip_gpu(tmp_path, merge, device_arrays):
    check_round_trip(*_gpu(), tmp_path, merge=merge, device_arrays=device_arrays)


# ------------------------------------------------------------------------------------------------ the bounds pass at its edges
def _edge_pool(sizes, seed):
    """instance clouds with what the pass can get wrong: negative values, -0.0 as the unambiguous extreme of an axis (all other values
    of the axis on one side of zero: numpy's answer does not depend on its reduction order), one point repeated, a 1e6 offset"""
    rng = np.random.default_rng(seed)
    clouds = [rng.standard_normal((n, 3)) * 0.2 for n in sizes]
    big = [i for i, n in enumerate(sizes) if n >= 64]
    if len(big) >= 1:
        c = clouds[big[0]]
        c[:, 0] = np.abs(c[:, 0]) + 0.5
        c[len(c) // 2, 0] = -0.0                               # min x = -0.0
        c[:, 1] = -np.abs(c[:, 1]) - 0.5
        c[-1, 1] = -0.0                                        # max y = -0.0
    if len(big) >= 2:
        clouds[big[1]][:] = clouds[big[1]][0]                  # one point, repeated
    if len(big) >= 3:
        clouds[big[-1]] += 1e6
    return clouds


def _want_boxes(clouds):
    out = np.zeros((len(clouds), 6), np.float64)               # (an empty instance: six zeros, include/hmsg.h)
    for i, c in enumerate(clouds):
        if len(c):
            out[i, :3], out[i, 3:] = c.min(axis=0), c.max(axis=0)
    return out


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


EDGE_SIZES = {
    "empty_in_the_middle_and_at_the_end": [1, 63, 64, 65, 256, 257, 5000, 0, 2, 0],
    "empty_at_the_start": [0, 3, 1100, 2048, 1023, 1, 1025],   # (a chunk of the pass is 1024 points)
    "one_instance": [777],
}


def check_bounds_edges(L, device, sizes, seed):
    from holoagent_amd.synth import SceneSpec
    spec = SceneSpec(seed=1, n_frames=1, feat_dim=8, n_masks=4, width=32, height=24)
    D = spec.feat_dim
    rng = np.random.default_rng(seed + 100)
    clouds = _edge_pool(sizes, seed)
    feats = rng.standard_normal((len(clouds), D)).astype(np.float32)
    cloud_map = rng.standard_normal((2500, 3)) * 2.0           # (three chunks of the pass, the last one partial)
    K = np.array([[30.0, 0, 16], [0, 30.0, 12], [0, 0, 1]])
    sc = _fresh(L, spec)
    sc.restore_stage(cloud_map, clouds, feats, K)
    assert sc.instance_sizes().tolist() == list(sizes)
    assert np.array_equal(_bits(sc.instance_boxes()), _bits(_want_boxes(clouds)))
    got = sc.instances()
    for a, b in zip(got, clouds):
        assert np.array_equal(_bits(a), _bits(b))
    assert np.array_equal(sc.instance_feats(), feats)
    assert np.array_equal(_bits(sc.map_points()), _bits(cloud_map))
    # the other calls the restore promises on such a handle: they get the boxes the pass made
    if sum(sizes):
        verts = [np.stack(np.meshgrid(np.arange(-3, 3, 0.1), np.arange(-3, 3, 0.1)), -1).reshape(-1, 2)]
        share = sc.instance_room_share(verts)
        assert share.shape == (len(sizes), 1) and np.isfinite(share).all() and all(share[i, 0] == 0.0 for i, n in enumerate(sizes) if n == 0)
        assert any(share[i, 0] > 0.0 for i, n in enumerate(sizes) if n > 0)
    sc.denoise_instances()
    after = sc.instance_sizes()
    assert (after <= np.asarray(sizes)).all() and all(after[i] == 0 for i, n in enumerate(sizes) if n == 0)
    sc.close()


@needs_emu
@pytest.mark.parametrize("case", sorted(EDGE_SIZES))
def test_bounds_edges_on_the_simulator(case):
    check_bounds_edges(*_emu(), EDGE_SIZES[case], seed=sorted(EDGE_SIZES).index(case))


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(EDGE_SIZES))
def test_bounds_edges_gpu(case):
    check_bounds_edges(*_gpu(), EDGE_SIZES[case], seed=sorted(EDGE_SIZES).index(case))


@pytest.mark.gpu
def test_bounds_pass_beyond_one_trip_of_the_grid_gpu():
    """The pass caps its grid at 2048 workgroups of four waves: only beyond 2048 * 4 chunks of 1024 points does a wave take a second
    chunk.  8.5 million points (200 MB) in three instances, one of them ending inside the second trip."""
    L, device = _gpu()
    from holoagent_amd.synth import SceneSpec
    spec = SceneSpec(seed=1, n_frames=1, feat_dim=8, n_masks=4, width=32, height=24)
    P = 2048 * 4 * 1024 + 100_000
    rng = np.random.default_rng(7)
    flat = rng.standard_normal((P, 3))
    off = np.array([0, 5, 2048 * 4 * 1024 + 37, P], np.int64)
    feats = np.zeros((3, spec.feat_dim), np.float32)
    sc = _fresh(L, spec)
    sc.restore_stage(flat[:3000], (off, flat), feats, np.eye(3))
    want = _want_boxes([flat[off[i]:off[i + 1]] for i in range(3)])
    assert np.array_equal(_bits(sc.instance_boxes()), _bits(want))
    sc.close()


def check_bad_input_leaves_the_handle_fresh(L, device):
    from holoagent_amd._lib import HmsgError
    from holoagent_amd.synth import SceneSpec
    spec = SceneSpec(seed=1, n_frames=1, feat_dim=8, n_masks=4, width=32, height=24)
    sizes = EDGE_SIZES["empty_at_the_start"]
    clouds = _edge_pool(sizes, 3)
    off = np.zeros(len(sizes) + 1, np.int64)
    off[1:] = np.cumsum(sizes)
    flat = np.concatenate(clouds)
    feats = np.ones((len(sizes), spec.feat_dim), np.float32)
    cloud_map = np.random.default_rng(2).standard_normal((1500, 3))
    K = np.eye(3)
    sc = _fresh(L, spec)

    def refused(m, o, f, what):
        with pytest.raises(HmsgError) as e:
            sc.restore_stage(m, (o, f), feats, K)
        assert str(e.value).startswith("[-1]") and what in str(e.value), str(e.value)
        assert sc.map_size() == -1 and sc.num_instances() == -1          # still fresh
    nan_last = flat.copy()
    nan_last[-1, 2] = np.nan                                   # the last point of the last instance
    refused(cloud_map, off, nan_last, "instance coordinate is not finite")
    inf_map = cloud_map.copy()
    inf_map[700, 1] = -np.inf
    refused(inf_map, off, flat, "map coordinate is not finite")
    down = off.copy()
    down[3] = down[2] - 1
    refused(cloud_map, down, flat, "must not decrease")
    shifted = off.copy()
    shifted[0] = 1
    refused(cloud_map, shifted, flat, "inst_off[0]")
    sc.restore_stage(cloud_map, (off, flat), feats, K)         # ... and the same handle takes a correct restore afterwards
    assert np.array_equal(_bits(sc.instance_boxes()), _bits(_want_boxes(clouds)))
    with pytest.raises(HmsgError, match="restored already"):
        sc.restore_stage(cloud_map, (off, flat), feats, K)
    sc.close()


@needs_emu
def test_bad_input_leaves_the_handle_fresh_on_the_simulator():
    check_bad_input_leaves_the_handle_fresh(*_emu())


@pytest.mark.gpu
def test_bad_input_leaves_the_handle_fresh_gpu():
    check_bad_input_leaves_the_handle_fresh(*_gpu())


def check_no_instances(L, device):
    """n_inst = 0: the graph has its rooms and views and no object"""
    from holoagent_amd._lib import SceneGraph
    spec, inp, sc = _build(L, device)
    xyz, rgb = sc.map_points(colors=True)
    F, D = spec.n_frames, spec.feat_dim
    poses = np.stack([np.asarray(inp["pose"][i], np.float64).reshape(4, 4) for i in range(F)])
    fg = inp["f_g"].cpu().numpy()
    sc2 = _fresh(L, spec)
    sc2.restore_stage(xyz, [], np.zeros((0, D), np.float32), inp["K"], map_colors=rgb)
    assert sc2.num_instances() == 0 and sc2.instance_boxes().shape == (0, 6)
    g = SceneGraph.build(sc2, poses, fg, None, None, num_views=5, host_threads=2)
    cnt = g.counts()
    assert cnt["floors"] >= 1 and cnt["rooms"] >= 1 and cnt["views"] == F and cnt["objects"] == 0 and cnt["view_object_links"] == 0
    for o in (g, sc, sc2):
        o.close()


@needs_emu
def test_no_instances_on_the_simulator():
    check_no_instances(*_emu())


@pytest.mark.gpu
def test_no_instances_gpu():
    check_no_instances(*_gpu())


# ------------------------------------------------------------------------------------------------ refusals
def check_refusals(L, device):
    from holoagent_amd._lib import HmsgError, _ptr
    spec, inp, art, want_inst = _built(L, device)
    K = inp["K"]
    # a handle that holds frames, or a map, does not take a restore
    sc = _fresh(L, spec)
    sc.add_frames(inp["rgb"], inp["depth"], inp["pose"], K)
    for step in (lambda: None, sc.finalize_map):
        step()
        with pytest.raises(HmsgError) as e:
            sc.restore_stage(art["xyz"], (art["off"], art["flat"]), art["feats"], K)
        assert str(e.value).startswith("[-1]") and "hmsg_reset first" in str(e.value)
    sc.reset()
    sc.restore_stage(art["xyz"], (art["off"], art["flat"]), art["feats"], K, map_colors=art["rgb"])       # (no map features)
    HW, D, M = spec.height * spec.width, spec.feat_dim, 32
    buf = np.zeros(max(HW * 4, len(art["xyz"]) * D * 2, 4096), np.float64)              # (room for whatever a call would write)
    th, n64a, n64b = C.c_double(), C.c_int64(), C.c_int64()
    one_size = np.array([1], np.int64)
    calls = {
        "hmsg_add_frames": lambda: L.c.hmsg_add_frames(sc.h, 1, _ptr(inp["rgb"]), _ptr(inp["depth"]), _ptr(inp["pose"]), _ptr(np.ascontiguousarray(K, np.float64))),
        "hmsg_add_frame_features": lambda: L.c.hmsg_add_frame_features(sc.h, 0, 1, M, _ptr(inp["masks"]), _ptr(inp["f_g"]), _ptr(inp["f_masked"]), _ptr(inp["f_crop"]), None),
        "hmsg_fuse_frames": lambda: L.c.hmsg_fuse_frames(sc.h),
        "hmsg_merge_instances": lambda: L.c.hmsg_merge_instances(sc.h),
        "hmsg_merge_tree_local": lambda: L.c.hmsg_merge_tree_local(sc.h, spec.n_frames, C.byref(th), C.byref(n64a), C.byref(n64b)),
        "hmsg_merge_tree_join": lambda: L.c.hmsg_merge_tree_join(sc.h, 1, _ptr(one_size), _ptr(buf), 0.5, 1),
        "hmsg_pool_instances": lambda: L.c.hmsg_pool_instances(sc.h),
        "hmsg_get_frame_nn": lambda: L.c.hmsg_get_frame_nn(sc.h, 0, _ptr(buf)),
        "hmsg_get_frame_fp": lambda: L.c.hmsg_get_frame_fp(sc.h, 0, _ptr(buf)),
        "hmsg_get_frame_mask_sizes": lambda: L.c.hmsg_get_frame_mask_sizes(sc.h, 0, _ptr(buf)),
        "hmsg_get_frame_mask_points": lambda: L.c.hmsg_get_frame_mask_points(sc.h, 0, _ptr(buf)),
        "hmsg_get_feature_sums": lambda: L.c.hmsg_get_feature_sums(sc.h, _ptr(buf), _ptr(buf)),
        "hmsg_set_feature_sums": lambda: L.c.hmsg_set_feature_sums(sc.h, _ptr(buf), _ptr(buf)),
        "hmsg_get_map_feats": lambda: L.c.hmsg_get_map_feats(sc.h, _ptr(buf), None),
    }
    for name, call in calls.items():
        assert call() == -1, name
        msg = L.c.hmsg_last_error(sc.h).decode()
        assert "restored" in msg and name in msg, (name, msg)
    assert L.c.hmsg_get_frame_num_masks(sc.h, 0) == -1
    assert not buf.any()                                       # nothing was written
    # the restored state is intact after all that
    assert np.array_equal(sc.instance_sizes(), np.diff(art["off"])) and sc.map_size() == len(art["xyz"])
    # hmsg_reset: an ordinary handle again -- A1..A7 on it give a fresh handle's instances
    sc.reset()
    sc.add_frames(inp["rgb"], inp["depth"], inp["pose"], K)
    sc.finalize_map()
    _rest(sc, inp)
    got = sc.instances()
    assert len(got) == len(want_inst) and all(np.array_equal(a, b) for a, b in zip(got, want_inst))
    assert np.array_equal(sc.instance_feats(), art["feats"]) and np.array_equal(sc.map_feats(), art["mf"])
    assert sc.frame_nn(0).shape == (spec.height, spec.width)
    sc.close()


@needs_emu
def test_refusals_on_the_simulator():
    check_refusals(*_emu())


@pytest.mark.gpu
def test_refusals_gpu():
    check_refusals(*_gpu())
