"""GPU parity at the sizes BASELINE.json's configs name: D = 512 / 768 with M = 32 at 640x480 against the oracle,
and size-independent properties of the full configs[1] build (1000 frames) that the oracle cannot reach."""
import os

import numpy as np
import pytest

from tests import parity_common as PC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    from holoagent_amd._lib import HmsgLib
    return HmsgLib()


@pytest.mark.parametrize("D,n_frames,W,H", [(512, 20, 640, 480), (768, 10, 320, 240)])
def test_build_at_config_shape_against_oracle(L, D, n_frames, W, H):
    """configs[1]'s kernel instances (k_fuse<4,2> for D=512, <4,3> for 768; M = 32; 640x480) stage-wise against the oracle."""
    from holoagent_amd.synth import SceneSpec, SynthScene
    spec = SceneSpec(seed=61, rooms_x=1, rooms_z=1, room_size=(4.5, 2.8, 3.8), objects_per_room=6, width=W, height=H,
                     n_frames=n_frames, n_masks=32, feat_dim=D, yaw_step_deg=18.0)
    scn = SynthScene(spec)
    frames = [scn.frame(i) for i in range(spec.n_frames)]
    cfg = dict(voxel_size=0.05, clip_masked_weight=0.4418, max_mask_distance=10000, feat_dim=D, init_overlap_thresh=0.75,
               overlap_thresh_factor=0.025, iou_thresh=0.05, merge_type="sequential")
    sc = PC.make_scene(L, frames, dict(feat_dim=D))
    S, ref_pts, ref_cols = PC.check_map(sc, frames, cfg)
    assert ref_pts.shape[0] > 5000
    ref_feats, _ = PC.check_fuse(sc, frames, S, cfg, ref_pts, ref_cols, check_masks=True)
    got, feats = PC.check_merge_pool(sc, frames, cfg, ref_pts, ref_feats)
    assert len(got) >= 5 and feats.shape[1] == D
    sc.close()


def test_filter_distance_drops_far_masks(L):
    """pipeline.max_mask_distance as a real threshold (the yaml documents 6.4239): masks whose mean camera depth exceeds
    it come back empty (generic.py:126-127), the others are untouched."""
    from holoagent_amd.synth import SceneSpec, SynthScene
    from oracle import hmsg_oracle as O
    from scipy.spatial import cKDTree
    spec = SceneSpec(seed=8, rooms_x=1, rooms_z=1, room_size=(5.0, 2.8, 4.0), objects_per_room=5, width=160, height=120,
                     n_frames=8, n_masks=12, feat_dim=32)
    scn = SynthScene(spec)
    frames = [scn.frame(i) for i in range(spec.n_frames)]
    thr = 2.2
    cfg = dict(voxel_size=0.05, clip_masked_weight=0.4418, max_mask_distance=thr, feat_dim=32, outlier_nb=300)
    sc = PC.make_scene(L, frames, dict(feat_dim=32, outlier_nb_points=300, max_mask_distance=thr))
    S, ref_pts, ref_cols = PC.check_map(sc, frames, cfg)
    PC.check_fuse(sc, frames, S, cfg, ref_pts, ref_cols, check_masks=True)
    n_empty = sum(1 for i in range(len(frames)) for m in sc.frame_masks3d(i) if len(m) == 0)
    n_all = sum(sc.frame_num_masks(i) for i in range(len(frames)))
    assert 0 < n_empty < n_all
    sc.close()


def test_configs1_full_size_properties(L):
    """The full configs[1] build (1000 frames, 640x480, M = 32, D = 512) on the device-rendered stream: properties that
    hold for any input, checked at the size the oracle cannot reach."""
    import torch
    import bench
    from holoagent_amd._lib import Scene, NodeIndex
    from holoagent_amd.synth import SceneSpec
    F, D, M = 1000, 512, 32
    spec = SceneSpec(seed=1234, n_frames=F, feat_dim=D, n_masks=M)
    device = torch.device("cuda", 0)
    inp = bench.build_scene_inputs(L, spec, device, torch)
    HW = spec.height * spec.width
    results = []
    for env in ({}, {"HMSG_DEBUG_NOANCHOR": "1"}):
        os.environ.pop("HMSG_DEBUG_NOANCHOR", None)
        os.environ.update(env)
        try:
            sc = Scene(lib_=L, height=spec.height, width=spec.width, max_frames=F, max_masks=M, feat_dim=D)
            sc.add_frames(inp["rgb"], inp["depth"], inp["pose"], inp["K"])
            sc.finalize_map()
            sc.add_frame_features(0, inp["masks"], inp["f_g"], inp["f_masked"], inp["f_crop"])
            sc.fuse_frames()
            sc.merge_instances()
            inst = sc.instances()
            if not env:
                V = sc.map_size()
                pts = sc.map_points()
                feats, counter = sc.map_feats(counter=True)
                # (1) counter = number of frames that touched the voxel: sum over frames of the distinct nearest voxels
                touched = 0
                mask_rows = []
                depth_h = inp["depth"].cpu().numpy().view(np.uint16)
                for f in range(F):
                    nn = sc.frame_nn(f)
                    assert ((nn >= 0) == (depth_h[f] > 0)).all()
                    u = np.unique(nn[nn >= 0])
                    assert u.size == 0 or u[-1] < V
                    touched += u.size
                    if f % 50 == 0:
                        mask_rows.append(np.concatenate(sc.frame_masks3d(f)))
                assert int(counter.sum()) == touched
                # (2) voxel features are means of unit-or-zero fp16 rows: norm <= 1 (+ rounding), zero where untouched
                nrm = np.linalg.norm(feats, axis=1)
                assert nrm.max() <= 1.0 + 1e-3 and np.all(nrm[counter == 0] == 0)
                # (3) every 3-D mask point is a mean of map points of one 5 cm voxel: within the map's bounding box and
                #     within sqrt(3) * 5 cm of a map point
                from scipy.spatial import cKDTree
                tree = cKDTree(pts)
                mp = np.concatenate(mask_rows)
                dmin, _ = tree.query(mp, k=1, workers=-1)
                assert dmin.max() <= 0.05 * np.sqrt(3) + 1e-9
                # (4) the fold only selects points: every instance point is one of the 3-D mask points (bit for bit)
                allm = np.concatenate([np.concatenate(sc.frame_masks3d(f)) for f in range(F)])
                keys = np.unique(np.ascontiguousarray(allm).view([("a", "V24")]).ravel())
                ip = np.concatenate(inst)
                ik = np.unique(np.ascontiguousarray(ip).view([("a", "V24")]).ravel())
                assert np.isin(ik, keys).all() and len(ip) <= len(allm)
                # (5) retrieval on the pooled table: indices and scores equal a float64 re-score on the host
                sc.pool_instances()
                emb = sc.instance_feats().astype(np.float64)
                text, _ = inp["scene"].text_table(64)
                ix = NodeIndex(emb, np.zeros(len(emb), np.int32), lib_=L)
                idx, _, score = ix.query_objects(text, np.zeros(64, np.int32), [[0]] * 64, 5)
                from oracle import hmsg_oracle as O
                for q in range(64):
                    top, s_ref = O.query_object(text[q], 0, emb, 5)
                    assert [int(v) for v in idx[q] if v >= 0] == [int(t) for t in top]
                    np.testing.assert_allclose(score[q][: len(top)], s_ref, rtol=0, atol=1e-12)
                ix.close()
            results.append(inst)
            sc.close()
        finally:
            os.environ.pop("HMSG_DEBUG_NOANCHOR", None)
    # (6) the merge fold's exact shortcuts change nothing at full size
    a, b = results
    assert len(a) == len(b) > 100
    for x, y in zip(a, b):
        assert x.shape == y.shape and np.array_equal(x, y)


def test_configs2_full_size_d1024_properties_and_retrieval_rate(L):
    """BASELINE.json configs[2] at FULL size: the same 1000-frame 640x480 scene with 1024-d features (the MFMA embedding x query GEMM
    path), whole graph behind the C ABI, 1000 coarse-to-fine queries.  Size-independent properties at a size the oracle cannot reach
    -- frame counters, feature norms, top-k equal to a float64 re-score on the host, graph counts -- and the retrieval RATE: round 4's
    D = 1024 line answered 40 k queries/s where D = 512 answered 400 k (an 8 MB pageable text table pinned on the fly, 24 ms); the
    two dimensions must stay within 2x of each other now."""
    import time
    import torch
    import bench
    from holoagent_amd._lib import Scene, SceneGraph
    from holoagent_amd.synth import SceneSpec
    from oracle import hmsg_oracle as O
    F, M, Q, k = 1000, 32, 1000, 5
    device = torch.device("cuda", 0)
    rate, counts = {}, {}
    for D in (1024, 512):
        spec = SceneSpec(seed=1234, n_frames=F, feat_dim=D, n_masks=M)
        inp = bench.build_scene_inputs(L, spec, device, torch)
        poses = np.ascontiguousarray(inp["pose"], np.float64).reshape(F, 4, 4)
        sc = Scene(lib_=L, height=spec.height, width=spec.width, max_frames=F, max_masks=M, feat_dim=D)
        sc.add_frames(inp["rgb"], inp["depth"], inp["pose"], inp["K"])
        sc.finalize_map()
        cg = SceneGraph.begin(sc, poses, inp["f_g"].cpu().numpy())
        sc.add_frame_features(0, inp["masks"], inp["f_g"], inp["f_masked"], inp["f_crop"])
        sc.fuse_frames()
        if D == 1024:
            feats, counter = sc.map_feats(counter=True)
            nrm = np.linalg.norm(feats, axis=1)
            assert feats.shape[1] == 1024 and nrm.max() <= 1.0 + 1e-3 and np.all(nrm[counter == 0] == 0) and counter.max() >= 2
            touched = sum(np.unique(nn[nn >= 0]).size for nn in (sc.frame_nn(f) for f in range(0, F, 25)))
            assert touched > 0 and int(counter.sum()) >= touched
        sc.merge_instances()
        sc.pool_instances()
        cg.finish()
        cnt = cg.counts()
        counts[D] = (cnt["floors"], cnt["rooms"], cnt["views"], cnt["objects"])
        assert cnt["floors"] == 1 and cnt["rooms"] >= 4 and cnt["views"] >= F and cnt["objects"] > 300 and cnt["view_object_links"] > 1000
        text, _ = inp["scene"].text_table(Q)
        rng = np.random.Generator(np.random.PCG64(4242))
        names = rng.standard_normal((cnt["rooms"], D))
        names /= np.linalg.norm(names, axis=1, keepdims=True)
        room_text = np.ascontiguousarray(names[rng.integers(0, cnt["rooms"], Q)], np.float32)
        ix = cg.index(names)
        zero = np.zeros(Q, np.int32)
        ix.query_hier(text, zero, room_text, zero, zero + 1, k)                    # (warm: buffers, pinned staging)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(3):
            sel, idx, room, score = ix.query_hier(text, zero, room_text, zero, zero + 1, k)
        rate[D] = 3 * Q / (time.perf_counter() - t0)
        # top-k bit-exact against a float64 re-score on the host: the objects of the selected rooms in room order, one negative prompt
        nodes, emb = sc.nodes(embeddings=True)
        emb = emb.astype(np.float64)
        node_room = np.array([int(n["room"]) for n in nodes])
        for q in range(0, Q, 37):
            cand = np.concatenate([np.nonzero(node_room == r)[0] for r in sel[q]]) if len(sel[q]) else np.zeros(0, np.int64)
            top, s_ref = O.query_object(text[q], 0, emb[cand], k)
            assert [int(v) for v in idx[q] if v >= 0] == [int(cand[t]) for t in top], (D, q)
            np.testing.assert_allclose(score[q][: len(top)], s_ref, rtol=0, atol=1e-12)
        ix.close()
        cg.close()
        sc.close()
        del inp
        torch.cuda.empty_cache()
    print("hierarchical queries / s: D = 1024: %.0f, D = 512: %.0f; graphs (floors, rooms, views, objects): %s" % (rate[1024], rate[512], counts))
    assert rate[1024] > 1e5, rate                                                   # (round 4's line: 4.0e4)
    assert rate[1024] * 2 >= rate[512], rate


def test_episode_shape_1280x720_three_floors_against_oracle(L):
    """configs[4]'s shape: 1280x720 frames of a three-storey scene (three one-floor scenes stacked 3.4 m apart), 12 frames,
    32 masks -- map, fusion, 3-D masks, sequential merge and pooling stage-wise against the oracle (bit-identical clouds,
    pooled features within 1e-5), with the incremental fold forced from the first step as well, and the floor
    segmentation of the mirror (graph.py:624-787) has to split the height into storeys."""
    from holoagent_amd.synth import SceneSpec, SynthScene
    from holoagent_amd.graph import Graph
    D, W, H, per_floor, storey = 32, 1280, 720, 4, 3.4
    frames = []
    for fl in range(3):
        spec = SceneSpec(seed=90 + fl, rooms_x=1, rooms_z=1, room_size=(4.6, 2.8, 4.0), objects_per_room=5, width=W, height=H,
                         n_frames=per_floor, n_masks=32, feat_dim=D, yaw_step_deg=24.0)
        scn = SynthScene(spec)
        for i in range(per_floor):
            fr = scn.frame(i)
            fr["pose"] = np.array(fr["pose"], np.float64)
            fr["pose"][1, 3] += fl * storey                  # up = +y
            frames.append(fr)
    cfg = dict(voxel_size=0.05, clip_masked_weight=0.4418, max_mask_distance=10000, feat_dim=D, init_overlap_thresh=0.75,
               overlap_thresh_factor=0.025, iou_thresh=0.05, merge_type="sequential", outlier_nb=400)
    for env in ({}, {"HMSG_FOLD_INCREMENTAL": "1"}):
        os.environ.pop("HMSG_FOLD_INCREMENTAL", None)
        os.environ.update(env)
        try:
            sc = PC.make_scene(L, frames, dict(feat_dim=D, outlier_nb_points=400))
            S, ref_pts, ref_cols = PC.check_map(sc, frames, cfg)
            assert ref_pts.shape[0] > 10000
            assert ref_pts[:, 1].max() - ref_pts[:, 1].min() > 2 * storey
            ref_feats, _ = PC.check_fuse(sc, frames, S, cfg, ref_pts, ref_cols, check_masks=True)
            got, feats = PC.check_merge_pool(sc, frames, cfg, ref_pts, ref_feats)
            assert len(got) >= 12
            if not env:
                g = Graph.from_scene(sc, lib=L)
                ranges = np.array(g.segment_floors_manually(None), np.float64).reshape(-1, 2)
                # (the peak logic of graph.py:660-760 -- pinned against the reference by tests/test_floors_golden.py --
                #  also reports the slabs between a ceiling and the next storey's floor: at least the three storeys,
                #  contiguous, covering the whole height)
                assert len(g.floors) >= 3, ranges
                assert np.all(ranges[1:, 0] == ranges[:-1, 1]) and ranges[-1, 1] - ranges[0, 0] > 2 * storey, ranges
            sc.close()
        finally:
            os.environ.pop("HMSG_FOLD_INCREMENTAL", None)


def test_many_masks_and_edge_frames_against_oracle(L):
    """Three- and four-word mask bitsets (150-200 masks per frame), a frame without masks and a frame without valid depth,
    on the real device against the oracle (the simulator variants live in tests/test_emu_parity.py)."""
    from tests import golden_io as GI
    from tests.test_emu_parity import test_four_word_mask_bitsets, test_frames_without_masks_or_depth
    assert GI.load("build_hier") is not None
    test_four_word_mask_bitsets(L)
    test_frames_without_masks_or_depth(L)


def test_fold_collector_is_exact_on_device(L):
    """Merger::collect (compaction of the fold's point pool, grid arenas reset; used by very long episodes) forced after
    every frame on a 60-frame device-rendered stream: instances identical to the plain fold, bit for bit."""
    import torch
    import bench
    from holoagent_amd._lib import Scene
    from holoagent_amd.synth import SceneSpec
    F, D, M = 60, 64, 32
    spec = SceneSpec(seed=77, n_frames=F, feat_dim=D, n_masks=M, width=320, height=240)
    inp = bench.build_scene_inputs(L, spec, torch.device("cuda", 0), torch)
    out = []
    for env in ({}, {"HMSG_DEBUG_GC_POINTS": "1"}):
        os.environ.pop("HMSG_DEBUG_GC_POINTS", None)
        os.environ.update(env)
        try:
            sc = Scene(lib_=L, height=spec.height, width=spec.width, max_frames=F, max_masks=M, feat_dim=D)
            for a in range(0, F, 25):                                   # chunked hand-over, like the streaming driver
                b = min(F, a + 25)
                sc.add_frames(inp["rgb"][a:b], inp["depth"][a:b], inp["pose"][a:b], inp["K"])
                sc.add_frame_features(a, inp["masks"][a:b], inp["f_g"][a:b], inp["f_masked"][a:b], inp["f_crop"][a:b])
            sc.finalize_map()
            sc.fuse_frames()
            sc.merge_instances()
            out.append(sc.instances())
            sc.close()
        finally:
            os.environ.pop("HMSG_DEBUG_GC_POINTS", None)
    assert len(out[0]) == len(out[1]) > 10
    for x, y in zip(out[0], out[1]):
        assert np.array_equal(x, y)


@pytest.mark.parametrize("mode", ["scene", "episode"])
def test_bench_rccl_path_with_one_rank(mode):
    """bench.py's multi-GPU code paths executed on the one GPU of this box (HMSG_BENCH_FORCE_DIST=1: process group on
    the nccl backend = RCCL, device tensors in the collectives): scene mode (all-gather of the node tables) and episode
    mode (all-reduce of the voxel feature sums, sharded merge tree, root-side pooling / retrieval).  The 8-GPU runs are
    the driver's; this keeps the RCCL code from rotting."""
    import json
    import subprocess
    import sys
    root = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
    env = dict(os.environ, HMSG_BENCH_FORCE_DIST="1", MASTER_ADDR="127.0.0.1", MASTER_PORT="29617", RANK="0", WORLD_SIZE="1", LOCAL_RANK="0")
    out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "1", "--warmup", "0", "--frames", "96",
                          "--queries", "64", "--cpu-frames", "0", "--mode", mode], env=env, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-3000:]
    rec = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    assert rec["rccl_ranks"] == 1 and rec["n_gpus"] == 1 and rec["value"] > 0
    assert rec["scaling"] == ("strong" if mode == "episode" else "weak")
    assert rec["nodes_local"] > 5 and rec["queries_per_sec"] > 0


def test_bench_plain_line_and_dump_outputs(tmp_path):
    """A plain `bench.py` run (no --full) times exactly --steps steps, reports `ms_per_step` and none of the --full legs, and
    --dump-outputs writes what the last timed step handed its caller: float32 / float64 arrays, 64 MB at most, retrieval
    answers that index the dumped node table."""
    import json
    import subprocess
    import sys
    root = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
    env = dict(os.environ)
    for k_ in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "HMSG_BENCH_FORCE_DIST"):
        env.pop(k_, None)
    out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--frames", "96",
                          "--queries", "64", "--dump-outputs", str(tmp_path)], env=env, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-3000:]
    rec = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    assert rec["steps"] == 2 and rec["warmup"] == 1 and rec["full"] is False and rec["unit"] == "frames/s"
    assert abs(rec["value"] - 96 / (rec["ms_per_step"] / 1e3)) < 1e-2 * rec["value"] + 1e-3
    for k_ in ("roofline", "cpu_baseline", "retrieval_resident", "scenes_in_flight", "rooms_handed_in", "encoder_handoff", "kernels_ms_last_step"):
        assert rec[k_] is None, k_
    got = {f[: -len(".npy")]: np.load(os.path.join(tmp_path, f)) for f in os.listdir(tmp_path)}
    for name in ("query_idx", "query_room", "query_score", "query_rooms_selected", "node_records", "node_embeddings", "graph_counts",
                 "graph_objects", "map_points"):
        assert name in got, name
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert sum(a.nbytes for a in got.values()) <= 64 << 20
    idx, score = got["query_idx"], got["query_score"]
    assert idx.shape == (64, 5) and score.shape == (64, 5) and (idx >= 0).any()
    assert idx.max() < got["node_records"].shape[0] and np.isfinite(score[idx >= 0]).all()
    assert got["node_embeddings"].shape == (got["node_records"].shape[0], 512) and got["map_points"].shape[1] == 3
    assert got["graph_counts"][3] == rec["graph_counts"]["objects"] == got["graph_objects"].shape[0]
