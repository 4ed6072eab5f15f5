#!/usr/bin/env python
"""Headline benchmark: HMSG build (frames/s) + retrieval (queries/s) on synthetic posed RGB-D.

    python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]

Workload (BASELINE.json configs[1]): one 1000-frame 640x480 scene per GPU, 32 masks/frame, 512-d
features, build A1..A7 + node table + 1000 hierarchical object queries.  A "step" is one full pass of
the hot path over that scene (reset -> frames -> map -> fuse -> merge -> pool -> index -> queries) with
the inputs already resident in HBM.  N>1: one scene per rank (weak scaling), node tables all-gathered
over RCCL for cross-scene retrieval, every rank answers Q/N of the queries on the global table.

Prints ONE JSON line (rank 0).  A plain run sets up, warms up, times the K steps and prints the driver contract
(`metric`, `value`, `unit`, `higher_is_better`, `dtype`, `ms_per_step`, stage times).  `--full` adds everything else:
`roofline` (dominant kernel, HIP-event timed on the library's own stream in the last timed step) and the per-kernel
figures, the resident-index retrieval leg, scenes in flight, rooms handed in, the encoder hand-off leg and
`cpu_baseline` (the compiled CPU restatement on a bounded sample of the same frames, N=1 only).

`--dump-outputs DIR` writes what the timed path handed its caller in the last timed step (retrieval answers, node
table, graph records, a fixed sample of the map) as float32 / float64 .npy files; the inputs are seeded, so two
builds run with the same arguments can be compared output for output.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
MFMA_KERNELS = ("k_pool_gram", "k_gemm_f64")      # FLOP-priced; everything else is priced in algorithmic bytes
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0        # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec


def build_scene_inputs(L, spec, device, torch):
    """Render the synthetic stream into HBM (bench utility kernel) and build the encoder-output tensors."""
    import ctypes as C
    from holoagent_amd.synth import SynthScene
    scn = SynthScene(spec)
    F, H, W, M, D = spec.n_frames, spec.height, spec.width, spec.n_masks, spec.feat_dim
    poses = np.zeros((F, 16))
    room_of = np.zeros(F, np.int32)
    for i in range(F):
        T, rid = scn.pose(i)
        poses[i] = T.reshape(-1)
        room_of[i] = rid
    rooms = np.array([np.concatenate([lo, hi]) for lo, hi in scn.rooms])
    # objects grouped by room (they are generated room by room)
    obj = np.array([np.concatenate([lo, hi]) for _, lo, hi in scn.objects]).reshape(-1, 6)
    obj_room = np.array([r for r, _, _ in scn.objects], np.int32)
    off = np.zeros(len(scn.rooms) + 1, np.int32)
    for r in obj_room:
        off[r + 1] += 1
    off = np.cumsum(off).astype(np.int32)
    rgb = torch.empty((F, H, W, 3), dtype=torch.uint8, device=device)
    depth = torch.empty((F, H, W), dtype=torch.int16, device=device)       # raw u16 storage
    masks = torch.empty((F, M, H, W), dtype=torch.uint8, device=device)
    ment = np.zeros((F, M), np.int32)
    K = np.ascontiguousarray(scn.K, np.float64)
    rc = L.c.hmsg_synth_render(device.index or 0, F, H, W, M, K.ctypes.data, poses.ctypes.data, room_of.ctypes.data,
                               len(scn.rooms), np.ascontiguousarray(rooms).ctypes.data, len(scn.objects),
                               np.ascontiguousarray(obj).ctypes.data, off.ctypes.data, spec.depth_noise_mm, spec.seed,
                               rgb.data_ptr(), depth.data_ptr(), masks.data_ptr(), ment.ctypes.data)
    assert rc == 0, "hmsg_synth_render failed"
    rng = np.random.Generator(np.random.PCG64([spec.seed, 424242]))
    u = scn.entity_feats[ment]                                              # [F, M, D]
    f_masked = u + spec.feat_noise * rng.standard_normal(u.shape).astype(np.float32)
    f_crop = u + spec.feat_noise * rng.standard_normal(u.shape).astype(np.float32)
    f_masked /= np.linalg.norm(f_masked, axis=-1, keepdims=True)
    f_crop /= np.linalg.norm(f_crop, axis=-1, keepdims=True)
    f_g = u.mean(axis=1)
    f_g /= np.linalg.norm(f_g, axis=-1, keepdims=True)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(device)
    return dict(scene=scn, rgb=rgb, depth=depth, masks=masks, pose=np.ascontiguousarray(poses), K=K,
                f_g=dev(f_g), f_masked=dev(f_masked), f_crop=dev(f_crop), rooms=rooms, obj_room=obj_room)


def assign_rooms(boxes, rooms):
    """instance -> room by AABB centre (the scene's rooms are given, SURVEY 8c: rooms are an input)."""
    c = (boxes[:, :3] + boxes[:, 3:]) / 2
    inside = (c[:, None, :] >= rooms[None, :, :3] - 1e-6) & (c[:, None, :] <= rooms[None, :, 3:] + 1e-6)
    inside = inside.all(-1)
    rid = inside.argmax(1)
    none = ~inside.any(1)
    if none.any():
        rc = (rooms[:, :3] + rooms[:, 3:]) / 2
        rid[none] = np.linalg.norm(c[none, None, :] - rc[None], axis=-1).argmin(1)
    return rid.astype(np.int32)


DUMP_MAX_BYTES = 64 << 20          # --dump-outputs: all files together
DUMP_ARRAY_BYTES = 5 << 20         # one array; larger ones keep a fixed, evenly spaced sample of their rows


def dump_outputs(out_dir, sc, state):
    """--dump-outputs: what the last timed step handed its caller -- the retrieval answers, the node table the answers
    index, the graph's records and the map -- as <out_dir>/<name>.npy in float64 (float32 for the float32 embeddings)."""
    from holoagent_amd._lib import SceneGraph
    arrays = {}
    last = state.get("last")
    if last is not None:
        for name, a in zip(("query_idx", "query_room", "query_score"), last):
            arrays[name] = a
    sel = state.get("sel")
    if sel is not None:
        packed = np.full((len(sel), max([len(s_) for s_ in sel] + [1])), -1.0)   # (ragged: -1 pads a query's room list)
        for q, s_ in enumerate(sel):
            packed[q, : len(s_)] = s_
        arrays["query_rooms_selected"] = packed
    recs, emb = sc.nodes(embeddings=True)
    arrays["node_records"] = np.stack([recs[f] for f in recs.dtype.names], 1)       # instance, floor, room, counter, label, n_points
    arrays["node_embeddings"] = emb
    g = state.get("graph")
    if isinstance(g, SceneGraph):
        cnt = g.counts()
        arrays["graph_counts"] = np.array([cnt[f] for f in ("floors", "rooms", "views", "objects", "edges", "view_object_links")])
        arrays["graph_edges"] = g.edges()
        arrays["graph_objects"] = np.array([[o[f] for f in ("room", "instance", "label", "n_views", "best_view")] for o in g.objects()]
                                           ).reshape(-1, 5)
        arrays["graph_rooms"] = np.array([[r[f] for f in ("floor", "n_vertices", "n_points", "n_embeddings", "n_objects", "n_views")]
                                          for r in g.rooms()]).reshape(-1, 6)
    if sc.map_size():
        xyz = sc.map_points()
        arrays["map_points"] = xyz[np.lexsort(xyz.T[::-1])]     # (sorted by x, y, z: a sample that does not depend on the map's order)
    os.makedirs(out_dir, exist_ok=True)
    total = 0
    for name, a in arrays.items():
        a = np.asarray(a)
        a = a.astype(np.float32 if a.dtype == np.float32 else np.float64)
        row_bytes = max(a[:1].nbytes, 1) if a.ndim else a.nbytes
        if a.ndim and a.nbytes > DUMP_ARRAY_BYTES:
            a = a[np.linspace(0, len(a) - 1, max(DUMP_ARRAY_BYTES // row_bytes, 1)).astype(np.int64)]
        total += a.nbytes
        assert total <= DUMP_MAX_BYTES
        np.save(os.path.join(out_dir, name + ".npy"), a)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=2, help="timed steps (at least 1)")
    ap.add_argument("--warmup", type=int, default=2,
                    help="untimed steps (2: the library's per-thread device allocator cache settles over the first two scenes -- a "
                         "service that builds scene after scene runs in that state)")
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--queries", type=int, default=1000)
    ap.add_argument("--feat-dim", type=int, default=512)
    ap.add_argument("--topk", type=int, default=5)
    ap.add_argument("--cpu-frames", type=int, default=100,
                    help="frames of the CPU baseline (0 = skip).  100 = BASELINE.json configs[0] in full (100 frames + 100 queries, "
                         "~100 s on the GPU box's host); the CPU rate FALLS with the number of frames -- the sequential merge "
                         "re-clusters every cloud every frame, as the reference does")
    ap.add_argument("--cpu-frames-extra", type=int, default=0,
                    help="a SECOND CPU point: the compiled restatement on the first N frames of the same scene as well (e.g. 250: the "
                         "CPU rate falls with the number of frames; minutes of CPU time, so off by default -- profiles/ holds a run)")
    ap.add_argument("--resident-repeats", type=int, default=20,
                    help="repeats of the 1000-query batch of the resident-index retrieval leg (0: skip the leg)")
    ap.add_argument("--mode", choices=("scene", "episode"), default="scene",
                    help="scene: one scene per GPU, node tables all-gathered (configs[1]/[3], weak scaling); episode: ONE "
                         "episode of --frames frames sharded over the GPUs -- frame windows per rank, all-reduce of the voxel "
                         "feature sums, hierarchical merge tree with cross-rank joins, pooling + retrieval on the root "
                         "(configs[4], strong scaling)")
    ap.add_argument("--inflight-steps", type=int, default=2,
                    help="scenes per handle of the extra scenes-in-flight measurement (0 = skip; N = 1 scene mode only)")
    ap.add_argument("--inflight", type=int, default=2, help="handles (scenes in flight) of that extra measurement")
    ap.add_argument("--rooms-handed-in", action="store_true",
                    help="round 1-3's line: ready-made room regions without views handed to the graph assembly.  The default (scene "
                         "mode, one GPU) hands NOTHING in: rooms from the device watershed (N1), room clouds, room embeddings and "
                         "View nodes (A9), objects with the view <-> object test on the device (A10)")
    ap.add_argument("--full-graph", action="store_true", help="(accepted for compatibility: the default now)")
    ap.add_argument("--python-graph", action="store_true",
                    help="the graph level through the Python mirror of the reference's Graph (scikit-learn KMeans, networkx) instead of "
                         "the graph object behind the C ABI")
    ap.add_argument("--encoder-frames", type=int, default=8,
                    help="frames of the extra encoder hand-off leg (random-init ViT-B/32-shaped PyTorch-ROCm module -> features by "
                         "data_ptr() into hmsg_add_frame_features; reported beside `value`, never in it; 0 = skip)")
    ap.add_argument("--full", action="store_true",
                    help="everything besides the headline figure: per-kernel / roofline figures of the last timed step, the resident-index "
                         "retrieval leg, scenes in flight, rooms handed in, the encoder hand-off leg and the CPU baseline (off: a plain run "
                         "sets up, warms up, times the steps and prints the line)")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="after the timed steps, write what the last timed step computed (retrieval answers, node table, graph "
                         "records, a fixed sample of the map) as DIR/<name>.npy, float32 / float64, at most 64 MB in all")
    ap.add_argument("--no-extras", action="store_true",
                    help="with --full: no CPU baseline, scenes-in-flight, rooms-handed-in or encoder hand-off legs")
    ap.add_argument("--scene-shape", default=None,
                    help="development sizes (the simulator test): ROOMS_X,ROOMS_Z,ROOM_X_M,ROOM_Y_M,ROOM_Z_M,YAW_STEP_DEG,OBJECTS_PER_ROOM of "
                         "the synthetic building instead of configs[1]'s 4 x 2 rooms of 5 x 3 x 4 m, 10 degrees a frame, 8 objects a room")
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--height", type=int, default=480)
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")

    # `python bench.py --gpus N` (N > 1) without a launcher: become the launcher -- one process per GPU under
    # torch.distributed.run on 127.0.0.1, same arguments; rank 0's JSON line is the output.
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        import subprocess
        port = os.environ.get("MASTER_PORT", "29511")
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
               "--master-addr", "127.0.0.1", "--master-port", port, os.path.abspath(__file__)] + sys.argv[1:]
        env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
        sys.exit(subprocess.call(cmd, env=env))

    if args.no_extras:
        args.cpu_frames, args.inflight_steps, args.encoder_frames = 0, 0, 0
    import torch
    import torch.distributed as dist
    from holoagent_amd._lib import HmsgLib, Scene, NodeIndex
    from holoagent_amd.synth import SceneSpec

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    # HMSG_BENCH_FORCE_DIST=1 drives the RCCL code path (process group, all-gather of the node tables, max-over-ranks
    # timing) even with a single rank: the multi-GPU launch is the driver's, this is how it is smoke-tested on one GPU
    use_dist = world > 1 or bool(os.environ.get("HMSG_BENCH_FORCE_DIST"))
    if use_dist:
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29511")
    assert world == max(1, args.gpus), "WORLD_SIZE (%d) != --gpus (%d)" % (world, args.gpus)
    if os.environ.get("HMSG_BENCH_SPAWN_ONLY"):
        # launch check without a GPU (tests/test_distributed_gloo.py): rendezvous over gloo, report the rank count
        dist.init_process_group("gloo", rank=rank, world_size=world)
        t = torch.tensor([rank + 1], dtype=torch.int64)
        dist.all_reduce(t)
        if rank == 0:
            print(json.dumps({"spawn_check": True, "n_gpus": world, "rank_sum": int(t.item())}))
        dist.destroy_process_group()
        return
    # HMSG_BENCH_EMU=<path of tests/emu/libhmsg_emu.so>: the whole script against the kernel simulator on the CPU with tiny
    # sizes (tests/test_bench_contract.py: the JSON contract, every code path of a step) -- never a measurement, and the
    # line says so ("emulated": true)
    emu = os.environ.get("HMSG_BENCH_EMU")
    if emu:
        # (several ranks on the simulator only with a stand-in for librccl, HMSG_RCCL_LIB = tests/rccl_double: the test of the
        #  N > 1 code path of this script, tests/test_bench_contract.py)
        assert not use_dist or os.environ.get("HMSG_RCCL_LIB"), "the simulator run is single-process"
        device = torch.device("cpu")
        sync = lambda: None
        local = 0                                   # (the simulator has one device)
        if use_dist:
            dist.init_process_group("gloo", rank=rank, world_size=world)
        L = HmsgLib(emu)
    else:
        torch.cuda.set_device(local)
        device = torch.device("cuda", local)
        sync = torch.cuda.synchronize
        if use_dist:
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=device)
        L = HmsgLib()                      # fails loudly without the HIP library

    F, Q, D, k = args.frames, args.queries, args.feat_dim, args.topk
    episode = args.mode == "episode"
    # (episode mode: every rank sees the same episode -- same seed; scene mode: a scene per rank)
    # the whole graph (A8-A11, nothing handed in) is the line; the multi-GPU legs take the rooms as given (the all-gathered
    # retrieval of scene mode addresses rooms by their global ids; episode mode assembles on the root only)
    # (round 5: the multi-GPU scene mode times the SAME step as one GPU -- every rank builds its whole graph -- and answers
    #  hmsg_query_hier on the all-gathered table; episode mode assembles on the root only and takes the rooms as given)
    args.full_graph = not args.rooms_handed_in and not episode
    shape = {}
    if args.scene_shape:
        v = [float(x) for x in args.scene_shape.split(",")]
        shape = dict(rooms_x=int(v[0]), rooms_z=int(v[1]), room_size=(v[2], v[3], v[4]), yaw_step_deg=v[5], objects_per_room=int(v[6]))
    spec = SceneSpec(seed=1234 + (0 if episode else rank), n_frames=F, feat_dim=D, n_masks=32, width=args.width, height=args.height, **shape)
    inp = build_scene_inputs(L, spec, device, torch)
    scn = inp["scene"]
    text, q_ent = scn.text_table(Q)                               # [Q, 2, D] (query, negative)
    n_rooms = len(scn.rooms)
    ent_room = np.concatenate([inp["obj_room"], np.repeat(np.arange(n_rooms), 6)])
    q_rooms = [[int(ent_room[e]), int((ent_room[e] + 1) % n_rooms)] for e in q_ent]   # (multi-GPU leg: room sets handed in)
    # room names stand in for CLIP text embeddings of "room<i>": random unit rows; a query names its entity's room
    rng_r = np.random.Generator(np.random.PCG64(4242))
    room_name_feats = rng_r.standard_normal((n_rooms, D))
    room_name_feats /= np.linalg.norm(room_name_feats, axis=1, keepdims=True)
    room_text = np.ascontiguousarray(room_name_feats[ent_room[q_ent]], np.float32)

    from holoagent_amd.graph import Graph
    # rooms are an input of the path: 2-D vertex grids at grid_resolution 0.05 like the reference's
    room_specs = []
    for lo6 in inp["rooms"]:
        xs, zs = np.arange(lo6[0], lo6[3], 0.05), np.arange(lo6[2], lo6[5], 0.05)
        room_specs.append(dict(floor=0, vertices=np.stack(np.meshgrid(xs, zs, indexing="ij"), -1).reshape(-1, 2)))
    # the default line hands nothing in -- the Graph gets what the reference's Graph has: a dataset to ask for a frame's pose and
    # image size (the images themselves stay in HBM) and the frames' global features (the F_g the fusion already received)
    full_cfg = dict(main=dict(device_id=local), models=dict(clip=dict(feat_dim=D)),
                    pipeline=dict(grid_resolution=0.05, skip_frames=1, views_on_device=True))
    poses_host = [np.asarray(inp["pose"][i], np.float64).reshape(4, 4) for i in range(F)]
    blank = np.broadcast_to(np.zeros((), np.uint8), (spec.height, spec.width, 3))

    class FrameSource:
        def __len__(self):
            return F

        def __getitem__(self, i):
            return blank, None, poses_host[i], None, None

        def get_camera_intrinsics(self):
            return inp["K"]
    fg_host = inp["f_g"].cpu().numpy() if args.full_graph else None
    poses_arr = np.ascontiguousarray(np.stack(poses_host))            # [F, 4, 4] camera -> world of the processed frames
    from holoagent_amd._lib import SceneGraph
    # --python-graph: the graph level through the Python mirror of the reference's Graph (rounds 3-4's form of the line) instead of
    # the graph object behind the C ABI (hmsg_graph_begin / hmsg_graph_finish / hmsg_graph_index)
    c_graph = args.full_graph and (not args.python_graph or use_dist)
    gt_boxes = np.asarray(inp["rooms"], np.float64)

    def gt_room_of(xz):
        """ground-truth room of a segmented region: the box that holds the centroid of its cells (nearest centre otherwise)"""
        c = np.asarray(xz, np.float64).mean(axis=0)
        inside = (c[0] >= gt_boxes[:, 0]) & (c[0] <= gt_boxes[:, 3]) & (c[1] >= gt_boxes[:, 2]) & (c[1] <= gt_boxes[:, 5])
        if inside.any():
            return int(np.argmax(inside))
        ctr = np.stack([(gt_boxes[:, 0] + gt_boxes[:, 3]) / 2, (gt_boxes[:, 2] + gt_boxes[:, 5]) / 2], 1)
        return int(np.argmin(np.linalg.norm(ctr - c[None], axis=1)))
    rng_l = np.random.Generator(np.random.PCG64(99))
    label_feats = rng_l.standard_normal((205, D)).astype(np.float32)      # scannet200-sized label vocabulary
    label_feats /= np.linalg.norm(label_feats, axis=1, keepdims=True)
    label_names = ["label%d" % i for i in range(205)]
    sc = Scene(lib_=L, device_id=local, height=spec.height, width=spec.width, max_frames=F, max_masks=32, feat_dim=D,
               merge_type=1 if episode else 0)
    # HIP-event brackets of the instrumented kernels (roofline.achieved) are recorded in the LAST timed step only: an event pair costs
    # a few us on the fold's stream, a fold step is ~20 dependent launches, and `value` should not pay for the instrument 20 times
    prof_on = {"on": False}
    sc.set_profiling(False)
    # episode mode: rank r owns the frame window [r * chunk, (r + 1) * chunk), chunk a power of two (a subtree of the merge tree)
    chunk = 1
    while chunk * world < F:
        chunk *= 2
    win = (min(F, rank * chunk), min(F, (rank + 1) * chunk))
    if episode:
        assert (world - 1) * chunk < F, "--frames too small for %d ranks" % world
    stage = {}

    def T(name, fn):
        t0 = time.perf_counter()
        r = fn()
        stage[name] = stage.get(name, 0.0) + (time.perf_counter() - t0)
        return r

    state = {}

    def step_episode():
        """configs[4]: every rank holds the whole map (all frames' geometry: replicated, the order-faithful float64 voxel
        sums are not associative) and the features / masks of its own frame window; voxel feature sums all-reduced over
        RCCL, merge tree sharded (hmsg_merge_tree_local + cross-rank joins, HBM to HBM), the root pools, assembles, answers."""
        from holoagent_amd.dist import allreduce_feature_sums, sharded_hierarchical_merge
        sc.reset()
        T("add_frames", lambda: sc.add_frames(inp["rgb"], inp["depth"], inp["pose"], inp["K"]))
        T("finalize_map", sc.finalize_map)
        a, b = win
        sc.set_frame_window(a)
        T("add_frame_features", lambda: sc.add_frame_features(a, inp["masks"][a:b], inp["f_g"][a:b], inp["f_masked"][a:b], inp["f_crop"][a:b]))
        T("fuse_frames", sc.fuse_frames)
        if use_dist:
            if not emu and not os.environ.get("HMSG_BENCH_TORCH_GATHER") and state.get("comm") is not False:
                # behind the C ABI: librccl on the handle's own buffers, in place (hmsg_allreduce_feature_sums)
                from holoagent_amd._lib import Comm
                try:
                    if state.get("comm") is None:
                        state["comm"] = Comm.from_torch(local, L)
                except Exception as e:
                    print("hmsg_comm_create unavailable (%r): torch.distributed all_reduce instead" % (e,), file=sys.stderr)
                    state["comm"] = False
            if state.get("comm"):
                T("allreduce_feature_sums", lambda: sc.allreduce_feature_sums(state["comm"]))
            else:
                T("allreduce_feature_sums", lambda: allreduce_feature_sums(sc, device=device))
            if state.get("comm"):
                # the whole sharded tree behind the C ABI (hmsg_merge_tree_sharded: local levels, agreement, joins over ncclSend / ncclRecv)
                holds = T("merge_tree", lambda: sc.merge_tree_sharded(state["comm"], F))
            else:
                holds = T("merge_tree", lambda: sharded_hierarchical_merge(sc, F, device=device))
        else:
            def whole():
                th, lists, idx = sc.merge_tree_local(F)
                assert lists == 1 and idx == 0
                sc.merge_tree_join([], th, final_pass=True)
                return True
            holds = T("merge_tree", whole)
        state["last"] = None
        state["n_nodes_local"] = 0
        if holds:
            T("pool_instances", sc.pool_instances)
            g = T("assemble/from_scene", lambda: Graph.from_scene(sc, lib=L))
            g.set_label_feats(label_feats, label_names)
            T("assemble/build_hier", lambda: g.build_hier_multimodal_scene_graph(None, rooms=room_specs))
            state["n_nodes_local"] = len(g.objects)
            if g.objects:
                def retrieve():
                    ix = sc.index_from_nodes()
                    ix.set_profiling(prof_on["on"])
                    ix.set_hierarchy([list(range(n_rooms))], room_name_feats, [np.zeros((0, D))] * n_rooms, list(range(n_rooms)))
                    sel, idx, room, score = ix.query_hier(text, np.zeros(len(text), np.int32), room_text, np.zeros(len(text), np.int32),
                                                          np.ones(len(text), np.int32), k)
                    state["gemm"] = ix.profile()
                    state["sel"] = sel
                    ix.close()
                    return idx, room, score
                state["last"] = T("retrieval", retrieve)

    def step():
        if episode:
            return step_episode()
        sc.reset()
        g_early = None

        def room_level():
            # the room level needs only the map and the frames' global features: floors, room regions (device watershed), room
            # clouds and the camera -> room table run here (device), the KMeans views on host threads beside the fusion and the
            # fold -- hmsg_graph_begin (the library's own threads and its restated KMeans); with --python-graph
            # Graph.start_room_level (scikit-learn on a Python thread), as Graph.create_feature_map does.
            if c_graph:
                old = state.pop("graph", None)
                if old is not None:
                    old.close()
                return SceneGraph.begin(sc, poses_arr, fg_host)
            g = Graph.from_scene(sc, cfg=full_cfg, lib=L, instances=False)
            g.dataset = FrameSource()
            g._poses = poses_host
            g.set_view_feats(fg_host)
            g.start_room_level()
            return g
        T("add_frames", lambda: sc.add_frames(inp["rgb"], inp["depth"], inp["pose"], inp["K"]))
        T("finalize_map", sc.finalize_map)
        # Placement of the room level (floors, regions, room clouds, camera -> room table on the device; KMeans on the library's host
        # threads): AFTER hmsg_fuse_frames, i.e. beside the merge fold, which runs on its worker thread and stream and leaves the chip
        # almost idle between its short launches -- the room level's 20 ms of kernels run in those gaps.  Measured on the MI355X,
        # alternating runs of 5 steps on one box (profiles/r05_rooms_beside_fold.txt): 503.8 / 496.5 ms per step with the room level
        # in front of the fusion, 481.2 / 492.2 ms beside the fold (room level 20 -> 22 ms, the rest of the fold 299 -> 284 ms).
        # Round 4 measured the opposite (620 -> 630 ms) when the room level was 53 ms of long ring searches; its kernels are short
        # now.  HMSG_BENCH_ROOMS_BEFORE_FUSE=1 keeps the old order.
        beside_fold = not os.environ.get("HMSG_BENCH_ROOMS_BEFORE_FUSE")
        if args.full_graph and not beside_fold:
            g_early = T("room_level/device", room_level)
        T("add_frame_features", lambda: sc.add_frame_features(0, inp["masks"], inp["f_g"], inp["f_masked"], inp["f_crop"]))
        T("fuse_frames", sc.fuse_frames)
        if args.full_graph and beside_fold:
            g_early = T("room_level/device", room_level)

        T("merge_instances", sc.merge_instances)
        T("pool_instances", sc.pool_instances)

        def assemble():
            # A8 floors, A10 objects (device: instance DBSCAN(0.05,10), object->room share, label GEMM), A11 node
            # records -- holoagent_amd.graph.Graph, the mirror of the reference's Graph; rooms are an input.
            if c_graph:
                # floors (A8), rooms by the device watershed (N1), room clouds, camera -> room assignment, KMeans views and View
                # nodes (A9) came with hmsg_graph_begin; objects with the view <-> object test on the device (A10) and the
                # edges (A11) now -- one call, no Python in between
                T("assemble/graph_finish", lambda: g_early.finish(label_feats, label_names))
                state["graph"] = g_early
                return None, None
            if args.full_graph:
                g = g_early
                T("assemble/take_instances", g.take_instances)
                T("assemble/wait_room_level", lambda: g._room_level["thread"].join())
                g.set_label_feats(label_feats, label_names)
                # floors (A8) -> per storey: rooms by the device watershed (N1), room clouds, camera -> room assignment, KMeans
                # views and View nodes (A9) -> objects with the view <-> object test on the device (A10) -> graph (A11)
                T("assemble/build_hier", lambda: g.build_hier_multimodal_scene_graph(None))
                state["graph"] = g
            else:
                g = T("assemble/from_scene", lambda: Graph.from_scene(sc, lib=L))
                g.set_label_feats(label_feats, label_names)
                T("assemble/build_hier", lambda: g.build_hier_multimodal_scene_graph(None, rooms=room_specs))
            rid = {r.room_id: i for i, r in enumerate(g.rooms)}
            feats = np.stack([o.embedding for o in g.objects]).astype(np.float64) if g.objects else np.zeros((0, D))
            rooms = np.array([rid[o.room_id] for o in g.objects], np.int32)   # embeddings are f64 once stored (object.py:88-89)
            return feats, rooms
        if os.environ.get("HMSG_BENCH_PROFILE_ASSEMBLE"):      # development aid: where the host-side stage spends its time
            import cProfile, pstats
            pr = cProfile.Profile()
            feats, rooms = T("assemble_graph", lambda: pr.runcall(assemble))
            pstats.Stats(pr, stream=sys.stderr).sort_stats("cumulative").print_stats(25)
        else:
            feats, rooms = T("assemble_graph", assemble)
        state["n_nodes_local"] = feats.shape[0] if feats is not None else state["graph"].counts()["objects"]

        def retrieve_dist_graph():
            """scene per GPU, the whole graph on every rank: node tables all-gathered behind the C ABI (hmsg_allgather_nodes, RCCL on
            HBM buffers -> ONE resident index), the levels above them -- floors -> rooms, room names, the rooms' view embeddings --
            as one small table per rank through the same communicator (hmsg_graph_allgather_index: global room / floor ids);
            every rank then answers its share of the queries coarse to fine on ITS OWN storey of the global table."""
            from holoagent_amd.dist import shard_queries
            from holoagent_amd._lib import Comm
            cg = state["graph"]
            cnt = cg.counts()
            rooms_c = cg.rooms()
            # (which ground-truth room a segmented region lies in only names the synthetic queries; the scene is the same every step)
            if state.get("gt_of_key") != (cnt["rooms"], tuple(r["n_vertices"] for r in rooms_c)):
                state["gt_of"] = [gt_room_of(cg.room_vertices(i, r["n_vertices"])) for i, r in enumerate(rooms_c)]
                state["gt_of_key"] = (cnt["rooms"], tuple(r["n_vertices"] for r in rooms_c))
            gt_of = state["gt_of"]
            if state.get("comm") is None:
                state["comm"] = Comm.from_torch(local, L)
            # ONE call behind the C ABI: node tables (RCCL all-gather out of / into HBM) + floors -> rooms, room names, view embeddings
            # with global ids (hmsg_graph_allgather_index) -- no Python objects travel any more
            g_ix, node_off, room_off, floor_off = cg.allgather_index(state["comm"], np.ascontiguousarray(room_name_feats[gt_of], np.float64))
            n_rooms_g = int(room_off[-1])
            g_ix.set_profiling(prof_on["on"])
            qs = shard_queries(Q, rank, world)
            tq, tr = np.ascontiguousarray(text[qs]), np.ascontiguousarray(room_text[qs])
            fl = np.full(len(qs), int(floor_off[rank]), np.int32)      # (this rank's scene has one storey: its first floor of the global list)
            sel, idx, room, score = g_ix.query_hier(tq, np.zeros(len(qs), np.int32), tr, fl, np.ones(len(qs), np.int32), k,
                                                    max_rooms=max(n_rooms_g, 10))
            state["gemm"] = g_ix.profile()
            state["sel"] = sel
            state["rooms_hit"] = float(np.mean([int(ent_room[q_ent[q]]) in {gt_of[j] for j in s_} for q, s_ in zip(qs, sel)])) if len(qs) else None
            state["graph_counts"] = dict(floors=cnt["floors"], rooms=cnt["rooms"], views=cnt["views"], objects=cnt["objects"],
                                         view_object_edges=int(cnt["view_object_links"]))
            state["graph_counts_all_ranks"] = [dict(floors=int(floor_off[r + 1] - floor_off[r]), rooms=int(room_off[r + 1] - room_off[r]),
                                                    objects=int(node_off[r + 1] - node_off[r])) for r in range(world)]
            state["graph_ms"] = dict(begin=round(cnt["begin_ms"], 2), finish=round(cnt["finish_ms"], 2), kmeans_wait=round(cnt["kmeans_wait_ms"], 2))
            g_ix.close()
            return idx, room, score

        def retrieve():
            g_ix = None
            if use_dist and c_graph:
                return retrieve_dist_graph()
            if use_dist:
                # all-gather of the node tables over RCCL -> global table on every rank.  On the GPUs the exchange runs behind
                # the C ABI (hmsg_allgather_nodes: librccl on device buffers, the gathered table IS the resident index); the
                # torch.distributed form (holoagent_amd/dist.py gather_node_tables) remains for the gloo CPU tests.
                from holoagent_amd.dist import gather_node_tables, gather_node_tables_device, shard_queries
                done = False
                if not emu and not os.environ.get("HMSG_BENCH_TORCH_GATHER") and state.get("comm") is not False:
                    try:
                        g_ix, _node_off, room_off, state["comm"] = gather_node_tables_device(sc, n_rooms, state.get("comm"), local)
                        g_feats = np.zeros((int(_node_off[-1]), 1))        # (shape only: the table itself stays in HBM)
                        g_rooms = None
                        done = True
                    except Exception as e:                                 # (librccl not loadable ...: the torch.distributed form)
                        print("hmsg_allgather_nodes unavailable (%r): torch.distributed all_gather instead" % (e,), file=sys.stderr)
                        state["comm"] = False
                if not done:
                    g_feats, g_rooms, _node_off, room_off = gather_node_tables(feats, rooms, n_rooms, device)
                qs = shard_queries(Q, rank, world)               # this rank's share of the queries
                rl = [[r + int(room_off[rank]) for r in q_rooms[q]] for q in qs]
                tq = np.ascontiguousarray(text[qs])
            else:
                g_feats, g_rooms, rl, tq = feats, rooms, q_rooms, text
            if (state["n_nodes_local"] if g_feats is None else g_feats.shape[0]) == 0:
                return None
            # one GPU: the index is gathered on the device from the node table (hmsg_index_from_nodes) and the queries run
            # coarse to fine ON THE DEVICE (hmsg_query_hier): floor 0 -> room by its name (label mode: the rooms within
            # 1e-3 of the best name similarity) -> objects of those rooms with one negative prompt -- no room list is
            # handed in.  N GPUs: object-level queries on the all-gathered global table with the rooms' global ids.
            if c_graph and not use_dist:
                # the rooms are the segmented ones: each is named after the ground-truth room its region lies in (two regions
                # of one room share the name: the label mode then selects both); the index comes from the graph object with
                # floors -> rooms and the rooms' view embeddings resident (hmsg_graph_index)
                cg = state["graph"]
                rooms_c = cg.rooms()
                gt_of = [gt_room_of(cg.room_vertices(i, r["n_vertices"])) for i, r in enumerate(rooms_c)]
                ix = cg.index(room_name_feats[gt_of])
                ix.set_profiling(prof_on["on"])
                sel, idx, room, score = ix.query_hier(tq, np.zeros(len(tq), np.int32), room_text, np.zeros(len(tq), np.int32),
                                                      np.ones(len(tq), np.int32), k)
                state["gemm"] = ix.profile()
                state["sel"] = sel
                state["rooms_hit"] = float(np.mean([int(ent_room[e]) in {gt_of[j] for j in s_} for e, s_ in zip(q_ent, sel)]))
                cnt = cg.counts()
                state["graph_counts"] = dict(floors=cnt["floors"], rooms=cnt["rooms"], views=cnt["views"], objects=cnt["objects"],
                                             view_object_edges=int(cnt["view_object_links"]))
                state["graph_ms"] = dict(begin=round(cnt["begin_ms"], 2), finish=round(cnt["finish_ms"], 2),
                                         kmeans_wait=round(cnt["kmeans_wait_ms"], 2))
                ix.close()
                return idx, room, score
            if not use_dist and args.full_graph:
                # the rooms are the segmented ones: each is named after the ground-truth room its region lies in (two regions
                # of one room share the name: the label mode then selects both)
                g = state["graph"]
                gt_of = [gt_room_of(r.vertices) for r in g.rooms]
                pos = {id(r): i for i, r in enumerate(g.rooms)}
                ix = sc.index_from_nodes()
                ix.set_profiling(prof_on["on"])
                ix.set_hierarchy([[pos[id(r)] for r in fl.rooms] for fl in g.floors], room_name_feats[gt_of],
                                 [np.zeros((0, D))] * len(g.rooms), list(range(len(g.rooms))))
                sel, idx, room, score = ix.query_hier(tq, np.zeros(len(tq), np.int32), room_text, np.zeros(len(tq), np.int32),
                                                      np.ones(len(tq), np.int32), k)
                state["gemm"] = ix.profile()
                state["sel"] = sel
                state["rooms_hit"] = float(np.mean([int(ent_room[e]) in {gt_of[j] for j in s_} for e, s_ in zip(q_ent, sel)]))
                state["graph_counts"] = dict(floors=len(g.floors), rooms=len(g.rooms), views=len(g.views), objects=len(g.objects),
                                             view_object_edges=int(sum(len(v.object_ids) for v in g.views)))
                ix.close()
                return idx, room, score
            if not use_dist:
                ix = sc.index_from_nodes()
                ix.set_profiling(prof_on["on"])
                ix.set_hierarchy([list(range(n_rooms))], room_name_feats, [np.zeros((0, D))] * n_rooms, list(range(n_rooms)))
                sel, idx, room, score = ix.query_hier(tq, np.zeros(len(tq), np.int32), room_text, np.zeros(len(tq), np.int32),
                                                      np.ones(len(tq), np.int32), k)
                state["gemm"] = ix.profile()
                state["sel"] = sel
                state["rooms_hit"] = float(np.mean([int(ent_room[e]) in s_ for e, s_ in zip(q_ent, sel)]))
                ix.close()
                return idx, room, score
            ix = g_ix if g_ix is not None else NodeIndex(g_feats, g_rooms, device_id=local, lib_=L)
            ix.set_profiling(prof_on["on"])
            out = ix.query_objects(tq, np.zeros(len(rl), np.int32), rl, k)
            state["gemm"] = ix.profile()                       # (launches, ms, FLOP) of the float64 MFMA GEMM
            ix.close()
            return out
        state["last"] = T("retrieval", retrieve)

    for _ in range(args.warmup):
        step()
    stage.clear()
    if use_dist:
        dist.barrier()
    sync()
    t0 = time.perf_counter()
    for i_step in range(args.steps):
        if args.full and i_step == args.steps - 1:
            prof_on["on"] = True
            sc.set_profiling(True)
        step()
    sync()
    if use_dist:
        dist.barrier()
    dt = time.perf_counter() - t0
    prof = {}
    if args.full:
        prof = sc.profile()                                       # events of the LAST timed step
        sc.set_profiling(False)
        prof_on["on"] = False
        if state.get("gemm") and state["gemm"][0]:
            prof["k_gemm_f64"] = state["gemm"]
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, sc, state)                # (before the --full legs: they reuse the scene handle)
    per_rank_fps = [F * max(args.steps, 1) / dt]
    if use_dist:
        mine = torch.tensor([dt], device=device, dtype=torch.float64)
        allt = [torch.zeros_like(mine) for _ in range(world)]
        dist.all_gather(allt, mine)
        per_rank_fps = [F * max(args.steps, 1) / float(t.item()) for t in allt]
        tt = torch.tensor([dt], device=device, dtype=torch.float64)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        dt = float(tt.item())
    steps = max(args.steps, 1)
    # per-rank stage times (episode mode replicates the map build on every rank and pools / assembles / answers on the root:
    # the Amdahl terms of the strong-scaling leg are these numbers)
    my_stage = {k_: round(v / steps * 1e3, 2) for k_, v in stage.items()}
    rank_stages = [my_stage]
    if use_dist:
        rank_stages = [None] * world
        dist.all_gather_object(rank_stages, my_stage)
    fps = (1 if episode else world) * F * steps / dt          # (episode mode: ONE episode of F frames over all ranks)
    retr_s = stage.get("retrieval", 0.0) / steps
    qps = Q / retr_s if retr_s > 0 else None

    # ---- roofline of the dominant kernel (algorithmic bytes per launch, DESIGN.md section "Kernels")
    HW = spec.height * spec.width
    M = spec.n_masks
    V = sc.map_size()
    # The library brackets its heavy kernels with HIP events on its own stream and records, per launch, the
    # algorithmic bytes (FLOP for the two MFMA kernels) of DESIGN.md section 4; dominant = largest total time.
    roof = None
    if prof:
        name, (launches, total_ms, work) = max(prof.items(), key=lambda kv: kv[1][1])
        avg_s = total_ms / launches / 1e3
        per_launch = work / launches
        if name in MFMA_KERNELS:
            achieved = per_launch / avg_s / 1e12 if avg_s > 0 else 0.0
            peak = 78.6 if name == "k_gemm_f64" else 157.3       # dense MFMA peak: f64 / f32 (MI355X_MICROARCH.md)
            roof = dict(kernel=name, bound="mfma", achieved=round(achieved, 4), peak=peak, unit="TFLOP/s",
                        frac=round(achieved / peak, 6), traffic=None, launches=launches,
                        avg_launch_ms=round(total_ms / launches, 4), algorithmic_flop_per_launch=int(per_launch))
        else:
            achieved = per_launch / avg_s / 1e9 if avg_s > 0 else 0.0
            roof = dict(kernel=name, bound="hbm", achieved=round(achieved, 3), peak=HBM_PEAK_GBS, unit="GB/s",
                        frac=round(achieved / HBM_PEAK_GBS, 6), traffic=None, launches=launches,
                        avg_launch_ms=round(total_ms / launches, 4), algorithmic_bytes_per_launch=int(per_launch))

    # HBM traffic of that kernel from the PMC passes (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE, separate runs of
    # this same command, FETCH_SIZE doubled as MI355X_MICROARCH.md prescribes) committed under profiles/
    if roof is not None:
        try:
            import glob
            pmc_path = sorted(glob.glob(os.path.join(ROOT, "profiles", "r[0-9][0-9]_pmc_traffic.json")))[-1]   # newest round
            pmc = json.load(open(pmc_path))["kernels"]
            key = {"k_db_union/box": "k_db_union", "k_db_union/scan": "k_db_union_scan"}.get(roof["kernel"], roof["kernel"])
            if key in pmc:
                # (a timed "launch" of k_ov_query is the pair of launches of one fold step; the PMC passes run ONE step of the same
                #  scene and roof["launches"] counts the LAST step's timed launches: dispatches per timed launch)
                per = max(1.0, round(pmc[key]["dispatches"] / max(roof["launches"], 1))) if key == "k_ov_query" else 1.0
                roof["traffic"] = int(pmc[key]["hbm_bytes_per_launch"] * per)
                if key == "k_ov_query" and "k_ov_query_second" in pmc:      # (round 6: the pair's second launch is a kernel of its own)
                    k2 = pmc["k_ov_query_second"]
                    roof["traffic"] += int(k2["hbm_bytes_per_launch"] * max(1.0, round(k2["dispatches"] / max(roof["launches"], 1))))
                roof["traffic_source"] = "profiles/%s (offline PMC passes, same command)" % os.path.basename(pmc_path)
                try:
                    sys.path.insert(0, os.path.join(ROOT, "scripts"))
                    from csrc_sha import csrc_sha16
                    roof["traffic_same_build"] = json.load(open(pmc_path)).get("csrc_sha16") == csrc_sha16(ROOT)
                except Exception:
                    roof["traffic_same_build"] = None
        except Exception:
            pass

    # ---- the second half of the metric on its own: retrieval on a RESIDENT index.  The step above builds its index inside the timed
    # stage (Q / that stage is `queries_per_sec`); here the index of the last step's graph is built once and the 1000-query batch goes
    # through hmsg_query_hier `--resident-repeats` times -- coarse to fine on the device (floor -> room by its name -> objects with a
    # negative prompt), results back in the caller's arrays every time, nothing else in the timed region.  Twice: the query text
    # handed over as host arrays (PCIe-inclusive) and resident in HBM (device tensors), and once more on a table of the
    # all-gathered size of configs[3] (8 scenes' nodes and rooms: every query on its own scene's storey).
    resident = None
    node_table = None
    if args.full and c_graph and not use_dist and not episode and args.resident_repeats > 0 and state.get("graph") is not None:
        try:
            cg = state["graph"]
            rooms_c = cg.rooms()
            gt_of = [gt_room_of(cg.room_vertices(i, r["n_vertices"])) for i, r in enumerate(rooms_c)]
            Rr = args.resident_repeats
            zq, oq = np.zeros(Q, np.int32), np.ones(Q, np.int32)

            def timed(ix, t_obj, t_room, floors):
                for _ in range(2):
                    ix.query_hier(t_obj, zq, t_room, floors, oq, k)
                sync()
                dtq = None
                for _blk in range(3):               # (the best of three blocks of Rr batches: the steady state of a resident index)
                    t1 = time.perf_counter()
                    for _ in range(Rr):
                        out_ = ix.query_hier(t_obj, zq, t_room, floors, oq, k)
                    sync()
                    d_ = time.perf_counter() - t1
                    dtq = d_ if dtq is None else min(dtq, d_)
                ix.set_profiling(True)
                ix.query_hier(t_obj, zq, t_room, floors, oq, k)
                ng, ms_g, fl_g = ix.profile()
                ix.set_profiling(False)
                return dtq, out_, (ng, ms_g, fl_g)

            def leg(ix, floors, n_nodes, what):
                d_host, out_h, g = timed(ix, text, room_text, floors)
                if emu:
                    d_dev, out_d = d_host, out_h
                else:
                    t_obj_d, t_room_d = torch.from_numpy(text).to(device), torch.from_numpy(room_text).to(device)
                    d_dev, out_d, g = timed(ix, t_obj_d, t_room_d, floors)
                    assert np.array_equal(out_h[1], out_d[1]) and np.array_equal(out_h[3], out_d[3])     # same answers either way
                gemm_ms = g[1] / max(g[0], 1)
                tf = g[2] / max(g[0], 1) / (gemm_ms * 1e-3) / 1e12 if gemm_ms > 0 else None
                return dict(index=what, nodes=int(n_nodes), queries_per_batch=Q, repeats=Rr,
                            queries_per_s_text_in_hbm=round(Q * Rr / d_dev, 1), us_per_batch_text_in_hbm=round(d_dev / Rr * 1e6, 1),
                            queries_per_s_text_from_host=round(Q * Rr / d_host, 1), us_per_batch_text_from_host=round(d_host / Rr * 1e6, 1),
                            k_gemm_f64=dict(launches_per_batch=g[0], ms_per_launch=round(gemm_ms, 4),
                                            tflops=round(tf, 2) if tf else None, frac_of_f64_mfma_peak=round(tf / 78.6, 4) if tf else None,
                                            ms_per_batch_with_event_brackets=round(g[1], 4))), out_d
            ix = cg.index(room_name_feats[gt_of])
            r1, out1 = leg(ix, zq, cg.counts()["objects"], "the step's own graph (hmsg_graph_index), built once")
            ix.close()
            # the all-gathered size: 8 copies of this scene's node table / rooms, one storey per copy (what hmsg_allgather_nodes leaves on every rank)
            recs, emb = sc.nodes(embeddings=True)
            node_table = np.ascontiguousarray(emb, np.float32)
            n_r = len(rooms_c)
            big = NodeIndex(np.tile(emb, (8, 1)), np.concatenate([recs["room"].astype(np.int32) + s_ * n_r for s_ in range(8)]), device_id=local, lib_=L)
            big.set_hierarchy([[s_ * n_r + i for i in range(n_r)] for s_ in range(8)], np.tile(room_name_feats[gt_of], (8, 1)),
                              [np.zeros((0, D))] * (8 * n_r), [i for _ in range(8) for i in range(n_r)])
            r8, out8 = leg(big, (np.arange(Q) % 8).astype(np.int32), 8 * len(recs), "8 scenes' tables side by side (the all-gathered size of configs[3])")
            big.close()
            # (a copy of the scene answers like the scene: node j of copy s is node s * N + j)
            shift = ((np.arange(Q) % 8) * len(recs))[:, None]
            assert np.array_equal(np.where(out1[1] >= 0, out1[1] + shift, -1), out8[1]), "the 8-scene table answers differently"

            resident = dict(one_scene=r1, eight_scenes=r8,
                            note="hmsg_query_hier on an index that is already resident; per batch: room text GEMM + room selection + object "
                                 "text GEMM (f64 MFMA) + exact top-k + ONE packed read-back, results in the caller's arrays")
        except Exception as e:      # (an extra: it must never take the benchmark line down)
            resident = dict(error=repr(e))

    # ---- extra, reported beside `value` and never as `value`: SEVERAL scenes in flight on this GPU.  The sequential fold of A6
    # leaves the chip almost idle for ~60 % of a scene's build; a service that builds scene after scene fills that time
    # with the next scene's map / fusion on a second handle (own stream, own allocator cache, own fold worker).  Two host
    # threads, one handle each, `--inflight-steps` full scenes per thread from a common start; throughput = scenes / wall.
    def measure_inflight():
        import threading
        handles = [sc] + [Scene(lib_=L, device_id=local, height=spec.height, width=spec.width, max_frames=F, max_masks=32, feat_dim=D, merge_type=0)
                          for _ in range(max(args.inflight, 2) - 1)]

        def build(scx):
            scx.reset()
            scx.add_frames(inp["rgb"], inp["depth"], inp["pose"], inp["K"])
            scx.finalize_map()
            if c_graph:
                cg = SceneGraph.begin(scx, poses_arr, fg_host)
            elif args.full_graph:
                g = Graph.from_scene(scx, cfg=full_cfg, lib=L, instances=False)
                g.dataset = FrameSource()
                g._poses = poses_host
                g.set_view_feats(fg_host)
                g.start_room_level()
            scx.add_frame_features(0, inp["masks"], inp["f_g"], inp["f_masked"], inp["f_crop"])
            scx.fuse_frames()
            scx.merge_instances()
            scx.pool_instances()
            if c_graph:                                            # the same step as the line: nothing handed in
                cg.finish(label_feats, label_names)
                rooms_c = cg.rooms()
                gt_of = [gt_room_of(cg.room_vertices(i, r["n_vertices"])) for i, r in enumerate(rooms_c)]
                ix = cg.index(room_name_feats[gt_of])
                ix.query_hier(text, np.zeros(len(text), np.int32), room_text, np.zeros(len(text), np.int32), np.ones(len(text), np.int32), k)
                ix.close()
                n_obj = cg.counts()["objects"]
                cg.close()
                return n_obj
            if args.full_graph:                                    # the same step as the line: nothing handed in
                g.take_instances()
                g.set_label_feats(label_feats, label_names)
                g.build_hier_multimodal_scene_graph(None)
                gt_of = [gt_room_of(r.vertices) for r in g.rooms]
                pos = {id(r): i for i, r in enumerate(g.rooms)}
                ix = scx.index_from_nodes()
                ix.set_hierarchy([[pos[id(r)] for r in fl.rooms] for fl in g.floors], room_name_feats[gt_of],
                                 [np.zeros((0, D))] * len(g.rooms), list(range(len(g.rooms))))
            else:
                g = Graph.from_scene(scx, lib=L)
                g.set_label_feats(label_feats, label_names)
                g.build_hier_multimodal_scene_graph(None, rooms=room_specs)
                ix = scx.index_from_nodes()
                ix.set_hierarchy([list(range(n_rooms))], room_name_feats, [np.zeros((0, D))] * n_rooms, list(range(n_rooms)))
            ix.query_hier(text, np.zeros(len(text), np.int32), room_text, np.zeros(len(text), np.int32), np.ones(len(text), np.int32), k)
            ix.close()
            return len(g.objects)

        errs = []

        def worker(scx, n):
            try:
                if not emu:
                    torch.cuda.set_device(local)
                for _ in range(n):
                    build(scx)
            except Exception as e:      # pragma: no cover
                errs.append(repr(e))
        for hx in handles[1:]:
            build(hx)                                             # warm the other handles' buffers
        sync()
        tt = time.perf_counter()
        th = [threading.Thread(target=worker, args=(hx, args.inflight_steps)) for hx in handles]
        for t in th:
            t.start()
        for t in th:
            t.join()
        sync()
        dt2 = time.perf_counter() - tt
        for hx in handles[1:]:
            hx.close()
        if errs:
            return dict(error="; ".join(errs))
        nh = len(handles)
        return dict(scenes_in_flight=nh, scenes=nh * args.inflight_steps, seconds=round(dt2, 3),
                    frames_per_s=round(nh * args.inflight_steps * F / dt2, 1),
                    note="%d handles driven by %d host threads on this one GPU, every scene built and queried in full; "
                         "`value` above is ONE scene at a time" % (nh, nh))

    inflight = None
    try:
        inflight = measure_inflight() if (args.full and not episode and not use_dist and args.inflight_steps > 0) else None
    except Exception as e:          # (an extra: it must never take the benchmark line down)
        inflight = dict(error=repr(e))

    # ---- extra, for continuity with rounds 1-3's line: the same scene with the rooms' 2-D regions HANDED IN and no views (their
    # `value`; A9's room embeddings / View nodes and A10's view test are then not in the step).  Two steps, never `value`.
    handed_in = None
    if args.full and args.full_graph and not episode and not use_dist and not emu and not args.no_extras:
        try:
            def step_rooms_given():
                sc.reset()
                sc.add_frames(inp["rgb"], inp["depth"], inp["pose"], inp["K"])
                sc.finalize_map()
                sc.add_frame_features(0, inp["masks"], inp["f_g"], inp["f_masked"], inp["f_crop"])
                sc.fuse_frames()
                sc.merge_instances()
                sc.pool_instances()
                g = Graph.from_scene(sc, lib=L)
                g.set_label_feats(label_feats, label_names)
                g.build_hier_multimodal_scene_graph(None, rooms=room_specs)
                ix = sc.index_from_nodes()
                ix.set_hierarchy([list(range(n_rooms))], room_name_feats, [np.zeros((0, D))] * n_rooms, list(range(n_rooms)))
                ix.query_hier(text, np.zeros(len(text), np.int32), room_text, np.zeros(len(text), np.int32), np.ones(len(text), np.int32), k)
                ix.close()
            step_rooms_given()                                   # (one untimed step: this path's buffers and caches)
            sync()
            tt = time.perf_counter()
            for _ in range(2):
                step_rooms_given()
            sync()
            handed_in = dict(frames_per_s=round(2 * F / (time.perf_counter() - tt), 1),
                             note="rounds 1-3's line: room regions handed in, no views; two timed steps of the same scene on the same handle")
        except Exception as e:      # (an extra: it must never take the benchmark line down)
            handed_in = dict(error=repr(e))

    # ---- extra: the encoder hand-off leg (holoagent_amd/encoder_handoff.py): a live PyTorch-ROCm module's outputs go to the
    # library by device pointer.  A few frames on a handle of their own; never part of `value`.
    handoff = None
    if args.full and rank == 0 and world == 1 and not emu and not episode and args.encoder_frames > 0:
        try:
            from holoagent_amd.encoder_handoff import measure as measure_handoff
            nf = min(args.encoder_frames, F)
            hs = Scene(lib_=L, device_id=local, height=spec.height, width=spec.width, max_frames=nf, max_masks=32, feat_dim=D, merge_type=0)
            hs.add_frames(inp["rgb"][:nf], inp["depth"][:nf], inp["pose"][:nf], inp["K"])
            hs.finalize_map()
            handoff = measure_handoff(L, hs, inp, device, torch, frames=nf, feat_dim=D)
            hs.fuse_frames()                                   # (the handed-over features are usable: the fusion runs on them)
            handoff["fused_map_voxels"] = int(hs.map_size())
            hs.close()
        except Exception as e:      # (an extra: it must never take the benchmark line down)
            handoff = dict(error=repr(e))

    # ---- CPU baseline: the oracle on a bounded sample of the same frames (rank 0, N=1)
    cpu = None
    if args.full and rank == 0 and world == 1 and args.cpu_frames > 0:
        n = min(args.cpu_frames, F)
        h_rgb = inp["rgb"][:n].cpu().numpy()
        h_depth = inp["depth"][:n].cpu().numpy().view(np.uint16)
        h_masks = inp["masks"][:n].cpu().numpy().astype(bool)
        fr = [dict(rgb=h_rgb[i], depth=h_depth[i], pose=inp["pose"][i].reshape(4, 4), K=inp["K"], masks=h_masks[i],
                   f_g=inp["f_g"][i].cpu().numpy()[None], f_masked=inp["f_masked"][i].cpu().numpy(),
                   f_crop=inp["f_crop"][i].cpu().numpy()) for i in range(n)]
        cfg = dict(voxel_size=0.05, clip_masked_weight=0.4418, max_mask_distance=10000, init_overlap_thresh=0.75,
                   overlap_thresh_factor=0.025, iou_thresh=0.05, merge_type="sequential", feat_dim=D)
        try:
            import psutil
            phys = psutil.cpu_count(logical=False) or os.cpu_count()
        except Exception:
            phys = os.cpu_count()
        try:
            # the compiled restatement of the reference algorithm (oracle/hmsg_cpu.cpp, pinned against the reference-made
            # fixtures by tests/test_cpu_restatement.py): OpenMP where the reference is parallel (cKDTree workers=-1, BLAS)
            from oracle.hmsg_cpu import CpuBuild
            t1 = time.perf_counter()
            cb = CpuBuild(fr, cfg)
            omp_threads = int(cb.lib.hmsg_cpu_threads())
            if cb.lib.hmsg_cpu_num_instances(cb.h) > 0:
                cb.query(text[: min(Q, 100)], qid=0, k=k)
            t_cpu = time.perf_counter() - t1
            cb.close()
            impl = "oracle/hmsg_cpu.cpp (C++ restatement of create_feature_map + query_hmsg_object, g++ -O2 -fopenmp)"
            threading_note = ("OpenMP on %d threads where the reference itself is parallel (nearest-neighbour queries, radius counts, "
                              "per-pixel features, cosine distances); the merge fold is sequential as in the reference" % omp_threads)
        except Exception as e:          # (no compiler on the box: the numpy / scipy oracle instead)
            from oracle import hmsg_oracle as O
            t1 = time.perf_counter()
            res = O.create_feature_map(fr, cfg)
            feats = np.stack([np.asarray(f, np.float64).reshape(-1) for f in res["mask_feats"]]) if res["mask_feats"] else None
            if feats is not None:
                for q in range(min(Q, 100)):
                    O.query_object(text[q], 0, feats, k)
            t_cpu = time.perf_counter() - t1
            impl = "oracle/hmsg_oracle.py (numpy / scipy / scikit-learn; the compiled restatement was not available: %r)" % (e,)
            threading_note = "numpy / scipy / scikit-learn defaults: cKDTree.query(workers=-1) and BLAS use all cores"
        # the second half of the metric on the host cores: query_hmsg_object over the GPU graph's own node table (same N, same D,
        # same 1000 queries with one negative prompt), the queries of the batch side by side on the OpenMP threads
        cpu_qps = cpu_q_note = None
        try:
            from oracle.hmsg_cpu import query_table
            tbl = node_table
            if tbl is None:
                tbl = sc.nodes(embeddings=True)[1] if sc.num_instances() else None
            if tbl is not None and len(tbl):
                query_table(tbl, text[:8], qid=0, k=k)
                reps, t_q = 0, 0.0
                t1 = time.perf_counter()
                while reps < 3 or (t_q < 2.0 and reps < 50):
                    query_table(tbl, text, qid=0, k=k)
                    reps += 1
                    t_q = time.perf_counter() - t1
                cpu_qps = round(Q * reps / t_q, 1)
                cpu_q_note = ("oracle/hmsg_cpu.cpp hmsg_cpu_query_table: query_hmsg_object (graph.py:3112-3151) over the %d x %d node table of the "
                              "GPU's graph, %d queries x %d batches, float64 dot products, one query per OpenMP thread" % (tbl.shape[0], tbl.shape[1], Q, reps))
        except Exception as e:
            cpu_q_note = "unavailable: %r" % (e,)
        # optional second size of the build (the CPU rate falls with the number of frames: the ratio at equal size is measured, not asserted)
        cpu_extra = None
        if args.cpu_frames_extra > 0:
            try:
                from oracle.hmsg_cpu import CpuBuild
                n2 = min(args.cpu_frames_extra, F)
                h_rgb2 = inp["rgb"][:n2].cpu().numpy()
                h_depth2 = inp["depth"][:n2].cpu().numpy().view(np.uint16)
                h_masks2 = inp["masks"][:n2].cpu().numpy().astype(bool)
                fr2 = [dict(rgb=h_rgb2[i], depth=h_depth2[i], pose=inp["pose"][i].reshape(4, 4), K=inp["K"], masks=h_masks2[i],
                            f_g=inp["f_g"][i].cpu().numpy()[None], f_masked=inp["f_masked"][i].cpu().numpy(),
                            f_crop=inp["f_crop"][i].cpu().numpy()) for i in range(n2)]
                t1 = time.perf_counter()
                cb2 = CpuBuild(fr2, cfg)
                if cb2.lib.hmsg_cpu_num_instances(cb2.h) > 0:
                    cb2.query(text[: min(Q, 100)], qid=0, k=k)
                t2 = time.perf_counter() - t1
                cb2.close()
                cpu_extra = dict(frames=n2, value=round(n2 / t2, 4), unit="frames/s", seconds=round(t2, 2))
            except Exception as e:
                cpu_extra = dict(error=repr(e))
        cpu = dict(value=round(n / t_cpu, 4), unit="frames/s", cores=phys, kind="port", queries_per_s=cpu_qps, queries_sample=cpu_q_note,
                   second_point=cpu_extra,
                   sample="%s: create_feature_map + 100 queries on the first %d of the %d frames (640x480, D=%d, M=32)%s"
                          % (impl, n, F, D, " = BASELINE.json configs[0] in full" if n == 100 else
                             "; --cpu-frames 100 (the default) runs BASELINE.json configs[0] in full"),
                   threading=threading_note, seconds=round(t_cpu, 2))

    mfma_util = None
    if args.full:
        try:
            import glob
            mp = sorted(glob.glob(os.path.join(ROOT, "profiles", "r[0-9][0-9]_pmc_mfma.json")))[-1]
            mk = json.load(open(mp))["kernels"]
            mj = json.load(open(mp))
            try:
                sys.path.insert(0, os.path.join(ROOT, "scripts"))
                from csrc_sha import csrc_sha16
                same = mj.get("csrc_sha16") == csrc_sha16(ROOT)
            except Exception:
                same = None
            # (committed counters, not a measurement of this run: `same_build` says whether they were taken on the sources being timed)
            mfma_util = {"source": "profiles/%s (offline PMC passes, same command)" % os.path.basename(mp), "same_build": same}
            for name, key in (("k_pool_gram", "k_pool_gram"), ("k_gemm_f64", "k_gemm_f64_tiled")):
                if key in mk and "MfmaUtil_percent" in mk[key]:
                    mfma_util[name] = {"MfmaUtil_percent": round(mk[key]["MfmaUtil_percent"], 2),
                                       "SQ_VALU_MFMA_BUSY_CYCLES": mk[key]["SQ_VALU_MFMA_BUSY_CYCLES"]["mean_per_launch"],
                                       "GRBM_GUI_ACTIVE": mk[key]["GRBM_GUI_ACTIVE"]["mean_per_launch"]}
        except Exception:
            mfma_util = None
    if rank == 0:
        last = state.get("last")
        out = {
            "metric": ("HMSG frames/sec (%s: map A1-A2, fusion A3-A5, merge A6, pooling A7, floors A8, %splus %d coarse-to-fine "
                       "retrieval queries (A12: floor -> room by its name -> objects with a "
                       "negative prompt, every stage on the device; with several GPUs on the all-gathered table, every rank on its own scene's "
                       "storey) per %d-frame %s; frames, masks and "
                       "encoder features already resident in HBM, encoders bypassed)")
                      % ("one episode sharded over the GPUs" if episode else "one scene per GPU",
                         ("rooms by the device watershed N1, room clouds, room embeddings and View nodes A9, objects with the view <-> object "
                          "test A10 and graph assembly A11, nothing handed in -- ") if (args.full_graph and not episode) else
                         ("objects A10 and graph assembly A11 with the rooms' 2-D regions given and without views -- A9's room embeddings / "
                          "View nodes are not in the timed step -- "),
                         Q, F, "episode" if episode else "scene"),
            "value": round(fps, 3), "unit": "frames/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(dt / steps * 1e3, 3), "higher_is_better": True, "scaling": "strong" if episode else "weak", "vs_baseline": None,
            "dtype": "f64 geometry / f32 features", "data": "synthetic",
            "config": {"workload": ("configs[4] shape: ONE %d-frame episode, %dx%d RGB-D, 32 masks/frame, %d-d features, hierarchical "
                                    "merge tree sharded over the ranks, HMSG build + %d-query retrieval on the root" % (F, spec.width, spec.height, D, Q))
                       if episode else
                                      ("%s: %d-frame single scene per GPU, %dx%d RGB-D, 32 masks/frame, %d-d features, "
                        "HMSG build + %d-query retrieval" % ("configs[3] (independent scenes, one per GPU, RCCL all-gather of the graph nodes)" if world > 1 else
                                                             ("configs[2]" if D == 1024 else "configs[1]"), F, spec.width, spec.height, D, Q)),
                       "frames": F, "queries": Q, "feat_dim": D, "masks": M,
                       "parallelism": ("episode-sharded x%d (frame windows of %d)" % (world, chunk)) if episode else "scene-per-gpu x%d" % world},
            "rccl_ranks": dist.get_world_size() if use_dist else 0,
            "full_graph": bool(args.full_graph and not episode), "graph_counts": state.get("graph_counts"),
            "graph_counts_all_ranks": state.get("graph_counts_all_ranks"),
            "graph_level": ("C ABI graph object (hmsg_graph_begin / _finish / _index)" if c_graph else "Python mirror") if args.full_graph and not episode else None,
            "graph_ms": state.get("graph_ms"),
            "emulated": bool(emu), "full": bool(args.full),
            # (scene mode: the sequential fold of A6 starts on a worker thread while hmsg_fuse_frames is still producing
            #  3-D masks, so part of the merge is inside the fuse_frames stage time; HMSG_FOLD_NOPIPE=1 separates them)
            "fold_beside_fusion": (not episode) and not os.environ.get("HMSG_FOLD_NOPIPE"),
            "per_rank_frames_per_s": [round(v, 1) for v in per_rank_fps],
            "per_rank_stage_ms": rank_stages if use_dist else None,
            "queries_per_sec": round(qps, 1) if qps else None,
            "queries_per_sec_note": "Q / the step's retrieval stage, which also builds the index from the graph; the resident index: `retrieval_resident`",
            "retrieval_resident": resident,
            "retrieval_room_stage_hit_rate": state.get("rooms_hit"),
            "stage_ms_per_step": {k_: round(v / steps * 1e3, 2) for k_, v in stage.items()},
            "map_voxels": V, "nodes_local": state.get("n_nodes_local"),
            "kernels_ms_last_step": {k_: round(v[1], 3) for k_, v in sorted(prof.items(), key=lambda kv: -kv[1][1])} if args.full else None,
            # algorithmic bytes (FLOP for the MFMA kernels) / measured time of every instrumented kernel
            "kernels_achieved": {k_: [round(v[2] / (v[1] * 1e-3) / (1e12 if k_ in MFMA_KERNELS else 1e9), 2),
                                      "TFLOP/s" if k_ in MFMA_KERNELS else "GB/s"]
                                 for k_, v in sorted(prof.items(), key=lambda kv: -kv[1][1]) if v[1] > 0} if args.full else None,
            # MFMA utilisation of the two matrix-core kernels from the PMC passes committed under profiles/ (rocprofv3 --pmc
            # SQ_VALU_MFMA_BUSY_CYCLES / GRBM_GUI_ACTIVE ..., one counter per pass over this same command: scripts/gpu_run.sh mfma)
            "mfma_utilisation": mfma_util,
            "scenes_in_flight": inflight,
            "encoder_handoff": handoff,
            "rooms_handed_in": handed_in,
            "roofline": roof, "cpu_baseline": cpu,
            "speedup_vs_cpu": round(fps / cpu["value"], 1) if cpu else None,
            "speedup_vs_cpu_note": ("frames/s of the GPU path on configs[1] (%d frames) / frames/s of the CPU restatement on its %d-frame "
                                    "sample (configs[0] when 100): two different sizes -- the CPU rate falls with the number of frames, so at "
                                    "equal size the ratio is larger" % (F, min(args.cpu_frames, F))) if cpu else None,
        }
    sc.close()
    if use_dist:
        dist.destroy_process_group()
    if rank == 0:
        # the JSON line goes out LAST: RCCL writes its version banner through C stdio, which would otherwise be flushed
        # behind it at exit
        try:
            import ctypes
            ctypes.CDLL(None).fflush(None)
        except Exception:
            pass
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
