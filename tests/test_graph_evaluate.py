"""hmsg_graph_evaluate (include/hmsg.h): the reference's evaluate_floors / evaluate_rooms / evaluate_objects of a graph in one call.
Three comparisons, every number the same bits:
  - against the same numbers put together from the library's pieces through the Python binding (eval_floors, Scene.eval_rooms,
    eval_hydra_means, lsap, eval_metrics_from_matrix, Scene.eval_object_matrices, eval_counts_at, Scene.eval_semantic_ranks, eval_top_k --
    each pinned by a test of its own);
  - against what the reference does with the matrices, restated in numpy and scipy alone (tests/eval_reference.py: scipy's
    linear_sum_assignment, the sweep on the OVERLAP matrix under either assignment, entry 6, the recount at 0.5, top-k over every
    assigned pair) -- so the composition inside the call is pinned by something that is not the library;
  - from C (tests/host_c/hmsg_host_eval.c, strict C99 against include/hmsg.h alone: hmsg_load -> hmsg_graph_evaluate).
Graphs: a saved directory written by hand (seconds; object ids whose text order is not the numeric one; embeddings and class table
with cosine gaps above 1e-3, so the ranks also equal the float64 model), and the synthetic scene of tests/test_scene_graph_cabi.py
built through the library, evaluated as built (the pieces in the built graph's own order) and again saved and loaded.

The ground truth is made up from the saved graph itself: its rooms flattened and shifted, one more room that nothing predicts, its
objects jittered plus a spurious one, a 40-class table with one duplicated name, categories in and outside the vocabulary.

Simulator without the gpu mark (the two-storey build only with HMSG_EMU_SLOW=1: minutes); -m gpu: libhmsg.so."""
import glob
import json
import os
import subprocess

import numpy as np
import pytest

from tests import eval_reference as R
from tests import parity_common as PC
from tests import test_eval_rooms as TR
from tests import test_eval_semantics as TS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host_c", "hmsg_host_eval.c")
INC = os.path.join(ROOT, "include")
LIB = os.path.join(ROOT, "holoagent_amd", "libhmsg.so")
TOP_K = [1, 5, 10]


def _compile(lib_path, out):
    cmd = ["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-O1", "-I", INC, SRC, "-o", out, lib_path,
           "-Wl,-rpath," + os.path.dirname(lib_path), "-Wl,-rpath,/opt/rocm/lib", "-Wl,--allow-shlib-undefined"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return out


def saved_graph(L, gdir):
    """the saved directory as load_hmsg_graph orders it -> floors, rooms, objects (lists of dicts with the clouds)"""
    from holoagent_amd._lib import read_ply
    out = []
    for kind in ("floors", "rooms", "objects"):
        items = []
        for ply in sorted(glob.glob(os.path.join(str(gdir), kind, "*.ply")), key=os.path.basename):
            rec = json.load(open(ply[:-4] + ".json"))
            rec["pts"] = read_ply(ply, lib_=L)
            items.append(rec)
        out.append(items)
    return out


def ground_truth(floors, rooms, objects, D):
    rng = np.random.default_rng(41)
    gt = {}
    pm = np.array([r["room_zero_level"] + r["room_height"] / 2 for r in rooms])          # what the reference's gate reads of a predicted room
    fid = [str(r["floor_id"]) for r in rooms]
    lower, upper = [], []
    for i, f in enumerate(floors):
        y = np.asarray(f["vertices"])[:, 1]
        mine = pm[[k for k in range(len(rooms)) if fid[k] == str(f["floor_id"])]]
        lower.append(min(y.min() - (0.8 if i == 0 else 0.2), mine.min() - 0.3 if len(mine) else np.inf))    # the lowest bound off by more than 0.5
        upper.append(max(y.max() + 0.1, mine.max() + 0.3 if len(mine) else -np.inf))
    gt["floor_lower"], gt["floor_upper"] = np.array(lower), np.array(upper)
    clouds, mn, mx, me = [], [], [], []
    for k, r in enumerate(rooms):
        p = np.array(r["pts"])
        bev = p[:: 3].copy() + [0.04, 0.0, -0.03]
        bev[:, 1] = pm[k] - 1.0                                          # the ground-truth room's min_height, where its bev cloud lies
        clouds.append(bev)
        mn.append(pm[k] - 1.0), mx.append(pm[k] + 1.0), me.append(pm[k])
    far = clouds[0] + [40.0, 0.0, 0.0]                                   # a room nothing predicts
    clouds.append(far), mn.append(mn[0]), mx.append(mx[0]), me.append(me[0])
    gt.update(room_clouds=clouds, room_min_h=np.array(mn), room_max_h=np.array(mx), room_mean_h=np.array(me))
    oc, center, dims = [], [], []
    for k, o in enumerate(objects):
        if k % 4 == 3:
            continue                                                     # a predicted object without ground truth
        p = np.array(o["pts"]) + rng.normal(0, 0.004, (len(o["pts"]), 3)) + (0.01 if k % 2 else 0.0)
        oc.append(p)
        center.append((p.min(0) + p.max(0)) / 2), dims.append(p.max(0) - p.min(0) + 0.02)
    spurious = rng.uniform(-0.1, 0.1, (200, 3)) + [25.0, 1.0, 25.0]
    oc.append(spurious), center.append(spurious.mean(0)), dims.append(np.ptp(spurious, axis=0))
    C = 40
    text = rng.standard_normal((C, D)).astype(np.float32)
    names = np.arange(C, dtype=np.int32)
    names[31] = names[7]                                                 # one name on two classes
    # the categories: the class nearest to the matching predicted object's embedding for some, a far one or none for others
    gt.update(obj_clouds=oc, obj_obb_center=np.array(center), obj_obb_dims=np.array(dims),
              obj_name_id=np.array([(-1 if k % 5 == 4 else int(names[rng.integers(0, C)])) for k in range(len(oc))], np.int32),
              text_feats=text, class_name_id=names)
    emb = [np.asarray(o["embedding"], np.float64) for o in objects]
    kept = [k for k in range(len(objects)) if k % 4 != 3]
    for j, k in enumerate(kept[: len(kept) // 2]):
        sim = (text / np.linalg.norm(text, axis=1, keepdims=True)) @ (emb[k] / np.linalg.norm(emb[k]))
        gt["obj_name_id"][j] = int(names[int(np.argsort(sim)[-1 - (j % 3)])])
    return gt


def pm_of(rooms):
    return [(r["room_zero_level"], r["room_height"], r["floor_id"], np.asarray(r["pts"])[:, 1].min(), np.asarray(r["pts"])[:, 1].max()) for r in rooms]


def pieces(L, scene, floors, rooms, objects, gt, eval_metric):
    """the call's numbers put together from the library's pieces, for the predicted rooms / objects in the order given
    -> metrics, the matrices and assignments behind them"""
    from holoagent_amd import _lib as B
    m, x = {}, {}
    m["floors"] = B.eval_floors(gt["floor_lower"], gt["floor_upper"], np.array([f["vertices"] for f in floors]), lib_=L)
    off = np.zeros(len(rooms) + 1, np.int64)
    off[1:] = np.cumsum([len(r["pts"]) for r in rooms])
    goff = np.zeros(len(gt["room_clouds"]) + 1, np.int64)
    goff[1:] = np.cumsum([len(c) for c in gt["room_clouds"]])
    assoc, over_pred, over_gt, _ = scene.eval_rooms(np.concatenate([r["pts"] for r in rooms]), off, [r["room_zero_level"] for r in rooms],
                                                    [r["room_height"] for r in rooms], np.concatenate(gt["room_clouds"]), goff, gt["room_min_h"],
                                                    gt["room_max_h"], gt["room_mean_h"], gt["floor_lower"], gt["floor_upper"])
    hp, hr = B.eval_hydra_means(over_pred, over_gt, lib_=L)
    row, col = B.lsap(assoc, maximize=True, lib_=L)
    ap, acc, prec, rec = B.eval_metrics_from_matrix(assoc, row, col, 6, lib_=L)
    m["rooms"] = {"acc@IoU=0.5": acc, "ap": ap, "prec@IoU=0.5": prec, "recall@IoU=0.5": rec, "gt": len(gt["room_clouds"]), "pred": len(rooms),
                  "hydra_prec": hp, "hydra_recall": hr}
    iou, ov, _ = scene.eval_object_matrices([o["pts"] for o in objects], gt["obj_clouds"], gt["obj_obb_center"], gt["obj_obb_dims"], 0.02)
    row, col = B.lsap(iou if eval_metric == "iou" else ov, maximize=True, lib_=L)
    ap = B.eval_metrics_from_matrix(ov, row, col, 6, lib_=L)[0]
    c = B.eval_counts_at(ov, row, col, 0.5, lib_=L)
    P, G = ov.shape
    emb = np.array([objects[r]["embedding"] for r in row], np.float64)
    rank = scene.eval_semantic_ranks(emb, gt["text_feats"], gt["class_name_id"], gt["obj_name_id"][col])
    tk, auc = B.eval_top_k(rank, len(gt["text_feats"]), TOP_K, lib_=L)
    m["objects"] = dict(instances=dict(ap=ap, gt=G, pred=P),
                        instances_iou50=dict(acc=c["acc"], prec=c["prec"], recall=c["recall"], tp=c["tp"], fp=c["fp"], fn=c["fn"], gt=G, pred=P),
                        ins_semantics=dict(tp_top_k_acc=tk, top_k_auc=auc))
    x.update(assoc=assoc, over_pred=over_pred, over_gt=over_gt, iou=iou, ov=ov, row=row, col=col, rank=rank, emb=emb)
    return m, x


def reference_composition(floors, gt, x, eval_metric, rank):
    """What the reference does with the matrices (hm3dsem_evaluator.py:193-263, :343-399, :460-589), in numpy and scipy alone
    (tests/eval_reference.py): independent of how the library composes its pieces.  The matrices (and, where given, the ranks) are the
    library's, each pinned by a test of its own."""
    from scipy.optimize import linear_sum_assignment
    fl = R.floors(gt["floor_lower"], gt["floor_upper"], [f["vertices"] for f in floors])
    m = {"floors": {k: (float(v) if k in ("acc", "prec", "recall") else int(v)) for k, v in fl.items()}}
    assoc = x["assoc"]
    P, G = assoc.shape
    hp, hr = R.hydra(x["over_pred"], x["over_gt"])
    row, col = linear_sum_assignment(assoc, maximize=True)
    s = R.sweep(assoc, row, col, P, G)
    m["rooms"] = {"acc@IoU=0.5": float(s["acc"][6]), "ap": float(s["ap"]), "prec@IoU=0.5": float(s["prec"][6]), "recall@IoU=0.5": float(s["rec"][6]),
                  "gt": G, "pred": P, "hydra_prec": float(hp), "hydra_recall": float(hr)}
    ov = x["ov"]
    P, G = ov.shape
    row, col = linear_sum_assignment(x["iou"] if eval_metric == "iou" else ov, maximize=True)
    assert np.array_equal(row, x["row"]) and np.array_equal(col, x["col"])
    s = R.sweep(ov, row, col, P, G)
    c = R.counts_at(ov, row, col, P, G, 0.5)
    acc, auc = R.top_k_from_ranks(rank, TOP_K, len(gt["text_feats"]))
    m["objects"] = dict(instances=dict(ap=float(s["ap"]), gt=G, pred=P),
                        instances_iou50=dict(acc=float(c["acc"]), prec=float(c["prec"]), recall=float(c["recall"]), tp=c["tp"], fp=c["fp"], fn=c["fn"],
                                             gt=G, pred=P),
                        ins_semantics=dict(tp_top_k_acc={k: float(v) for k, v in acc.items()}, top_k_auc=float(auc)))
    return m


def flat(m, assigned):
    """the C host's order"""
    f, r, o = m["floors"], m["rooms"], m["objects"]
    i50 = o["instances_iou50"]
    return [f["tp"], f["tn"], f["fp"], f["fn"], f["acc"], f["prec"], f["recall"], r["acc@IoU=0.5"], r["ap"], r["prec@IoU=0.5"], r["recall@IoU=0.5"],
            r["gt"], r["pred"], r["hydra_prec"], r["hydra_recall"], o["instances"]["ap"], o["instances"]["gt"], o["instances"]["pred"], i50["tp"],
            i50["fp"], i50["fn"], i50["acc"], i50["prec"], i50["recall"], o["ins_semantics"]["top_k_auc"], assigned] + [
                o["ins_semantics"]["tp_top_k_acc"][k] for k in TOP_K]


def c_host(lib_path, gdir, gt, D, tmp_path):
    """tests/host_c/hmsg_host_eval.c on the saved directory -> its 26 + len(TOP_K) numbers"""
    pp = np.concatenate(gt["room_clouds"])
    po = np.concatenate(gt["obj_clouds"])
    roff = np.concatenate([[0], np.cumsum([len(c) for c in gt["room_clouds"]])]).astype(np.int64)
    ooff = np.concatenate([[0], np.cumsum([len(c) for c in gt["obj_clouds"]])]).astype(np.int64)
    with open(tmp_path / "gt.bin", "wb") as f:
        np.array([len(gt["floor_lower"]), len(gt["room_clouds"]), len(gt["obj_clouds"]), len(gt["text_feats"]), D, len(TOP_K), 1, 0], np.int32).tofile(f)
        np.array([len(pp), len(po)], np.int64).tofile(f)
        for a, dt in ((gt["floor_lower"], np.float64), (gt["floor_upper"], np.float64), (pp, np.float64), (roff, np.int64),
                      (gt["room_min_h"], np.float64), (gt["room_max_h"], np.float64), (gt["room_mean_h"], np.float64), (po, np.float64),
                      (ooff, np.int64), (gt["obj_obb_center"], np.float64), (gt["obj_obb_dims"], np.float64), (gt["obj_name_id"], np.int32),
                      (gt["text_feats"], np.float32), (gt["class_name_id"], np.int32), (TOP_K, np.int32)):
            np.ascontiguousarray(a, dt).tofile(f)
    exe = _compile(lib_path, str(tmp_path / "hmsg_host_eval"))
    r = subprocess.run([exe, str(gdir), str(tmp_path / "gt.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    return np.fromfile(tmp_path / "out.bin", np.float64).tolist()


def check_loaded(L, lib_path, gdir, gt, D, tmp_path, separated_table=False):
    """a saved directory: hmsg_load -> hmsg_graph_evaluate against the pieces, against the reference's composition in numpy / scipy,
    and from C; the refusals.  -> the metrics per eval_metric"""
    from holoagent_amd._lib import Scene, SceneGraph, HmsgError
    floors, rooms, objects = saved_graph(L, gdir)
    lg = SceneGraph.load(gdir, lib_=L)
    small = Scene(lib_=L, height=8, width=8, max_frames=1, max_masks=1, feat_dim=16)
    out = {}
    for metric in ("overlap", "iou"):
        want, x = pieces(L, small, floors, rooms, objects, gt, metric)
        got = lg.evaluate(gt, eval_metric=metric, top_k=TOP_K)
        assert got == want, (metric, got, want)
        rank = x["rank"]
        if separated_table:               # the ranks from the float64 model as well: the table's cosines are more than 1e-3 apart
            rank = TS.separated(x["emb"], gt["text_feats"], gt["class_name_id"], gt["obj_name_id"][x["col"]])
            assert np.array_equal(rank, x["rank"])
        assert got == reference_composition(floors, gt, x, metric, rank), metric
        # the scene says something: rooms and objects are found, not all of them, the ranks are spread
        assert (x["assoc"] > 0.5).any() and (x["assoc"] == 0).any() and (x["ov"] > 0.5).sum() >= 2 and len(set(x["rank"].tolist())) >= 3, (x, pm_of(rooms))
        assert 0 < want["rooms"]["hydra_recall"] < 1 and want["floors"]["tp"] < len(floors) + 1 and want["objects"]["instances_iou50"]["tp"] >= 2
        assert 0 < want["objects"]["ins_semantics"]["top_k_auc"] < 1
        out[metric] = (want, len(x["row"]))
    assert c_host(lib_path, gdir, gt, D, tmp_path) == [float(v) for v in flat(*out["overlap"])]
    # ---- refusals: unequal floor counts, a class table of another width
    bad = dict(gt)
    bad["floor_lower"], bad["floor_upper"] = np.append(gt["floor_lower"], 9.0), np.append(gt["floor_upper"], 12.0)
    with pytest.raises(HmsgError, match="floors"):
        lg.evaluate(bad, top_k=TOP_K)
    bad = dict(gt)
    bad["text_feats"] = gt["text_feats"][:, :8]
    with pytest.raises(HmsgError, match="feat_dim"):
        lg.evaluate(bad, top_k=TOP_K)
    small.close()
    lg.close()
    return out


def _run(lib_path, device, tmp_path, storeys):
    """a graph built through the library, evaluated as built, saved, and evaluated again as loaded and from C"""
    from holoagent_amd._lib import HmsgLib, Scene, SceneGraph
    from tests.test_scene_graph_cabi import _build, _rest
    L = HmsgLib(lib_path)
    spec, inp, sc = _build(L, device, storeys=storeys)
    F, D = spec.n_frames, spec.feat_dim
    poses = np.stack([np.asarray(inp["pose"][i], np.float64).reshape(4, 4) for i in range(F)])
    cg = SceneGraph.begin(sc, poses, inp["f_g"].cpu().numpy(), poses_inv=np.linalg.inv(poses), num_views=5, host_threads=2)
    _rest(sc, inp)
    cg.finish(None, None)
    gdir = tmp_path / "graph"
    cg.save(gdir)
    floors, rooms, objects = saved_graph(L, gdir)
    assert len(floors) == storeys and len(rooms) >= storeys and len(objects) >= 4
    gt = ground_truth(floors, rooms, objects, D)
    check_loaded(L, lib_path, gdir, gt, D, tmp_path)
    # ---- the built graph: the same records in ITS order (load_hmsg_graph sorts the ids as text), every number again
    by_id = {o["object_id"]: o for o in objects}
    room_by_id = {r["room_id"]: r for r in rooms}
    b_objects = [by_id[o["object_id"]] for o in cg.objects()]
    b_rooms = [room_by_id[r["room_id"]] for r in cg.rooms()]
    assert len(b_objects) == len(objects) and len(b_rooms) == len(rooms)
    small = Scene(lib_=L, height=8, width=8, max_frames=1, max_masks=1, feat_dim=16)
    for metric in ("overlap", "iou"):
        want, x = pieces(L, small, floors, b_rooms, b_objects, gt, metric)
        built = cg.evaluate(gt, eval_metric=metric, top_k=TOP_K)
        assert built == want, (metric, built, want)
        assert built == reference_composition(floors, gt, x, metric, x["rank"])
    small.close()
    cg.close()
    sc.close()


def write_graph_dir(L, gdir, D=16):
    """a saved graph written by hand, as save_hmsg_graph lays it out: two storeys, three rooms, fourteen objects -- eleven of them in
    one room, so that load_hmsg_graph's text order of the ids ("0_0_10" before "0_0_2") is not the numeric one.  The embeddings are
    those of tests/test_eval_semantics.py::table, whose cosines against its class table are more than 1e-3 apart.
    -> the class table (text, names)"""
    from holoagent_amd._lib import write_ply
    rng = np.random.default_rng(77)
    for sub in ("floors", "rooms", "objects", "views"):
        os.makedirs(os.path.join(str(gdir), sub))

    def put(kind, name, rec, pts):
        write_ply(os.path.join(str(gdir), kind, name + ".ply"), np.ascontiguousarray(pts, np.float64), lib_=L)
        json.dump(rec, open(os.path.join(str(gdir), kind, name + ".json"), "w"))

    def corners(lo, hi):
        return [[x, y, z] for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])]
    room_box = {"0_0": (0.0, 4.0, 0.1), "0_1": (4.5, 8.0, 0.15), "1_0": (0.0, 4.0, 3.3)}         # x0, x1, zero level
    n_obj = {"0_0": 11, "0_1": 2, "1_0": 1}
    emb, text, names, _ = TS.table(D, 40, sum(n_obj.values()), seed=23, n_dup_names=1)
    for f, (y0, y1) in enumerate(((0.0, 2.8), (3.2, 6.0))):
        rids = [r for r in room_box if r.startswith("%d_" % f)]
        put("floors", str(f), dict(floor_id=str(f), name="floor_%d" % f, rooms=rids, vertices=corners((0.0, y0, 0.0), (8.0, y1, 3.0)),
                                   floor_height=y1 - y0, floor_zero_level=y0), TR.rect(rng, 500, 0.0, 8.0, 0.0, 3.0, y0, y1))
    k = 0
    for rid, (x0, x1, zero) in room_box.items():
        oids = ["%s_%d" % (rid, i) for i in range(n_obj[rid])]
        put("rooms", rid, dict(room_id=rid, name="room_" + rid, floor_id=rid[0], objects=oids, views=[], vertices=[[x0, 0.0], [x1, 0.0], [x1, 3.0], [x0, 3.0]],
                               room_height=2.6, room_zero_level=zero, embeddings=[], represent_images=[], sample_images=[], clip_embeddings=[]),
            TR.rect(rng, 1500, x0, x1, 0.0, 3.0, zero, zero + 2.6))
        for i, oid in enumerate(oids):
            c = np.array([x0 + 0.3 + 0.33 * i, zero + 0.6, 0.5 + 0.2 * (i % 5)])
            half = rng.uniform(0.08, 0.14, 3)
            p = rng.uniform(c - half, c + half, (300, 3))
            axis, side = rng.integers(0, 3, 300), rng.integers(0, 2, 300)
            p[np.arange(300), axis] = np.where(side == 0, (c - half)[axis], (c + half)[axis])     # on the box's surface
            put("objects", oid, dict(object_id=oid, vertices=corners(p.min(0), p.max(0)), room_id=rid, name="object_" + oid,
                                     embedding=[float(v) for v in emb[k]], view_ids=[], best_view_id=None), p)
            k += 1
    return text, names


def _loaded_only(lib_path, tmp_path):
    from holoagent_amd._lib import HmsgLib
    L = HmsgLib(lib_path)
    gdir, D = tmp_path / "graph", 16
    text, names = write_graph_dir(L, gdir, D)
    floors, rooms, objects = saved_graph(L, gdir)
    assert [o["object_id"] for o in objects][:3] == ["0_0_0", "0_0_1", "0_0_10"]
    gt = ground_truth(floors, rooms, objects, D)
    rng = np.random.default_rng(5)
    gt["text_feats"], gt["class_name_id"] = text, names
    gt["obj_name_id"] = np.array([(-1 if k % 5 == 4 else int(names[rng.integers(0, len(names))])) for k in range(len(gt["obj_clouds"]))], np.int32)
    check_loaded(L, lib_path, gdir, gt, D, tmp_path, separated_table=True)


needs_emu = pytest.mark.skipif(not os.path.exists(PC.EMU_PATH), reason="kernel simulator not built")


@needs_emu
def test_loaded_graph_evaluate_on_the_simulator(tmp_path):
    _loaded_only(PC.EMU_PATH, tmp_path)


@needs_emu
def test_built_graph_evaluate_on_the_simulator(tmp_path):
    import torch
    _run(PC.EMU_PATH, torch.device("cpu"), tmp_path, storeys=1)


@needs_emu
@pytest.mark.skipif(not os.environ.get("HMSG_EMU_SLOW"), reason="an extra: two storeys take minutes on the kernel simulator (HMSG_EMU_SLOW=1); its twin runs on the MI355X")
def test_two_storey_graph_evaluate_on_the_simulator(tmp_path):
    import torch
    _run(PC.EMU_PATH, torch.device("cpu"), tmp_path, storeys=2)


@pytest.mark.gpu
def test_loaded_graph_evaluate_gpu(tmp_path):
    _loaded_only(LIB, tmp_path)


@pytest.mark.gpu
@pytest.mark.parametrize("storeys", [1, 2])
def test_graph_evaluate_gpu(tmp_path, storeys):
    import torch
    _run(LIB, torch.device("cuda", 0), tmp_path, storeys)
