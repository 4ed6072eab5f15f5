"""The view level of the slow path on the graph object (include/hmsg.h: hmsg_graph_get_views, _get_view_objects, _find_view,
_object_best_views, _goal_views, _rematch_in_views, _object_view_depths) against numpy restatements of
Graph.query_room_obj_slow_reasoning's steps (fsr_vln/memory/hmsg/graph/graph.py:2759-2765 best view, :2864-2897 goal images,
:2962-2986 re-match, :3011-3022 + utils/graph_utils.py:49-70 / :95-157 the two distances), every case on a BUILT graph and on the
same graph after hmsg_save -> hmsg_load.

The scene is the two-storey one of tests/test_scene_graph_cabi.py, with one change to the pose table the GRAPH is given: the cameras
of frames FAR stand 30 m back along their optical axes, so their views see every object of their room beyond max_view_depth.  That
gives the four properties the cases need, asserted on the built and on the loaded graph: >= 2 rooms on >= 1 floor, a view with >= 2
objects, a view with none (a FAR view), an object without a best view (one that only the FAR frames saw).  A third graph, loaded from
a copy of the saved directory in which one best_view_id names no view and one is null, covers the id that hmsg_load cannot resolve.
Seed 7 of the text rows: numpy alone excuses no rank (no two neighbouring scores within 1e-9; asserted for every k)."""
import json
import os
import shutil

import numpy as np
import pytest

from tests import parity_common as PC
from tests.test_query_views import ref_avg_distance, ref_check_object_in_view
from tests.test_scene_graph_cabi import _build, _rest


def ref_goal_views(T64, rooms_list, k):
    """graph.py:2864-2897 for one text row: rooms_list = [(global room, sample_images, clip_embeddings)]"""
    ids, rooms, embs = [], [], []
    for r, img_ids, e in rooms_list:
        assert len(img_ids) == len(e)                                       # :2870
        ids.extend(img_ids)
        rooms.extend([r] * len(img_ids))
        embs.extend(e)
    if not ids:
        return [], [], np.zeros(0), None
    sims = np.dot(T64, np.stack(embs).astype(np.float64).T)                 # :2888-2892
    top_k = min(k, sims.shape[0])                                           # :2896
    top = np.argsort(sims)[-top_k:][::-1]                                   # :2897
    return [ids[i] for i in top], [rooms[i] for i in top], sims[top], ids[int(np.argmax(sims))]


FAR = (4, 5)


def check_views(L, device, tmp_path, storeys=2, merge=False):
    import holoagent_amd.graph as G
    from holoagent_amd._lib import HmsgError, SceneGraph
    spec, inp, sc = _build(L, device, storeys)
    F, D = spec.n_frames, spec.feat_dim
    poses = np.array(np.asarray(inp["pose"], np.float64).reshape(F, 4, 4))
    for i in FAR:
        poses[i, :3, 3] -= poses[i, :3, 2] * 30.0
    inv = np.stack([np.linalg.inv(p) for p in poses])
    K = np.asarray(inp["K"], np.float64).reshape(3, 3)
    wh = [spec.width, spec.height]
    fg = inp["f_g"].cpu().numpy()
    paths = ["img/%05d.png" % i for i in range(F)]
    cg = SceneGraph.begin(sc, poses, fg, poses_inv=inv, img_paths=paths, num_views=5, host_threads=2, merge_objects_graph=1 if merge else 0)
    # an unfinished graph: every call of the group refuses, and a listing call made now leaves nothing behind that is stale later
    for call in (lambda: cg.goal_views(np.zeros((1, D), np.float32), [-1]), cg.views, lambda: cg.view_objects(0, n=1), lambda: cg.find_view(img_id=0),
                 lambda: cg.find_view(img_path=paths[0]), lambda: cg.object_best_views([0]), lambda: cg.rematch_in_views(np.zeros((1, D), np.float32), [0]),
                 lambda: cg.object_view_depths([0], inv[:1], wh, K)):
        with pytest.raises(HmsgError):
            call()
    assert L.c.hmsg_graph_get_views(cg.g, None, 0) != 0
    _rest(sc, inp)
    lf = np.ones((1, D), np.float32) / np.sqrt(D)
    cg.finish(lf if merge else None, ["thing"] if merge else None)
    clouds = sc.instances()
    cg.save(tmp_path / "c")
    lg = SceneGraph.load(tmp_path / "c", lib_=L)
    # the saved directory with the edges the scene lacks
    shutil.copytree(tmp_path / "c", tmp_path / "e")
    d0 = cg.to_dict()
    full = max(d0["views"], key=lambda v: len(v["object_ids"]))
    vpath = tmp_path / "e" / "views" / (full["view_id"] + ".json")
    m = json.load(open(vpath))
    m["object_ids"], m["text_discription"] = [], []
    json.dump(m, open(vpath, "w"))
    o_null, o_dangling = [o["object_id"] for o in d0["objects"] if o["best_view_id"] is not None][:2]
    for oid, val in ((o_null, None), (o_dangling, "9_9_9")):
        opath = tmp_path / "e" / "objects" / (oid + ".json")
        m = json.load(open(opath))
        m["best_view_id"] = val
        json.dump(m, open(opath, "w"))
    eg = SceneGraph.load(tmp_path / "e", lib_=L)

    rng = np.random.default_rng(7)
    Q = 4
    T = rng.standard_normal((Q, D)).astype(np.float32)
    T /= np.linalg.norm(T, axis=1, keepdims=True)
    T64 = T.astype(np.float64)
    emb_of = {f[:-5]: np.array(json.load(open(tmp_path / "c" / "objects" / f))["embedding"], np.float64)
              for f in os.listdir(tmp_path / "c" / "objects") if f.endswith(".json")}
    # an object's cloud: what hmsg_save wrote (byte for byte the mirror's file, tests/test_scene_graph_cabi.py) -- after
    # merge_objects_graph the concatenated parts; without it also the instance cloud of the scene
    cloud_of = {f[:-4]: np.asarray(G._read_ply(str(tmp_path / "c" / "objects" / f)), np.float64).reshape(-1, 3)
                for f in os.listdir(tmp_path / "c" / "objects") if f.endswith(".ply")}
    if not merge:
        for o in cg.objects():
            assert np.array_equal(cloud_of[o["object_id"]], np.asarray(clouds[o["instance"]], np.float64))
    else:
        assert len(cg.objects()) < len(sc.nodes()), "no pair of objects was merged"
    results = {}
    for tag, g in (("built", cg), ("loaded", lg), ("edited", eg)):
        d = g.to_dict()
        objs, views, rooms = g.objects(), g.views(), g.rooms()
        nV, nO = len(d["views"]), len(d["objects"])
        first_obj = {}
        for k, o in enumerate(d["objects"]):
            first_obj.setdefault(o["object_id"], k)
        first_view = {}
        for k, v in enumerate(d["views"]):
            first_view.setdefault(v["view_id"], k)
        room_of = {r["room_id"]: k for k, r in enumerate(d["rooms"])}
        # ---- lists, lookups, best views = what hmsg_graph_to_json says
        assert [v["view"] for v in views] == list(range(nV))
        lists = []
        for k, v in enumerate(d["views"]):
            want = [first_obj[i] for i in v["object_ids"] if i in first_obj]                 # :2968-2973
            lists.append(want)
            assert views[k]["n_objects"] == len(want) and g.view_objects(k).tolist() == want
            assert views[k]["img_id"] == (v["img_id"] if v["img_id"] is not None else -1)
            rid = v["room_id"] if isinstance(v["room_id"], str) else d["floors"][int(v["view_id"].split("_")[0])]["rooms"][v["room_id"]]
            assert views[k]["room"] == room_of[rid]
            assert g.find_view(img_path=v["img_path"]) == next(j for j, w in enumerate(d["views"]) if w["img_path"] == v["img_path"])   # :2566-2570
            assert g.find_view(img_id=v["img_id"]) == next(j for j, w in enumerate(d["views"]) if w["img_id"] == v["img_id"])
        assert g.find_view(img_path="no/such.png") == -1 and g.find_view(img_id=10 ** 9) == -1
        bv, bimg = g.object_best_views(np.arange(nO))
        for k, o in enumerate(d["objects"]):
            want = first_view.get(o["best_view_id"], -1) if o["best_view_id"] is not None else -1     # :2759-2765
            assert bv[k] == want and objs[k]["best_view"] == want, (tag, k)
            assert bimg[k] == (d["views"][want]["img_id"] if want >= 0 else -1)                       # :2830
        # ---- the properties the fixture must keep
        assert len(d["rooms"]) >= 2 and len(d["floors"]) >= 1
        assert any(len(l) >= 2 for l in lists)
        assert any(len(l) == 0 for l in lists)
        assert (bv == -1).any() and (bv >= 0).any()
        assert any(o["best_view_id"] is None for o in d["objects"])
        if tag == "edited":
            assert bv[first_obj[o_null]] == -1 and bv[first_obj[o_dangling]] == -1
        # ---- goal views
        table = {k: (k, r["sample_images"], [fg[i] for i in r["sample_images"]]) for k, r in enumerate(d["rooms"])}
        n_img = sum(len(r["sample_images"]) for r in d["rooms"])
        assert n_img >= 5
        floors = [-1] + list(range(len(d["floors"])))
        excused = 0
        for kk in (1, 24, n_img + 3):
            for f in floors:
                fl = np.full(Q, f, np.int32)
                img, room, score, n = g.goal_views(T, fl, k=kk)
                order = list(range(len(d["rooms"]))) if f == -1 else [room_of[r] for r in d["floors"][f]["rooms"]]
                for q in range(Q):
                    ids, rms, sims, best = ref_goal_views(T64[q], [table[r] for r in order], kk)
                    assert n[q] == len(ids)
                    assert (img[q, n[q]:] == -1).all() and (room[q, n[q]:] == -1).all()
                    np.testing.assert_allclose(score[q, : n[q]], sims, rtol=0, atol=1e-12)
                    if len(ids):
                        assert img[q, 0] == best                                                      # np.argmax, :2893
                    for j in range(len(ids)):
                        near = (j > 0 and abs(sims[j - 1] - sims[j]) <= 1e-9) or (j + 1 < len(ids) and abs(sims[j] - sims[j + 1]) <= 1e-9)
                        if near:
                            excused += 1
                            continue
                        assert img[q, j] == ids[j] and room[q, j] == rms[j], (tag, kk, f, q, j)
        assert excused == 0, "the text seed gives near-ties in numpy alone: choose another"
        if tag == "built" and not merge:
            # the mirror's rank_goal_views gives the same images (graph.py of this package; it takes room objects)
            class R:
                pass
            mg = G.Graph(dict(main=dict(), models=dict(clip=dict(feat_dim=D))), lib=L)
            mg.get_text_feats_multiple_templates = lambda words: np.stack([T[int(w)] for w in words])
            rl = []
            for k, r in enumerate(d["rooms"]):
                o = R()
                o.sample_images, o.clip_embeddings = r["sample_images"], [fg[i] for i in r["sample_images"]]
                rl.append(o)
            img, _, _, n = g.goal_views(T, np.full(Q, -1, np.int32), k=24)
            for q in range(Q):
                best, top, _ = mg.rank_goal_views(str(q), rl, top_k=24)
                assert best == img[q, 0] and top == img[q, : n[q]].tolist()
        # ---- re-match of every view for 3 queries, with the distance of the chosen object in that view's camera
        E = np.stack([emb_of[o["object_id"]] for o in d["objects"]])
        vq = np.repeat(np.arange(nV), 3).astype(np.int32)
        Tq = np.ascontiguousarray(np.tile(T[:3], (nV, 1)))
        cams = np.stack([inv[v["img_id"]] for v in d["views"]])[vq]
        obj, score, dist = g.rematch_in_views(Tq, vq, pose_inv=cams, wh=wh, K=K)
        obj2, score2, none = g.rematch_in_views(Tq, vq)
        assert none is None and np.array_equal(obj, obj2) and np.array_equal(score, score2)
        for i, v in enumerate(vq):
            l = lists[v]
            if not l:
                assert obj[i] == -1 and np.isnan(dist[i])                                             # :2974 skips
                continue
            sims = np.dot(T64[i % 3], E[l].T)                                                         # :2977-2979
            j = int(np.argmax(sims))                                                                  # :2980
            top2 = np.sort(sims)[-2:]
            if len(l) == 1 or top2[1] - top2[0] > 1e-9:
                assert obj[i] == l[j], (tag, i)
            assert abs(score[i] - sims[j]) <= 1e-12
            if True:
                want = ref_avg_distance(cloud_of[d["objects"][obj[i]]["object_id"]], cams[i])         # :2994-2996
                assert np.isnan(dist[i]) == np.isnan(want)
                if not np.isnan(want):
                    np.testing.assert_allclose(dist[i], want, rtol=1e-13, atol=0)
        assert 0 <= obj.max() < nO
        # ---- check_object_in_view(return_depth=True) of every object in its own best view (:3011-3022)
        have = np.nonzero(bv >= 0)[0]
        vis, md = g.object_view_depths(have, np.stack([inv[d["views"][bv[k]]["img_id"]] for k in have]), wh, K)
        if True:
            for i, k in enumerate(have):
                rv, rd = ref_check_object_in_view(wh[0], wh[1], K, inv[d["views"][bv[k]]["img_id"]], cloud_of[d["objects"][k]["object_id"]])
                assert bool(vis[i]) == bool(rv) and np.isfinite(md[i]) == np.isfinite(rd)
                if np.isfinite(rd):
                    np.testing.assert_allclose(md[i], rd, rtol=1e-13, atol=0)
            assert vis.any()
        results[tag] = dict(match={(d["views"][v]["view_id"], i % 3): (d["objects"][obj[i]]["object_id"] if obj[i] >= 0 else None, score[i], dist[i])
                                   for i, v in enumerate(vq)}, goal=g.goal_views(T, np.full(Q, -1, np.int32), k=24))
        # ---- errors
        with pytest.raises(HmsgError):
            g.rematch_in_views(T[:1], [nV])
        with pytest.raises(HmsgError):
            g.rematch_in_views(T[:1], [-1])
        with pytest.raises(HmsgError):
            g.object_view_depths([nO], inv[:1], wh, K)
        with pytest.raises(HmsgError):
            g.goal_views(T[:1], [len(d["floors"])])
        with pytest.raises(HmsgError):
            g.view_objects(nV, n=1)
    # ---- built and loaded agree (by id: the loader sorts views and objects by file name): objects, scores, distances, goal images
    b, l = results["built"], results["loaded"]
    assert sorted(b["match"]) == sorted(l["match"])
    for key, (oid, sc_b, dist_b) in b["match"].items():
        assert l["match"][key][0] == oid, key
        assert abs(l["match"][key][1] - sc_b) <= 1e-12
        np.testing.assert_allclose(l["match"][key][2], dist_b, rtol=1e-13, atol=0, equal_nan=True)
    assert np.array_equal(b["goal"][0], l["goal"][0]) and np.array_equal(b["goal"][3], l["goal"][3])
    np.testing.assert_allclose(b["goal"][2], l["goal"][2], rtol=0, atol=1e-12)
    # ---- a room whose sample_images and clip_embeddings differ in length (:2870)
    shutil.copytree(tmp_path / "c", tmp_path / "bad")
    rid = d0["rooms"][0]["room_id"]
    m = json.load(open(tmp_path / "bad" / "rooms" / (rid + ".json")))
    m["sample_images"] = m["sample_images"][:-1]
    json.dump(m, open(tmp_path / "bad" / "rooms" / (rid + ".json"), "w"))
    bg = SceneGraph.load(tmp_path / "bad", lib_=L)
    with pytest.raises(HmsgError, match=rid):
        bg.goal_views(T[:1], [-1])
    for g in (bg, eg, lg, cg):
        g.close()
    sc.close()


_emu = pytest.mark.skipif(not os.path.exists(PC.EMU_PATH), reason="kernel simulator not built")
_slow = pytest.mark.skipif(not os.environ.get("HMSG_EMU_SLOW"), reason="minutes on the kernel simulator (HMSG_EMU_SLOW=1); its twin runs on the MI355X")


@_emu
def test_view_calls_refuse_an_unfinished_graph_on_the_simulator():
    """hmsg_graph_begin without hmsg_graph_finish: no view exists yet, and every call of the group says so"""
    import torch
    from holoagent_amd._lib import HmsgError, HmsgLib, SceneGraph
    L = HmsgLib(PC.EMU_PATH)
    spec, inp, sc = _build(L, torch.device("cpu"))
    F, D = spec.n_frames, spec.feat_dim
    poses = np.asarray(inp["pose"], np.float64).reshape(F, 4, 4)
    cg = SceneGraph.begin(sc, poses, inp["f_g"].cpu().numpy(), num_views=5, host_threads=2)
    K = np.asarray(inp["K"], np.float64).reshape(3, 3)
    for call in (cg.views, lambda: cg.view_objects(0, n=1), lambda: cg.find_view(img_id=0), lambda: cg.find_view(img_path="img/00000.png"),
                 lambda: cg.object_best_views([0]), lambda: cg.goal_views(np.zeros((1, D), np.float32), [-1]),
                 lambda: cg.rematch_in_views(np.zeros((1, D), np.float32), [0]), lambda: cg.object_view_depths([0], np.eye(4)[None], [96, 72], K)):
        with pytest.raises(HmsgError, match="hmsg_graph_finish"):
            call()
    assert L.c.hmsg_graph_get_views(cg.g, None, 0) != 0
    cg.close()
    sc.close()


@_slow
@_emu
def test_graph_views_two_storeys_on_the_simulator(tmp_path):
    import torch
    from holoagent_amd._lib import HmsgLib
    check_views(HmsgLib(PC.EMU_PATH), torch.device("cpu"), tmp_path)


@pytest.mark.gpu
def test_graph_views_two_storeys_gpu(tmp_path):
    import torch
    from holoagent_amd._lib import HmsgLib
    check_views(HmsgLib(), torch.device("cuda", 0), tmp_path)


@_slow
@_emu
def test_graph_views_after_merge_objects_on_the_simulator(tmp_path):
    """merge_objects_graph: re-match returns indices into hmsg_graph_get_objects' (merged) list, the cloud is the concatenated parts"""
    import torch
    from holoagent_amd._lib import HmsgLib
    check_views(HmsgLib(PC.EMU_PATH), torch.device("cpu"), tmp_path, merge=True)


@pytest.mark.gpu
def test_graph_views_after_merge_objects_gpu(tmp_path):
    import torch
    from holoagent_amd._lib import HmsgLib
    check_views(HmsgLib(), torch.device("cuda", 0), tmp_path, merge=True)
