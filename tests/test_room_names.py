"""Room names on the device (include/hmsg.h: hmsg_denoise_feats_batch, hmsg_graph_name_rooms, hmsg_graph_set_room_names;
holoagent_amd/csrc/hmsg_roomnames.hip) and the mirror's Graph.generate_room_names(generate_method="obj_embedding"):

  * against tests/golden/roomnames_obj.npz (scripts/gen_golden_room_names.py: the reference's own generate_room_names, sklearn's DBSCAN):
    representatives bit for bit in float32 and float64, names, the view-embedding names, the label-mode room and object answers;
  * the graph object on a small synthetic scene: a built graph named and saved, a saved graph loaded, named and queried in label mode,
    both against the mirror;
  * a room without objects fails the whole call and renames nothing;
  * -m gpu: the same, and one large batch (~10^4 objects, 60 rooms, D = 512) against a float64 numpy / sklearn restatement."""
import json
import os

import numpy as np
import pytest

from tests import parity_common as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "roomnames_obj.npz")
needs_emu = pytest.mark.skipif(not os.path.exists(PC.EMU_PATH), reason="kernel simulator not built")


def _sets(z, key):
    off = z["room_off"]
    return [z[key][off[k]:off[k + 1]] for k in range(len(off) - 1)]


def _mirror(L, z, dt):
    """the mirror's Graph holding the fixture's rooms (objects in dtype dt, views float64) and its text table"""
    from holoagent_amd.graph import Floor, Graph, Object, Room
    D = z["emb64"].shape[1]
    g = Graph(dict(main=dict(), models=dict(clip=dict(feat_dim=D))), lib=L)
    table = {str(w): v for w, v in zip(z["words"], z["table"])}
    g.get_text_feats_multiple_templates = lambda words: np.stack([table[w] for w in words]).astype(np.float32)
    fl = Floor("0", name="floor_0")
    fl.floor_zero_level = 0.0
    g.floors, g.rooms, g.objects = [fl], [], []
    voff = z["view_off"]
    for r, objs in enumerate(_sets(z, "emb64")):
        room = Room("0_%d" % r, "0", name="room%d" % r)
        room.embeddings = [v for v in z["view64"][voff[r]:voff[r + 1]]]
        for i, e in enumerate(objs.astype(dt)):
            o = Object("0_%d_%d" % (r, i), room.room_id, name="thing")
            o.embedding = e
            room.add_object(o)
            g.objects.append(o)
        g.rooms.append(room)
        fl.rooms.append(room)
    g._index = None
    return g


def check_fixture(L):
    from holoagent_amd._lib import denoise_feats_batch
    z = np.load(GOLD)
    T, types = z["type_feats"], [str(t) for t in z["types"]]
    for tag, dt in (("64", np.float64), ("32", np.float32)):
        rep, ncl = denoise_feats_batch(_sets(z, "emb" + tag), lib_=L)
        assert rep.dtype == dt and np.array_equal(rep, z["ref_rep" + tag]), tag
        assert ncl[0] == 0 and ncl[3] == 0                                  # all noise; a single object
        assert [types[int(np.argmax(r @ T.T))] for r in rep] == [str(n) for n in z["ref_names" + tag]], tag
        g = _mirror(L, z, dt)
        g.generate_room_names(generate_method="obj_embedding", default_room_types=types)
        assert [r.name for r in g.rooms] == [str(n) for n in z["ref_names" + tag]], tag
        if tag == "64":
            for q in range(len(z["ref_label_rooms"])):
                room_q, obj_q = types[q % 3], "thing%d" % q
                rl = g.query_hmsg_room(room_q, floor_id=-1, query_method="label")
                want = [int(v) for v in z["ref_label_rooms"][q] if v >= 0]
                assert rl == want, q
                oi, ri, sc = g.query_hmsg_object(obj_q, floor_id=-1, room_ids=rl, top_k=5, negative_prompt=["background"])
                n = len(oi)
                assert oi == [int(v) for v in z["ref_obj_idx"][q][:n]] and (n == 5 or z["ref_obj_idx"][q][n] < 0), q
                assert ri == [int(v) for v in z["ref_obj_room"][q][:n]], q
                np.testing.assert_allclose(sc, z["ref_obj_score"][q][:n], rtol=0, atol=1e-12)
                # the batched driver path (label mode on the device from the names' text features)
                (sel, idx, room, score), = g.query_hierarchy_batch([(-1, room_q, obj_q, ["background"])], top_k=5)
                assert list(sel) == want and idx == oi and room == ri, q
            g.generate_room_names(generate_method="view_embedding", default_room_types=types)
            assert [r.name for r in g.rooms] == [str(n) for n in z["ref_view_names"]]
    assert z["ref_names64"][6] != z["ref_view_names"][6]                  # the two methods disagree on room 6


def check_empty_room(L):
    from holoagent_amd._lib import HmsgError, denoise_feats_batch
    z = np.load(GOLD)
    with pytest.raises(HmsgError, match="set 1 is empty"):
        denoise_feats_batch([z["emb64"][:3], np.zeros((0, 32)), z["emb64"][3:5]], lib_=L)
    g = _mirror(L, z, np.float64)
    g.rooms[2].objects = []
    with pytest.raises(HmsgError):
        g.generate_room_names(generate_method="obj_embedding", default_room_types=[str(t) for t in z["types"]])
    assert [r.name for r in g.rooms] == ["room%d" % r for r in range(len(g.rooms))]       # all or nothing
    with pytest.raises(NotImplementedError, match="LLM"):
        g.rooms[0].infer_room_type_from_objects("label", [str(t) for t in z["types"]])


def check_graph_object(L, device, tmp_path):
    """the synthetic scene of tests/test_scene_graph_cabi.py: build + save, then name the built graph and a loaded copy"""
    from holoagent_amd._lib import SceneGraph
    from holoagent_amd.graph import Graph
    from tests.test_scene_graph_cabi import _build, _rest
    spec, inp, sc = _build(L, device)
    F, D = spec.n_frames, spec.feat_dim
    poses = np.stack([np.asarray(inp["pose"][i], np.float64).reshape(4, 4) for i in range(F)])
    rng = np.random.Generator(np.random.PCG64(77))
    label_feats = rng.standard_normal((4, D)).astype(np.float32)
    label_feats /= np.linalg.norm(label_feats, axis=1, keepdims=True)
    cg = SceneGraph.begin(sc, poses, inp["f_g"].cpu().numpy(), poses_inv=np.linalg.inv(poses), num_views=5, host_threads=2)
    _rest(sc, inp)
    cg.finish(label_feats, ["a", "b", "c", "d"])
    cg.save(tmp_path / "c")
    types = ["Pantry", "Office", "Office-Pantry", "Kitchen"]
    T = rng.standard_normal((len(types), D)).astype(np.float32)
    T /= np.linalg.norm(T, axis=1, keepdims=True)
    words = {t: T[i] for i, t in enumerate(types)}
    for i in range(6):
        v = rng.standard_normal(D).astype(np.float32)
        words["q%d" % i] = v / np.linalg.norm(v)
    words["background"] = T[0] * 0.5 + words["q0"] * 0.5

    def mirror(f32):
        g = Graph(dict(main=dict(), models=dict(clip=dict(feat_dim=D))), lib=L)
        g.load_hmsg_graph(str(tmp_path / "c"))
        g.get_text_feats_multiple_templates = lambda ws: np.stack([words[w] for w in ws]).astype(np.float32)
        if f32:                                        # the built graph's float32 pooled features (saved as float32 text)
            for o in g.objects:
                o.embedding = np.asarray(o.embedding, np.float32)
        g.generate_room_names(generate_method="obj_embedding", default_room_types=types)
        return g
    # ---- built: name, save; the saved names are the mirror's, every other byte is unchanged
    want = mirror(True)
    t_built = cg.name_rooms("obj_embedding", T, types)
    assert [types[t] for t in t_built] == [r.name for r in want.rooms]
    assert [r["name"] for r in cg.rooms()] == [r.name for r in want.rooms]
    assert [r["name"] for r in cg.to_dict()["rooms"]] == [r.name for r in want.rooms]
    cg.save(tmp_path / "c2")
    (tmp_path / "py").mkdir()
    for r in want.rooms:
        r.save(str(tmp_path / "py"), lib=L)
        got = json.load(open(tmp_path / "c2" / "rooms" / (r.room_id + ".json")))
        assert got["name"] == json.load(open(tmp_path / "py" / (r.room_id + ".json")))["name"] == r.name
        before = json.load(open(tmp_path / "c" / "rooms" / (r.room_id + ".json")))
        before["name"] = r.name
        assert got == before
    # ---- loaded (float64): name, then a label-mode query with room_name_emb formed from the types
    g64 = mirror(False)
    lg = SceneGraph.load(tmp_path / "c", lib_=L)
    t_loaded = lg.name_rooms("obj_embedding", T, types)
    assert [types[t] for t in t_loaded] == [r.name for r in g64.rooms]
    names_emb = np.ascontiguousarray(T[t_loaded].astype(np.float64))
    Q = 6
    qs = [(-1, types[q % len(types)], "q%d" % q, ["background"]) for q in range(Q)]
    ref = g64.query_hierarchy_batch(qs, top_k=3)
    T_obj = np.stack([np.stack([words["q%d" % q], words["background"]]) for q in range(Q)]).astype(np.float32)
    T_room = np.stack([words[types[q % len(types)]] for q in range(Q)]).astype(np.float32)
    zero = np.zeros(Q, np.int32)
    sel, idx, room, score = lg.query(T_obj, zero, T_room, zero - 1, zero + 1, 3, room_name_emb=names_emb)
    for q in range(Q):
        keep = idx[q] >= 0
        assert sel[q] == list(ref[q][0]) and idx[q][keep].tolist() == ref[q][1], q
        np.testing.assert_array_equal(score[q][keep], ref[q][3])
    # the view vote through the graph object equals the mirror's (loaded: float64 view embeddings)
    g64.generate_room_names(generate_method="view_embedding", default_room_types=types)
    t_view = lg.name_rooms("view_embedding", T, types)
    assert [r["name"] for r in lg.rooms()] == [r.name for r in g64.rooms]
    assert all(t >= 0 for t in t_view)
    # set_room_names, and the all-or-nothing refusal
    lg.set_room_names(["x%d" % i for i in range(len(g64.rooms))])
    assert [r["name"] for r in lg.to_dict()["rooms"]] == ["x%d" % i for i in range(len(g64.rooms))]
    lg.close()
    cg.close()
    sc.close()
    return t_built, t_loaded


@needs_emu
def test_fixture_on_the_simulator():
    from holoagent_amd._lib import HmsgLib
    check_fixture(HmsgLib(PC.EMU_PATH))


@needs_emu
def test_empty_room_on_the_simulator():
    from holoagent_amd._lib import HmsgLib
    check_empty_room(HmsgLib(PC.EMU_PATH))


@needs_emu
def test_graph_object_on_the_simulator(tmp_path):
    import torch
    from holoagent_amd._lib import HmsgLib
    check_graph_object(HmsgLib(PC.EMU_PATH), torch.device("cpu"), tmp_path)


@pytest.mark.gpu
def test_fixture_gpu():
    from holoagent_amd._lib import HmsgLib
    check_fixture(HmsgLib())


@pytest.mark.gpu
def test_empty_room_gpu():
    from holoagent_amd._lib import HmsgLib
    check_empty_room(HmsgLib())


@pytest.mark.gpu
def test_graph_object_gpu(tmp_path):
    import torch
    from holoagent_amd._lib import HmsgLib
    check_graph_object(HmsgLib(), torch.device("cuda", 0), tmp_path)


def _large_batch(D=512, R=60, seed=11):
    """~10^4 objects in 60 rooms (one of 3000 rows: many Gram tiles per side), tight clusters near the types plus outliers; every
    intra-cluster distance is ~0.005 and every other ~1, far from eps = 0.02"""
    rng = np.random.Generator(np.random.PCG64(seed))
    T = rng.standard_normal((3, D)).astype(np.float32)
    T /= np.linalg.norm(T, axis=1, keepdims=True)
    sizes = list(rng.integers(20, 230, R - 1)) + [3000]
    sets = []
    for n in sizes:
        k = max(1, int(n) // 40)
        cen = T[rng.integers(0, 3, k)] + 0.5 * rng.standard_normal((k, D)) / np.sqrt(D)
        cen /= np.linalg.norm(cen, axis=1, keepdims=True)
        lab = rng.integers(0, k + 1, int(n))                  # label k: an outlier
        X = np.where((lab < k)[:, None], cen[np.minimum(lab, k - 1)] + 0.003 * rng.standard_normal((int(n), D)), rng.standard_normal((int(n), D)))
        sets.append(X)
    return sets, T


def _restate(X, eps=0.02, min_samples=2):
    """feats_denoise_dbscan restated: sklearn's DBSCAN, Counter.most_common, np.mean"""
    from collections import Counter
    from sklearn.cluster import DBSCAN
    lab = DBSCAN(eps=eps, min_samples=min_samples, metric="cosine").fit(X).labels_
    c = Counter(lab)
    c.pop(-1, None)
    if not c:
        return np.mean(X, axis=0)
    f = X[lab == c.most_common(1)[0][0]]
    return np.mean(f, axis=0) if len(f) > 1 else f[0]


@pytest.mark.gpu
def test_large_batch_gpu():
    from holoagent_amd._lib import HmsgLib, denoise_feats_batch
    L = HmsgLib()
    sets, T = _large_batch()
    assert 9000 <= sum(len(s) for s in sets) <= 13000
    try:
        import sklearn  # noqa: F401
        have_sklearn = True
    except Exception:
        have_sklearn = False
    for dt in (np.float64, np.float32):
        rows = [s.astype(dt) for s in sets]
        rep, ncl = denoise_feats_batch(rows, lib_=L)
        assert rep.dtype == dt and np.isfinite(rep).all() and (ncl > 0).all()
        if not have_sklearn:
            continue
        for k, X in enumerate(rows):
            want = _restate(X)
            if dt == np.float64:
                np.testing.assert_allclose(rep[k], want, rtol=0, atol=1e-12)
            else:
                np.testing.assert_allclose(rep[k], want, rtol=0, atol=1e-6)
            s_got, s_want = rep[k].astype(np.float64) @ T.T.astype(np.float64), want.astype(np.float64) @ T.T.astype(np.float64)
            assert int(np.argmax(s_got)) == int(np.argmax(s_want)), k
