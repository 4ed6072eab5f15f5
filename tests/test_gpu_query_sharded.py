"""The sharded query on the MI355X (include/hmsg.h: hmsg_graphs_query, hmsg_graph_query_sharded): graphs built on the device, one
of them saved and reloaded, queried in place against hmsg_query_hier on ONE index over their concatenated float64 tables, bit for
bit; one real RCCL rank against hmsg_graph_query; and the GEMM-kernel statement the contract rests on (an entry of S has the same
bits from the one-wave kernel and from the tiled one)."""
import json
import os
import signal

import numpy as np
import pytest

from tests import parity_common as PC

pytestmark = pytest.mark.gpu
D = 64


@pytest.fixture(autouse=True)
def _bounded():
    """every case ends within its time (a hang fails the case instead of holding the device)"""
    def boom(*_):
        raise TimeoutError("case over its time")
    old = signal.signal(signal.SIGALRM, boom)
    signal.alarm(240)
    yield
    signal.alarm(0)
    signal.signal(signal.SIGALRM, old)


def _graph(L, seed):
    from holoagent_amd._lib import SceneGraph
    from holoagent_amd.synth import SceneSpec, SynthScene
    spec = SceneSpec(seed=seed, rooms_x=2, rooms_z=1, room_size=(4.0, 2.5, 3.5), objects_per_room=8, width=128, height=96, n_frames=16,
                     n_masks=16, feat_dim=D, yaw_step_deg=25.0)
    scn = SynthScene(spec)
    frames = [scn.frame(i) for i in range(spec.n_frames)]
    S = PC.stack_frames(frames)
    sc = PC.make_scene(L, frames, dict(feat_dim=D, outlier_nb_points=20, outlier_radius=0.3, feat_dbscan_min=8))
    sc.add_frames(S["rgb"], S["depth"], S["pose"], S["K"])
    sc.finalize_map()
    sc.add_frame_features(0, S["masks"], S["f_g"], S["f_masked"], S["f_crop"], S["n_masks"])
    sc.fuse_frames()
    sc.merge_instances()
    sc.pool_instances()
    return sc, SceneGraph.build(sc, S["pose"], S["f_g"], num_views=4, host_threads=4)


def _tables(g, sc=None, directory=None):
    rooms = g.rooms()
    if sc is not None:                          # built: the node table as the index takes it (float32 -> float64)
        nodes, emb = sc.nodes(embeddings=True)
        emb = np.asarray(emb, np.float32).reshape(-1, D).astype(np.float64)
        room = np.array([int(n["room"]) for n in nodes], np.int32)
        views = [np.asarray(g.room_embeddings(i, D), np.float32).reshape(-1, D).astype(np.float64) for i in range(len(rooms))]
    else:                                       # loaded: the saved float64 rows
        objs = g.objects()
        emb = np.asarray([json.load(open(os.path.join(directory, "objects", o["object_id"] + ".json")))["embedding"] for o in objs],
                         np.float64).reshape(-1, D)
        room = np.array([o["room"] for o in objs], np.int32)
        views = [np.asarray(json.load(open(os.path.join(directory, "rooms", r["room_id"] + ".json"))).get("embeddings") or [], np.float64)
                 .reshape(-1, D) for r in rooms]
    return dict(emb=emb, room=room, views=views, keys=[int(r["room_id"].split("_")[-1]) for r in rooms],
                floors=[[i for i, r in enumerate(rooms) if r["floor"] == f] for f in range(g.counts()["floors"])])


def _reference(L, tabs, names):
    from holoagent_amd._lib import NodeIndex
    roff = np.concatenate([[0], np.cumsum([len(t["keys"]) for t in tabs])])
    ix = NodeIndex(np.concatenate([t["emb"] for t in tabs]), np.concatenate([t["room"] + roff[s] for s, t in enumerate(tabs)]).astype(np.int32), lib_=L)
    ix.set_hierarchy([[int(roff[s] + r) for r in fl] for s, t in enumerate(tabs) for fl in t["floors"]], np.concatenate(names),
                     [v for t in tabs for v in t["views"]], [k for t in tabs for k in t["keys"]])
    return ix


def _names(seed, n):
    rng = np.random.Generator(np.random.PCG64(seed))
    a = rng.standard_normal((n, D))
    return a / np.linalg.norm(a, axis=1, keepdims=True)


def _queries(n_floors, emb, Q=256, C=3):
    rng = np.random.Generator(np.random.PCG64(17))
    T = rng.standard_normal((Q, C, D))
    T[:, 0] += 3.0 * emb[rng.integers(0, len(emb), Q)]
    T = (T / np.linalg.norm(T, axis=2, keepdims=True)).astype(np.float32)
    Tr = rng.standard_normal((Q, D))
    Tr = (Tr / np.linalg.norm(Tr, axis=1, keepdims=True)).astype(np.float32)
    return T, (np.arange(Q) % C).astype(np.int32), Tr, (np.arange(Q) % (n_floors + 1) - 1).astype(np.int32)


def _answer(fn, mode, neg, k, q, RM=32):
    from holoagent_amd._lib import HmsgError
    T, qid, Tr, fl = q
    try:
        out = fn(T, qid, Tr, fl, np.full(len(T), mode, np.int32), k, neg, RM)
    except HmsgError as e:
        return ("error", "room stage" in str(e))
    return (np.array([s + [-1] * (RM - len(s)) for s in out[0]], np.int32), out[1], out[2], out[3].view(np.int64))


def _same(a, b, what):
    if isinstance(a[0], str) or isinstance(b[0], str):
        assert a == b, what
        return
    for x, y in zip(a, b):
        assert np.array_equal(x, y), what


def test_graphs_query_over_built_and_reloaded_graphs_gpu(tmp_path):
    from holoagent_amd._lib import HmsgLib, SceneGraph, query_graphs
    L = HmsgLib()
    built = [_graph(L, 70 + i) for i in range(4)]
    d = str(tmp_path / "saved")
    built[1][1].save(d)
    loaded = SceneGraph.load(d, lib_=L)
    shards = [(built[0][1], _tables(built[0][1], built[0][0])), (loaded, _tables(loaded, directory=d))] + \
             [(g, _tables(g, sc)) for sc, g in built[2:]]
    gs = [g for g, _ in shards]
    tabs = [t for _, t in shards]
    n_obj = sum(len(t["emb"]) for t in tabs)
    print("objects per graph", [len(t["emb"]) for t in tabs], "rooms", [len(t["keys"]) for t in tabs])
    assert all(len(t["emb"]) for t in tabs) and n_obj >= 40
    names = [_names(5 + i, len(t["keys"])) for i, t in enumerate(tabs)]
    q = _queries(sum(len(t["floors"]) for t in tabs), np.concatenate([t["emb"] for t in tabs]))
    ref = _reference(L, tabs, names)
    hits = 0
    for mode in (0, 1, 2, 3):
        for neg, k in ((1, 5), (0, 1)):
            want = _answer(lambda T, qid, Tr, fl, m, k_, n_, RM: ref.query_hier(T, qid, Tr, fl, m, k_, use_negatives=n_, max_rooms=RM), mode, neg, k, q)
            got = _answer(lambda T, qid, Tr, fl, m, k_, n_, RM: query_graphs(gs, names, T, qid, Tr, fl, m, k_, use_negatives=n_, max_rooms=RM)[:4],
                          mode, neg, k, q)
            _same(got, want, (mode, neg, k))
            hits += 0 if isinstance(want[0], str) else int((want[1] >= 0).sum())
    assert hits > 0
    ref.close()
    loaded.close()
    for sc, g in built:
        g.close()
        sc.close()


def test_graph_query_sharded_with_one_rccl_rank_gpu():
    from holoagent_amd._lib import Comm, HmsgLib
    L = HmsgLib()
    cm = Comm.create(Comm.unique_id(L), 0, 1, 0, L)
    sc, g = _graph(L, 90)
    t = _tables(g, sc)
    names = _names(3, len(t["keys"]))
    q = _queries(len(t["floors"]), t["emb"], Q=128)
    for mode in (0, 1, 2, 3):
        a = _answer(lambda T, qid, Tr, fl, m, k, n, RM: g.query_sharded(cm, T, qid, Tr, fl, m, k, use_negatives=n, room_name_emb=names,
                                                                         max_rooms=RM)[:4], mode, 1, 5, q)
        b = _answer(lambda T, qid, Tr, fl, m, k, n, RM: g.query(T, qid, Tr, fl, m, k, use_negatives=n, room_name_emb=names, max_rooms=RM),
                    mode, 1, 5, q)
        _same(a, b, mode)
    out = g.query_sharded(cm, *q[:3], q[3], np.zeros(len(q[0]), np.int32), 3, room_name_emb=names)
    assert out[4].tolist() == [0, len(t["emb"])] and out[5].tolist() == [0, len(t["keys"])]
    g.close()
    sc.close()
    cm.close()


def test_gemm_kernels_agree_bit_for_bit_gpu():
    """S over a table of >= 64 rows with >= 64 text rows (the tiled kernel) against the same rows split into tables of < 64 (the
    one-wave kernel): every entry has the same bits, D a multiple of 16 and not"""
    from holoagent_amd._lib import HmsgLib, NodeIndex
    L = HmsgLib()
    rng = np.random.Generator(np.random.PCG64(23))
    for d in (64, 40):
        E = rng.standard_normal((150, d))
        T = rng.standard_normal((96, d)).astype(np.float32)
        full = NodeIndex(E, np.zeros(150, np.int32), lib_=L)
        S = full.similarity(T)
        parts = []
        for a, b in ((0, 40), (40, 100), (100, 150)):
            ix = NodeIndex(np.ascontiguousarray(E[a:b]), np.zeros(b - a, np.int32), lib_=L)
            parts.append(ix.similarity(T))
            ix.close()
        full.close()
        assert np.array_equal(S.view(np.int64), np.concatenate(parts, axis=1).view(np.int64)), d
