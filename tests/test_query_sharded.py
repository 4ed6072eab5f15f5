"""The sharded query (include/hmsg.h: hmsg_graph_query_sharded, hmsg_graphs_query; holoagent_amd/csrc/hmsg_query_sharded.hip) on the
kernel simulator: tables stay on their shard, and the answer equals hmsg_query_hier on ONE index over the concatenated tables -- sel,
nsel, idx, room and the float64 score, bit for bit -- for every room mode, floor -1 and every global floor, use_negatives 0 / 1 and
k = 1 / 3.  World > 1 runs over the RCCL test double (tests/rccl_double, as tests/test_comm_world.py does).

Shards are built graphs (a small synthetic scene each; one rank with rooms but no object), the same graphs saved and reloaded, a mix,
and saved graphs written here directly (several floors and rooms, duplicate embeddings across shards for exact score ties, a table
of >= 64 nodes over shards of < 64 each with Q >= 64: the GEMM-kernel choice differs between a shard and the concatenation)."""
import json
import os
import subprocess

import numpy as np
import pytest

from tests import parity_common as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DOUBLE_SRC = os.path.join(ROOT, "tests", "rccl_double", "rccl_double.cpp")
DOUBLE = os.path.join(ROOT, "tests", "rccl_double", "librccl_double.so")
D = 16

pytestmark = pytest.mark.skipif(not os.path.exists(PC.EMU_PATH), reason="kernel simulator not built")


def _double():
    if not os.path.exists(DOUBLE) or os.path.getmtime(DOUBLE) < os.path.getmtime(DOUBLE_SRC):
        subprocess.run(["g++", "-O2", "-shared", "-fPIC", "-o", DOUBLE, DOUBLE_SRC, "-lpthread", "-lrt"], check=True)
    return DOUBLE


def _wait_id(path):
    import time
    for _ in range(20000):
        if os.path.exists(path):
            return open(path, "rb").read()
        time.sleep(0.005)
    raise RuntimeError("no communicator id")


def _spawn(fn, world, *args):
    import torch.multiprocessing as mp
    mp.spawn(fn, args=(world,) + args, nprocs=world, join=True)


# ---- shards ----
def _built_graph(L, seed, empty=False):
    """a small synthetic scene through the whole path into a graph; empty: no masks, so rooms and views but no object"""
    from holoagent_amd._lib import SceneGraph
    from holoagent_amd.synth import SceneSpec, SynthScene
    spec = SceneSpec(seed=seed, rooms_x=1, rooms_z=1, room_size=(3.6, 2.5, 3.2), objects_per_room=4, width=64, height=48, n_frames=6,
                     n_masks=8, feat_dim=D, yaw_step_deg=25.0)
    scn = SynthScene(spec)
    frames = [scn.frame(i) for i in range(spec.n_frames)]
    S = PC.stack_frames(frames)
    sc = PC.make_scene(L, frames, dict(feat_dim=D, outlier_nb_points=20, outlier_radius=0.3, feat_dbscan_min=8))
    sc.add_frames(S["rgb"], S["depth"], S["pose"], S["K"])
    sc.finalize_map()
    sc.add_frame_features(0, S["masks"], S["f_g"], S["f_masked"], S["f_crop"], S["n_masks"] * (0 if empty else 1))
    sc.fuse_frames()
    sc.merge_instances()
    sc.pool_instances()
    g = SceneGraph.build(sc, S["pose"], S["f_g"], num_views=3, host_threads=1)
    assert (g.counts()["objects"] == 0) == empty
    return sc, g


def _built_tables(sc, g):
    """the graph's tables as its index holds them: the node table (float32 -> float64), rooms, floors, keys, view embeddings"""
    nodes, emb = sc.nodes(embeddings=True)
    rooms = g.rooms()
    return dict(emb=np.asarray(emb, np.float32).reshape(-1, D).astype(np.float64), room=np.array([int(n["room"]) for n in nodes], np.int32),
                floors=[[i for i, r in enumerate(rooms) if r["floor"] == f] for f in range(g.counts()["floors"])],
                keys=[int(r["room_id"].split("_")[-1]) for r in rooms],
                views=[np.asarray(g.room_embeddings(i, D), np.float32).reshape(-1, D).astype(np.float64) for i in range(len(rooms))])


def _saved_tables(g, directory):
    """a loaded graph's tables as hmsg_load reads them: float64 rows of the saved JSON"""
    rooms, objs = g.rooms(), g.objects()
    emb = [json.load(open(os.path.join(directory, "objects", o["object_id"] + ".json")))["embedding"] for o in objs]
    views = []
    for r in rooms:
        e = json.load(open(os.path.join(directory, "rooms", r["room_id"] + ".json"))).get("embeddings") or []
        views.append(np.asarray(e, np.float64).reshape(-1, D))
    return dict(emb=np.asarray(emb, np.float64).reshape(-1, D), room=np.array([o["room"] for o in objs], np.int32),
                floors=[[i for i, r in enumerate(rooms) if r["floor"] == f] for f in range(g.counts()["floors"])],
                keys=[int(r["room_id"].split("_")[-1]) for r in rooms], views=views)


def _write_graph(L, directory, seed, n_floors, rooms_per_floor, objs_per_room, n_views=2, shared=None):
    """a saved graph written directly (the files hmsg_save writes, the fields hmsg_load reads).  shared: rows every graph holds too
    (exact score ties across shards)."""
    from holoagent_amd._lib import write_ply
    rng = np.random.Generator(np.random.PCG64(seed))
    for sub in ("floors", "rooms", "objects", "views"):
        os.makedirs(os.path.join(directory, sub), exist_ok=True)
    pts = rng.standard_normal((5, 3))

    def unit(a):
        return a / np.linalg.norm(a, axis=-1, keepdims=True)
    n_obj = 0
    for f in range(n_floors):
        write_ply(os.path.join(directory, "floors", "%d.ply" % f), pts, lib_=L)
        json.dump(dict(name="floor_%d" % f, floor_height=2.5, floor_zero_level=0.0), open(os.path.join(directory, "floors", "%d.json" % f), "w"))
        for r in range(rooms_per_floor):
            rid = "%d_%d" % (f, r)
            write_ply(os.path.join(directory, "rooms", rid + ".ply"), pts, lib_=L)
            json.dump(dict(name="room_" + rid, embeddings=unit(rng.standard_normal((n_views, D))).tolist()),
                      open(os.path.join(directory, "rooms", rid + ".json"), "w"))
            for o in range(objs_per_room):
                e = unit(rng.standard_normal(D))
                if shared is not None and n_obj < len(shared):
                    e = shared[n_obj]
                n_obj += 1
                oid = "%s_%d" % (rid, o)
                write_ply(os.path.join(directory, "objects", oid + ".ply"), pts, lib_=L)
                json.dump(dict(name="object_" + oid, embedding=list(map(float, e))), open(os.path.join(directory, "objects", oid + ".json"), "w"))
    return directory


def _names(seed, n_rooms):
    rng = np.random.Generator(np.random.PCG64(seed))
    n = rng.standard_normal((max(n_rooms, 1), D))[:n_rooms]
    return n / np.maximum(np.linalg.norm(n, axis=1, keepdims=True), 1e-12)


# ---- the reference: ONE index over the concatenated float64 tables, global ids ----
def _reference(L, tabs, names):
    from holoagent_amd._lib import NodeIndex
    roff = np.concatenate([[0], np.cumsum([len(t["keys"]) for t in tabs])]).astype(np.int64)
    emb = np.concatenate([t["emb"] for t in tabs])
    room = np.concatenate([t["room"] + roff[s] for s, t in enumerate(tabs)]).astype(np.int32)
    floors = [[int(roff[s] + r) for r in fl] for s, t in enumerate(tabs) for fl in t["floors"]]
    ix = NodeIndex(emb, room, lib_=L)
    ix.set_hierarchy(floors, None if names is None else np.concatenate(names), [v for t in tabs for v in t["views"]],
                     [k for t in tabs for k in t["keys"]])
    return ix


def _queries(n_floors, Q=12, C=3, seed=5, emb=None):
    """every floor id (-1 and each global floor) in turn; object rows near nodes so that the negative prompts filter"""
    rng = np.random.Generator(np.random.PCG64(seed))
    T = rng.standard_normal((Q, C, D))
    if emb is not None and len(emb):
        T[:, 0] += 3.0 * emb[rng.integers(0, len(emb), Q)]
    T = (T / np.linalg.norm(T, axis=2, keepdims=True)).astype(np.float32)
    Tr = rng.standard_normal((Q, D))
    Tr = (Tr / np.linalg.norm(Tr, axis=1, keepdims=True)).astype(np.float32)
    qid = (np.arange(Q) % C).astype(np.int32)
    fl = (np.arange(Q) % (n_floors + 1) - 1).astype(np.int32)
    return T, qid, Tr, fl


CASES = [(m, neg, k) for m in (0, 1, 2, 3) for neg in (0, 1) for k in (1, 3)]


def _answer(fn, T, qid, Tr, fl, mode, neg, k, RM=16):
    """-> (sel padded, nsel, idx, room, score), or ("error", is-the-room-stage-error)"""
    from holoagent_amd._lib import HmsgError
    try:
        out = fn(T, qid, Tr, fl, np.full(len(T), mode, np.int32), k, neg, RM)
    except HmsgError as e:
        return ("error", "room stage" in str(e))
    sel = out[0]
    return (np.array([s + [-1] * (RM - len(s)) for s in sel], np.int32), np.array([len(s) for s in sel]), out[1], out[2], out[3])


def _same(a, b, what):
    if isinstance(a[0], str) or isinstance(b[0], str):
        assert a == b, (what, a[:1], b[:1])
        return
    assert len(a) == len(b), what
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and np.array_equal(x, y), what
        if x.dtype == np.float64:
            assert np.array_equal(x.view(np.int64), y.view(np.int64)), what        # bit for bit (the sign of a zero included)


def _ref_fn(ix):
    return lambda T, qid, Tr, fl, m, k, neg, RM: ix.query_hier(T, qid, Tr, fl, m, k, use_negatives=neg, max_rooms=RM)


def _graphs_fn(gs, names):
    from holoagent_amd._lib import query_graphs
    return lambda T, qid, Tr, fl, m, k, neg, RM: query_graphs(gs, names, T, qid, Tr, fl, m, k, use_negatives=neg, max_rooms=RM)


def _sharded_fn(g, comm, names):
    return lambda T, qid, Tr, fl, m, k, neg, RM: g.query_sharded(comm, T, qid, Tr, fl, m, k, use_negatives=neg, room_name_emb=names,
                                                                 max_rooms=RM)[:4]


def _count_answers(r):
    return 0 if isinstance(r[0], str) else int((r[2] >= 0).sum())


# ---- one process: hmsg_graphs_query ----
def test_graphs_query_three_saved_graphs_equals_the_concatenated_index(tmp_path):
    from holoagent_amd._lib import HmsgLib, SceneGraph, query_graphs
    L = HmsgLib(PC.EMU_PATH)
    rng = np.random.Generator(np.random.PCG64(77))
    shared = rng.standard_normal((3, D))
    shared /= np.linalg.norm(shared, axis=1, keepdims=True)
    specs = [(1, 2, 3), (2, 3, 2), (1, 1, 4)]
    dirs = [_write_graph(L, str(tmp_path / ("g%d" % i)), 10 + i, *s, shared=shared) for i, s in enumerate(specs)]
    gs = [SceneGraph.load(d, lib_=L) for d in dirs]
    tabs = [_saved_tables(g, d) for g, d in zip(gs, dirs)]
    names = [_names(30 + i, len(t["keys"])) for i, t in enumerate(tabs)]
    T, qid, Tr, fl = _queries(4, emb=np.concatenate([t["emb"] for t in tabs]))
    ref = _reference(L, tabs, names)
    hits = 0
    for case in CASES:
        want = _answer(_ref_fn(ref), T, qid, Tr, fl, *case)
        _same(_answer(_graphs_fn(gs, names), T, qid, Tr, fl, *case), want, case)
        hits += _count_answers(want)
    assert hits > 0
    ref.close()
    out = query_graphs(gs, names, T, qid, Tr, fl, np.zeros(len(T), np.int32), 3, max_rooms=16)
    assert out[4].tolist() == [0, 6, 18, 22] and out[5].tolist() == [0, 2, 8, 9] and out[6].tolist() == [0, 1, 3, 4]
    for g in gs:
        g.close()


def test_graphs_query_across_the_gemm_kernel_switch(tmp_path):
    """>= 64 nodes and Q * C >= 64 in the concatenation (the tiled GEMM), < 64 nodes per shard (the one-wave kernel)"""
    from holoagent_amd._lib import HmsgLib, SceneGraph
    L = HmsgLib(PC.EMU_PATH)
    dirs = [_write_graph(L, str(tmp_path / ("g%d" % i)), 50 + i, 1, 2, 12 + 4 * i, n_views=1) for i in range(3)]
    gs = [SceneGraph.load(d, lib_=L) for d in dirs]
    tabs = [_saved_tables(g, d) for g, d in zip(gs, dirs)]
    sizes = [len(t["emb"]) for t in tabs]
    assert max(sizes) < 64 and sum(sizes) >= 64
    names = [_names(60 + i, len(t["keys"])) for i, t in enumerate(tabs)]
    T, qid, Tr, fl = _queries(3, Q=64, C=2, seed=9, emb=np.concatenate([t["emb"] for t in tabs]))
    ref = _reference(L, tabs, names)
    for case in [(0, 1, 3), (1, 0, 3), (2, 1, 1)]:
        want = _answer(_ref_fn(ref), T, qid, Tr, fl, *case)
        assert _count_answers(want) > 0
        _same(_answer(_graphs_fn(gs, names), T, qid, Tr, fl, *case), want, case)
    ref.close()
    for g in gs:
        g.close()


def test_world_one_without_a_communicator_equals_graph_query(tmp_path):
    from holoagent_amd._lib import Comm, HmsgLib, SceneGraph
    L = HmsgLib(PC.EMU_PATH)
    g = SceneGraph.load(_write_graph(L, str(tmp_path / "g"), 3, 2, 2, 3), lib_=L)
    names = _names(4, 4)
    comm = Comm.single(lib_=L)
    T, qid, Tr, fl = _queries(2)

    def plain(T, qid, Tr, fl, m, k, neg, RM):
        return g.query(T, qid, Tr, fl, m, k, use_negatives=neg, room_name_emb=names, max_rooms=RM)
    for case in CASES:
        _same(_answer(_sharded_fn(g, comm, names), T, qid, Tr, fl, *case), _answer(plain, T, qid, Tr, fl, *case), case)
    comm.close()
    g.close()


def test_label_mode_without_room_names_is_an_error(tmp_path):
    from holoagent_amd._lib import HmsgError, HmsgLib, SceneGraph, query_graphs
    L = HmsgLib(PC.EMU_PATH)
    gs = [SceneGraph.load(_write_graph(L, str(tmp_path / ("g%d" % i)), i, 1, 2, 2), lib_=L) for i in range(2)]
    T, qid, Tr, fl = _queries(2)
    with pytest.raises(HmsgError, match="room name"):
        query_graphs(gs, [_names(1, 2), None], T, qid, Tr, fl, np.ones(len(T), np.int32), 2)
    sel = query_graphs(gs, [_names(1, 2), None], T, qid, Tr, fl, np.zeros(len(T), np.int32), 2)[0]     # (no label mode: fine)
    assert len(sel) == len(T)
    for g in gs:
        g.close()


# ---- several ranks: hmsg_graph_query_sharded over the RCCL test double ----
def _comm(L, rank, world, tmp):
    from holoagent_amd._lib import Comm
    idp = os.path.join(tmp, "id.bin")
    if rank == 0:
        open(idp + ".tmp", "wb").write(Comm.unique_id(lib_=L))
        os.replace(idp + ".tmp", idp)
    return Comm.create(_wait_id(idp), rank, world, lib_=L)


def _run_cases(g, comm, names, q):
    return {case: _answer(_sharded_fn(g, comm, names), *q, *case) for case in CASES}


def _built_worker(rank, world, tmp, empty_rank):
    """built graphs (one rank without objects): query_sharded against allgather_index(...).query_hier on every rank; then the same graphs
    saved and reloaded, and a mix (rank 0 loaded, the others built: with 3 ranks a loaded and a built node table meet in the object
    stage) -- answers kept for the parent's concatenated reference"""
    import pickle
    os.environ["HMSG_RCCL_LIB"] = DOUBLE
    from holoagent_amd._lib import HmsgLib, SceneGraph
    L = HmsgLib(PC.EMU_PATH)
    comm = _comm(L, rank, world, tmp)
    sc, g = _built_graph(L, 40 + rank, empty=rank == empty_rank)
    names = _names(100 + rank, g.counts()["rooms"])
    tabs = _built_tables(sc, g)
    q = _queries(world, seed=11)                                       # (the same on every rank; one storey per synthetic scene)
    ix, noff, roff, foff = g.allgather_index(comm, names)
    res = {"built": _run_cases(g, comm, names, q)}
    for case in CASES:
        _same(res["built"][case], _answer(_ref_fn(ix), *q, *case), ("built vs allgather_index", rank, case))
    ix.close()
    d = os.path.join(tmp, "saved%d" % rank)
    g.save(d)
    lg = SceneGraph.load(d, lib_=L)
    res["loaded"] = _run_cases(lg, comm, names, q)
    res["mix"] = _run_cases(lg if rank == 0 else g, comm, names, q)          # (rank 0 loaded: float64 rows from JSON; rank 2 built)
    pickle.dump(dict(res=res, built=tabs, saved=_saved_tables(lg, d), names=names, q=q), open(os.path.join(tmp, "r%d.pkl" % rank), "wb"))
    lg.close()
    g.close()
    sc.close()
    comm.close()


@pytest.mark.parametrize("world,empty_rank", [(2, 1), (3, 1)])
def test_query_sharded_with_several_ranks(tmp_path, world, empty_rank):
    import pickle
    from holoagent_amd._lib import HmsgLib
    _double()
    _spawn(_built_worker, world, str(tmp_path), empty_rank)
    L = HmsgLib(PC.EMU_PATH)
    rs = [pickle.load(open(tmp_path / ("r%d.pkl" % r), "rb")) for r in range(world)]
    assert len(rs[empty_rank]["built"]["emb"]) == 0 and all(len(r["built"]["emb"]) for i, r in enumerate(rs) if i != empty_rank)
    q = rs[0]["q"]
    names = [r["names"] for r in rs]
    kinds = [("built", ["built"] * world), ("loaded", ["saved"] * world), ("mix", ["saved"] + ["built"] * (world - 1))]
    hits = 0
    for kind, tab_of in kinds:
        ref = _reference(L, [rs[s][tab_of[s]] for s in range(world)], names)
        for case in CASES:
            want = _answer(_ref_fn(ref), *q, *case)
            hits += _count_answers(want)
            for r in range(world):
                _same(rs[r]["res"][kind][case], want, (kind, r, case))
        ref.close()
    assert hits > 0


def _names_missing_worker(rank, world, tmp):
    os.environ["HMSG_RCCL_LIB"] = DOUBLE
    from holoagent_amd._lib import HmsgError, HmsgLib, SceneGraph
    L = HmsgLib(PC.EMU_PATH)
    comm = _comm(L, rank, world, tmp)
    g = SceneGraph.load(_write_graph(L, os.path.join(tmp, "g%d" % rank), rank, 1, 2, 2), lib_=L)
    T, qid, Tr, fl = _queries(world)
    try:
        g.query_sharded(comm, T, qid, Tr, fl, np.ones(len(T), np.int32), 2, room_name_emb=None if rank == 1 else _names(rank, 2))
        res = "no error"
    except HmsgError as e:
        res = "failed: " + str(e)
    open(os.path.join(tmp, "res%d.txt" % rank), "w").write(res)
    g.close()
    comm.close()


def test_a_rank_without_room_names_fails_every_rank(tmp_path):
    """label mode, rank 1 without room_name_emb: its own check fails, the header exchange carries that, and EVERY rank returns an
    error -- nobody is left waiting (the ranks run in a thread that must finish in time)"""
    import threading
    _double()
    t = threading.Thread(target=_spawn, args=(_names_missing_worker, 2, str(tmp_path)), daemon=True)
    t.start()
    t.join(300)
    assert not t.is_alive(), "a rank hung"
    r0, r1 = open(tmp_path / "res0.txt").read(), open(tmp_path / "res1.txt").read()
    assert r1.startswith("failed") and "room name" in r1
    assert r0.startswith("failed") and "cannot take part" in r0


def _default_rooms_worker(rank, world, tmp):
    """12 rooms on rank 0, 3 on rank 1: max_rooms left to its default, which must be the concatenation's max(15, 10) on every rank"""
    import pickle
    os.environ["HMSG_RCCL_LIB"] = DOUBLE
    from holoagent_amd._lib import HmsgLib, SceneGraph
    L = HmsgLib(PC.EMU_PATH)
    comm = _comm(L, rank, world, tmp)
    d = _write_graph(L, os.path.join(tmp, "g%d" % rank), 70 + rank, 2 if rank == 0 else 1, 6 if rank == 0 else 3, 2, n_views=1)
    g = SceneGraph.load(d, lib_=L)
    names = _names(80 + rank, g.counts()["rooms"])
    q = _queries(3, seed=13)
    res = {}
    for case in [(m, 1, 3) for m in (0, 1, 2, 3)]:
        res[case] = _answer(lambda T, qid, Tr, fl, m, k, neg, RM: g.query_sharded(comm, T, qid, Tr, fl, m, k, use_negatives=neg,
                                                                                 room_name_emb=names)[:4], *q, *case, RM=15)
    pickle.dump(dict(res=res, tab=_saved_tables(g, d), names=names, q=q), open(os.path.join(tmp, "d%d.pkl" % rank), "wb"))
    g.close()
    comm.close()


def test_default_max_rooms_is_the_concatenations(tmp_path):
    import pickle
    from holoagent_amd._lib import HmsgLib
    _double()
    _spawn(_default_rooms_worker, 2, str(tmp_path))
    L = HmsgLib(PC.EMU_PATH)
    rs = [pickle.load(open(tmp_path / ("d%d.pkl" % r), "rb")) for r in range(2)]
    assert [len(r["tab"]["keys"]) for r in rs] == [12, 3]
    ref = _reference(L, [r["tab"] for r in rs], [r["names"] for r in rs])
    q = rs[0]["q"]
    full = 0
    for case in rs[0]["res"]:
        want = _answer(lambda T, qid, Tr, fl, m, k, neg, RM: ref.query_hier(T, qid, Tr, fl, m, k, use_negatives=neg), *q, *case, RM=15)
        for r in range(2):
            _same(rs[r]["res"][case], want, (r, case))
        full += 0 if isinstance(want[0], str) else int((want[1] > 10).sum())
    assert full > 0                                         # (floor -1, mode 0: all 15 rooms -- more than the old local default)
    ref.close()


def _k_differs_worker(rank, world, tmp):
    os.environ["HMSG_RCCL_LIB"] = DOUBLE
    from holoagent_amd._lib import HmsgError, HmsgLib, SceneGraph
    L = HmsgLib(PC.EMU_PATH)
    comm = _comm(L, rank, world, tmp)
    g = SceneGraph.load(_write_graph(L, os.path.join(tmp, "g%d" % rank), rank, 1, 2, 2), lib_=L)
    T, qid, Tr, fl = _queries(world)
    try:
        g.query_sharded(comm, T, qid, Tr, fl, np.zeros(len(T), np.int32), 2 + rank, max_rooms=16)
        res = "no error"
    except HmsgError as e:
        res = "failed: " + str(e)
    open(os.path.join(tmp, "res%d.txt" % rank), "w").write(res)
    g.close()
    comm.close()


def test_ranks_with_different_query_arguments_all_fail(tmp_path):
    """k = 2 on rank 0, 3 on rank 1: the header exchange shows it, and every rank returns the error (none waits)"""
    import threading
    _double()
    t = threading.Thread(target=_spawn, args=(_k_differs_worker, 2, str(tmp_path)), daemon=True)
    t.start()
    t.join(300)
    assert not t.is_alive(), "a rank hung"
    for r in range(2):
        res = open(tmp_path / ("res%d.txt" % r)).read()
        assert res.startswith("failed") and "queries differ" in res, res
