"""The object stage of the graph beside the pooling (hmsg_pool_instances starts it for the graph that hmsg_graph_begin registered on the
scene, hmsg_graph_finish takes its result over; holoagent_amd/csrc/hmsg_scene_graph.hip: EarlyObjects).

Nothing it computes may differ from the serial path, and nothing of it may show between the two calls:

  * the same scene built with HMSG_GRAPH_EARLY_OBJECTS = 1 (in front of the pooling), = 2 (behind k_pool_gram's launch) and = 0 (off)
    give, bit for bit, the instances read between pool and finish, the pooled features and node records, the object records and
    view lists, the edges and counts, and the instances read after finish;
  * the test hook (include/hmsg_test.h: hmsg_test_graph_early_objects) says what happened -- a silent fallback would pass every
    comparison: "consumed" with the switch on; "never made" with the switch off, for a graph begun after the pooling, without a graph;
  * order and lifetime: a graph closed between begin and pool, a reset between pool and finish followed by a second build on the
    handle, a scene destroyed after pool without a finish ("discarded" each), two handles driven by two threads at once; no case
    leaves a thread of the stage behind (the hook counts the ones not joined);
  * a stage that throws on the host (HMSG_DEBUG_EARLY_OBJECTS_THROW, simulator only) is not reported by hmsg_pool_instances: finish
    recomputes and the results are equal.

The shape is tests/test_scene_graph_cabi.py's: 12 frames of 96 x 72, 32 masks, D = 16, 2 x 1 rooms."""
import ctypes as C
import os
import threading

import numpy as np
import pytest

from tests import parity_common as PC

NEVER_MADE, CONSUMED, DISCARDED, PENDING = 0, 1, 2, 3
_cache = {}


def _lib(kind):
    from holoagent_amd._lib import HmsgLib
    import torch
    if kind == "emu":
        return HmsgLib(PC.EMU_PATH), torch.device("cpu")
    return HmsgLib(), torch.device("cuda", 0)


def _inputs(kind):
    """the scene's inputs and label table, made once per library"""
    if ("inp", kind) not in _cache:
        import torch
        import bench
        from holoagent_amd.synth import SceneSpec
        L, device = _lib(kind)
        spec = SceneSpec(seed=1234, n_frames=12, feat_dim=16, n_masks=32, width=96, height=72, rooms_x=2, rooms_z=1, room_size=(3.2, 2.6, 3.0),
                         yaw_step_deg=36.0, objects_per_room=3)
        inp = bench.build_scene_inputs(L, spec, device, torch)
        F, D = spec.n_frames, spec.feat_dim
        poses = np.stack([np.asarray(inp["pose"][i], np.float64).reshape(4, 4) for i in range(F)])
        rng = np.random.Generator(np.random.PCG64(99))
        label_feats = rng.standard_normal((9, D)).astype(np.float32)
        label_feats /= np.linalg.norm(label_feats, axis=1, keepdims=True)
        _cache[("inp", kind)] = dict(L=L, spec=spec, inp=inp, poses=poses, poses_inv=np.stack([np.linalg.inv(p) for p in poses]),
                                     fg=inp["f_g"].cpu().numpy(), label_feats=label_feats, label_names=["label%d" % i for i in range(9)])
    return _cache[("inp", kind)]


def hook(L, graph=None, scene=None):
    """(state, threads of the stage not joined) of a graph, or of a scene's last registration"""
    st, live = C.c_int32(-1), C.c_int32(-1)
    assert L.c.hmsg_test_graph_early_objects(graph.g if graph is not None else None, scene.h if scene is not None else None,
                                             C.byref(st), C.byref(live)) == 0
    return st.value, live.value


def _scene(W):
    from holoagent_amd._lib import Scene
    spec = W["spec"]
    return Scene(lib_=W["L"], device_id=0, height=spec.height, width=spec.width, max_frames=spec.n_frames, max_masks=32, feat_dim=spec.feat_dim)


def _map(W, sc):
    inp = W["inp"]
    sc.add_frames(inp["rgb"], inp["depth"], inp["pose"], inp["K"])
    sc.finalize_map()


def _begin(W, sc):
    from holoagent_amd._lib import SceneGraph
    return SceneGraph.begin(sc, W["poses"], W["fg"], poses_inv=W["poses_inv"], img_paths=["img/%05d.png" % i for i in range(len(W["poses"]))],
                            num_views=5, host_threads=2)


def _to_pool(W, sc):
    inp = W["inp"]
    sc.add_frame_features(0, inp["masks"], inp["f_g"], inp["f_masked"], inp["f_crop"])
    sc.fuse_frames()
    sc.merge_instances()
    sc.pool_instances()


def _mid(sc):
    """what a caller can read between pool and finish"""
    return dict(inst=[a.tobytes() for a in sc.instances()], boxes=sc.instance_boxes().tobytes(), feats=sc.instance_feats().tobytes(),
                n_nodes=len(sc.nodes()))


def _end(sc, cg):
    nodes, emb = sc.nodes(embeddings=True)
    cnt = cg.counts()
    return dict(inst=[a.tobytes() for a in sc.instances()], boxes=sc.instance_boxes().tobytes(), feats=sc.instance_feats().tobytes(),
                nodes=nodes.tobytes(), node_emb=emb.tobytes(), objects=cg.objects(), graph=cg.to_dict(), edges=cg.edges().tobytes(),
                counts={k: v for k, v in cnt.items() if not k.endswith("_ms")})


def _finish(W, cg):
    cg.finish(W["label_feats"], W["label_names"])


def _build(W):
    """one whole build through the graph object -> (scene, graph, mid, end)"""
    sc = _scene(W)
    _map(W, sc)
    cg = _begin(W, sc)
    _to_pool(W, sc)
    mid = _mid(sc)
    _finish(W, cg)
    return sc, cg, mid, _end(sc, cg)


def _reference(kind, monkeypatch):
    """the serial path: the switch off"""
    if ("ref", kind) not in _cache:
        W = _inputs(kind)
        monkeypatch.setenv("HMSG_GRAPH_EARLY_OBJECTS", "0")
        sc, cg, mid, end = _build(W)
        assert hook(W["L"], graph=cg) == (NEVER_MADE, 0) and hook(W["L"], scene=sc) == (NEVER_MADE, 0)
        assert end["counts"]["objects"] >= 3 and end["counts"]["view_object_links"] >= 3 and len(mid["inst"]) >= 3
        assert mid["inst"] != end["inst"], "the per-object DBSCAN changed no instance: the scene does not exercise the commit"
        cg.close()
        sc.close()
        _cache[("ref", kind)] = (mid, end)
        monkeypatch.delenv("HMSG_GRAPH_EARLY_OBJECTS")
    return _cache[("ref", kind)]


def check_switch(kind, monkeypatch, mode):
    ref_mid, ref_end = _reference(kind, monkeypatch)
    W = _inputs(kind)
    if mode is not None:
        monkeypatch.setenv("HMSG_GRAPH_EARLY_OBJECTS", mode)
    sc, cg, mid, end = _build(W)
    assert hook(W["L"], graph=cg) == (CONSUMED, 0) and hook(W["L"], scene=sc) == (CONSUMED, 0)
    assert mid == ref_mid, "between pool and finish the handle is not what the serial path leaves"
    assert end == ref_end
    cg.close()
    sc.close()


def check_never_made(kind, monkeypatch):
    ref_mid, ref_end = _reference(kind, monkeypatch)
    W = _inputs(kind)
    # no graph at all while the scene is pooled ...
    sc = _scene(W)
    _map(W, sc)
    _to_pool(W, sc)
    assert hook(W["L"], scene=sc) == (NEVER_MADE, 0)
    assert _mid(sc) == ref_mid
    # ... and a graph begun after the pooling
    cg = _begin(W, sc)
    _finish(W, cg)
    assert hook(W["L"], graph=cg) == (NEVER_MADE, 0) and hook(W["L"], scene=sc) == (NEVER_MADE, 0)
    assert _end(sc, cg) == ref_end
    cg.close()
    sc.close()


def check_closed_before_pool(kind, monkeypatch):
    ref_mid, ref_end = _reference(kind, monkeypatch)
    W = _inputs(kind)
    sc = _scene(W)
    _map(W, sc)
    _begin(W, sc).close()
    assert hook(W["L"], scene=sc) == (DISCARDED, 0)
    _to_pool(W, sc)                                  # (nothing is registered: nothing starts)
    assert hook(W["L"], scene=sc) == (DISCARDED, 0) and _mid(sc) == ref_mid
    cg = _begin(W, sc)
    _finish(W, cg)
    assert hook(W["L"], graph=cg) == (NEVER_MADE, 0)
    assert _end(sc, cg) == ref_end
    cg.close()
    sc.close()


def check_reset_then_second_build(kind, monkeypatch):
    ref_mid, ref_end = _reference(kind, monkeypatch)
    W = _inputs(kind)
    sc = _scene(W)
    _map(W, sc)
    cg = _begin(W, sc)
    _to_pool(W, sc)
    sc.reset()
    assert hook(W["L"], graph=cg) == (DISCARDED, 0) and hook(W["L"], scene=sc) == (DISCARDED, 0)
    cg.close()
    _map(W, sc)
    cg = _begin(W, sc)
    _to_pool(W, sc)
    mid = _mid(sc)
    _finish(W, cg)
    assert hook(W["L"], graph=cg) == (CONSUMED, 0)
    assert mid == ref_mid and _end(sc, cg) == ref_end
    cg.close()
    sc.close()


def check_destroy_without_finish(kind, monkeypatch):
    W = _inputs(kind)
    sc = _scene(W)
    _map(W, sc)
    cg = _begin(W, sc)
    _to_pool(W, sc)
    assert hook(W["L"], graph=cg) == (PENDING, 0)
    sc.close()
    assert hook(W["L"], graph=cg) == (DISCARDED, 0)
    cg.close()


def check_two_handles(kind, monkeypatch):
    ref_mid, ref_end = _reference(kind, monkeypatch)
    W = _inputs(kind)
    out, errs = [None, None], []

    def work(i):
        try:
            sc, cg, mid, end = _build(W)
            out[i] = (hook(W["L"], graph=cg)[0], mid, end)
            cg.close()
            sc.close()
        except BaseException as e:       # noqa: B036 (reported by the main thread)
            errs.append(e)
    ts = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errs, errs
    for st, mid, end in out:
        assert st == CONSUMED and mid == ref_mid and end == ref_end
    dummy = _scene(W)
    assert hook(W["L"], scene=dummy)[1] == 0
    dummy.close()


CASES = dict(switch_on=lambda k, m: check_switch(k, m, None), switch_behind_gram=lambda k, m: check_switch(k, m, "2"),
             never_made=check_never_made, closed_before_pool=check_closed_before_pool, reset_then_second_build=check_reset_then_second_build,
             destroy_without_finish=check_destroy_without_finish, two_handles=check_two_handles)


# (a build of this scene takes about a minute on the simulator: the second start point of the stage, a development switch, is
#  compared there only on request -- its twin runs on the MI355X in a fraction of a second)
@pytest.mark.skipif(not os.path.exists(PC.EMU_PATH), reason="kernel simulator not built")
@pytest.mark.parametrize("case", sorted(c for c in CASES if c != "switch_behind_gram" or os.environ.get("HMSG_EMU_SLOW")))
def test_early_objects_on_the_simulator(case, monkeypatch):
    monkeypatch.delenv("HMSG_GRAPH_EARLY_OBJECTS", raising=False)
    CASES[case]("emu", monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(CASES))
def test_early_objects_gpu(case, monkeypatch):
    monkeypatch.delenv("HMSG_GRAPH_EARLY_OBJECTS", raising=False)
    CASES[case]("gpu", monkeypatch)


@pytest.mark.skipif(not os.path.exists(PC.EMU_PATH), reason="kernel simulator not built")
def test_a_stage_that_throws_is_recomputed_by_finish_on_the_simulator(monkeypatch):
    monkeypatch.delenv("HMSG_GRAPH_EARLY_OBJECTS", raising=False)
    ref_mid, ref_end = _reference("emu", monkeypatch)
    W = _inputs("emu")
    monkeypatch.setenv("HMSG_DEBUG_EARLY_OBJECTS_THROW", "1")
    sc = _scene(W)
    _map(W, sc)
    cg = _begin(W, sc)
    _to_pool(W, sc)                                  # (Scene._ck raises on any status but HMSG_OK)
    assert hook(W["L"], graph=cg) == (DISCARDED, 0)
    mid = _mid(sc)
    _finish(W, cg)
    assert hook(W["L"], graph=cg) == (DISCARDED, 0)
    assert mid == ref_mid and _end(sc, cg) == ref_end
    cg.close()
    sc.close()
