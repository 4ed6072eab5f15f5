"""Caller arrays in device memory (include/hmsg.h: "input pointers may be host OR device pointers"; the staging helpers of
holoagent_amd/csrc/hmsg_common.h: copy_in / stage_in / copy_out / stage_out).  Every entry point below is called once with
numpy arrays and once with the same numbers as contiguous torch tensors on the device -- inputs and, where the ABI allows it,
outputs.  Both calls run the same kernels on the same data, so the results are equal bit for bit; there is no tolerance.

Sizes sit on both sides of the two thresholds of the pinned bounce buffers (h2d_bounce: 65 536 bytes, d2h_bounce: 4 096), so
the host call takes the plain copy in one case and the bounce in the other."""
import ctypes as C

import numpy as np
import pytest

from tests import parity_common as PC

pytestmark = pytest.mark.gpu

D_TEXT = 512


def _lib():
    from holoagent_amd._lib import HmsgLib
    return HmsgLib()


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", 0)).contiguous()


def _dev_like(a):
    import torch
    return torch.zeros(a.shape, dtype=getattr(torch, str(a.dtype)), device=torch.device("cuda", 0))


def _host(a):
    return a if isinstance(a, np.ndarray) else a.cpu().numpy()


def _unit_rows(rng, n, d, dtype):
    x = rng.standard_normal((n, d))
    return np.ascontiguousarray(x / np.linalg.norm(x, axis=1, keepdims=True), dtype)


# ------------------------------------------------------------------------------------------------ hmsg_points_view_depths
@pytest.mark.parametrize("n_points", [2000, 3000])          # 48 000 and 72 000 bytes of float64 points
def test_points_view_depths_device_points(n_points):
    from holoagent_amd._lib import _ptr
    L = _lib()
    rng = np.random.Generator(np.random.PCG64(n_points))
    sizes = [n_points // 2, 0, n_points - n_points // 2 - 301, 301]          # (an empty cloud, an odd one)
    P = len(sizes)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    pts = np.ascontiguousarray(rng.uniform(-1.5, 1.5, (n_points, 3)) + [0.0, 0.0, 2.0])
    pose_inv = np.ascontiguousarray(np.tile(np.eye(4).reshape(16), (P, 1)))
    pose_inv[2, 11] = -5.0                                                    # (camera 2 looks at the cloud from behind)
    wh = np.ascontiguousarray(np.tile(np.array([128, 96], np.int32), (P, 1)))
    K = np.array([100.0, 0, 64, 0, 100.0, 48, 0, 0, 1])

    def run(p):
        avg, vis, md = np.zeros(P), np.zeros(P, np.uint8), np.zeros(P)
        rc = L.c.hmsg_points_view_depths(0, P, _ptr(off), _ptr(p), _ptr(pose_inv), _ptr(wh), _ptr(K), 0.5, 10.0, _ptr(avg), _ptr(vis), _ptr(md))
        assert rc == 0
        return avg, vis, md

    want, got = run(pts), run(_dev(pts))
    assert want[1].any() and not want[1].all()
    for w, g in zip(want, got):
        assert np.array_equal(w, g, equal_nan=w.dtype.kind == "f")
        assert w.tobytes() == g.tobytes()


# ------------------------------------------------------------------------------------------------ hmsg_denoise_feats_batch
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("n_sets, rows", [(4, 50), (20, 15)])
def test_denoise_feats_batch_device_in_and_out(dtype, n_sets, rows):
    # 64-d rows: 4 x 50 rows = 51 200 / 102 400 bytes in, 1 / 2 KB out; 20 x 15 rows = 76 800 / 153 600 bytes in, 5 / 10 KB out
    from holoagent_amd._lib import _ptr
    L = _lib()
    dim = 64
    rng = np.random.Generator(np.random.PCG64(n_sets * 100 + rows))
    X = np.empty((n_sets * rows, dim), dtype)
    for k in range(n_sets):
        centres = _unit_rows(rng, 2, dim, np.float64)
        which = (np.arange(rows) % 3 == 0).astype(int)                       # a cluster of 2/3 of the rows, one of 1/3
        X[k * rows:(k + 1) * rows] = centres[which] + 0.004 * rng.standard_normal((rows, dim))
    X[rows - 1] = _unit_rows(rng, 1, dim, np.float64)[0]                      # (a noise row)
    off = (np.arange(n_sets + 1) * rows).astype(np.int64)

    def run(x, out):
        ncl = np.zeros(n_sets, np.int32)
        rc = L.c.hmsg_denoise_feats_batch(0, n_sets, _ptr(off), _ptr(x), int(dtype == np.float64), dim, 0.02, 2, _ptr(out), _ptr(ncl))
        assert rc == 0
        return _host(out), ncl

    want, n_want = run(X, np.zeros((n_sets, dim), dtype))
    assert (n_want > rows // 2).all() and (n_want < rows).all()
    for x, out in ((_dev(X), _dev_like(want)), (_dev(X), np.zeros_like(want)), (X, _dev_like(want))):
        got, n_got = run(x, out)
        assert got.dtype == want.dtype and np.array_equal(want, got) and np.array_equal(n_want, n_got)


# ------------------------------------------------------------------------------------------------ hmsg_merge_room_objects
def test_merge_room_objects_device_points():
    from holoagent_amd._lib import Scene, _ptr
    sc = Scene(lib_=_lib(), height=8, width=8, max_frames=1, max_masks=1, feat_dim=8)
    rng = np.random.Generator(np.random.PCG64(7))
    a, b = rng.uniform(-0.2, 0.2, (300, 3)), rng.uniform(-0.2, 0.2, (257, 3)) + [2.0, 0.0, 0.0]
    # two same-name pairs: "chair" overlaps (a copy moved by a millimetre), "table" does not (two metres apart)
    clouds = [a, b, rng.uniform(-0.2, 0.2, (150, 3)) + [0.0, 3.0, 0.0], a[:280] + 0.001, b + [0.0, 0.0, 2.0]]
    names = ["chair", "table", "lamp", "chair", "table"]
    assert sc.merge_room_objects(clouds, names) == [[0, 3], [1], [2], [4]]
    n = len(clouds)
    off = np.concatenate([[0], np.cumsum([len(c) for c in clouds])]).astype(np.int64)
    pts = np.ascontiguousarray(np.concatenate(clouds))
    name_id = np.array([0, 1, 2, 0, 1], np.int32)

    def run(p):
        ng, goff, mem = C.c_int32(), np.zeros(n + 1, np.int32), np.zeros(n * (n + 1), np.int32)
        sc._ck(sc.L.c.hmsg_merge_room_objects(sc.h, n, _ptr(p), _ptr(off), _ptr(name_id), 0.01, 0.1, C.byref(ng), _ptr(goff), _ptr(mem), len(mem)))
        return ng.value, goff, mem

    want, got = run(pts), run(_dev(pts))
    assert want[0] == got[0] == 4 and np.array_equal(want[1], got[1]) and np.array_equal(want[2], got[2])
    sc.close()


# ------------------------------------------------------------------------------------------------ hmsg_index_create
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("n_nodes", [12, 40])               # 512-d rows: 24 576 / 49 152 bytes and 81 920 / 163 840 bytes
def test_index_from_a_device_table(dtype, n_nodes):
    from holoagent_amd._lib import _P, NodeIndex, _ptr
    L = _lib()
    rng = np.random.Generator(np.random.PCG64(n_nodes))
    emb = _unit_rows(rng, n_nodes, D_TEXT, dtype)
    rooms = (np.arange(n_nodes) % 3).astype(np.int32)
    T = _unit_rows(rng, 5, D_TEXT, np.float32)

    def make(e, r):
        ix = _P()
        assert L.c.hmsg_index_create(0, D_TEXT, n_nodes, _ptr(e), int(dtype == np.float64), _ptr(r), C.byref(ix)) == 0
        return NodeIndex._wrap(L, ix, n_nodes, D_TEXT)

    out = []
    for e, r in ((emb, rooms), (_dev(emb), rooms), (_dev(emb), _dev(rooms))):
        ix = make(e, r)
        out.append((ix.similarity(T),) + ix.query_objects(T[:, None, :], np.zeros(5, np.int32), [[2, 0]] * 5, 7, use_negatives=False))
        ix.close()
    assert np.abs(out[0][0]).max() > 0 and (out[0][1] >= 0).any()
    for got in out[1:]:
        for w, g in zip(out[0], got):
            assert np.array_equal(w, g)


# ------------------------------------------------------------------------------------------------ hmsg_query_hier / hmsg_query_objects
def _hier_index(L, rng, n_nodes=45):
    from holoagent_amd._lib import NodeIndex
    ix = NodeIndex(_unit_rows(rng, n_nodes, D_TEXT, np.float64), (np.arange(n_nodes) % 6).astype(np.int32), lib_=L)
    # two floors of three rooms; key = a room's position on its floor
    ix.set_hierarchy([[0, 1, 2], [3, 4, 5]], _unit_rows(rng, 6, D_TEXT, np.float64), [_unit_rows(rng, 2 + r % 2, D_TEXT, np.float64) for r in range(6)],
                     [0, 1, 2, 0, 1, 2])
    return ix


@pytest.mark.parametrize("Q", [8, 20])                      # C = 2 text rows a query: 16 x 512 and 40 x 512 float32
def test_query_hier_device_text_and_outputs(Q):
    from holoagent_amd._lib import _ptr
    L = _lib()
    rng = np.random.Generator(np.random.PCG64(Q))
    ix = _hier_index(L, rng)
    Cn, k, RM = 2, 5, 10
    T_obj, T_room = _unit_rows(rng, Q * Cn, D_TEXT, np.float32).reshape(Q, Cn, D_TEXT), _unit_rows(rng, Q, D_TEXT, np.float32)
    qid = (np.arange(Q) % Cn).astype(np.int32)
    floor_id = (np.arange(Q) % 3 - 1).astype(np.int32)
    room_mode = (np.arange(Q) % 4).astype(np.int32)
    shapes = [((Q, RM), np.int32), ((Q,), np.int32), ((Q, k), np.int32), ((Q, k), np.int32), ((Q, k), np.float64)]   # sel, nsel, idx, room, score

    def run(t_obj, q_id, t_room, outs):
        ix._ck(L.c.hmsg_query_hier(ix.ix, Q, Cn, _ptr(t_obj), _ptr(q_id), _ptr(t_room), _ptr(floor_id), _ptr(room_mode), k, 1, RM,
                                   *[_ptr(o) for o in outs]))
        sel, nsel, idx, room, score = [_host(o) for o in outs]
        return [sel[q, :nsel[q]].tolist() for q in range(Q)], nsel, idx, room, score

    want = run(T_obj, qid, T_room, [np.zeros(s, d) for s, d in shapes])
    assert (want[2] >= 0).any() and (want[1] > 0).all()
    host_outs = lambda: [np.zeros(s, d) for s, d in shapes]
    dev_outs = lambda: [_dev_like(np.zeros(s, d)) for s, d in shapes]
    mixed = lambda: [o if i % 2 else _dev_like(o) for i, o in enumerate(host_outs())]
    for args in ((_dev(T_obj), _dev(qid), _dev(T_room), dev_outs()), (_dev(T_obj), _dev(qid), _dev(T_room), host_outs()),
                 (T_obj, qid, T_room, dev_outs()), (_dev(T_obj), qid, T_room, mixed())):
        got = run(*args)
        assert got[0] == want[0]
        for w, g in zip(want[1:], got[1:]):
            assert np.array_equal(w, g)
    ix.close()


@pytest.mark.parametrize("Q", [8, 20])
def test_query_objects_device_text_ids_and_room_lists(Q):
    # (hmsg_query_objects returns into host arrays: include/hmsg.h names no device outputs for it)
    from holoagent_amd._lib import _ptr
    L = _lib()
    rng = np.random.Generator(np.random.PCG64(100 + Q))
    ix = _hier_index(L, rng)
    Cn, k = 2, 6
    T = _unit_rows(rng, Q * Cn, D_TEXT, np.float32).reshape(Q, Cn, D_TEXT)
    qid = (np.arange(Q) % Cn).astype(np.int32)
    lists = [[(q + j) % 6 for j in range(1 + q % 3)] for q in range(Q)]
    off = np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.int32)
    rooms = np.concatenate(lists).astype(np.int32)

    def run(t, q_id, r_off, r):
        idx, room, score = np.zeros((Q, k), np.int32), np.zeros((Q, k), np.int32), np.zeros((Q, k), np.float64)
        ix._ck(L.c.hmsg_query_objects(ix.ix, Q, Cn, _ptr(t), _ptr(q_id), _ptr(r_off), _ptr(r), k, 1, _ptr(idx), _ptr(room), _ptr(score)))
        return idx, room, score

    want = run(T, qid, off, rooms)
    assert (want[0] >= 0).any()
    for args in ((_dev(T), _dev(qid), _dev(off), _dev(rooms)), (_dev(T), qid, off, _dev(rooms)), (T, _dev(qid), _dev(off), rooms)):
        for w, g in zip(want, run(*args)):
            assert np.array_equal(w, g)
    ix.close()


# ------------------------------------------------------------------------------------------------ hmsg_get / hmsg_set_feature_sums
def test_feature_sums_to_and_from_device_arrays():
    from holoagent_amd.synth import SceneSpec, SynthScene
    spec = SceneSpec(seed=3, rooms_x=1, rooms_z=1, room_size=(3.6, 2.5, 3.2), objects_per_room=4, width=128, height=96, n_frames=6, n_masks=8,
                     feat_dim=64)
    scn = SynthScene(spec)
    frames = [scn.frame(i) for i in range(spec.n_frames)]
    sc = PC.make_scene(_lib(), frames, dict(feat_dim=64, outlier_nb_points=200))
    S = PC.stack_frames(frames)
    sc.add_frames(S["rgb"], S["depth"], S["pose"], S["K"])
    sc.finalize_map()
    sc.add_frame_features(0, S["masks"], S["f_g"], S["f_masked"], S["f_crop"], S["n_masks"])
    sc.fuse_frames()
    V, D = sc.map_size(), sc.cfg.feat_dim
    s0, c0 = np.zeros((V, D), np.float32), np.zeros(V, np.uint32)
    sc.feature_sums_into(s0, c0)
    assert V > 100 and np.abs(s0).sum() > 0 and c0.max() > 0
    s_d, c_d = _dev_like(s0), _dev(np.zeros(V, np.int32))                    # (torch has no uint32 arithmetic; the bits are what counts)
    sc.feature_sums_into(s_d, c_d)
    assert np.array_equal(s0, _host(s_d)) and np.array_equal(c0, _host(c_d).view(np.uint32))
    sc.feature_sums_into(s_d, None)                                          # (either may be NULL on get)
    sc.feature_sums_into(None, c_d)
    # set: other sums from the host, then the same from the device
    s1, c1 = np.ascontiguousarray(s0[::-1] * np.float32(3.0)), np.ascontiguousarray(c0[::-1] + np.uint32(1))
    sc.set_feature_sums_from(s1, c1)
    want = sc.map_feats().copy()
    sc.set_feature_sums_from(s0, c0)
    assert not np.array_equal(want, sc.map_feats())
    sc.set_feature_sums_from(_dev(s1), _dev(c1.view(np.int32)))
    assert np.array_equal(want, sc.map_feats())
    back_s, back_c = np.zeros_like(s0), np.zeros_like(c0)
    sc.feature_sums_into(back_s, back_c)
    assert np.array_equal(back_s, s1) and np.array_equal(back_c, c1)
    sc.close()
