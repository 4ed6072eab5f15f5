"""The kernels of the slow path's view level at table level (holoagent_amd/csrc/hmsg_query_views.hip; include/hmsg.h:
hmsg_index_set_views, hmsg_rematch_in_views, hmsg_points_view_depths) on synthetic tables that reach their edges.

Re-match (fsr_vln/memory/hmsg/graph/graph.py:2962-2986): the text row against the embeddings of a view's objects in
view.object_ids order, np.argmax (first maximum).  Views with 0, 1, 2, 63, 64, 65 and 257 objects (a wave pass takes 16, a
workgroup pass 64: less than one pass, exactly one, one more, several), a view that lists a node twice, two nodes with
duplicate embeddings (exact ties go to the first position) and a view whose maximum is its last entry.  The score must have the
bits of hmsg_similarity's entry and agree with numpy to 1e-12 (the tolerance of tests/parity_common.py for query scores).

Distances (fsr_vln/memory/hmsg/utils/graph_utils.py:49-70 avg_distance, :95-157 check_object_in_view): clouds of 0, 1, 63, 64, 65
and 5 000 points (the last spans several workgroups), all points behind the camera, exactly half of a cloud inside the image (the
min_visible_ratio boundary counts as visible), a mean depth just over / just under max_depth, points that project exactly onto
u = 0 (inside) and u = W (outside).  mean_depth and avg_z_front to rtol 1e-13, the tolerance tests/test_object_views.py uses for
mean_depth; two runs of the same input give the same bits."""
import os

import numpy as np
import pytest

from tests import parity_common as PC

N, Q = 300, 5
DUP_A, DUP_B = 10, 20


def _tables(D, seed):
    rng = np.random.default_rng(seed)
    E = rng.standard_normal((N, D)) / np.sqrt(D)
    T = (rng.standard_normal((Q, D)) / np.sqrt(D)).astype(np.float32)
    t0 = T[0].astype(np.float64)
    E[DUP_A] = E[DUP_B] = t0 * (4.0 / float(t0 @ t0))          # query 0 scores 4 on both, far above every other node
    others = [n for n in range(N) if n not in (DUP_A, DUP_B)]
    pick = lambda n: [int(v) for v in rng.permutation(others)[:n]]
    views = {
        "empty": [], "one": pick(1), "two": pick(2), "63": pick(63), "64": pick(64), "65": pick(65), "257": pick(257),
        "twice_and_duplicates": [7, DUP_A, 7, DUP_B, DUP_A],     # first maximum of query 0: position 1 (node DUP_A)
        "duplicates_other_order": [DUP_B, 3, DUP_A],             # ... here position 0 (node DUP_B)
        "max_is_last": pick(64) + [DUP_A],
        "max_is_last_of_many": pick(256) + [DUP_B],
    }
    return E, T, views


def check_rematch(L, D, seed):
    from holoagent_amd._lib import HmsgError, NodeIndex
    E, T, views = _tables(D, seed)
    ix = NodeIndex(E, np.zeros(N, np.int32), lib_=L)
    with pytest.raises(HmsgError):                                # no view table yet
        ix.rematch_in_views(T, np.zeros(Q, np.int32))
    names = list(views)
    ix.set_views([views[n] for n in names])
    S_dev = ix.similarity(T)
    T64 = T.astype(np.float64)
    compared = 0
    for vi, name in enumerate(names):
        nodes = views[name]
        node, score = ix.rematch_in_views(T, np.full(Q, vi, np.int32))
        if not nodes:
            assert (node == -1).all() and (score == 0.0).all()
            continue
        sims = np.dot(T64, E[nodes].T)                            # graph.py:2977-2979 on the gathered rows
        for q in range(Q):
            j = int(np.argmax(sims[q]))                           # :2980
            top2 = np.sort(sims[q])[-2:]
            if len(nodes) == 1 or top2[1] - top2[0] > 1e-9:
                assert node[q] == nodes[j], (name, q)
                compared += 1
            assert node[q] in nodes
            assert score[q] == S_dev[q, node[q]], (name, q)       # hmsg_similarity's bits
            assert abs(score[q] - sims[q, j]) <= 1e-12, (name, q)
    assert compared >= (len(names) - 3) * Q
    # the constructed exact ties and maxima of query 0
    v = {n: i for i, n in enumerate(names)}
    node, score = ix.rematch_in_views(T[:1].repeat(4, 0), [v["twice_and_duplicates"], v["duplicates_other_order"], v["max_is_last"], v["max_is_last_of_many"]])
    assert node.tolist() == [DUP_A, DUP_B, DUP_A, DUP_B]
    assert (score == S_dev[0, DUP_A]).all() and S_dev[0, DUP_A] == S_dev[0, DUP_B]
    assert S_dev[0, DUP_A] > np.delete(S_dev[0], [DUP_A, DUP_B]).max() + 1.0
    # a mixed batch: every query its own view
    mixed = np.array([v["257"], v["empty"], v["one"], v["65"], v["64"]], np.int32)
    node, score = ix.rematch_in_views(T, mixed)
    for q in range(Q):
        nodes = views[names[mixed[q]]]
        assert node[q] == (nodes[int(np.argmax(np.dot(T64[q], E[nodes].T)))] if nodes else -1)
    # errors: a view index out of range, an object index out of range, offsets that decrease
    for bad in (-1, len(names)):
        with pytest.raises(HmsgError):
            ix.rematch_in_views(T[:1], [bad])
    with pytest.raises(HmsgError):
        ix.set_views([[0, N]])
    off = np.array([0, 2, 1], np.int64)
    assert L.c.hmsg_index_set_views(ix.ix, 2, off.ctypes.data, np.zeros(2, np.int32).ctypes.data) != 0
    ix.close()


# ---- the reference's two distance functions, restated
def ref_avg_distance(pts, pose_inv):
    """visualize_pcd_on_image, utils/graph_utils.py:49-70 (the drawing left out): None -> NaN"""
    if pts.shape[0] == 0:
        return np.nan
    cam = (pose_inv @ np.hstack((pts, np.ones((pts.shape[0], 1)))).T).T[:, :3]
    cam = cam[cam[:, 2] > 0]
    return float(np.mean(cam[:, 2])) if cam.shape[0] else np.nan


def ref_check_object_in_view(w, h, K, pose_inv, pts, min_visible_ratio=0.5, max_depth=10.0):
    """check_object_in_view(..., return_depth=True), utils/graph_utils.py:95-157"""
    if pts.shape[0] == 0:
        return False, np.inf
    cam = (pose_inv @ np.hstack([pts, np.ones((pts.shape[0], 1))]).T).T[:, :3]
    cam = cam[cam[:, 2] > 0]
    if cam.shape[0] == 0:
        return False, np.inf
    px = (K @ cam.T).T
    px = px[:, :2] / px[:, 2:3]
    inside = (px[:, 0] >= 0) & (px[:, 0] < w) & (px[:, 1] >= 0) & (px[:, 1] < h)
    if not np.any(inside):
        return False, np.inf
    if np.sum(inside) / pts.shape[0] < min_visible_ratio:
        return False, np.inf
    md = np.mean(cam[inside, 2])
    return (False, md) if md > max_depth else (True, md)


W_, H_ = 96, 72
K_ = np.array([[64.0, 0.0, 48.0], [0.0, 64.0, 36.0], [0.0, 0.0, 1.0]])      # powers of two: the border cases are exact


def _depth_cases():
    rng = np.random.default_rng(17)
    eye = np.eye(4)
    c, s = np.cos(0.3), np.sin(0.3)
    turned = np.array([[c, 0, s, 0.2], [0, 1, 0, -0.1], [-s, 0, c, 0.4], [0, 0, 0, 1.0]])   # world -> camera of a turned, shifted camera
    inside = lambda n, z=3.0: np.column_stack([rng.uniform(-0.5, 0.5, n), rng.uniform(-0.4, 0.4, n), np.full(n, z)])
    cases = []
    for n in (0, 1, 63, 64, 65, 5000):
        cases.append(("front_%d" % n, rng.uniform(-1.5, 1.5, (n, 3)) + [0.0, 0.0, 3.0], turned))
    cases.append(("all_behind", rng.uniform(-1, 1, (200, 3)) - [0.0, 0.0, 3.0], eye))
    half = np.concatenate([inside(32), inside(32) + [40.0, 0.0, 0.0]])          # 32 inside, 32 in front but far outside: ratio 0.5
    cases.append(("exactly_half_inside", half[rng.permutation(64)], eye))
    cases.append(("one_less_than_half", np.concatenate([inside(31), inside(33) + [40.0, 0.0, 0.0]]), eye))
    cases.append(("just_over_max_depth", inside(70, 10.0 + 1e-9), eye))
    cases.append(("just_under_max_depth", inside(70, 10.0 - 1e-9), eye))
    # u = (64 x + 48 z) / z: x = -1.5, z = 2 gives exactly 0 (inside), x = 1.5 exactly W (outside); half of the cloud each
    cases.append(("on_u0_and_uW", np.array([[-1.5, 0.0, 2.0]] * 3 + [[1.5, 0.0, 2.0]] * 3), eye))
    cases.append(("big_mixed", np.concatenate([rng.uniform(-3, 3, (4000, 3)) + [0.0, 0.0, 1.0], inside(3000, 5.0)]), turned))
    return cases


def check_depths(L):
    from holoagent_amd._lib import points_view_depths
    cases = _depth_cases()
    clouds = [c for _, c, _ in cases]
    poses = np.stack([p for _, _, p in cases])
    avg, vis, md = points_view_depths(clouds, poses, [W_, H_], K_, lib_=L)
    want = {}
    for i, (name, c, p) in enumerate(cases):
        rv, rd = ref_check_object_in_view(W_, H_, K_, p, c)
        ra = ref_avg_distance(c, p)
        want[name] = (rv, rd, ra)
        assert bool(vis[i]) == bool(rv), name
        assert np.isfinite(md[i]) == np.isfinite(rd) and (np.isfinite(rd) or md[i] == np.inf), name
        if np.isfinite(rd):
            np.testing.assert_allclose(md[i], rd, rtol=1e-13, atol=0, err_msg=name)
        assert np.isnan(avg[i]) == np.isnan(ra), name
        if not np.isnan(ra):
            np.testing.assert_allclose(avg[i], ra, rtol=1e-13, atol=0, err_msg=name)
    # the cases are what their names say
    assert want["front_0"] == (False, np.inf, want["front_0"][2]) and np.isnan(want["front_0"][2])
    assert want["all_behind"][:2] == (False, np.inf) and np.isnan(want["all_behind"][2])
    assert want["exactly_half_inside"][0] and not want["one_less_than_half"][0] and np.isfinite(want["one_less_than_half"][2])
    assert not want["just_over_max_depth"][0] and np.isfinite(want["just_over_max_depth"][1]) and want["just_under_max_depth"][0]
    assert want["on_u0_and_uW"][0] and want["on_u0_and_uW"][1] == 2.0
    assert want["front_5000"][0] or np.isfinite(want["front_5000"][2])
    # the same input again: the same bits
    avg2, vis2, md2 = points_view_depths(clouds, poses, [W_, H_], K_, lib_=L)
    assert avg.tobytes() == avg2.tobytes() and md.tobytes() == md2.tobytes() and np.array_equal(vis, vis2)
    # other thresholds than the defaults reach the kernel
    _, v3, _ = points_view_depths(clouds, poses, [W_, H_], K_, min_visible_ratio=0.51, max_depth=10.0 + 1e-8, lib_=L)
    names = [n for n, _, _ in cases]
    assert not v3[names.index("exactly_half_inside")] and v3[names.index("just_over_max_depth")]
    # no pair at all
    a0, v0, m0 = points_view_depths([], np.zeros((0, 16)), np.zeros((0, 2), np.int32), K_, lib_=L)
    assert len(a0) == 0 and len(v0) == 0 and len(m0) == 0


_emu = pytest.mark.skipif(not os.path.exists(PC.EMU_PATH), reason="kernel simulator not built")


@_emu
@pytest.mark.parametrize("D", [512, 1])
def test_rematch_in_views_emu(D):
    from holoagent_amd._lib import HmsgLib
    check_rematch(HmsgLib(PC.EMU_PATH), D, seed=23)


@_emu
def test_points_view_depths_emu():
    from holoagent_amd._lib import HmsgLib
    check_depths(HmsgLib(PC.EMU_PATH))


@pytest.mark.gpu
@pytest.mark.parametrize("D", [512, 1])
def test_rematch_in_views_gpu(D):
    from holoagent_amd._lib import HmsgLib
    check_rematch(HmsgLib(), D, seed=23)


@pytest.mark.gpu
def test_points_view_depths_gpu():
    from holoagent_amd._lib import HmsgLib
    check_depths(HmsgLib())
