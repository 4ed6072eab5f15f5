"""hmsg_eval_rooms (include/hmsg.h; holoagent_amd/csrc/hmsg_eval.hip: k_evr_keys, k_evr_heads, k_evr_walk, k_evr_flatten, k_evr_same)
against the literal restatement of evaluate_rooms' two loop nests (tests/eval_reference.py::room_matrices: the loops of
hm3dsem_evaluator.py:278-341 with oracle.hmsg_oracle.o3d_voxel_down_sample, tests.overlap_cases.brute_f32 for the faiss form and
scipy's cKDTree for the share).  The three matrices must be equal BIT FOR BIT.

What the cases are meant to contain is asserted on the restatement, not on the library: ground-truth versions that differ between
visits, a room visited under two floors, flattened y values that are not min_height, a share above 1.

Simulator here; tests/test_eval_rooms_gpu.py runs the same checks on the library (host arrays and torch device tensors)."""
import os

import numpy as np
import pytest

from tests import eval_reference as R
from tests import parity_common as PC

HMSG_ERR_INVALID = -1
SWITCH = "HMSG_DEBUG_EVAL_ROOMS_PER_PAIR"


class Hook:
    def __init__(self, L, wrap=None):
        from holoagent_amd._lib import Scene
        self.L, self.wrap = L, wrap or (lambda a: a)
        self.scene = Scene(lib_=L, height=8, width=8, max_frames=1, max_masks=1, feat_dim=16, overlap_distance_form=0)

    def close(self):
        self.scene.close()

    def matrices(self, c, voxel=0.05, radius=0.05):
        pp, po = csr(c["pred"])
        gp, go = csr(c["gt"])
        f = lambda k: self.wrap(np.ascontiguousarray(c[k], np.float64))
        before = pp.copy()
        out = self.scene.eval_rooms(self.wrap(pp), self.wrap(po), f("zl"), f("ht"), self.wrap(gp), self.wrap(go), f("min_h"), f("max_h"), f("mean_h"),
                                    f("lower"), f("upper"), voxel, radius)
        assert np.array_equal(before, pp), "the predicted clouds were written to"
        return out


def csr(clouds):
    off = np.zeros(len(clouds) + 1, np.int64)
    off[1:] = np.cumsum([len(c) for c in clouds])
    pts = np.concatenate([np.asarray(c, np.float64).reshape(-1, 3) for c in clouds] + [np.zeros((0, 3))])
    return np.ascontiguousarray(pts), off


def reference(c, voxel=0.05, radius=0.05):
    return R.room_matrices(c["pred"], c["zl"], c["ht"], c["gt"], c["min_h"], c["max_h"], c["mean_h"], c["lower"], c["upper"], voxel, radius)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.int64), np.ascontiguousarray(b).view(np.int64))


def check(hk, c, voxel=0.05, radius=0.05):
    want = reference(c, voxel, radius)
    got = hk.matrices(c, voxel, radius)
    for name, g, w in zip(("assoc", "over_pred", "over_gt"), got[:3], want[:3]):
        assert same_bits(g, w), (name, np.argwhere(g != w)[:5].tolist(), g[g != w][:5].tolist(), w[g != w][:5].tolist())
    return got, want


def rect(rng, n, x0, x1, z0, z1, y0, y1, pitch=None):
    """n points in a box; pitch: snapped to a lattice of that pitch in x and z (piles of points per voxel)"""
    p = np.stack([rng.uniform(x0, x1, n), rng.uniform(y0, y1, n), rng.uniform(z0, z1, n)], 1)
    if pitch:
        p[:, 0] = np.round(p[:, 0] / pitch) * pitch
        p[:, 2] = np.round(p[:, 2] / pitch) * pitch
    return p


def storey_scene(seed, P, G, shift=(0.0, 0.0, 0.0), n_pred=1500, n_gt=1200):
    """two storeys (0 .. 3 and 3 .. 6 m), G ground-truth rooms side by side (bev clouds at their floor height, 3 cm jittered pitch:
    down-sampling them twice changes them), P predicted rooms that overlap them partly"""
    rng = np.random.default_rng(seed)
    shift = np.asarray(shift, np.float64)
    gt, min_h, max_h, mean_h, pred, zl, ht = [], [], [], [], [], [], []
    for g in range(G):
        level = 3.0 * (g % 2)
        x0 = 4.0 * (g // 2)
        h0 = level + float(rng.uniform(0.0, 0.2))
        gt.append(rect(rng, n_gt, x0, x0 + 3.5, 0.0, 3.0, h0, h0) + rng.normal(0, 0.004, (n_gt, 3)) * [1, 0, 1] + shift)
        min_h.append(h0 + shift[1])
        max_h.append(h0 + 2.6 + shift[1])
        mean_h.append(h0 + 1.3 + shift[1])
    for p in range(P):
        level = 3.0 * (p % 2)
        x0 = 4.0 * ((p // 2) % max(1, (G + 1) // 2)) + float(rng.uniform(-1.0, 1.0))
        z = float(level + rng.uniform(0.1, 0.3))
        pred.append(rect(rng, n_pred, x0, x0 + 3.0, 0.3, 2.8, z, z + 2.4, pitch=(0.02 if p % 3 == 0 else None)) + shift)
        zl.append(z + shift[1])
        ht.append(2.4)
    lower, upper = np.array([-0.5, 2.9]) + shift[1], np.array([2.9, 6.5]) + shift[1]
    return dict(pred=pred, zl=np.array(zl), ht=np.array(ht), gt=gt, min_h=np.array(min_h), max_h=np.array(max_h), mean_h=np.array(mean_h),
                lower=lower, upper=upper)


def lattice_room():
    """the issue's lattice: 150 x 100 points of 2 cm pitch from (1.003, 0.3, -2.001)"""
    ix, iz = np.meshgrid(np.arange(150), np.arange(100), indexing="ij")
    return np.stack([1.003 + 0.02 * ix.ravel(), np.full(ix.size, 0.3), -2.001 + 0.02 * iz.ravel()], 1)


# ---- the cases
def versions_differ(hk):
    """one ground-truth room (the 2 cm lattice) visited by three predicted rooms: loop 1 reads vds^1 .. vds^3, loop 2 vds^4 .. vds^6"""
    rng = np.random.default_rng(3)
    gt = lattice_room()
    sizes = [len(gt)]
    v = gt
    for _ in range(3):
        v = R.vds(v, 0.05)
        sizes.append(len(v))
    assert sizes == [15000, 2501, 2400, 2400], sizes
    pred = [rect(rng, 1200, 0.8 + 0.4 * p, 3.0 + 0.3 * p, -2.2, 0.2, 0.4, 2.5) for p in range(3)]
    c = dict(pred=pred, zl=np.full(3, 0.4), ht=np.full(3, 2.1), gt=[gt], min_h=np.array([0.3]), max_h=np.array([2.9]), mean_h=np.array([1.6]),
             lower=np.array([0.0]), upper=np.array([3.0]))
    got, want = check(hk, c)
    assert want[3].tolist() == [3] and got[3] == 3
    assert (want[0] > 0).all() and len(set(want[0].ravel().tolist())) == 3
    # the versions matter: with the first version everywhere the first loop's later cells differ
    first = R.vds(gt, 0.05)
    flat = np.array(pred[2])
    flat[:, 1] = 0.3
    assert R.overlapping_ratio_faiss(R.vds(flat, 0.05), first, 0.05) != want[0][2, 0]


def two_floors(hk):
    """a room whose mean height lies inside two floors: visited under both, the later visit (later versions) keeps the cell"""
    c = storey_scene(5, 3, 2, n_pred=900, n_gt=800)
    c["lower"], c["upper"] = np.array([-0.5, 1.0]), np.array([2.0, 6.5])       # room 0 (mean about 1.4) lies in both
    assert ((c["mean_h"][0] > c["lower"]) & (c["mean_h"][0] < c["upper"])).all()
    got, want = check(hk, c)
    assert want[3].tolist() == [4, 1] and (want[0][:, 0] > 0).sum() == 2


def strict_gates(hk):
    """gates exactly ON min_height, max_height, lower and upper are excluded"""
    c = storey_scene(7, 5, 4, n_pred=600, n_gt=600)
    c["zl"][0], c["ht"][0] = c["min_h"][0], 0.0   # pred 0 sits exactly on room 0's min_height
    c["zl"][2], c["ht"][2] = c["max_h"][2], 0.0   # pred 2 exactly on room 2's max_height
    c["lower"][1] = c["mean_h"][1]               # room 1 exactly on the second floor's lower bound
    c["upper"][1] = c["mean_h"][3]               # room 3 exactly on its upper bound
    assert c["zl"][0] + c["ht"][0] / 2 == c["min_h"][0] and c["zl"][2] + c["ht"][2] / 2 == c["max_h"][2]
    got, want = check(hk, c)
    assert want[0][0, 0] == 0 and want[0][2, 2] == 0 and (want[0][:, 1] == 0).all() and (want[0][:, 3] == 0).all()
    base = reference(storey_scene(7, 5, 4, n_pred=600, n_gt=600))
    assert base[0][0, 0] > 0 and base[0][2, 2] > 0 and (base[0][:, 1] > 0).any() and (base[0][:, 3] > 0).any(), "the gates decide nothing here"
    assert want[0][4, 0] > 0                    # (a fifth predicted room, off every bound, still counts)


def flattened_y(hk):
    """voxels of 7 and more points with min_h = 0.1 + 0.2: the flattened y is (h + ... + h) / k, not h"""
    rng = np.random.default_rng(9)
    h = 0.1 + 0.2
    pile = np.tile([[1.26, 1.0, 0.73]], (7, 1)) + rng.uniform(-0.004, 0.004, (7, 3))
    pred = [np.concatenate([pile, rect(rng, 1500, 0.0, 0.6, 0.0, 0.5, 0.5, 2.0, pitch=0.01), rect(rng, 300, 0.6, 2.0, 0.0, 1.5, 0.5, 2.0)])]
    flat = np.array(pred[0])
    flat[:, 1] = h
    ys = R.vds(flat, 0.05)[:, 1]
    assert (ys != h).sum() >= 10 and (ys == h).sum() >= 10
    s = 0.0
    for _ in range(7):
        s += h
    assert s / 7 != h
    gt = [rect(rng, 1500, 0.0, 2.0, 0.0, 1.5, h, h)]
    c = dict(pred=pred, zl=np.array([0.5]), ht=np.array([1.5]), gt=gt, min_h=np.array([h]), max_h=np.array([2.7]), mean_h=np.array([1.5]),
             lower=np.array([0.0]), upper=np.array([3.0]))
    check(hk, c)


def small_rooms(hk):
    """an empty predicted room, one of one point (between four ground-truth voxels: a share above 1, cut to 1), a ground-truth room of
    one point and an empty one"""
    rng = np.random.default_rng(11)
    ix, iz = np.meshgrid(np.arange(40), np.arange(40), indexing="ij")
    grid = np.stack([0.05 * ix.ravel() + 0.025, np.full(ix.size, 0.2), 0.05 * iz.ravel() + 0.025], 1)
    one = np.array([[1.0, 1.3, 1.0]])                                        # 3.5 cm from four sites of the grid
    pred = [np.zeros((0, 3)), one, rect(rng, 800, 0.0, 2.0, 0.0, 2.0, 0.3, 2.0)]
    gt = [grid, np.array([[1.01, 0.2, 0.99]]), np.zeros((0, 3))]
    c = dict(pred=pred, zl=np.full(3, 0.3), ht=np.full(3, 2.0), gt=gt, min_h=np.full(3, 0.2), max_h=np.full(3, 2.8), mean_h=np.full(3, 1.5),
             lower=np.array([0.0]), upper=np.array([3.0]))
    flat = one.copy()
    flat[:, 1] = 0.2
    assert R.intersection_share(R.vds(R.vds(grid, 0.05), 0.05), flat, 0.05) > 1
    got, want = check(hk, c)
    assert (want[0][0] == 0).all() and (want[1][0] == 0).all() and (want[2][0] == 0).all()        # the empty predicted room
    assert want[1][1, 0] == 1.0 and 0 < want[2][1, 0] < 1
    assert (want[0][:, 2] == 0).all() and want[0][1, 1] == 1.0
    assert got[3] == 9


def far_from_the_origin(hk):
    check(hk, storey_scene(13, 3, 3, shift=(50.0, -12.0, -47.0), n_pred=900, n_gt=900))


def one_by_one(hk):
    got, want = check(hk, storey_scene(17, 1, 1))
    assert want[0][0, 0] > 0


def six_by_five(hk):
    got, want = check(hk, storey_scene(19, 6, 5, n_pred=1000, n_gt=1000))
    assert (want[0] > 0).sum() >= 8 and (want[0] == 0).sum() >= 8 and got[3] == int((want[3]).sum())
    # other voxel size and radius
    check(hk, storey_scene(19, 6, 5, n_pred=500, n_gt=500), voxel=0.08, radius=0.11)


def debug_switch(hk):
    """per-pair down-sampling of the whole flattened cloud gives the same bits"""
    c = storey_scene(23, 4, 3, n_pred=900, n_gt=700)
    a = hk.matrices(c)
    assert os.environ.get(SWITCH) is None
    os.environ[SWITCH] = "1"
    try:
        b = hk.matrices(c)
        check(hk, c)
    finally:
        del os.environ[SWITCH]
    assert all(same_bits(x, y) for x, y in zip(a[:3], b[:3])) and a[3] == b[3] and (a[0] > 0).any()


def raw(hk, c, voxel=0.05, radius=0.05, P=None, G=None, po=None, go=None):
    pp, po0 = csr(c["pred"])
    gp, go0 = csr(c["gt"])
    po, go = (po0 if po is None else po), (go0 if go is None else go)
    P, G = (len(po) - 1 if P is None else P), (len(go) - 1 if G is None else G)
    out = [np.full((max(P, 1), max(G, 1)), 7.5) for _ in range(3)]
    f = lambda k: np.ascontiguousarray(c[k], np.float64)
    keep = [f(k) for k in ("zl", "ht", "min_h", "max_h", "mean_h", "lower", "upper")]
    rc = hk.L.c.hmsg_eval_rooms(hk.scene.h, P, pp.ctypes.data, po.ctypes.data, keep[0].ctypes.data, keep[1].ctypes.data, G, gp.ctypes.data,
                                go.ctypes.data, keep[2].ctypes.data, keep[3].ctypes.data, keep[4].ctypes.data, len(keep[5]), keep[5].ctypes.data,
                                keep[6].ctypes.data, float(voxel), float(radius), out[0].ctypes.data, out[1].ctypes.data, out[2].ctypes.data, None)
    return rc, out


def refusals(hk):
    c = storey_scene(29, 2, 2, n_pred=300, n_gt=300)
    rc, out = raw(hk, c)
    assert rc == 0 and all((o != 7.5).all() for o in out)
    _, po = csr(c["pred"])
    bad_start, decreasing = po.copy(), po.copy()
    bad_start[0] = 1
    decreasing[1] = po[2] + 1
    nan, inf = dict(c), dict(c)
    nan["pred"] = [c["pred"][0].copy(), c["pred"][1]]
    nan["pred"][0][5, 0] = np.nan
    inf["gt"] = [c["gt"][0], c["gt"][1].copy()]
    inf["gt"][1][7, 2] = -np.inf
    refused = [dict(P=0), dict(G=0), dict(po=bad_start), dict(po=decreasing), dict(go=bad_start), dict(voxel=0.0), dict(voxel=-0.05),
               dict(voxel=float("nan")), dict(radius=0.0), dict(radius=-1.0), dict(radius=float("inf"))]
    for kw in refused:
        rc, out = raw(hk, c, **kw)
        assert rc == HMSG_ERR_INVALID, kw
        assert all((o == 7.5).all() for o in out), ("a refused call wrote its output", kw)
        assert len(hk.L.c.hmsg_last_error(hk.scene.h)) > 0
    for bad in (nan, inf):
        rc, out = raw(hk, bad)
        assert rc == HMSG_ERR_INVALID and all((o == 7.5).all() for o in out)
    # a NaN in a predicted room that no gate lets through is refused all the same
    nan["zl"] = c["zl"] + 100.0
    assert raw(hk, nan)[0] == HMSG_ERR_INVALID
    # any output may be NULL
    pp, po = csr(c["pred"])
    gp, go = csr(c["gt"])
    only = np.full((2, 2), 7.5)
    k = [np.ascontiguousarray(c[n], np.float64) for n in ("zl", "ht", "min_h", "max_h", "mean_h", "lower", "upper")]
    rc = hk.L.c.hmsg_eval_rooms(hk.scene.h, 2, pp.ctypes.data, po.ctypes.data, k[0].ctypes.data, k[1].ctypes.data, 2, gp.ctypes.data, go.ctypes.data,
                                k[2].ctypes.data, k[3].ctypes.data, k[4].ctypes.data, 2, k[5].ctypes.data, k[6].ctypes.data, 0.05, 0.05, None,
                                only.ctypes.data, None, None)
    assert rc == 0 and same_bits(only, reference(c)[1])
    assert hk.L.c.hmsg_eval_rooms(None, 2, None, None, None, None, 2, None, None, None, None, None, 0, None, None, 0.05, 0.05, None, None, None,
                                  None) == HMSG_ERR_INVALID


CASES = dict(versions_differ=versions_differ, two_floors=two_floors, strict_gates=strict_gates, flattened_y=flattened_y, small_rooms=small_rooms,
             far_from_the_origin=far_from_the_origin, one_by_one=one_by_one, six_by_five=six_by_five, debug_switch=debug_switch, refusals=refusals)

needs_emu = pytest.mark.skipif(not os.path.exists(PC.EMU_PATH), reason="kernel simulator not built")


@pytest.fixture(scope="module")
def emu():
    from holoagent_amd._lib import HmsgLib
    hk = Hook(HmsgLib(PC.EMU_PATH))
    yield hk
    hk.close()


@needs_emu
@pytest.mark.parametrize("case", list(CASES))
def test_eval_rooms_simulator(emu, case):
    CASES[case](emu)
