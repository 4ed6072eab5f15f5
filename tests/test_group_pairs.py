"""The candidate pairs of a level batch of the hierarchical merge (hmsg_set_merge_tree_batch): the two pair kernels behind
hmsg_test_group_pairs against the same float64 expression (bbox_iou, graph_utils.py:883-915, as the host's pair loop evaluates
it) written in numpy here.  The list must be equal in content AND order: ascending (i, j), pairs inside a group only.  The CPU
form runs on the kernel simulator, the same cases marked `gpu` on the library."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import parity_common as PC

SIZES = [0, 1, 2, 65, 300]          # an empty group, a lone box, one pair, past a wave, past a 256-wide tile


def ref_pairs(boxes, group_off, th):
    """(i, j), i < j, of one group, with `iou > th`: the host's early reject, then ov / (va + vb - ov) in its order of operations;
    np.where spells the selections out as the comparisons std::max / std::min make (0/0 -> NaN -> not a pair)."""
    out = []
    mn, mx = boxes[:, :3], boxes[:, 3:]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for g in range(len(group_off) - 1):
            a0, a1 = int(group_off[g]), int(group_off[g + 1])
            for i in range(a0, a1 - 1):
                bmn, bmx = mn[i + 1:a1], mx[i + 1:a1]
                amn, amx = mn[i][None], mx[i][None]
                reject = ((amx <= bmn) | (bmx <= amn)).any(axis=1)
                ov, va, vb = np.ones(len(bmn)), np.ones(len(bmn)), np.ones(len(bmn))
                for k in range(3):
                    omin = np.where(amn[:, k] < bmn[:, k], bmn[:, k], amn[:, k])
                    omax = np.where(bmx[:, k] < amx[:, k], bmx[:, k], amx[:, k])
                    d = omax - omin
                    ov = ov * np.where(d < 0.0, 0.0, d)
                    va = va * (amx[:, k] - amn[:, k])
                    vb = vb * (bmx[:, k] - bmn[:, k])
                iou = ov / (va + vb - ov)
                hit = ~reject & (iou > th)
                out += [(i, i + 1 + int(q)) for q in np.nonzero(hit)[0]]
    return np.array(out, np.int32).reshape(-1, 2)


def iou_of(a, b):
    """the same expression for ONE pair, as a float64 (NaN for 0/0)"""
    mn = np.stack([a[:3], b[:3]])
    mx = np.stack([a[3:], b[3:]])
    if ((mx[0] <= mn[1]) | (mx[1] <= mn[0])).any():
        return 0.0
    ov = va = vb = np.float64(1.0)
    for k in range(3):
        omin = mn[1, k] if mn[0, k] < mn[1, k] else mn[0, k]
        omax = mx[1, k] if mx[1, k] < mx[0, k] else mx[0, k]
        d = omax - omin
        ov = ov * (np.float64(0.0) if d < 0.0 else d)
        va = va * (mx[0, k] - mn[0, k])
        vb = vb * (mx[1, k] - mn[1, k])
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.float64(ov) / (va + vb - ov)


def make_case(th):
    rng = np.random.Generator(np.random.PCG64(20))
    groups = []
    for m in SIZES:
        # boxes of a room: corners on a 1 cm lattice, so faces that touch (mx == mn) and identical boxes do occur
        lo = np.round(rng.uniform(0.0, 3.0, (m, 3)), 2)
        ext = np.round(rng.uniform(0.0, 1.5, (m, 3)), 2)
        b = np.concatenate([lo, lo + ext], axis=1)
        if m >= 65:
            b[5] = b[4]                                   # identical boxes
            b[7] = b[6]
            b[8, 3:] = b[8, :3]                           # a point: zero volume
            b[9] = b[8]                                   # ... twice: 0/0
            b[10, 5] = b[10, 2]                           # a flat box inside whatever it meets
            b[11] = [1.0, 1.0, 1.0, 2.0, 2.0, 2.0]
            b[12] = [2.0, 1.0, 1.0, 3.0, 2.0, 2.0]        # touches [11] on a face
            b[13] = [1.0, 2.0, 1.0, 2.0, 3.0, 2.0]
            b[14] = [1e300, 1e300, 1e300, -1e300, -1e300, -1e300]      # how the merge hands an empty cloud over
        if m == 300:
            b[60:260] = b[60]                             # 200 identical boxes across the tile edge: 19900 pairs of one row range
        groups.append(b)
    # pairs placed around the threshold: b = a slab of the unit cube a, IoU = its thickness t up to rounding; t one ulp below
    # th, at th, one ulp above, and a little further out.  Only cases whose numpy IoU is strictly off the threshold stay.
    a = np.array([0.0, 0.0, 0.0, 1.0, 1.0, 1.0])
    kept = 0
    base = th if th > 0.0 else 0.0
    ts = [base]
    for _ in range(3):
        ts = [np.nextafter(ts[0], -1.0)] + ts + [np.nextafter(ts[-1], 2.0)]
    ts += [base * (1.0 - 1e-9), base * (1.0 + 1e-9), base + 1e-300, base + 1e-12]
    for shift in (0.0, 0.25, 3.0):
        for t in ts:
            if t < 0.0:
                continue
            b = np.array([0.0, 0.0, shift, 1.0, 1.0, shift + t])
            a2 = a.copy()
            a2[[2, 5]] += shift
            v = iou_of(a2, b)
            if np.isnan(v) or v == th:
                continue                                  # an undefined tie is no test
            groups.append(np.stack([a2, b]))
            kept += 1
    assert kept >= (8 if th > 0.0 else 4)
    off = np.concatenate([[0], np.cumsum([len(g) for g in groups])]).astype(np.int64)
    return np.ascontiguousarray(np.concatenate(groups)), off


def run_hook(L, boxes, off, th, capacity):
    out = np.full((max(capacity, 1), 2), -7, np.int32)
    n = C.c_int64(-1)
    rc = L.c.hmsg_test_group_pairs(0, len(boxes), boxes.ctypes.data, len(off) - 1, off.ctypes.data, float(th), out.ctypes.data,
                                   capacity, C.byref(n))
    assert rc == 0
    return out, int(n.value)


def check(L, th):
    boxes, off = make_case(th)
    ref = ref_pairs(boxes, off, th)
    # GroupPairs::run (hmsg_merge.hip) lets the first fill write max(4 n, 4096) pairs and allocates twice the request at most: this
    # list is longer than either, so the truncated fill, the regrown buffer and the second fill all run
    assert len(ref) > 2 * max(4 * len(boxes), 4096) + 1
    got, n = run_hook(L, boxes, off, th, len(ref) + 5)
    assert n == len(ref)
    assert np.array_equal(got[:n], ref)
    assert (got[n:] == -7).all()
    # the near-threshold groups of two: both sides occur
    tail = ref[ref[:, 0] >= off[len(SIZES)]]
    n_tail = len(off) - 1 - len(SIZES)
    assert 0 < len(tail) and (len(tail) < n_tail or th == 0.0)     # (nothing lies strictly below a threshold of 0)
    # a short buffer gets the first pairs and the true count
    got, n = run_hook(L, boxes, off, th, 100)
    assert n == len(ref) and np.array_equal(got, ref[:100])
    got, n = run_hook(L, boxes, off, th, 0)
    assert n == len(ref)


def check_refusals(L):
    boxes = np.zeros((4, 6))
    n = C.c_int64(0)
    out = np.zeros((8, 2), np.int32)
    for off in ([0, 3], [0, 3, 2, 4], [1, 4]):            # does not end at n / descends / does not start at 0
        o = np.array(off, np.int64)
        assert L.c.hmsg_test_group_pairs(0, 4, boxes.ctypes.data, len(o) - 1, o.ctypes.data, 0.05, out.ctypes.data, 8, C.byref(n)) != 0
    o = np.array([0, 0], np.int64)                         # nothing at all
    assert L.c.hmsg_test_group_pairs(0, 0, None, 1, o.ctypes.data, 0.05, out.ctypes.data, 8, C.byref(n)) == 0 and n.value == 0


@pytest.fixture(scope="module")
def emu():
    from holoagent_amd._lib import HmsgLib
    return HmsgLib(PC.EMU_PATH)


@pytest.fixture(scope="module")
def gpu():
    from holoagent_amd._lib import HmsgLib
    return HmsgLib()


needs_emu = pytest.mark.skipif(not os.path.exists(PC.EMU_PATH), reason="kernel simulator not built")


@needs_emu
@pytest.mark.parametrize("th", [0.05, 0.0])
def test_group_pairs_equal_the_host_expression(emu, th):
    check(emu, th)


@needs_emu
def test_group_pairs_refusals(emu):
    check_refusals(emu)


@pytest.mark.gpu
@pytest.mark.parametrize("th", [0.05, 0.0])
def test_group_pairs_equal_the_host_expression_gpu(gpu, th):
    check(gpu, th)


@pytest.mark.gpu
def test_group_pairs_refusals_gpu(gpu):
    check_refusals(gpu)
