"""hmsg_eval_semantic_ranks (include/hmsg.h; holoagent_amd/csrc/hmsg_eval.hip: k_evs_ranks) against a float64 numpy model
(tests/eval_reference.py::semantic_ranks): the rank of the ground-truth category among the classes by cosine similarity, in the order of
np.argsort(kind="stable")[::-1].

The kernel sums in float32 in its own order, so the inputs are BUILT such that every class of another name differs from a target
class's cosine by more than 1e-3 in float64 -- a condition the test asserts itself, not a tolerance: the worst-case error of a
float32 dot product of normalised rows is 2 (D + 2) 2^-24, about 1.2e-4 for D <= 1024 -- or is a row of the same bits as the target's
(an exact tie, decided by the index).  The table has controlled cosines against two orthogonal directions; the embeddings are
positive multiples of either.

Simulator here; tests/test_eval_semantics_gpu.py runs the same checks on the library (host arrays and torch device tensors)."""
import os

import numpy as np
import pytest

from tests import eval_reference as R
from tests import parity_common as PC

HMSG_ERR_INVALID = -1
SHAPES = [(8, 3, 1), (8, 40, 33), (8, 1030, 1), (512, 3, 33), (512, 40, 33), (512, 1030, 1)]          # (D, C, n)


class Hook:
    def __init__(self, L, wrap=None):
        from holoagent_amd._lib import Scene
        self.L, self.wrap = L, wrap or (lambda a: a)
        self.scene = Scene(lib_=L, height=8, width=8, max_frames=1, max_masks=1, feat_dim=16)

    def close(self):
        self.scene.close()

    def ranks(self, emb, text, names, target):
        w = self.wrap
        return self.scene.eval_semantic_ranks(w(np.ascontiguousarray(emb)), w(np.ascontiguousarray(text, np.float32)),
                                              w(np.ascontiguousarray(names, np.int32)), w(np.ascontiguousarray(target, np.int32)))


def table(D, C, n, seed, n_ties=0, n_dup_names=0):
    """-> emb float32 [n][D], text float32 [C][D], class_name_id [C], target_name_id [n]"""
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.normal(size=(D, D)))
    e1, e2, rest = q[:, 0], q[:, 1], q[:, 2:]
    grid = np.linspace(-0.65, 0.65, C) if C > 1 else np.zeros(1)
    a, b = grid[rng.permutation(C)], grid[rng.permutation(C)]
    u = rng.normal(size=(C, D - 2))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    text = (a[:, None] * e1 + b[:, None] * e2 + np.sqrt(1 - a * a - b * b)[:, None] * (u @ rest.T)) * rng.uniform(0.5, 3.0, (C, 1))
    text = text.astype(np.float32)
    names = np.arange(C, dtype=np.int32)
    for _ in range(n_ties):                                  # rows of the same bits under different names: exact ties
        i, j = rng.choice(C, 2, replace=False)
        text[j] = text[i]
    for _ in range(n_dup_names):                             # one name on two classes: the better of the two counts
        i, j = rng.choice(C, 2, replace=False)
        names[j] = names[i]
    emb = (np.where(rng.random(n) < 0.5, 1.0, 0.0)[:, None] * (e1 - e2) + e2) * rng.uniform(0.2, 5.0, (n, 1))
    target = names[rng.integers(0, C, n)].astype(np.int32)
    return emb.astype(np.float32), text, names, target


def separated(emb, text, names, target):
    """the condition the comparison rests on; -> the model's ranks"""
    rank, sims = R.semantic_ranks(emb, text, names, target)
    for s, t in zip(sims, target):
        for c in np.flatnonzero(names == t):
            other = names != t
            same_row = (text == text[c]).all(1)
            gap = np.abs(s[other & ~same_row] - s[c])
            gap = gap[np.isfinite(gap)]                      # (NaN of a zero row: ordered by rule, not by value)
            assert gap.size == 0 or gap.min() > 1e-3, gap.min()
    return rank


def shapes(hk, D, C, n):
    emb, text, names, target = table(D, C, n, seed=D + C + n, n_ties=(0 if C < 10 else 3), n_dup_names=(0 if C < 10 else 2))
    want = separated(emb, text, names, target)
    got = hk.ranks(emb, text, names, target)
    assert np.array_equal(got, want), (got.tolist(), want.tolist())
    if n > 1 and C > 3:
        assert len(set(want.tolist())) > min(n, C) // 3        # the ranks are spread over the table
    # float64 embeddings are cast to float32 first
    got64 = hk.ranks(emb.astype(np.float64), text, names, target)
    assert np.array_equal(got64, want)


def ties_and_names(hk):
    """exact ties of bit-identical rows follow the stable argsort read from its end (the HIGHER index first); a name on two classes
    takes the better rank; a target that no class carries, or -1, gives C"""
    D, C = 8, 40
    emb, text, names, _ = table(D, C, 1, seed=5)
    s = R.semantic_ranks(emb, text, names, [0])[1][0]
    order = np.argsort(s, kind="stable")[::-1]
    best, second, worst = int(order[0]), int(order[1]), int(order[-1])
    lo, hi = min(best, second), max(best, second)
    text2 = text.copy()
    text2[lo] = text[best]
    text2[hi] = text[best]                                     # the two best classes are now one row under two names
    for tgt, want in ((lo, 1), (hi, 0)):
        t = np.array([names[tgt]], np.int32)
        assert separated(emb, text2, names, t).tolist() == [want]
        assert hk.ranks(emb, text2, names, t).tolist() == [want]
    dup = names.copy()
    dup[worst] = names[best]                                   # the worst class carries the best one's name
    for tgt in (best, worst):
        t = np.array([dup[tgt]], np.int32)
        assert separated(emb, text, dup, t).tolist() == [0] and hk.ranks(emb, text, dup, t).tolist() == [0]
    for t in (-1, 1000):
        assert hk.ranks(emb, text, names, np.array([t], np.int32)).tolist() == [C]
    # a table of one name: rank 0 whatever the embedding
    assert hk.ranks(emb, text, np.zeros(C, np.int32), np.array([0], np.int32)).tolist() == [0]


def zero_norm(hk):
    """a row of norm zero gives NaN similarities, ordered as numpy sorts them (include/hmsg.h): above every number, ties by index"""
    D, C = 8, 40
    emb, text, names, _ = table(D, C, 3, seed=9)
    target = np.array([4, 17, 39], np.int32)
    zero = np.zeros_like(emb)
    want = R.semantic_ranks(zero, text, names, target)[0]
    assert want.tolist() == [C - 1 - 4, C - 1 - 17, 0]
    assert hk.ranks(zero, text, names, target).tolist() == want.tolist()
    text0 = text.copy()
    text0[11] = 0.0                                            # a zero class: first for every embedding
    tg = np.array([11, 4, 17], np.int32)
    want = separated(emb, text0, names, tg)
    plain = R.semantic_ranks(emb, text, names, tg)[0]
    assert want[0] == 0 and (want[1:] >= plain[1:]).all() and (want[1:] <= plain[1:] + 1).all()
    assert hk.ranks(emb, text0, names, tg).tolist() == want.tolist()


def refusals(hk):
    emb, text, names, target = table(8, 3, 2, seed=1)
    rank = np.full(2, 77, np.int32)
    f = hk.L.c.hmsg_eval_semantic_ranks
    h = hk.scene.h
    args = lambda: (emb.ctypes.data, 0, 8, 3, text.ctypes.data, names.ctypes.data, target.ctypes.data, rank.ctypes.data)
    assert f(h, 2, *args()) == 0 and (rank != 77).all()
    rank[:] = 77
    assert f(None, 2, *args()) == HMSG_ERR_INVALID
    assert f(h, -1, *args()) == HMSG_ERR_INVALID
    assert f(h, 2, emb.ctypes.data, 0, 0, 3, text.ctypes.data, names.ctypes.data, target.ctypes.data, rank.ctypes.data) == HMSG_ERR_INVALID
    assert f(h, 2, emb.ctypes.data, 0, 8, 0, text.ctypes.data, names.ctypes.data, target.ctypes.data, rank.ctypes.data) == HMSG_ERR_INVALID
    assert f(h, 2, None, 0, 8, 3, text.ctypes.data, names.ctypes.data, target.ctypes.data, rank.ctypes.data) == HMSG_ERR_INVALID
    assert f(h, 2, emb.ctypes.data, 0, 8, 3, None, names.ctypes.data, target.ctypes.data, rank.ctypes.data) == HMSG_ERR_INVALID
    assert (rank == 77).all() and len(hk.L.c.hmsg_last_error(h)) > 0
    assert f(h, 0, None, 0, 8, 3, text.ctypes.data, names.ctypes.data, None, None) == 0


needs_emu = pytest.mark.skipif(not os.path.exists(PC.EMU_PATH), reason="kernel simulator not built")


@pytest.fixture(scope="module")
def emu():
    from holoagent_amd._lib import HmsgLib
    hk = Hook(HmsgLib(PC.EMU_PATH))
    yield hk
    hk.close()


@needs_emu
@pytest.mark.parametrize("D,C,n", SHAPES)
def test_shapes_simulator(emu, D, C, n):
    shapes(emu, D, C, n)


@needs_emu
def test_ties_and_names_simulator(emu):
    ties_and_names(emu)


@needs_emu
def test_zero_norm_simulator(emu):
    zero_norm(emu)


@needs_emu
def test_refusals_simulator(emu):
    refusals(emu)
