"""Label propagation's round order (pool_cluster, hmsg_pool.hip): the open-row list is built behind the FIRST round, the second
round runs over it with the count still on the device, the later ones over the same list sized by the host.  The sets below are the
ones that order can get wrong and tests/test_feats_dbscan_exact.py does not single out; they go through hmsg_denoise_feats_batch in
ONE batch, against the exact integer reference of tests/dbscan_cases.py (n_in_cluster exactly, the representative bit for bit).

  last core     a set whose only -- hence lowest -- core row is its last row
  no core       a set without a core row, next to a dense one
  one round     a set that is finished after the first round (every core row adjacent to the lowest one), next to a 400-hop chain
  interleaved   two chains of many rounds side by side, their sizes no multiple of 64: one wave of the listing kernel holds open
                rows of both, and both sets' rows stay in the list for many rounds

What a set is there for is asserted on the integer model before anything runs."""
import os

import numpy as np
import pytest

from tests import dbscan_cases as DC
from tests import parity_common as PC

needs_emu = pytest.mark.skipif(not os.path.exists(PC.EMU_PATH), reason="kernel simulator not built")
D, EPS, M, MS = 16, 1e-4, 3, 3


def after_first_round(case):
    """labels behind the first round and its pointer jumping, on the model: a core row takes its smallest core neighbour below
    itself, then follows the chain of labels to its end.  -> (labels of the core rows, lowest core row)"""
    e = case.expect(MS)
    cores = np.flatnonzero(e.core)
    lab = np.arange(len(case.X))
    for i in cores:
        nb = np.flatnonzero(case.adj[i] & e.core)
        lab[i] = min(int(nb.min()), i)
    for i in cores:
        while lab[lab[i]] < lab[i]:
            lab[i] = lab[lab[i]]
    return lab[cores], (int(cores[0]) if len(cores) else -1)


def chain(rng, n_draw, dt):
    """one chain on one plane, rows permuted, row 0 next to the chain's end: the label 0 has the whole way to go"""
    _, pmax = DC.lattice_limits(EPS, M)
    pos = np.cumsum(rng.choice([1, 2, 3], n_draw, p=[0.05, 0.1, 0.85]))
    pos = pos[pos <= pmax]
    o = rng.permutation(len(pos))
    at = int(np.flatnonzero(o == 1)[0])
    o[0], o[at] = o[at], o[0]
    return DC.lattice_from_model(rng, np.zeros(len(pos), np.int64), pos[o], D, EPS, M, dt)


def round_sets(dt):
    """-> [(case, what)] in batch order"""
    rng = np.random.default_rng(123)
    out = []
    # the only core row is the last one: position 3 sees 0 and 6 (three rows with itself), they see two; isolated rows in front
    pos = [20, 30, 40, 50, 0, 6, 3]
    c = DC.lattice_from_model(rng, [0] * len(pos), pos, D, EPS, M, dt)
    e = c.expect(MS)
    assert list(np.flatnonzero(e.core)) == [len(pos) - 1] and e.n_in_cluster == 3
    out.append((c, "lowest core row is the last row"))
    # no core row at all (every row alone), then a dense set: every row a core row and adjacent to every other
    c = DC.lattice_from_model(rng, [0] * 45, list(7 * np.arange(45)), D, EPS, M, dt)
    assert not c.expect(MS).core.any() and c.expect(MS).n_in_cluster == 0
    out.append((c, "no core row"))
    c = DC.lattice_from_model(rng, [0] * 100, list(rng.integers(0, 3, 100)), D, EPS, M, dt)
    assert c.expect(MS).core.all() and c.adj.all()
    out.append((c, "dense"))
    # a 400-hop chain, and next to it a set that the first round finishes: a dense group behind three rows that are not core rows
    c = chain(rng, 700, dt)
    assert DC.hops(c, MS) >= 400 and c.expect(MS).n_clusters == 1
    lab, lowest = after_first_round(c)
    assert (lab != lowest).sum() > 100                                # most of it is still open behind the first round
    out.append((c, "chain of 400 hops"))
    c = DC.lattice_from_model(rng, [0] * 73, [40, 60, 80] + list(rng.integers(0, 4, 70)), D, EPS, M, dt)
    lab, lowest = after_first_round(c)
    assert lowest == 3 and len(lab) == 70 and (lab == lowest).all()
    out.append((c, "finished after the first round"))
    # two chains side by side, 64 dividing neither their sizes nor the row offset between them
    a, b = chain(rng, 190, dt), chain(rng, 230, dt)
    for c in (a, b):
        lab, lowest = after_first_round(c)
        assert DC.hops(c, MS) >= 50 and (lab != lowest).sum() > 30 and len(c.X) % 64 != 0
        out.append((c, "interleaved chains"))
    assert sum(len(c.X) for c, _ in out[:-1]) % 64 != 0
    return out


def check_rounds(L):
    from tests.test_feats_dbscan_exact import assert_exact, pack, raw_batch
    for dt in (np.float32, np.float64):
        sets = round_sets(dt)
        X, off = pack([c for c, _ in sets], range(len(sets)), 0)
        rep, ncl = raw_batch(L, X, off, EPS, MS)
        for k, (c, what) in enumerate(sets):
            assert_exact(rep[k], ncl[k], c, MS, what)


def test_sets_hold_what_they_are_for():
    assert len(round_sets(np.float64)) == 7


@needs_emu
def test_rounds_on_the_simulator():
    from holoagent_amd._lib import HmsgLib
    check_rounds(HmsgLib(PC.EMU_PATH))


@pytest.mark.gpu
def test_rounds_gpu():
    from holoagent_amd._lib import HmsgLib
    check_rounds(HmsgLib())
