"""The room calls on the kernel simulator (include/hmsg.h, N11: hmsg_nav_room_labels, hmsg_nav_doors, hmsg_nav_path_rooms,
hmsg_nav_room_doors): every case function of tests/navrooms_cases.py (the module tests/test_navrooms_gpu.py imports too) against
the scipy restatement of tests/navrooms_reference.py, every output by array_equal; the capacities and the refusals;
NavigationGraph.room_map / doors / rooms_along on a storey and Graph.room_doors / room_graph / rooms_on_route on a scene built from
frames."""
import os

import numpy as np
import pytest

from tests import navrooms_cases as GC
from tests import navrooms_reference as GR
from tests import parity_common as PC

needs_emu = pytest.mark.skipif(not os.path.exists(PC.EMU_PATH), reason="kernel simulator not built")


@pytest.fixture(scope="module")
def emu():
    from holoagent_amd._lib import HmsgLib
    return HmsgLib(PC.EMU_PATH)


@needs_emu
@pytest.mark.parametrize("case", GC.ALL, ids=[f.__name__ for f in GC.ALL])
def test_nav_rooms_simulator(emu, case):
    case(GC.api(emu))


@needs_emu
def test_nav_rooms_capacities_simulator(emu):
    GC.capacities_too_small(emu)


@needs_emu
def test_nav_rooms_refusals_simulator(emu):
    GC.refusals(GC.api(emu), emu)


@needs_emu
def test_navigation_graph_rooms_simulator(emu):
    GC.navigation_graph_rooms(emu)


@needs_emu
def test_graph_rooms_simulator(emu, tmp_path):
    GC.graph_rooms(emu, tmp_path)


def test_the_two_forms_of_the_label_rule_agree():
    """G2's two forms restated independently (a Dijkstra per room and an argmin; one field and a pass in ascending dist) give the
    same labels on the random map with 9 rooms, ties included"""
    from tests import navroute_cases as NC
    p = NC.random_map()
    rng = np.random.default_rng(17)
    free = np.argwhere(p != 0)
    seeds = [free[rng.integers(0, len(free), int(k))] for k in rng.integers(1, 6, 9)]
    a, b = GR.labels(p, seeds, graph=NC.ref_graph("random")), GR.labels_by_order(p, seeds, graph=NC.ref_graph("random"))
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
