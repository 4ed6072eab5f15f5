"""The calls that route across storeys on the kernel simulator (include/hmsg.h, N9: hmsg_nav_seeded_fields,
hmsg_nav_building_fields, hmsg_nav_building_paths, hmsg_nav_building_route): every case function of tests/navbuilding_cases.py (the
module tests/test_navbuilding_gpu.py imports too) against scipy's Dijkstra on the layered graph (tests/navbuilding_reference.py),
every output by array_equal; the refusals and the path capacity; BuildingNavigation on two storeys made from clouds and
Graph.route_across_floors on a scene built from frames."""
import os

import pytest

from tests import navbuilding_cases as BC
from tests import parity_common as PC

needs_emu = pytest.mark.skipif(not os.path.exists(PC.EMU_PATH), reason="kernel simulator not built")


@pytest.fixture(scope="module")
def emu():
    from holoagent_amd._lib import HmsgLib
    return HmsgLib(PC.EMU_PATH)


@needs_emu
@pytest.mark.parametrize("case", BC.ALL, ids=[f.__name__ for f in BC.ALL])
def test_nav_building_simulator(emu, case):
    case(BC.api(emu))


@needs_emu
def test_nav_building_refusals_simulator(emu):
    BC.refusals(BC.api(emu), emu)
    BC.path_capacity_too_small(emu)


@needs_emu
def test_building_navigation_simulator(emu):
    BC.building_navigation(emu)


@needs_emu
def test_stairs_track_helper_simulator(emu):
    BC.stairs_track_helper(emu)


@needs_emu
def test_graph_route_across_floors_simulator(emu, tmp_path):
    BC.graph_route_across_floors(emu, tmp_path)
