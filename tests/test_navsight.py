"""N10 on the kernel simulator (include/hmsg.h: hmsg_nav_height_map, hmsg_nav_viewpoints_h, hmsg_nav_view_route_h): the three
properties the sight rule was checked for on the restatement alone, the restatement's numpy form against its loops, then every case
function of tests/navsight_cases.py (the module tests/test_navsight_gpu.py imports too) against tests/navsight_reference.py, every
output by array_equal; both LDS layouts of the sight kernel; the refusals and the path capacity; the slab forms, NavigationGraph and
Graph on small scenes.  The 300 x 520 case at the 255-cell limit is left to the GPU module for its run time here."""
import os

import pytest

from tests import navsight_cases as SC
from tests import parity_common as PC

needs_emu = pytest.mark.skipif(not os.path.exists(PC.EMU_PATH), reason="kernel simulator not built")


@pytest.fixture(scope="module")
def emu():
    from holoagent_amd._lib import HmsgLib
    return HmsgLib(PC.EMU_PATH)


def test_the_rule_contains_v2():
    SC.property_contains_v2()


def test_the_motivating_case_and_the_footprint():
    SC.property_motivating_case()
    SC.property_footprint()


def test_the_vectorised_restatement_equals_the_loops():
    SC.loops_against_numpy()


@needs_emu
@pytest.mark.parametrize("case", SC.SIGHT_CASES, ids=[f.__name__ for f in SC.SIGHT_CASES])
def test_nav_sight_simulator(emu, case):
    case(SC.api(emu))


@needs_emu
def test_nav_sight_layouts_simulator(emu):
    SC.both_layouts(SC.api(emu), emu)


@needs_emu
def test_nav_sight_refusals_simulator(emu):
    SC.refusals(SC.api(emu), emu)
    SC.height_map_refusals(SC.api(emu), emu)
    SC.view_route_h_capacity_too_small(emu)


@needs_emu
def test_nav_height_map_slab_forms_simulator(emu, tmp_path):
    SC.slab_forms(emu, tmp_path)


@needs_emu
def test_navigation_graph_heights_simulator(emu):
    SC.navigation_graph_heights(emu)


@needs_emu
def test_graph_view_routes_heights_simulator(emu, tmp_path):
    SC.graph_view_routes_heights(emu, tmp_path)
