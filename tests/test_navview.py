"""The viewpoint calls on the kernel simulator (include/hmsg.h, N8: hmsg_nav_viewpoints, hmsg_nav_view_route): the line rule on the
restatement alone, the vectorised restatement against its loops, then every case function of tests/navview_cases.py (the module
tests/test_navview_gpu.py imports too) against tests/navview_reference.py, every output by array_equal; the refusals and the path
capacity; NavigationGraph.route_to_view on a storey and Graph.view_routes_to_objects on a scene built from frames.  The 300 x 520
case at the 255-cell limit is left to the GPU module for its run time here."""
import os

import pytest

from tests import navview_cases as VC
from tests import parity_common as PC

needs_emu = pytest.mark.skipif(not os.path.exists(PC.EMU_PATH), reason="kernel simulator not built")


@pytest.fixture(scope="module")
def emu():
    from holoagent_amd._lib import HmsgLib
    return HmsgLib(PC.EMU_PATH)


def test_the_line_rule():
    VC.line_rule()


def test_the_vectorised_restatement_equals_the_loops():
    VC.vectorised_against_loops()


@needs_emu
@pytest.mark.parametrize("case", VC.VIEW_CASES, ids=[f.__name__ for f in VC.VIEW_CASES])
def test_nav_view_simulator(emu, case):
    case(VC.api(emu))


@needs_emu
def test_nav_view_refusals_simulator(emu):
    VC.refusals(VC.api(emu), emu)
    VC.view_route_capacity_too_small(emu)


@needs_emu
def test_navigation_graph_route_to_view_simulator(emu):
    VC.navigation_graph_route_to_view(emu)


@needs_emu
def test_graph_view_routes_to_objects_simulator(emu, tmp_path):
    VC.graph_view_routes_to_objects(emu, tmp_path)
