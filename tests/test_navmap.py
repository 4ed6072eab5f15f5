"""The navigation maps on the kernel simulator (include/hmsg.h: hmsg_nav_grid, hmsg_nav_floor_maps and their hmsg_graph_* forms):
every case function of tests/navmap_cases.py (the module tests/test_navmap_gpu.py imports too): the maps against the numpy / scipy /
sklearn restatement of tests/navmap_reference.py, every output by array_equal; the refusals; the graph call and the scene call
against the generic call on the slab read back from the map; Graph.create_nav_graph on a scene built from frames; and the Voronoi
graph of holoagent_amd/nav_graph.py on the library's maps against the same function on the restatement's maps."""
import os

import numpy as np
import pytest

from tests import navmap_cases as NC
from tests import parity_common as PC

needs_emu = pytest.mark.skipif(not os.path.exists(PC.EMU_PATH), reason="kernel simulator not built")


@pytest.fixture(scope="module")
def emu():
    from holoagent_amd._lib import HmsgLib
    return HmsgLib(PC.EMU_PATH)


@needs_emu
@pytest.mark.parametrize("case", NC.ALL, ids=[f.__name__ for f in NC.ALL])
def test_nav_maps_simulator(emu, case):
    case(NC.runner(emu))


@needs_emu
def test_nav_maps_refusals_simulator(emu):
    NC.refusals(NC.runner(emu), NC.raises)
    NC.capacity_too_small(emu)


@needs_emu
def test_graph_nav_maps_simulator(emu, tmp_path):
    NC.graph_call_equals_generic_call(emu, tmp_path)


@needs_emu
def test_voronoi_graph_simulator(emu, tmp_path):
    NC.voronoi_graph(emu, tmp_path)


@needs_emu
def test_create_nav_graph_on_a_built_scene_simulator(emu, tmp_path):
    NC.create_nav_graph_on_a_built_scene(emu, tmp_path)


def test_compat_import_paths():
    from holoagent_amd.compat.hmsg.graph.navigation_graph import NavigationGraph as A
    from holoagent_amd.compat.memory.hmsg.graph.navigation_graph import NavigationGraph as B
    from holoagent_amd.nav_graph import NavigationGraph
    assert A is NavigationGraph and B is NavigationGraph
