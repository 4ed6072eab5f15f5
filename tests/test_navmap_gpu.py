"""The navigation maps on the GPU build of the library: the cases of tests/navmap_cases.py from host arrays and from torch device
tensors, plus the larger storey (3 * 10^5 points, 700 x 500 cells) that the simulator leaves out for its run time; the refusals,
the graph and scene calls, Graph.create_nav_graph on a built scene and the Voronoi graph."""
import numpy as np
import pytest

from tests import navmap_cases as NC

pytestmark = pytest.mark.gpu


def _device(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def lib():
    from holoagent_amd._lib import HmsgLib
    return HmsgLib()


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("case", NC.ALL, ids=[f.__name__ for f in NC.ALL])
def test_nav_maps_gpu(lib, case, where):
    case(NC.runner(lib, _device if where == "device" else None))


@pytest.mark.parametrize("where", ["host", "device"])
def test_nav_maps_larger_gpu(lib, where):
    NC.larger(NC.runner(lib, _device if where == "device" else None))


def test_nav_maps_refusals_gpu(lib):
    NC.refusals(NC.runner(lib), NC.raises)
    NC.capacity_too_small(lib)


def test_graph_nav_maps_gpu(lib, tmp_path):
    NC.graph_call_equals_generic_call(lib, tmp_path)


@pytest.mark.parametrize("where", ["host", "device"])
def test_voronoi_graph_gpu(lib, tmp_path, where):
    NC.voronoi_graph(lib, tmp_path, _device if where == "device" else None)


def test_create_nav_graph_on_a_built_scene_gpu(lib, tmp_path):
    NC.create_nav_graph_on_a_built_scene(lib, tmp_path)
