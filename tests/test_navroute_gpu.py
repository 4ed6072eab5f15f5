"""The routing calls on the GPU build of the library: the cases of tests/navroute_cases.py from host arrays and from torch device
tensors, plus the 500 x 700 rooms map that the simulator leaves out for its run time; the refusals and the path capacity,
NavigationGraph.route and Graph.route_to_objects on a built scene."""
import numpy as np
import pytest

from tests import navroute_cases as NC

pytestmark = pytest.mark.gpu


def _device(a):
    import torch
    return torch.from_numpy(np.array(a, order="C")).cuda()                  # (a copy: the shared maps are read-only)


@pytest.fixture(scope="module")
def lib():
    from holoagent_amd._lib import HmsgLib
    return HmsgLib()


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("case", NC.ALL, ids=[f.__name__ for f in NC.ALL])
def test_nav_route_gpu(lib, case, where):
    case(NC.api(lib, _device if where == "device" else None))


@pytest.mark.parametrize("where", ["host", "device"])
def test_nav_route_rooms_large_gpu(lib, where):
    NC.rooms_large(NC.api(lib, _device if where == "device" else None))


def test_nav_route_refusals_gpu(lib):
    NC.refusals(NC.api(lib), lib)
    NC.path_capacity_too_small(lib)


@pytest.mark.parametrize("where", ["host", "device"])
def test_navigation_graph_route_gpu(lib, where):
    NC.navigation_graph_route(lib, _device if where == "device" else None)


def test_graph_route_to_objects_gpu(lib, tmp_path):
    NC.graph_route_to_objects(lib, tmp_path)
