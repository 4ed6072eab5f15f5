"""The viewpoint calls on the GPU build of the library: the cases of tests/navview_cases.py from host arrays and from torch device
tensors, plus the 300 x 520 map at the 255-cell limit that the simulator leaves out for its run time; the refusals and the path
capacity, NavigationGraph.route_to_view and Graph.view_routes_to_objects on a built scene."""
import numpy as np
import pytest

from tests import navview_cases as VC

pytestmark = pytest.mark.gpu


def _device(a):
    import torch
    return torch.from_numpy(np.array(a, order="C")).cuda()                  # (a copy: the shared maps are read-only)


@pytest.fixture(scope="module")
def lib():
    from holoagent_amd._lib import HmsgLib
    return HmsgLib()


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("case", VC.VIEW_CASES, ids=[f.__name__ for f in VC.VIEW_CASES])
def test_nav_view_gpu(lib, case, where):
    case(VC.api(lib, _device if where == "device" else None))


@pytest.mark.parametrize("where", ["host", "device"])
def test_nav_view_large_window_gpu(lib, where):
    VC.large_window(VC.api(lib, _device if where == "device" else None))


def test_nav_view_refusals_gpu(lib):
    VC.refusals(VC.api(lib), lib)
    VC.view_route_capacity_too_small(lib)


@pytest.mark.parametrize("where", ["host", "device"])
def test_navigation_graph_route_to_view_gpu(lib, where):
    VC.navigation_graph_route_to_view(lib, _device if where == "device" else None)


def test_graph_view_routes_to_objects_gpu(lib, tmp_path):
    VC.graph_view_routes_to_objects(lib, tmp_path)
