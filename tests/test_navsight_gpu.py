"""N10 on the GPU build of the library: the cases of tests/navsight_cases.py from host arrays and from torch device tensors, plus
the 300 x 520 map at the 255-cell limit that the simulator leaves out for its run time; both LDS layouts, the refusals and the path
capacity, the slab forms, NavigationGraph and Graph on small scenes."""
import numpy as np
import pytest

from tests import navsight_cases as SC

pytestmark = pytest.mark.gpu


def _device(a):
    import torch
    return torch.from_numpy(np.array(a, order="C")).cuda()                  # (a copy: the shared maps are read-only)


@pytest.fixture(scope="module")
def lib():
    from holoagent_amd._lib import HmsgLib
    return HmsgLib()


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("case", SC.SIGHT_CASES, ids=[f.__name__ for f in SC.SIGHT_CASES])
def test_nav_sight_gpu(lib, case, where):
    case(SC.api(lib, _device if where == "device" else None))


@pytest.mark.parametrize("where", ["host", "device"])
def test_nav_sight_large_window_gpu(lib, where):
    SC.large_window(SC.api(lib, _device if where == "device" else None))


def test_nav_sight_layouts_gpu(lib):
    SC.both_layouts(SC.api(lib), lib)


def test_nav_sight_refusals_gpu(lib):
    SC.refusals(SC.api(lib), lib)
    SC.height_map_refusals(SC.api(lib), lib)
    SC.view_route_h_capacity_too_small(lib)


def test_nav_height_map_slab_forms_gpu(lib, tmp_path):
    SC.slab_forms(lib, tmp_path)


@pytest.mark.parametrize("where", ["host", "device"])
def test_navigation_graph_heights_gpu(lib, where):
    SC.navigation_graph_heights(lib, _device if where == "device" else None)


def test_graph_view_routes_heights_gpu(lib, tmp_path):
    SC.graph_view_routes_heights(lib, tmp_path)
