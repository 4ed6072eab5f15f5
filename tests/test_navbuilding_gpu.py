"""The calls that route across storeys on the GPU build of the library: the cases of tests/navbuilding_cases.py from host arrays and
from torch device tensors; the refusals and the path capacity; BuildingNavigation and Graph.route_across_floors."""
import numpy as np
import pytest

from tests import navbuilding_cases as BC

pytestmark = pytest.mark.gpu


def _device(a):
    import torch
    return torch.from_numpy(np.array(a, order="C")).cuda()                  # (a copy: the shared maps are read-only)


@pytest.fixture(scope="module")
def lib():
    from holoagent_amd._lib import HmsgLib
    return HmsgLib()


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("case", BC.ALL, ids=[f.__name__ for f in BC.ALL])
def test_nav_building_gpu(lib, case, where):
    case(BC.api(lib, _device if where == "device" else None))


def test_nav_building_refusals_gpu(lib):
    BC.refusals(BC.api(lib), lib)
    BC.path_capacity_too_small(lib)


@pytest.mark.parametrize("where", ["host", "device"])
def test_building_navigation_gpu(lib, where):
    BC.building_navigation(lib, _device if where == "device" else None)


def test_graph_route_across_floors_gpu(lib, tmp_path):
    BC.graph_route_across_floors(lib, tmp_path)
