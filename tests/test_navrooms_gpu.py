"""The room calls on the GPU build of the library: the cases of tests/navrooms_cases.py from host arrays and from torch device
tensors, plus the 500 x 700 rooms map that the simulator leaves out for its run time; the capacities and the refusals,
NavigationGraph's and Graph's room methods on a built scene."""
import numpy as np
import pytest

from tests import navrooms_cases as GC

pytestmark = pytest.mark.gpu


def _device(a):
    import torch
    return torch.from_numpy(np.array(a, order="C")).cuda()                  # (a copy: the shared maps are read-only)


@pytest.fixture(scope="module")
def lib():
    from holoagent_amd._lib import HmsgLib
    return HmsgLib()


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("case", GC.ALL, ids=[f.__name__ for f in GC.ALL])
def test_nav_rooms_gpu(lib, case, where):
    case(GC.api(lib, _device if where == "device" else None))


@pytest.mark.parametrize("where", ["host", "device"])
def test_nav_rooms_large_gpu(lib, where):
    GC.rooms_large(GC.api(lib, _device if where == "device" else None))


def test_nav_rooms_capacities_gpu(lib):
    GC.capacities_too_small(lib)


def test_nav_rooms_refusals_gpu(lib):
    GC.refusals(GC.api(lib), lib)


@pytest.mark.parametrize("where", ["host", "device"])
def test_navigation_graph_rooms_gpu(lib, where):
    GC.navigation_graph_rooms(lib, _device if where == "device" else None)


def test_graph_rooms_gpu(lib, tmp_path):
    GC.graph_rooms(lib, tmp_path)
