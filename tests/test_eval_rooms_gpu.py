"""hmsg_eval_rooms on the GPU build of the library: the cases of tests/test_eval_rooms.py from host arrays and from torch device
tensors, and two calls on the same inputs compared with each other."""
import numpy as np
import pytest

from tests import test_eval_rooms as TR

pytestmark = pytest.mark.gpu


def _device(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module", params=["host", "device"])
def rooms(request):
    from holoagent_amd._lib import HmsgLib
    h = TR.Hook(HmsgLib(), wrap=_device if request.param == "device" else None)
    yield h
    h.close()


@pytest.mark.parametrize("case", [c for c in TR.CASES if c != "refusals"])
def test_eval_rooms_gpu(rooms, case):
    TR.CASES[case](rooms)


def test_eval_rooms_refusals_gpu():
    from holoagent_amd._lib import HmsgLib
    h = TR.Hook(HmsgLib())
    TR.refusals(h)
    h.close()


def test_eval_rooms_twice_gpu(rooms):
    """two calls on the same inputs give the same bits (integer counts, no floating-point atomics)"""
    c = TR.storey_scene(31, 5, 4, n_pred=1200, n_gt=1000)
    a, b = rooms.matrices(c), rooms.matrices(c)
    assert all(TR.same_bits(x, y) for x, y in zip(a[:3], b[:3])) and (a[0] > 0).any()
