"""hmsg_eval_semantic_ranks on the GPU build of the library: the cases of tests/test_eval_semantics.py from host arrays and from torch
device tensors, plus the largest shape (D = 512, C = 1030, n = 33), which the simulator leaves out for its run time."""
import numpy as np
import pytest

from tests import test_eval_semantics as TS

pytestmark = pytest.mark.gpu


def _device(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module", params=["host", "device"])
def sem(request):
    from holoagent_amd._lib import HmsgLib
    h = TS.Hook(HmsgLib(), wrap=_device if request.param == "device" else None)
    yield h
    h.close()


@pytest.mark.parametrize("D,C,n", TS.SHAPES + [(512, 1030, 33)])
def test_semantic_ranks_shapes_gpu(sem, D, C, n):
    TS.shapes(sem, D, C, n)


def test_semantic_ranks_ties_and_names_gpu(sem):
    TS.ties_and_names(sem)


def test_semantic_ranks_zero_norm_gpu(sem):
    TS.zero_norm(sem)


def test_semantic_ranks_refusals_gpu():
    from holoagent_amd._lib import HmsgLib
    h = TS.Hook(HmsgLib())
    TS.refusals(h)
    h.close()
