"""The semantic segmentation score on the GPU build of the library: the cases of tests/test_semseg.py from host arrays and from torch
device tensors, plus the instance-label shape (D = 512, C = 1030, n = 33) that the simulator leaves out for its run time, and
hmsg_knn_labels with every array -- the outputs too -- in device memory."""
import numpy as np
import pytest

from tests import test_semseg as TS

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


@pytest.fixture(scope="module")
def host():
    from holoagent_amd._lib import HmsgLib
    h = TS.Hook(HmsgLib())
    yield h
    h.close()


@pytest.mark.parametrize("n,m,k,classes", TS.KNN_SHAPES)
def test_knn_against_sklearn_gpu(sem, n, m, k, classes):
    TS.knn_against_sklearn(sem, n, m, k, classes)


def test_knn_exact_ties_gpu(sem):
    TS.knn_exact_ties(sem)


def test_knn_dropped_rows_gpu(sem):
    TS.knn_dropped_rows(sem)


def test_knn_refusals_gpu(host):
    TS.knn_refusals(host)


def test_knn_device_outputs_gpu(host):
    import torch
    pts, lab, q, sk, want, nn = TS.sklearn_case(*TS.KNN_SHAPES[0])
    k = TS.KNN_SHAPES[0][2]
    out = torch.full((len(q),), -7, dtype=torch.int32, device="cuda")
    idx = torch.full((len(q), k), -7, dtype=torch.int32, device="cuda")
    host.scene.knn_labels(_device(pts), _device(lab), _device(q), k, return_index=True, out=out, out_index=idx)
    assert np.array_equal(out.cpu().numpy(), sk) and np.array_equal(idx.cpu().numpy(), nn)


@pytest.mark.parametrize("D,C_,n", TS.LABEL_SHAPES + [(512, 1030, 33)])
def test_instance_labels_gpu(sem, D, C_, n):
    TS.instance_labels(sem, D, C_, n)


def test_instance_labels_ties_and_zero_gpu(sem):
    TS.instance_labels_ties_and_zero(sem)


@pytest.mark.parametrize("L,m", TS.CONF_SHAPES)
def test_confusion_gpu(host, L, m):
    TS.confusion_case(host, L, m)


@pytest.mark.parametrize("L,m", [(40, 100003), (1030, 257)])
def test_confusion_device_arrays_gpu(sem, L, m):
    rng = np.random.default_rng(L + m)
    gt, pred = rng.integers(0, L, m).astype(np.int32), rng.integers(0, L, m).astype(np.int32)
    assert np.array_equal(sem.confusion(gt, pred, L), TS.R.confusion(gt, pred, L))


def test_metrics_golden_gpu(host):
    TS.metrics_golden(host)
