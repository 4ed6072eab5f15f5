"""The reference's eval_utils.py names as holoagent_amd/semseg.py keeps them, and the shims under holoagent_amd/compat/ that re-export
them and metric.py under the reference's import paths: knn_interpolation against sklearn's BallTree + np.bincount (the reference's
own calls), Tree_interpolation against scipy's cKDTree, text_prompt against a float64 cosine, sim_2_label as np.argmax of the matrix
it is GIVEN (an edited matrix included), load_feature_map on a map written to disk with one pcd_i.ply missing.  Kernel simulator;
the GPU twins are marked gpu."""
import importlib
import os
import sys

import numpy as np
import pytest

from tests import parity_common as PC
from tests import semseg_reference as R
from tests import test_semseg as TS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def interpolations(L):
    from holoagent_amd import semseg as S
    from scipy.spatial import cKDTree
    from sklearn.neighbors import BallTree
    pts, lab, q = TS.two_boxes(900, 700, 5, 9, seed=21)
    labf = lab.astype(np.float64)
    labf[::4] = -1                                            # unlabelled rows are dropped ...
    cum = np.column_stack([pts, labf])
    cum[4, :3] = np.nan                                       # ... whatever they hold (row 4 is one of them)
    full = np.column_stack([q, np.arange(len(q)) % 7])        # x y z + a ground-truth column, as the reference's callers pass it
    labeled = cum[cum[:, -1] != -1]
    tree = BallTree(labeled[:, :3], metric="minkowski")
    dist = tree.query(full[:, :3], k=6)[0]
    assert (dist[:, 5] > dist[:, 4]).all()                    # no tie at the 5th place: the reference's answer is defined
    knn_classes = labeled[tree.query(full[:, :3], k=5)[1]][:, :, -1].astype(int)
    want = np.array([np.bincount(row).argmax() for row in knn_classes], np.float64)
    with S.using(L):
        out = S.knn_interpolation(cum, full, 5)
        assert out.shape == (len(q), 5) and out.dtype == np.float64
        assert np.array_equal(out[:, :-1], full) and np.array_equal(out[:, -1], want)
        # Tree_interpolation: labels are whatever the last column holds (floats here), picked by the nearest row
        pred = np.column_stack([pts, np.round(np.linspace(0.5, 40.5, len(pts)))])
        d, i = cKDTree(pred[:, :3]).query(full[:, :3], k=2)
        assert (d[:, 1] > d[:, 0]).all()
        got = S.Tree_interpolation(pred, full)
        assert got.shape == (len(q),) and np.array_equal(got, pred[:, -1][i[:, 0]])


def labels_from_similarity(L):
    from holoagent_amd import semseg as S
    emb, text, names, _ = TS.TS.table(32, 12, 20, seed=4)
    words = ["w%d" % i for i in range(12)]
    ids = [100 + 3 * i for i in range(12)]
    calls = []

    def clip(ws):
        calls.append(list(ws))
        return text

    class WithTemplates:
        def get_text_feats_multiple_templates(self, ws):
            return text

        def encode_text(self, ws):
            raise AssertionError("templates=True asks for get_text_feats_multiple_templates")

    class Plain:
        def encode_text(self, ws):
            return text
    with S.using(L):
        sim = S.text_prompt(clip, 32, emb, words)
        assert type(sim) is np.ndarray and sim.dtype == np.float32 and sim.shape == (20, 12) and calls == [words]
        want_lab, want_sim = R.instance_labels(emb, text, ids)
        assert np.abs(sim - want_sim).max() < 2 * (32 + 2) * 2.0 ** -24          # a float32 dot product of normalised rows
        assert np.array_equal(S.text_prompt(WithTemplates(), 32, emb, words), sim)
        assert np.array_equal(S.text_prompt(Plain(), 32, emb, words, templates=False), sim)
        got = S.sim_2_label(sim, ids)
        assert np.array_equal(got, want_lab)
        # the matrix is the argument: what the caller does to it between the two calls counts
        c = int(sim[0].argmax())
        edited = sim.copy()
        edited[:, c] = -1
        relabelled = S.sim_2_label(edited, ids)
        assert np.array_equal(relabelled, np.asarray(ids)[edited.argmax(axis=1)]) and ids[c] not in relabelled.tolist()
        sim[:, c] = -1                                        # ... in place too
        assert np.array_equal(S.sim_2_label(sim, ids), relabelled)
        tie = np.array([[0.5, 0.7, 0.7], [0.1, 0.1, 0.0]], np.float32)
        assert S.sim_2_label(tie, ["a", "b", "c"]).tolist() == ["b", "a"]        # the first of equal entries
        # a zero embedding: every cosine is 0, class 0 (graph.py:479-483)
        zero = S.text_prompt(clip, 32, np.zeros((2, 32), np.float32), words)
        assert (zero == 0).all() and S.sim_2_label(zero, ids).tolist() == [ids[0], ids[0]]


def feature_map_from_disk(L, tmp_path):
    import torch
    from holoagent_amd import semseg as S
    from holoagent_amd._lib import write_ply
    rng = np.random.default_rng(8)
    clouds = [rng.standard_normal((n, 3)) for n in (5, 1, 17, 9)]
    feats = (rng.standard_normal((4, 16)) * 3).astype(np.float64)
    root = tmp_path / "map"
    os.makedirs(root / "objects")
    torch.save(torch.from_numpy(feats), str(root / "mask_feats.pt"))
    for i, c in enumerate(clouds):
        if i != 2:                                            # pcd_2.ply is missing, and a file of another kind keeps the count at four
            write_ply(root / "objects" / ("pcd_%d.ply" % i), c, lib_=L)
    (root / "objects" / "notes.txt").write_text("pcd_2 was not saved\n")
    with S.using(L):
        pcds, mf = S.load_feature_map(str(root))
        assert len(pcds) == 3 and mf.shape == (3, 16) and mf.dtype == np.float32
        for p, c in zip(pcds, [clouds[0], clouds[1], clouds[3]]):
            assert np.array_equal(np.asarray(p.points), c)
        f32 = feats.astype(np.float32)
        want = torch.nn.functional.normalize(torch.from_numpy(f32), p=2, dim=-1).numpy()[[0, 1, 3]]
        assert np.array_equal(mf, want)
        assert np.array_equal(S.load_feature_map(str(root), normalize=False)[1], f32[[0, 1, 3]])
        with pytest.raises(FileNotFoundError):
            S.load_feature_map(str(tmp_path / "nowhere"))
        os.makedirs(tmp_path / "bare")
        torch.save(torch.from_numpy(feats), str(tmp_path / "bare" / "mask_feats.pt"))
        with pytest.raises(FileNotFoundError):
            S.load_feature_map(str(tmp_path / "bare"))


def test_shims_reexport_the_module(monkeypatch):
    """memory.hmsg.utils.eval_utils / metric and hmsg.utils.eval_utils / metric resolve, with holoagent_amd/compat on the path, to the
    functions of holoagent_amd/semseg.py"""
    from holoagent_amd import semseg as S
    monkeypatch.syspath_prepend(os.path.join(ROOT, "holoagent_amd", "compat"))
    for pkg in ("memory.hmsg.utils", "hmsg.utils"):
        for m in [k for k in sys.modules if k == pkg.split(".")[0] or k.startswith(pkg.split(".")[0] + ".")]:
            monkeypatch.delitem(sys.modules, m)
        eu = importlib.import_module(pkg + ".eval_utils")
        me = importlib.import_module(pkg + ".metric")
        assert os.path.join("holoagent_amd", "compat") in eu.__file__ and os.path.join("holoagent_amd", "compat") in me.__file__
        for name in ("text_prompt", "sim_2_label", "knn_interpolation", "Tree_interpolation", "load_feature_map"):
            assert getattr(eu, name) is getattr(S, name), name
        for name in ("pixel_accuracy", "mean_accuracy", "per_class_iou", "mean_iou", "frequency_weighted_iou", "EvalSegErr"):
            assert getattr(me, name) is getattr(S, name), name
        for m in [k for k in sys.modules if k == pkg.split(".")[0] or k.startswith(pkg.split(".")[0] + ".")]:
            sys.modules.pop(m)                                # (what this test imported; monkeypatch puts back what was there before)


needs_emu = pytest.mark.skipif(not os.path.exists(PC.EMU_PATH), reason="kernel simulator not built")


@pytest.fixture(scope="module")
def emu():
    from holoagent_amd._lib import HmsgLib
    return HmsgLib(PC.EMU_PATH)


@needs_emu
def test_interpolations_simulator(emu):
    interpolations(emu)


@needs_emu
def test_labels_from_similarity_simulator(emu):
    labels_from_similarity(emu)


@needs_emu
def test_feature_map_from_disk_simulator(emu, tmp_path):
    feature_map_from_disk(emu, tmp_path)


@needs_emu
def test_shimmed_metric_through_the_import_path_simulator(emu, monkeypatch):
    """the five numbers through `memory.hmsg.utils.metric`, on a golden case recorded from the reference"""
    from holoagent_amd import semseg as S
    monkeypatch.syspath_prepend(os.path.join(ROOT, "holoagent_amd", "compat"))
    for m in [k for k in sys.modules if k == "memory" or k.startswith("memory.")]:
        monkeypatch.delitem(sys.modules, m)
    M = importlib.import_module("memory.hmsg.utils.metric")
    i, gt, pred, ignore, scores, classes, per_class = next(c for c in TS.golden_cases() if len(c[3]))
    with S.using(emu):
        got = [M.pixel_accuracy(pred, gt, ignore.tolist()), M.mean_accuracy(pred, gt, ignore.tolist()), M.mean_iou(pred, gt, ignore.tolist()),
               M.frequency_weighted_iou(pred, gt, ignore.tolist())]
        assert np.array_equal(got, scores, equal_nan=True)
        assert np.array_equal(M.per_class_iou(pred, gt, ignore.tolist()), per_class)
        with pytest.raises(M.EvalSegErr):
            M.mean_iou(pred[:, :-1], gt)
    for m in [k for k in sys.modules if k == "memory" or k.startswith("memory.")]:
        sys.modules.pop(m)


@pytest.mark.gpu
def test_interpolations_gpu():
    from holoagent_amd._lib import HmsgLib
    interpolations(HmsgLib())


@pytest.mark.gpu
def test_feature_map_from_disk_gpu(tmp_path):
    from holoagent_amd._lib import HmsgLib
    feature_map_from_disk(HmsgLib(), tmp_path)
