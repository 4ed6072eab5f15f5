"""The REFERENCE's own stage artefacts through hmsg_restore_stage: map (Open3D's voxel order and grid origin, outlier filter applied --
not the library's voxel order), map features, instance clouds and pooled features of the reference's create_feature_map run in
tests/golden/build_seq.npz go back into a handle, and the sequence of tests/test_objects_golden.py runs on it: segment_floors_manually,
the two given rooms, the labels, segment_hmsg_objects.  Object ids, parent rooms, point counts after the per-object DBSCAN and names
are those of the reference's own segment_hmsg_objects (tests/golden/objects.npz), the floors within that test's 1e-9, and with
pipeline.views_on_device the view <-> object topology is tests/golden/objects_views.json.  No frame is replayed, so -- unlike
test_objects_golden, which rebuilds the scene from its 36 frames -- the simulator twin belongs to the default CPU suite."""
import json
import os

import numpy as np
import pytest

from tests import golden_io as GI
from tests import parity_common as PC


def _check(L):
    from holoagent_amd._lib import Scene
    from holoagent_amd.graph import Graph
    from oracle.refdrive.gen_golden import objects_case_inputs
    z, zo = GI.load("build_seq"), GI.load("objects")
    cfg = GI.unpack_cfg(z)
    H, W = np.asarray(z["depth"]).shape[1:]
    D = int(cfg["feat_dim"])
    sc = Scene(lib_=L, height=int(H), width=int(W), max_frames=1, max_masks=1, feat_dim=D, voxel_size=float(cfg["voxel_size"]))
    off = np.ascontiguousarray(z["ref_mask_off"], np.int64)
    sc.restore_stage(z["ref_cloud"], (off, np.ascontiguousarray(z["ref_mask_pts"], np.float64)), z["ref_mask_feats"], z["K"],
                     map_colors=z["ref_cloud_cols"], map_feats=z["ref_full_feats"])
    assert sc.map_size() == len(z["ref_cloud"]) and np.array_equal(sc.map_points(), z["ref_cloud"])
    assert np.array_equal(sc.map_feats(), z["ref_full_feats"]) and np.array_equal(sc.instance_sizes(), np.diff(off))
    rooms, text, classes = objects_case_inputs(z)
    zv = json.load(open(os.path.join(GI.GOLDEN, "objects_views.json")))

    class DS:
        def get_camera_intrinsics(self):
            return np.asarray(z["K"])

        def __getitem__(self, i):
            return np.asarray(z["rgb"][i]), None, np.asarray(z["pose"][i]), None, None
    g = Graph.from_scene(sc, cfg=dict(main=dict(), models=dict(clip=dict(feat_dim=D)), pipeline=dict(views_on_device=True)), lib=L)
    g.dataset = DS()
    g.segment_floors_manually(None)
    np.testing.assert_allclose([f.floor_zero_level for f in g.floors], zo["floor_zero"], rtol=0, atol=1e-9)
    np.testing.assert_allclose([f.floor_height for f in g.floors], zo["floor_height"], rtol=0, atol=1e-9)
    g.set_rooms([dict(floor=0, vertices=v, view_frames=zv["view_frames"][k]) for k, v in enumerate(rooms)])
    g.set_label_feats(text, classes)
    g.segment_hmsg_objects()
    assert [o.object_id for o in g.objects] == [str(v) for v in zo["obj_id"]]
    assert [o.room_id for o in g.objects] == [str(v) for v in zo["obj_room"]]
    assert [len(o.pcd.points) for o in g.objects] == zo["obj_npts"].tolist()
    assert [o.name for o in g.objects] == [str(v) for v in zo["obj_name"]]
    assert [(o.object_id, list(o.view_ids), o.best_view_id) for o in g.objects] == \
        [(o["object_id"], o["view_ids"], o["best_view_id"]) for o in zv["objects"]]
    assert [(v.view_id, v.room_id, int(v.img_id), list(v.object_ids)) for v in g.views] == \
        [(v["view_id"], v["room_id"], v["img_id"], v["object_ids"]) for v in zv["views"]]
    assert sum(len(v.object_ids) for v in g.views) > 10
    sc.close()


@pytest.mark.skipif(not os.path.exists(PC.EMU_PATH), reason="kernel simulator not built")
def test_reference_artefacts_on_the_simulator():
    from holoagent_amd._lib import HmsgLib
    _check(HmsgLib(PC.EMU_PATH))


@pytest.mark.gpu
def test_reference_artefacts_gpu():
    from holoagent_amd._lib import HmsgLib
    _check(HmsgLib())
