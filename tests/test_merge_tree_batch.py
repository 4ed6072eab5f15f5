"""The hierarchical merge with a level of its tree run as batches (hmsg_set_merge_tree_batch, include/hmsg.h): the instances are
the pair-by-pair tree's, bit for bit; a whole level per batch needs one DBSCAN batch per level; the sharded tree
(hmsg_merge_tree_local / _join) honours the setting; the setter's refusals.

The CPU form runs on the kernel simulator, whose DBSCAN costs about a third of a millisecond per point: there every case runs on
a small synthetic episode (24 x 18 pixels, 5 masks a frame, 15 cm voxels: a build with its merge in about three seconds) at an
odd and an even frame count, and only the cases on the golden fixture, ten seconds to minutes each, wait for HMSG_EMU_SLOW=1 as
the merge test of tests/test_emu_parity.py does.  The same cases, fixture and small episode, run marked `gpu` on the library."""
import math
import os

import numpy as np
import pytest

from tests import golden_io as GI
from tests import parity_common as PC

HMSG_ERR_INVALID = -1
COUNTS = [1, 2, 3, 5, 6, 7, "all"]          # odd counts: the carried-up last list at several levels
MODES = ["whole", "single", "third"]        # a whole level per batch / every pair a batch of its own / about a third of level 0
UNION = "k_db_union/scan"                   # one launch per DBSCAN batch (hmsg_profile_entry)

needs_emu = pytest.mark.skipif(not os.path.exists(PC.EMU_PATH), reason="kernel simulator not built")
emu_slow = pytest.mark.skipif(not os.environ.get("HMSG_EMU_SLOW"), reason="slow on the simulator (minutes); covered on the GPU")


def _lib(which):
    from holoagent_amd._lib import HmsgLib
    return HmsgLib(PC.EMU_PATH) if which == "emu" else HmsgLib()


@pytest.fixture(scope="module")
def libs():
    got = {}

    def get(which):
        if which not in got:
            got[which] = _lib(which)
        return got[which]
    return get


# ---- inputs ------------------------------------------------------------------------------------------------------
_fixture = {}


def fixture_frames(count):
    """frames of tests/golden/build_hier (built as tests/test_gpu_parity.py builds them) and the scene's settings; below the full
    fixture the outlier filter is relaxed as the simulator tests do (few frames: the literal filter would delete the map)"""
    if not _fixture:
        z = GI.load("build_hier")
        _fixture.update(z=z, frames=GI.unpack_frames(z), cfg=GI.unpack_cfg(z))
    frames, cfg = _fixture["frames"], _fixture["cfg"]
    n = len(frames) if count == "all" else count
    over = dict(feat_dim=cfg["feat_dim"])
    if n < len(frames):
        over.update(outlier_nb_points=300)
    return frames[:n], over


SMALL = ["s5", "s8"]                        # the small episode at 5 frames (a carried-up list at two levels) and 8 (a full tree)


def small_frames(n_frames=8):
    """a room seen by a turning camera, sized for the simulator: voxels, the DBSCAN radius and the outlier filter are coarsened with
    the image, so that masks still overlap, merge and survive the 10-point rules (8 frames: 40 masks -> about 20 instances)"""
    from holoagent_amd.synth import SceneSpec, SynthScene
    spec = SceneSpec(seed=31, rooms_x=1, rooms_z=1, room_size=(3.6, 2.5, 3.2), objects_per_room=4, width=24, height=18,
                     n_frames=n_frames, n_masks=5, feat_dim=16, yaw_step_deg=25.0)
    scn = SynthScene(spec)
    return [scn.frame(i) for i in range(n_frames)], dict(feat_dim=16, voxel_size=0.15, merge_dbscan_eps=0.35, outlier_nb_points=5,
                                                         outlier_radius=0.6, feat_dbscan_min=8)


def frames_of(key):
    return small_frames(int(key[1:])) if isinstance(key, str) and key[0] == "s" else fixture_frames(key)


def fused_scene(L, frames, over, merge_type=1, window=None):
    S = PC.stack_frames(frames)
    sc = PC.make_scene(L, frames, dict(over, merge_type=merge_type))
    sc.add_frames(S["rgb"], S["depth"], S["pose"], S["K"])
    sc.finalize_map()
    a, b = window if window is not None else (0, len(frames))
    if window is not None:
        sc.set_frame_window(a)
    sc.add_frame_features(a, S["masks"][a:b], S["f_g"][a:b], S["f_masked"][a:b], S["f_crop"][a:b], S["n_masks"][a:b])
    sc.fuse_frames()
    return sc


def level0_bounds(sc, n_frames):
    """the three settings of a scene: a whole level; below the smallest pair of level 0 (every pair goes alone); a third of level 0"""
    pts = [sum(len(m) for m in sc.frame_masks3d(f)) for f in range(n_frames)]
    pairs = [pts[2 * k] + pts[2 * k + 1] for k in range(n_frames // 2)]
    small = max(1, min(pairs) - 1) if pairs else 1
    third = max(1, sum(pairs) // 3) if pairs else 1
    return {"whole": -1, "single": small, "third": third}


def outcome(sc):
    sizes = sc.instance_sizes()
    inst = sc.instances()
    pts = np.concatenate(inst) if len(inst) else np.zeros((0, 3))
    boxes = sc.instance_boxes()
    sc.pool_instances()
    return dict(sizes=sizes, pts=pts, boxes=boxes, feats=sc.instance_feats())


def same(a, b):
    return all(np.array_equal(a[k], b[k]) for k in ("sizes", "pts", "boxes", "feats"))


# builds are shared between the tests of a module run: (library, input, setting) -> outcome + DBSCAN batches of the merge
_built = {}
_bounds = {}


def built(libs, which, key, mode):
    k = (which, key, mode)
    if k in _built:
        return _built[k]
    frames, over = frames_of(key)
    sc = fused_scene(libs(which), frames, over)
    if (which, key) not in _bounds:
        _bounds[(which, key)] = level0_bounds(sc, len(frames))
    batch = 0 if mode == "serial" else _bounds[(which, key)][mode]
    sc.set_merge_tree_batch(batch)
    sc.set_profiling(True)
    sc.merge_instances()
    launches = sc.profile().get(UNION, (0,))[0]
    sc.set_profiling(False)
    r = outcome(sc)
    r.update(launches=launches, n_frames=len(frames), batch=batch)
    sc.close()
    _built[k] = r
    return r


# ---- 1. same instances, bit for bit --------------------------------------------------------------------------------
def check_same_instances(libs, which, key, mode):
    ref = built(libs, which, key, "serial")
    got = built(libs, which, key, mode)
    if ref["n_frames"] >= 3:
        assert len(ref["sizes"]) > 0                      # (a scene with something to merge)
    for k in ("sizes", "pts", "boxes", "feats"):
        assert np.array_equal(got[k], ref[k]), (key, mode, got["batch"], k)


@needs_emu
@emu_slow
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("count", COUNTS)
def test_same_instances(libs, count, mode):
    check_same_instances(libs, "emu", count, mode)


@needs_emu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("key", SMALL)
def test_same_instances_small_episode(libs, key, mode):
    check_same_instances(libs, "emu", key, mode)
    assert len(built(libs, "emu", key, "serial")["sizes"]) >= 5


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("count", COUNTS + SMALL)
def test_same_instances_gpu(libs, count, mode):
    check_same_instances(libs, "gpu", count, mode)


def check_reference_run(L):
    """the full fixture with a whole level per batch against the reference run's own instances (the hierarchical branch of
    tests/parity_common.py, as tests/test_gpu_parity.py drives it)"""
    z = GI.load("build_hier")
    frames = GI.unpack_frames(z)
    cfg = GI.unpack_cfg(z)
    assert cfg["merge_type"] == "hierarchical"
    sc = PC.make_scene(L, frames, dict(feat_dim=cfg["feat_dim"], merge_type=1))
    S, ref_pts, ref_cols = PC.check_map(sc, frames, cfg)
    ref_feats, _ = PC.check_fuse(sc, frames, S, cfg, ref_pts, ref_cols, check_masks=False)
    sc.set_merge_tree_batch(-1)
    got, feats = PC.check_merge_pool(sc, frames, cfg, ref_pts, ref_feats)
    PC.check_against_reference_run("build_hier, a level per batch", z, sc, got, feats)
    sc.close()


@needs_emu
@emu_slow
def test_whole_levels_against_the_reference_run(libs):
    check_reference_run(libs("emu"))


@pytest.mark.gpu
def test_whole_levels_against_the_reference_run_gpu(libs):
    check_reference_run(libs("gpu"))


# ---- 2. launch counts ----------------------------------------------------------------------------------------------
def check_launches(libs, which, key):
    """With a whole level per batch the merge over F frames runs one DBSCAN batch per level of the tree and one for the final
    pass at most: ceil(log2 F) + 1 (fewer where a level has nothing to cluster) -- the tree's shape, not a measurement."""
    whole = built(libs, which, key, "whole")
    F = whole["n_frames"]
    assert whole["launches"] <= math.ceil(math.log2(F)) + 1, (F, whole["launches"])
    return whole["launches"], built(libs, which, key, "serial")["launches"]


@needs_emu
@pytest.mark.parametrize("count", [pytest.param(c, marks=emu_slow) for c in COUNTS] + SMALL)
def test_one_dbscan_batch_per_level(libs, count):
    whole, serial = check_launches(libs, "emu", count)
    assert whole <= serial
    if count == "all" or count in SMALL:
        assert whole < serial


@pytest.mark.gpu
@pytest.mark.parametrize("count", COUNTS + SMALL)
def test_one_dbscan_batch_per_level_gpu(libs, count):
    whole, serial = check_launches(libs, "gpu", count)
    assert whole <= serial
    if count == "all" or count in SMALL:
        assert whole < serial


# ---- 3. the sharded tree ---------------------------------------------------------------------------------------------
def check_sharded(libs, which, key, F):
    """two handles with the frame windows [0, F/2) and [F/2, F): merge_tree_local on both, merge_tree_join on the first (how
    holoagent_amd/dist.py drives them), a whole level per batch on both -- against ONE handle's pair-by-pair tree"""
    L = libs(which)
    frames, over = small_frames(F) if key == "small" else fixture_frames(F)
    assert len(frames) == F and F & (F - 1) == 0
    one = fused_scene(L, frames, over)
    one.merge_instances()
    ref = outcome(one)
    one.close()
    parts = []
    for w in ((0, F // 2), (F // 2, F)):
        sc = fused_scene(L, frames, over, window=w)
        sc.set_merge_tree_batch(-1)
        sc.set_profiling(True)
        th, lists, idx = sc.merge_tree_local(F)
        assert lists == 2 and idx == len(parts)
        # the window's own levels, each one DBSCAN batch at most
        assert sc.profile().get(UNION, (0,))[0] <= math.ceil(math.log2(F // 2))
        parts.append((sc, th))
    (a, th_a), (b, th_b) = parts
    assert th_a == th_b
    a.merge_tree_join(b.instances(), th_a, final_pass=True)
    # (the features are pooled from the whole map: the handle of a window holds its own frames' features only)
    got = dict(sizes=a.instance_sizes(), pts=np.concatenate(a.instances()), boxes=a.instance_boxes())
    for k in got:
        assert np.array_equal(got[k], ref[k]), k
    assert len(ref["sizes"]) > 0
    a.close()
    b.close()


@needs_emu
def test_sharded_tree_small_episode(libs):
    check_sharded(libs, "emu", "small", 8)


@needs_emu
@emu_slow
def test_sharded_tree(libs):
    check_sharded(libs, "emu", "fixture", 16)


@pytest.mark.gpu
@pytest.mark.parametrize("key,F", [("fixture", 16), ("small", 8)])
def test_sharded_tree_gpu(libs, key, F):
    check_sharded(libs, "gpu", key, F)


# ---- 5. refusals -----------------------------------------------------------------------------------------------------
def check_refusals(libs, which):
    """the setter before and after hmsg_merge_instances, and hmsg_reset bringing the setting back to 0"""
    L = libs(which)
    frames, over = small_frames()
    sc = fused_scene(L, frames, over)
    setter = lambda v: L.c.hmsg_set_merge_tree_batch(sc.h, v)
    assert setter(-2) == HMSG_ERR_INVALID and setter(2 ** 31) == HMSG_ERR_INVALID and setter(-2 ** 40) == HMSG_ERR_INVALID
    assert b"max_batch_points" in L.c.hmsg_last_error(sc.h)
    assert setter(2 ** 31 - 1) == 0 and setter(0) == 0 and setter(-1) == 0
    sc.set_profiling(True)
    sc.merge_instances()
    whole = sc.profile()[UNION][0]
    assert setter(0) == HMSG_ERR_INVALID and setter(-1) == HMSG_ERR_INVALID          # after the merge
    first = outcome(sc)
    # hmsg_reset: the setter is accepted again, and the setting is back at 0 -- the same frames now take the pair-by-pair
    # tree's DBSCAN batches, one per pair
    sc.reset()
    S = PC.stack_frames(frames)
    sc.add_frames(S["rgb"], S["depth"], S["pose"], S["K"])
    sc.finalize_map()
    sc.add_frame_features(0, S["masks"], S["f_g"], S["f_masked"], S["f_crop"], S["n_masks"])
    sc.fuse_frames()
    sc.merge_instances()
    serial = sc.profile()[UNION][0]
    assert serial == built(libs, which, "s8", "serial")["launches"] > whole
    assert same(outcome(sc), first)
    sc.reset()
    assert setter(5) == 0
    sc.close()


def check_refused_after_tree_local(libs, which):
    L = libs(which)
    frames, over = small_frames()
    sc = fused_scene(L, frames, over, window=(0, 4))
    assert L.c.hmsg_set_merge_tree_batch(sc.h, 7) == 0
    sc.merge_tree_local(len(frames))
    assert L.c.hmsg_set_merge_tree_batch(sc.h, -1) == HMSG_ERR_INVALID
    assert L.c.hmsg_set_merge_tree_batch(None, -1) == HMSG_ERR_INVALID
    sc.close()


def check_sequential_unaffected(libs, which):
    L = libs(which)
    frames, over = small_frames()
    res = []
    for batch in (None, -1):
        sc = fused_scene(L, frames, over, merge_type=0)
        if batch is not None:
            sc.set_merge_tree_batch(batch)
        sc.merge_instances()
        res.append(outcome(sc))
        sc.close()
    assert len(res[0]["sizes"]) > 0
    assert same(res[1], res[0])


def check_value_range(libs, which):
    """the values the setter takes, on a scene that holds nothing yet"""
    from holoagent_amd._lib import Scene
    L = libs(which)
    sc = Scene(lib_=L, height=48, width=64, max_frames=2, max_masks=4, feat_dim=16)
    for v, rc in ((-2, HMSG_ERR_INVALID), (2 ** 31, HMSG_ERR_INVALID), (-2 ** 40, HMSG_ERR_INVALID), (2 ** 31 - 1, 0), (1, 0), (0, 0), (-1, 0)):
        assert L.c.hmsg_set_merge_tree_batch(sc.h, v) == rc, v
    assert L.c.hmsg_set_merge_tree_batch(None, -1) == HMSG_ERR_INVALID
    sc.set_merge_tree_batch(4096)
    with pytest.raises(Exception):
        sc.set_merge_tree_batch(-5)
    sc.close()


@needs_emu
def test_setter_value_range(libs):
    check_value_range(libs, "emu")


@pytest.mark.gpu
def test_setter_value_range_gpu(libs):
    check_value_range(libs, "gpu")


@needs_emu
def test_setter_refusals_and_reset(libs):
    check_refusals(libs, "emu")


@needs_emu
def test_setter_refused_after_tree_local(libs):
    check_refused_after_tree_local(libs, "emu")


@pytest.mark.gpu
def test_setter_refused_after_tree_local_gpu(libs):
    check_refused_after_tree_local(libs, "gpu")


@needs_emu
def test_sequential_merge_ignores_the_setting(libs):
    check_sequential_unaffected(libs, "emu")


@pytest.mark.gpu
def test_setter_refusals_and_reset_gpu(libs):
    check_refusals(libs, "gpu")


@pytest.mark.gpu
def test_sequential_merge_ignores_the_setting_gpu(libs):
    check_sequential_unaffected(libs, "gpu")
