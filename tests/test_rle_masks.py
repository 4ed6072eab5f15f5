"""Masks handed over as SAM's uncompressed run-length records (include/hmsg.h: hmsg_add_frame_features_rle, hmsg_rle_to_bitsets,
hmsg_rle_to_masks; holoagent_amd/rle.py).  CPU side: the format in numpy, and the kernels on the kernel simulator (tests/emu)
against bitsets computed in numpy from the dense masks -- a reference that does not go through k_bitset -- and against the dense
hand-over of the same scene, bit for bit.  The malformed records live here only: they must never reach a GPU kernel.

The simulator has ONE address space (its hipPointerGetAttributes calls every pointer host memory), so "device arrays" cannot be told
apart on it.  The library therefore has one validation path for both: run_off is read to the host (the staging helper's read_in),
the per-mask sums always come from k_rle_scan and one flag is read back -- what these tests drive with host arrays is what a device
array takes; tests/test_rle_masks_gpu.py hands the same valid cases over from torch device tensors."""
import ctypes as C
import os

import numpy as np
import pytest

from holoagent_amd import rle
from tests import golden_io as GI
from tests import parity_common as PC
from tests import rle_cases as RC

emu = pytest.mark.skipif(not os.path.exists(PC.EMU_PATH), reason="kernel simulator not built")
HMSG_ERR_INVALID = -1


@pytest.fixture(scope="module")
def L():
    from holoagent_amd._lib import HmsgLib
    return HmsgLib(PC.EMU_PATH)


@pytest.fixture(scope="module")
def scene_and_dense(L):
    frames = RC.small_scene()
    return frames, RC.build(L, frames, RC.dense_hand_over)


# ------------------------------------------------------------------------------------------------------------------- the format
def test_encode_literal_cases():
    assert rle.encode(np.array([[0, 1], [1, 1], [0, 0]])).tolist() == [1, 1, 1, 2, 1]
    assert rle.encode(np.array([[1, 0]])).tolist() == [0, 1, 1]
    assert rle.encode(np.zeros((2, 2), bool)).tolist() == [4]
    assert rle.encode(np.ones((2, 2), bool)).tolist() == [0, 4]
    assert rle.encode(np.ones((2, 2), bool)).dtype == np.uint32
    assert rle.decode([1, 1, 1, 2, 1], 3, 2).tolist() == [[False, True], [True, True], [False, False]]
    assert rle.decode([0, 0, 2, 0, 2], 2, 2).tolist() == [[False, False], [False, False]]      # zero counts are empty runs
    with pytest.raises(ValueError):
        rle.decode([3], 2, 2)


def test_round_trip_on_the_reference_run_fixtures():
    n = ones_first = 0
    for name in ("build_seq", "build_hier", "build_ragged"):
        for f in GI.unpack_frames(GI.load(name)):
            H, W = f["depth"].shape
            for m in f["masks"]:
                c = rle.encode(m)
                assert int(c.astype(np.int64).sum()) == H * W and (c[1:] > 0).all()
                assert np.array_equal(rle.decode(c, H, W), m.astype(bool))
                n += 1
                ones_first += int(c[0] == 0)
    assert n == 1472 and ones_first == 88


def test_from_sam_and_pack():
    m = np.array([[0, 1], [1, 1], [0, 0]], bool)
    rec = {"size": [3, 2], "counts": [1, 1, 1, 2, 1]}
    assert rle.from_sam(rec, 3, 2).tolist() == [1, 1, 1, 2, 1] and rle.from_sam({"segmentation": rec, "bbox": [0, 0, 2, 2]}).dtype == np.uint32
    assert np.array_equal(rle.decode(rle.from_sam(rec), 3, 2), m)
    for bad in ({"size": [2, 3], "counts": [1, 1, 1, 2, 1]}, ):
        with pytest.raises(ValueError):
            rle.from_sam(bad, 3, 2)
    with pytest.raises(ValueError):
        rle.from_sam({"size": [3, 2], "counts": [1, 1, 1, 2]})            # sums to 5
    with pytest.raises(ValueError):
        rle.from_sam({"size": [3, 2], "counts": "52203"})                 # COCO's compressed string
    counts, run_off, n_masks = rle.pack([[[1, 1, 1, 2, 1], [6]], [], [[0, 6]]])
    assert counts.dtype == np.uint32 and run_off.dtype == np.int64 and n_masks.dtype == np.int32
    assert counts.tolist() == [1, 1, 1, 2, 1, 6, 0, 6] and run_off.tolist() == [0, 5, 6, 8] and n_masks.tolist() == [2, 0, 1]
    assert rle.is_rle_records([rec]) and rle.is_rle_records([{"segmentation": rec}]) and not rle.is_rle_records(np.zeros((1, 3, 2), bool))
    assert not rle.is_rle_records([{"segmentation": m}])


# ---------------------------------------------------------------------------------------- the two handle-less calls, simulator
@emu
@pytest.mark.parametrize("M", RC.M_CASES)
def test_rle_to_bitsets_and_masks_emu(L, M):
    from holoagent_amd._lib import rle_to_bitsets, rle_to_masks
    for name, counts, dense in RC.frames_for(M):
        want = RC.numpy_bitsets(dense)
        got = rle_to_bitsets(counts, RC.H0, RC.W0, lib_=L)
        assert got.dtype == np.uint64 and got.shape == want.shape and np.array_equal(got, want), (M, name)
        assert np.array_equal(rle_to_masks(counts, RC.H0, RC.W0, lib_=L), dense.astype(np.uint8)), (M, name)
    if M >= 64:       # the frame whose masks all cover one pixel: every full word of that pixel has all its bits
        p = RC.SAME_PIXEL[0] * RC.W0 + RC.SAME_PIXEL[1]
        assert (got[p, : M // 64] == np.uint64(0xFFFFFFFFFFFFFFFF)).all()


@emu
def test_rle_no_masks_emu(L):
    from holoagent_amd._lib import rle_to_bitsets, rle_to_masks
    got = rle_to_bitsets([], 5, 70, lib_=L)                   # (two column tiles, the second one 6 columns wide)
    assert got.shape == (350, 1) and not got.any()
    assert rle_to_masks([], 5, 70, lib_=L).shape == (0, 5, 70)


# ---------------------------------------------------------------------------------------------- build equality, simulator
@emu
@pytest.mark.parametrize("how", ["one call", "one call per frame", "several staging chunks"])
def test_build_equals_dense_emu(L, scene_and_dense, how, monkeypatch):
    frames, dense = scene_and_dense
    assert [f["masks"].shape[0] for f in frames] == [3, 6, 0, 5, 1, 4] and len(dense["instances"]) >= 2
    rles = RC.frame_rles(frames)
    if how == "several staging chunks":                     # (a frame has ~100 counts: three or four chunks, checked in a pass of
        monkeypatch.setenv("HMSG_DEBUG_RLE_CHUNK_COUNTS", "150")   # their own before the first bitset is written)

    def hand_over(sc, S):
        if how == "one call per frame":
            for f in range(len(frames)):
                sc.add_frame_features_rle(f, [rles[f]], S["f_g"][f:f + 1], S["f_masked"][f:f + 1], S["f_crop"][f:f + 1])
        else:
            sc.add_frame_features_rle(0, rles, S["f_g"], S["f_masked"], S["f_crop"])
    RC.assert_same_build(dense, RC.build(L, frames, hand_over))


# ---------------------------------------------------------------------------------------------- malformed records, simulator
def _malformed(frames):
    """[(name, (counts, run_off, n_masks), what the message must name)] for the hand-over of ALL frames; mask 9 is frame 3's first"""
    counts, run_off, n_masks = rle.pack(RC.frame_rles(frames))
    out = []
    ro = run_off.copy(); ro[0] = 1
    out.append(("run_off[0] != 0", (counts, ro, n_masks), "mask 0"))
    ro = run_off.copy(); ro[10] = ro[9] - 1
    out.append(("run_off decreases", (counts, ro, n_masks), "mask 9"))
    ro = run_off.copy(); ro[10] = ro[9]
    out.append(("a mask with no counts", (counts, ro, n_masks), "mask 9"))
    c = counts.copy(); c[run_off[9]] += 1
    out.append(("sum too long", (c, run_off, n_masks), "mask 9 "))
    c = counts.copy(); j = run_off[9] + int(np.argmax(counts[run_off[9]:run_off[10]])); c[j] -= 1
    out.append(("sum too short", (c, run_off, n_masks), "mask 9 "))
    c = counts.copy(); c[run_off[18]:run_off[19]] = 0xFFFFFFFF                      # (sums past 2^32: the totals are 64-bit)
    out.append(("sum overflows 32 bits", (c, run_off, n_masks), "mask 18 "))
    nm = n_masks.copy(); nm[4] = 7
    out.append(("n_masks above M", (counts, run_off, nm), "frame 4"))
    nm = n_masks.copy(); nm[2] = -1
    out.append(("n_masks negative", (counts, run_off, nm), "frame 2"))
    return out


@emu
def test_malformed_records_are_refused_emu(L, scene_and_dense):
    from holoagent_amd._lib import HmsgError
    frames, dense = scene_and_dense
    assert sum(f["masks"].shape[0] for f in frames) == 19

    def hand_over(sc, S):
        for name, bad, names in _malformed(frames):
            with pytest.raises(HmsgError) as e:
                sc.add_frame_features_rle(0, bad, S["f_g"], S["f_masked"], S["f_crop"])
            assert str(e.value).startswith("[%d]" % HMSG_ERR_INVALID) and names in str(e.value), (name, str(e.value))
            assert sc.frame_num_masks(0) == -1, name                               # nothing was handed over
        # ... and after a good first half a bad second one leaves the first as it was
        half = 3
        sc.add_frame_features_rle(0, RC.frame_rles(frames[:half]), S["f_g"][:half], S["f_masked"][:half], S["f_crop"][:half])
        counts, run_off, n_masks = rle.pack(RC.frame_rles(frames[half:]))
        c = counts.copy(); c[-1] += 5
        with pytest.raises(HmsgError, match="mask 9 "):                            # (its last mask: frame 2 of the hand-over, mask 3)
            sc.add_frame_features_rle(half, (c, run_off, n_masks), S["f_g"][half:], S["f_masked"][half:], S["f_crop"][half:])
        assert sc.frame_num_masks(half - 1) == 0 and sc.frame_num_masks(half) == -1
        sc.add_frame_features_rle(half, (counts, run_off, n_masks), S["f_g"][half:], S["f_masked"][half:], S["f_crop"][half:])
    RC.assert_same_build(dense, RC.build(L, frames, hand_over))


@emu
def test_malformed_records_handle_less_emu(L):
    counts, run_off, _ = rle.pack([[rle.encode(np.eye(4, 5, dtype=bool)), rle.encode(np.zeros((4, 5), bool))]])
    out = np.full((20, 1), 7, np.uint64)
    dense = np.full((2, 4, 5), 7, np.uint8)
    for c, ro in ((counts, run_off + 1), (counts, np.array([0, 3, 2], np.int64)), (counts, np.array([0, len(counts), len(counts)], np.int64)),
                  (np.concatenate([counts[:-1], [19]]).astype(np.uint32), run_off)):
        assert L.c.hmsg_rle_to_bitsets(0, 4, 5, 2, C.c_void_p(c.ctypes.data), C.c_void_p(ro.ctypes.data), C.c_void_p(out.ctypes.data)) == HMSG_ERR_INVALID
        assert L.c.hmsg_rle_to_masks(0, 4, 5, 2, C.c_void_p(c.ctypes.data), C.c_void_p(ro.ctypes.data), C.c_void_p(dense.ctypes.data)) == HMSG_ERR_INVALID
    assert (out == 7).all() and (dense == 7).all()          # nothing was written
    assert L.c.hmsg_rle_to_bitsets(0, 4, 5, 257, None, C.c_void_p(run_off.ctypes.data), C.c_void_p(out.ctypes.data)) == HMSG_ERR_INVALID


@emu
def test_other_refusals_match_the_dense_call_emu(L, scene_and_dense):
    """the order check and the missing n_masks: the run-length call refuses what the dense call refuses"""
    from holoagent_amd._lib import HmsgError, _ptr
    frames, _ = scene_and_dense
    sc = PC.make_scene(L, frames, dict(RC.SCENE_OVER, feat_dim=32))
    S = PC.stack_frames(frames)
    sc.add_frames(S["rgb"], S["depth"], S["pose"], S["K"])
    r1 = RC.frame_rles(frames[1:2])
    with pytest.raises(HmsgError, match="order"):
        sc.add_frame_features_rle(1, r1, S["f_g"][1:2], S["f_masked"][1:2], S["f_crop"][1:2])
    counts, run_off, _ = rle.pack(r1)
    rc = L.c.hmsg_add_frame_features_rle(sc.h, 0, 1, 6, _ptr(counts), _ptr(run_off), None, _ptr(S["f_g"]), _ptr(S["f_masked"]), _ptr(S["f_crop"]))
    assert rc == HMSG_ERR_INVALID and b"n_masks" in L.c.hmsg_last_error(sc.h)
    sc.close()


# ---------------------------------------------------------------------------------------------- the strict-C host, simulator
@emu
def test_c_host_rle_emu(L, scene_and_dense, tmp_path):
    frames, dense = scene_and_dense
    sizes = RC.c_host_instances(PC.EMU_PATH, tmp_path, frames, RC.SCENE_OVER)
    assert sizes == [len(p) for p in dense["instances"]] and len(sizes) >= 2


# ---------------------------------------------------------------------------------------------- Graph.create_feature_map
@emu
def test_graph_create_feature_map_takes_rle_records_emu(L):
    from holoagent_amd.graph import Graph
    from tests.graph_fixture import SynthDataset, SynthEncoders, tiny_scene

    class RleEncoders(SynthEncoders):
        dense_seen = 0

        def extract(self, rgb):
            o = super().extract(rgb)
            H, W = o["masks"].shape[1:]
            o["masks"] = [dict(segmentation={"size": [H, W], "counts": rle.encode(m).tolist()}, bbox=[0, 0, W, H]) for m in o["masks"]]
            return o

    got = []
    for enc_cls in (SynthEncoders, RleEncoders):
        ds = SynthDataset(tiny_scene(3, 32))
        enc = enc_cls(ds, ["background", "wall"])
        cfg = dict(main=dict(device_id=0), models=dict(clip=dict(type="ViT-B/32", feat_dim=32)),
                   pipeline=dict(voxel_size=0.07, skip_frames=1, merge_type="sequential", max_masks=8, room_level_beside_fusion=False))
        g = Graph(cfg, dataset=ds, encoders=enc, lib=L)

        def cheap_scene(H, W, max_frames, rle_only=enc_cls is RleEncoders):
            # coarse voxels and a small outlier filter (the config's literal 1000 neighbours cost the simulator half a minute);
            # with run-length records the dense call must not be reached
            from holoagent_amd._lib import Scene
            sc = Scene(lib_=L, feat_dim=32, height=H, width=W, max_frames=max_frames, max_masks=8, **RC.SCENE_OVER)
            if rle_only:
                sc.add_frame_features = None
            return sc
        g._scene_from_config = cheap_scene
        g.create_feature_map()
        got.append(([np.asarray(p.points) for p in g.mask_pcds], [np.asarray(f) for f in g.mask_feats]))
    (pa, fa), (pb, fb) = got
    assert len(pa) == len(pb) >= 1
    for x, y in zip(pa, pb):
        assert np.array_equal(x, y)
    for x, y in zip(fa, fb):
        assert np.array_equal(x, y)
