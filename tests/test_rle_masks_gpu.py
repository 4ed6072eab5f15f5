"""Run-length masks on the MI355X (include/hmsg.h: hmsg_add_frame_features_rle, hmsg_rle_to_bitsets, hmsg_rle_to_masks): the decode
kernels against bitsets computed in numpy, from host arrays and from torch device tensors; the reference-run fixtures handed over as
run-length records through every check the dense build gets (tests/parity_common.py) and bit-equal with the dense build; the strict-C
host; the encoder hand-off with the masks made on the device from the records.  Only well-formed records here: the malformed ones
are refused before a kernel writes anything, and that is pinned on the kernel simulator (tests/test_rle_masks.py)."""
import os

import numpy as np
import pytest

from holoagent_amd import rle
from tests import golden_io as GI
from tests import parity_common as PC
from tests import rle_cases as RC

pytestmark = pytest.mark.gpu

LIB = os.path.join(RC.ROOT, "holoagent_amd", "libhmsg.so")


@pytest.fixture(scope="module")
def L():
    from holoagent_amd._lib import HmsgLib
    return HmsgLib()          # raises if the HIP library is missing -- no fallback


def _dev(a):
    import torch
    if a.dtype == np.uint32:                                  # (same bits; torch's uint32 support is partial)
        a = a.view(np.int32)
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", 0)).contiguous()


def _check_frame(L, counts, dense, H, W, tag):
    from holoagent_amd._lib import rle_to_bitsets, rle_to_masks
    want = RC.numpy_bitsets(dense)
    want_masks = dense.astype(np.uint8)
    got = rle_to_bitsets(counts, H, W, lib_=L)
    assert got.dtype == np.uint64 and got.shape == want.shape and np.array_equal(got, want), tag
    assert np.array_equal(rle_to_masks(counts, H, W, lib_=L), want_masks), tag
    c, ro, _ = rle.pack([counts])
    d_bits = rle_to_bitsets((_dev(c), _dev(ro)), H, W, lib_=L)
    d_masks = rle_to_masks((_dev(c), _dev(ro)), H, W, lib_=L)
    assert d_bits.is_cuda and d_masks.is_cuda
    assert np.array_equal(d_bits.cpu().numpy().view(np.uint64), want), tag
    assert np.array_equal(d_masks.cpu().numpy(), want_masks), tag
    return got


@pytest.mark.parametrize("M", RC.M_CASES)
def test_rle_to_bitsets_and_masks(L, M):
    for name, counts, dense in RC.frames_for(M):
        got = _check_frame(L, counts, dense, RC.H0, RC.W0, (M, name))
    if M >= 64:
        p = RC.SAME_PIXEL[0] * RC.W0 + RC.SAME_PIXEL[1]
        assert (got[p, : M // 64] == np.uint64(0xFFFFFFFFFFFFFFFF)).all()


def test_rle_to_bitsets_and_masks_640x480(L):
    from holoagent_amd.synth import SceneSpec, SynthScene
    spec = SceneSpec(seed=11, rooms_x=1, rooms_z=1, room_size=(4.0, 2.6, 3.5), objects_per_room=6, width=640, height=480, n_frames=2,
                     n_masks=32, feat_dim=8)
    dense = SynthScene(spec).frame(1)["masks"].astype(bool)
    assert dense.shape == (32, 480, 640) and dense.any(axis=(1, 2)).sum() >= 4
    _check_frame(L, [rle.encode(m) for m in dense], dense, 480, 640, "640x480")


def _rle_scene(L, frames, cfg_over):
    H, W = frames[0]["depth"].shape
    over = dict(height=H, width=W, max_frames=len(frames), max_masks=max(max(f["masks"].shape[0] for f in frames), 1))
    over.update(cfg_over)
    return RC.rle_scene_class()(lib_=L, **over)


@pytest.mark.parametrize("name", ["build_hier", "build_ragged"])
def test_reference_run_fixtures_as_rle(L, name):
    """What tests/test_gpu_parity.py::test_full_build_against_oracle_and_reference_golden checks on the dense build, on a build whose
    masks went over run-length coded (build_ragged: 1 .. 70 masks per frame, two bitset words), in two hand-overs as there; then bit
    equality with the dense build at every getter."""
    z = GI.load(name)
    frames = GI.unpack_frames(z)
    cfg = GI.unpack_cfg(z)
    over = dict(feat_dim=cfg["feat_dim"], merge_type=1 if cfg["merge_type"] == "hierarchical" else 0)
    sc = _rle_scene(L, frames, over)
    S, ref_pts, ref_cols = PC.check_map(sc, frames, cfg)
    assert np.array_equal(ref_pts, z["ref_cloud"])
    ref_feats, _ = PC.check_fuse(sc, frames, S, cfg, ref_pts, ref_cols, check_masks=True)
    got_rle = dict(fp=[sc.frame_fp(i) for i in range(len(frames))], masks3d=[sc.frame_masks3d(i) for i in range(len(frames))],
                   map_feats=sc.map_feats(counter=True))
    got, feats = PC.check_merge_pool(sc, frames, cfg, ref_pts, ref_feats)
    PC.check_against_reference_run(name, z, sc, got, feats)
    got_rle.update(instances=got, pooled=feats)
    sc.close()
    RC.assert_same_build(RC.build(L, frames, RC.dense_hand_over, over), got_rle)


def test_device_tensors_hand_over(L):
    """counts, run_off, n_masks and the F tables as torch device tensors: the same build as from numpy arrays"""
    frames = RC.small_scene()
    want = RC.build(L, frames, RC.dense_hand_over)

    def hand_over(sc, S):
        counts, run_off, n_masks = rle.pack(RC.frame_rles(frames))
        sc.add_frame_features_rle(0, (_dev(counts), _dev(run_off), _dev(n_masks)), _dev(S["f_g"]), _dev(S["f_masked"]), _dev(S["f_crop"]))
    RC.assert_same_build(want, RC.build(L, frames, hand_over))


def test_c_host_rle(L, tmp_path):
    frames = RC.small_scene()
    want = RC.build(L, frames, RC.dense_hand_over)
    sizes = RC.c_host_instances(LIB, tmp_path, frames, RC.SCENE_OVER)
    assert sizes == [len(p) for p in want["instances"]] and len(sizes) >= 2


def test_encoder_handoff_rle(L):
    """encoder_handoff.handoff_frame_rle: records -> device masks -> encoder inputs -> module -> hmsg_add_frame_features_rle gives the
    features and the map of the dense hand-off (embed_frame_reference_inputs + add_frame_features) bit for bit."""
    import torch
    from holoagent_amd.encoder_handoff import embed_frame_reference_inputs, handoff_frame_rle, make_vit_b32
    from holoagent_amd.synth import SceneSpec, SynthScene
    dev = torch.device("cuda", 0)
    spec = SceneSpec(seed=21, rooms_x=1, rooms_z=1, room_size=(3.6, 2.5, 3.2), objects_per_room=4, width=128, height=96, n_frames=2, n_masks=4,
                     feat_dim=64)
    scn = SynthScene(spec)
    frames = [scn.frame(i) for i in range(spec.n_frames)]
    S = PC.stack_frames(frames)
    torch.manual_seed(1)
    enc = make_vit_b32(torch, dim_out=64, width=128, layers=2, heads=4, patch=32, image=224).to(dev).half().eval()
    maps = []
    for route in ("dense", "rle"):
        sc = PC.make_scene(L, frames, dict(feat_dim=64, outlier_nb_points=200))
        sc.add_frames(S["rgb"], S["depth"], S["pose"], S["K"])
        sc.finalize_map()
        feats = []
        for f in range(spec.n_frames):
            seg = np.ascontiguousarray(S["masks"][f])
            bbox = np.zeros((seg.shape[0], 4))
            for m in range(seg.shape[0]):
                ys, xs = np.nonzero(seg[m])
                bbox[m] = [xs.min(), ys.min(), xs.max() - xs.min() + 1, ys.max() - ys.min() + 1] if len(xs) else [0, 0, 8, 8]
            image = torch.from_numpy(np.ascontiguousarray(S["rgb"][f])).to(dev)
            if route == "dense":
                t_seg = torch.from_numpy(seg).to(dev)
                f_g, f_masked, f_crop = embed_frame_reference_inputs(L, enc, image, t_seg, bbox, torch)
                sc.add_frame_features(f, t_seg[None], f_g, f_masked[None], f_crop[None])
            else:
                counts, run_off, _ = rle.pack([[rle.encode(m) for m in seg]])
                f_g, f_masked, f_crop, t_seg = handoff_frame_rle(L, sc, enc, f, image, (counts, run_off), bbox, torch)
                assert t_seg.is_cuda and np.array_equal(t_seg.cpu().numpy(), seg)
            feats.append(torch.cat([f_g, f_masked, f_crop]).cpu().numpy())
        sc.fuse_frames()
        maps.append((feats, sc.map_feats(counter=True), [sc.frame_fp(f) for f in range(spec.n_frames)]))
        sc.close()
    (fa, ma, pa), (fb, mb, pb) = maps
    assert all(np.array_equal(x, y) for x, y in zip(fa, fb)) and all(np.array_equal(x, y) for x, y in zip(pa, pb))
    assert np.array_equal(ma[0], mb[0]) and np.array_equal(ma[1], mb[1]) and np.abs(ma[0]).sum() > 0
