"""The CLIP preprocess on the device (include/hmsg.h: hmsg_clip_preprocess_batch, hmsg_frame_encoder_inputs) against Pillow's
own bits: open_clip's inference transform Resize(S, BICUBIC) -> CenterCrop(S) -> ToTensor -> Normalize, which the reference
runs on every crop and frame (utils/clip_utils.py:72-73, 88-89).  The oracle is Pillow (tests/golden/clip_preprocess.npz, made
by scripts/gen_golden_clip_preprocess.py, and the installed Pillow where it imports); the numpy restatement
(tests/clip_preprocess_oracle.py) is checked against both and stands in only where Pillow is missing.  Everything is compared
with np.array_equal: the transform is integer arithmetic on host-made tables, so there is no tolerance to state."""
import functools
import hashlib
import os

import numpy as np
import pytest

from tests import clip_preprocess_oracle as O
from tests import parity_common as PC

GOLD = os.path.join(os.path.dirname(__file__), "golden", "clip_preprocess.npz")
CROPS = os.path.join(os.path.dirname(__file__), "golden", "crops.npz")
CASE = {c[0]: c for c in O.CASES}
ALL = [(c[0], k) for c in O.CASES for k in O.KINDS]
SIM = ["upscale", "pixel", "crop512"]            # sides of at most 128, plus one 512 -> 224 image (crop512's first)


def _have_pil():
    try:
        import PIL  # noqa: F401
        return True
    except ImportError:
        return False


@functools.lru_cache(maxsize=None)
def _gold():
    return np.load(GOLD)


def _check_gold(name, kind, u8):
    """u8 [n, S, S, 3] (the first n images of the case) against the golden file's sub-samples and SHA-1s"""
    z, key = _gold(), f"{name}_{kind}"
    assert [int(v) for v in z[key + "_shape"]] == list(CASE[name][1:]) and int(z[key + "_seed"]) == O.case_seed(name, kind)
    for i, r in enumerate(u8):
        assert np.array_equal(O.subsample(r, i), z[key + "_sub"][i]), (key, i)
        assert hashlib.sha1(np.ascontiguousarray(r).tobytes()).hexdigest() == str(z[key + "_sha1"][i]), (key, i)


@functools.lru_cache(maxsize=None)
def _reference(name, kind):
    """(input u8 [B, H, W, 3], expected u8 [B, S, S, 3]): Pillow where it imports, else the restatement; made once, read-only"""
    imgs = O.make_input(name, kind)
    resize = O.pil_resize if _have_pil() else O.resize_bicubic_u8
    ref = np.stack([O.resize_center_crop_u8(im, CASE[name][4], resize) for im in imgs])
    _check_gold(name, kind, ref)
    imgs.setflags(write=False)
    ref.setflags(write=False)
    return imgs, ref


# ------------------------------------------------------------------ 1. CPU, no library
@pytest.mark.parametrize("name,kind", ALL)
def test_restatement_equals_golden(name, kind):
    S = CASE[name][4]
    _check_gold(name, kind, [O.resize_center_crop_u8(im, S) for im in O.make_input(name, kind)])


@pytest.mark.parametrize("name,kind", ALL)
def test_restatement_equals_live_pillow(name, kind):
    pytest.importorskip("PIL")
    S = CASE[name][4]
    for im in O.make_input(name, kind):
        assert np.array_equal(O.resize_center_crop_u8(im, S), O.resize_center_crop_u8(im, S, O.pil_resize))


def test_size_rules():
    assert O.resize_dims(480, 641, 224) == (299, 224) and O.center_crop_offset(299, 224) == 38       # 37.5 -> 38
    assert O.resize_dims(480, 640, 224) == (298, 224) and O.center_crop_offset(298, 224) == 37
    assert O.resize_dims(100, 37, 224) == (224, 605) and O.center_crop_offset(605, 224) == 190       # 190.5 -> 190
    assert O.resize_dims(224, 500, 224) == (500, 224) and O.resize_dims(300, 224, 224) == (224, 300)


def test_float_stage_equals_torch_cpu():
    """ToTensor + Normalize as torchvision does them on the CPU, on all 256 x 3 values; float16 = .half()"""
    import torch
    u8 = np.ascontiguousarray(np.broadcast_to(np.arange(256, dtype=np.uint8)[:, None, None], (256, 1, 3)))     # an [H = 256, W = 1, 3] image
    t = torch.from_numpy(u8).permute(2, 0, 1).contiguous().to(torch.float32).div(255)                             # ToTensor
    mean, std = torch.as_tensor(O.MEAN, dtype=torch.float32), torch.as_tensor(O.STD, dtype=torch.float32)
    t = t.sub(mean.view(-1, 1, 1)).div(std.view(-1, 1, 1))                                                        # Normalize
    mine = O.to_tensor_normalize(u8)
    assert np.array_equal(t.numpy(), mine) and np.array_equal(mine[:, :, 0], O.normalize_table())
    assert np.array_equal(t.half().numpy(), mine.astype(np.float16))


# ------------------------------------------------------------------ 2. / 3. the library
def check_lib(L, names):
    from holoagent_amd._lib import HmsgClipPreprocess, HmsgError, HmsgLib, _ptr, clip_preprocess  # noqa: F401
    import ctypes as C
    sim = L.path == PC.EMU_PATH
    for name in names:
        for kind in O.KINDS:
            imgs, ref = _reference(name, kind)
            if sim and name == "crop512":
                imgs, ref = imgs[:1], ref[:1]
            out, u8 = clip_preprocess(imgs, size=CASE[name][4], return_u8=True, lib_=L)
            assert np.array_equal(u8, ref), (name, kind)
            want = O.to_tensor_normalize(ref)
            assert out.dtype == np.float32 and np.array_equal(out, want), (name, kind)
            half = clip_preprocess(imgs, size=CASE[name][4], f16=True, lib_=L)
            assert half.dtype == np.float16 and np.array_equal(half, want.astype(np.float16)), (name, kind)
    imgs, ref = _reference("upscale", "bytes")
    mean, std = (0.5, 0.25, 0.125), (0.5, 2.0, 0.3)                                          # a non-default mean / std
    assert np.array_equal(clip_preprocess(imgs, mean=mean, std=std, lib_=L), O.to_tensor_normalize(ref, mean, std))
    assert np.array_equal(clip_preprocess(imgs[0], lib_=L), O.to_tensor_normalize(ref[0]))  # a single [H, W, 3] image
    one, one_ref = _reference("pixel", "bytes")
    assert np.array_equal(clip_preprocess(one[0], lib_=L), O.to_tensor_normalize(one_ref[0]))  # 3 bytes in all: no room for a 4-byte load
    # B = 0 is OK and touches nothing; the refusals
    p = HmsgClipPreprocess()
    L.c.hmsg_clip_default_preprocess(C.byref(p))
    assert p.size == 224 and p.out_f16 == 0 and list(p.mean) == [np.float32(v) for v in O.MEAN] and list(p.std) == [np.float32(v) for v in O.STD]
    img = np.ascontiguousarray(imgs[0])
    out = np.zeros((1, 3, 224, 224), np.float32)
    call = L.c.hmsg_clip_preprocess_batch
    assert call(0, C.byref(p), 0, 100, 37, None, None, None, None) == 0
    assert call(0, C.byref(p), 1, 100, 37, _ptr(img), _ptr(out), None, None) == 0 and np.array_equal(out[0], O.to_tensor_normalize(ref[0]))
    assert call(0, None, 1, 100, 37, _ptr(img), _ptr(out), None, None) == -1
    assert call(0, C.byref(p), 1, 100, 37, None, _ptr(out), None, None) == -1
    assert call(0, C.byref(p), 1, 100, 37, _ptr(img), None, None, None) == -1
    assert call(0, C.byref(p), -1, 100, 37, _ptr(img), _ptr(out), None, None) == -1
    for size in (0, 2000):
        with pytest.raises(HmsgError):
            clip_preprocess(img, size=size, lib_=L)
    for std in ((0.3, 0.0, 0.3), (0.3, 0.3, float("nan")), (float("inf"), 0.3, 0.3)):
        with pytest.raises(HmsgError):
            clip_preprocess(img, std=std, lib_=L)
    assert call(0, C.byref(p), 1, 20000, 1, _ptr(img), _ptr(out), None, None) == -3          # a side above the cap: refused before any read


@pytest.mark.skipif(not os.path.exists(PC.EMU_PATH), reason="kernel simulator not built")
def test_simulator_equals_pillow():
    from holoagent_amd._lib import HmsgLib
    check_lib(HmsgLib(PC.EMU_PATH), SIM)


@pytest.mark.gpu
def test_gpu_equals_pillow():
    from holoagent_amd._lib import lib
    check_lib(lib(), [c[0] for c in O.CASES])


# ------------------------------------------------------------------ 4. device pointers
@pytest.mark.gpu
def test_gpu_device_pointers():
    """images and outputs resident in HBM (how the encoder consumes them): the same bits as the host-pointer call"""
    import torch
    from holoagent_amd._lib import clip_preprocess
    dev = torch.device("cuda:0")
    for name in ("crop512", "halfeven", "cropx"):
        imgs, ref = _reference(name, "bytes")
        for f16 in (False, True):
            host = clip_preprocess(imgs, f16=f16)
            out, u8 = clip_preprocess(torch.from_numpy(np.array(imgs)).to(dev), f16=f16, return_u8=True)
            assert out.is_cuda and u8.is_cuda and np.array_equal(out.cpu().numpy(), host) and np.array_equal(u8.cpu().numpy(), ref)


# ------------------------------------------------------------------ 5. one frame's encoder inputs
def _gold_frame():
    z = np.load(CROPS)
    masks = [{"segmentation": s, "bbox": [int(v) for v in b]} for s, b in zip(z["segs"], z["bbox"])]
    return z["image"], masks


@pytest.mark.skipif(not os.path.exists(PC.EMU_PATH), reason="kernel simulator not built")
def test_simulator_frame_encoder_inputs():
    """a small frame on the simulator: rows in the order frame, masked crops, plain crops, against the crop oracle + Pillow"""
    from holoagent_amd._lib import HmsgError, HmsgLib, frame_encoder_inputs
    from oracle import crop_oracle as CO
    L = HmsgLib(PC.EMU_PATH)
    rng = np.random.default_rng(11)
    H, W, M = 48, 70, 3
    image = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    masks = []
    for m in range(M):
        x, y, w, h = 5 + 9 * m, 3 + 4 * m, 20 + m, 17 - m
        seg = np.zeros((H, W), bool)
        seg[y:y + h, x:x + w] = rng.random((h, w)) < 0.6
        masks.append({"segmentation": seg, "bbox": [x, y, w, h]})
    resize = O.pil_resize if _have_pil() else O.resize_bicubic_u8
    crops = CO.crop_all_bounding_boxs(image, masks, True, 6, size=64) + CO.crop_all_bounding_boxs(image, masks, False, 6, size=64)
    want = O.to_tensor_normalize(np.stack([O.resize_center_crop_u8(np.ascontiguousarray(c), 40, resize) for c in [image] + crops]))
    assert np.array_equal(frame_encoder_inputs(image, masks, 6, size=40, crop_size=64, lib_=L), want)
    assert np.array_equal(frame_encoder_inputs(image, masks, 6, size=40, crop_size=64, f16=True, lib_=L), want.astype(np.float16))
    assert np.array_equal(frame_encoder_inputs(image, [], 6, size=40, crop_size=64, lib_=L), want[:1])
    with pytest.raises(HmsgError):
        frame_encoder_inputs(image, [dict(masks[0], bbox=[5, 5, 0, 10])], 0, size=40, crop_size=64, lib_=L)
    assert np.array_equal(frame_encoder_inputs(image, masks, 6, size=40, crop_size=64, lib_=L), want)     # (a refused call leaves nothing behind)


@pytest.mark.gpu
def test_gpu_frame_encoder_inputs():
    import ctypes as C
    import torch
    from holoagent_amd._lib import HmsgError, _clip_params, _ptr, clip_preprocess, crop_all_bounding_boxs, frame_encoder_inputs, lib
    L = lib()
    image, masks = _gold_frame()
    M = len(masks)
    whole = clip_preprocess(image)
    for margin in (0, 50):
        plain, masked = crop_all_bounding_boxs(image, masks, margin)            # (pinned against the reference's crops by tests/test_crops.py)
        got = frame_encoder_inputs(image, masks, margin)
        assert got.shape == (1 + 2 * M, 3, 224, 224)
        assert np.array_equal(got[0], whole)
        assert np.array_equal(got[1:1 + M], clip_preprocess(masked)) and np.array_equal(got[1 + M:], clip_preprocess(plain))
    half = frame_encoder_inputs(image, masks, 50, f16=True)
    assert np.array_equal(half, got.astype(np.float16))
    # image, masks and output as device tensors
    dev = torch.device("cuda:0")
    t_img = torch.from_numpy(image).to(dev)
    t_seg = torch.from_numpy(np.stack([m["segmentation"] for m in masks]).astype(np.uint8)).to(dev)
    t_out = torch.zeros((1 + 2 * M, 3, 224, 224), dtype=torch.float32, device=dev)
    bbox = np.ascontiguousarray([m["bbox"] for m in masks], dtype=np.float64)
    prm = _clip_params(L, 224, False, None, None)
    H, W = image.shape[:2]
    assert L.c.hmsg_frame_encoder_inputs(0, C.byref(prm), H, W, _ptr(t_img), M, _ptr(t_seg), _ptr(bbox), 50.0, 512, _ptr(t_out), None) == 0
    assert np.array_equal(t_out.cpu().numpy(), got)
    assert np.array_equal(frame_encoder_inputs(image, [], 50), whole[None])     # a frame without masks: the frame's row alone
    bad = masks[:2] + [dict(masks[2], bbox=[5, 5, 0, 10])]                      # an empty crop: as in the crop call
    with pytest.raises(HmsgError):
        frame_encoder_inputs(image, bad, 0)
    with pytest.raises(HmsgError):
        frame_encoder_inputs(image, masks, 0, crop_size=510)                    # not a multiple of 4
    assert np.array_equal(frame_encoder_inputs(image, masks, 50), got)          # a refused call launched nothing: the next one is whole


# ------------------------------------------------------------------ 6. the hand-off
@pytest.mark.gpu
def test_gpu_handoff_features_equal_features_of_host_made_inputs():
    """embed_frame_reference_inputs: the module sees the same input bits as with inputs made on the host by Pillow (or the
    restatement) and uploaded, so the features are equal; Scene.add_frame_features takes them as they are."""
    import torch
    from holoagent_amd._lib import HmsgLib
    from holoagent_amd.encoder_handoff import embed_frame_reference_inputs, make_vit_b32
    from holoagent_amd.synth import SceneSpec, SynthScene
    from oracle import crop_oracle as CO
    L = HmsgLib()
    dev = torch.device("cuda", 0)
    spec = SceneSpec(seed=21, rooms_x=1, rooms_z=1, room_size=(3.6, 2.5, 3.2), objects_per_room=4, width=128, height=96, n_frames=2, n_masks=4,
                     feat_dim=64)
    scn = SynthScene(spec)
    frames = [scn.frame(i) for i in range(spec.n_frames)]
    S = PC.stack_frames(frames)
    torch.manual_seed(1)
    enc = make_vit_b32(torch, dim_out=64, width=128, layers=2, heads=4, patch=32, image=224).to(dev).half().eval()
    resize = O.pil_resize if _have_pil() else O.resize_bicubic_u8
    sc = PC.make_scene(L, frames, dict(feat_dim=64, outlier_nb_points=200))
    sc.add_frames(S["rgb"], S["depth"], S["pose"], S["K"])
    sc.finalize_map()
    for f in range(spec.n_frames):
        image, seg = np.ascontiguousarray(S["rgb"][f]), np.ascontiguousarray(S["masks"][f])
        M = seg.shape[0]
        masks = []
        for m in range(M):
            ys, xs = np.nonzero(seg[m])
            box = [int(xs.min()), int(ys.min()), int(xs.max() - xs.min() + 1), int(ys.max() - ys.min() + 1)] if len(xs) else [0, 0, 8, 8]
            masks.append({"segmentation": seg[m].astype(bool), "bbox": box})
        bbox = np.array([m["bbox"] for m in masks], np.float64)
        # the host route: the reference's crops (oracle/crop_oracle.py), then preprocess per image
        crops = CO.crop_all_bounding_boxs(image, masks, True, 50) + CO.crop_all_bounding_boxs(image, masks, False, 50)
        u8 = np.stack([O.resize_center_crop_u8(np.ascontiguousarray(c), 224, resize) for c in [image] + crops])
        x = torch.from_numpy(O.to_tensor_normalize(u8).astype(np.float16)).to(dev)
        with torch.no_grad():
            want = torch.nn.functional.normalize(enc(x).float(), dim=-1)
        t_seg = torch.from_numpy(seg).to(dev)
        f_g, f_masked, f_crop = embed_frame_reference_inputs(L, enc, torch.from_numpy(image).to(dev), t_seg, bbox, torch)
        assert f_g.shape == (1, 64) and f_masked.shape == (M, 64) and f_crop.shape == (M, 64)
        assert torch.equal(torch.cat([f_g, f_masked, f_crop]), want)
        sc.add_frame_features(f, t_seg[None], f_g, f_masked[None], f_crop[None])
    sc.fuse_frames()
    assert np.abs(sc.map_feats()).sum() > 0
    sc.close()
