"""hmsg_sam_postprocess on the MI355X (include/hmsg.h) against the restatement tests/sam_post_oracle.py, exactly: the case table of
tests/sam_post_cases.py from host arrays and from torch device tensors (outputs left on the device), one batch at the workload's
size, and the hand-off of a frame from the decoder's logits on (encoder_handoff.handoff_frame_logits)."""
import numpy as np
import pytest

from tests import parity_common as PC
from tests import sam_post_cases as CS
from tests import sam_post_oracle as O
from tests.test_sam_postprocess import GOLDEN, assert_equal, expected

pytestmark = pytest.mark.gpu
CASES = {c[0]: c for c in CS.cases()}


@pytest.fixture(scope="module")
def L():
    from holoagent_amd._lib import HmsgLib
    return HmsgLib()          # raises if the HIP library is missing -- no fallback


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", 0)).contiguous()


def _to_host(r):
    out = dict(r)
    for k in CS.RESULT_KEYS:
        assert r[k].is_cuda, k
        a = r[k].cpu().numpy()
        out[k] = a.view(np.uint32) if k == "counts" else a
    return out


@pytest.mark.parametrize("name", list(CASES))
def test_case_from_host_arrays_and_device_tensors(L, golden, name):
    from holoagent_amd._lib import sam_postprocess
    _, logits, iou, prm = CASES[name]
    want = expected(golden, name)
    assert_equal(sam_postprocess(logits, iou, lib_=L, **prm), want, name + " (host arrays)")
    assert_equal(_to_host(sam_postprocess(_dev(logits), _dev(iou), lib_=L, **prm)), want, name + " (device tensors)")


def test_short_arrays_on_the_device(L, golden):
    """the refusal leaves device arrays as they were, and the binding's second call fills arrays of the size the first asked for"""
    import ctypes as C
    import torch
    from holoagent_amd._lib import _ptr, sam_post_params, sam_postprocess
    _, logits, iou, prm = CASES["seeded_area12"]
    want = expected(golden, "seeded_area12")
    n, nc = len(want["keep_idx"]), len(want["counts"])
    d_logits, d_iou = _dev(logits), _dev(iou)
    H, W = logits.shape[-2:]
    for max_out, cap in ((n - 1, nc), (n, nc - 1)):
        bufs = [torch.full((k,), 0x5a, dtype=torch.uint8, device=d_logits.device) for k in (4 * n, 4 * nc, 8 * (n + 1), 32 * n, 4 * n, 4 * n, n * H * W)]
        g_n, g_nc = C.c_int32(-7), C.c_int64(-7)
        rc = L.c.hmsg_sam_postprocess(0, C.byref(sam_post_params(L, **prm)), len(iou), H, W, _ptr(d_logits), _ptr(d_iou), max_out, cap,
                                      C.byref(g_n), C.byref(g_nc), *[_ptr(b) for b in bufs], None)
        assert rc == -1 and (g_n.value, g_nc.value) == (n, nc) and all(bool((b == 0x5a).all()) for b in bufs)
    assert_equal(_to_host(sam_postprocess(d_logits, d_iou, max_out=1, counts_cap=1, lib_=L, **prm)), want, "after one retry")


def test_workload_size_640x480_144(L):
    """N = 144 logit images of 640 x 480 (177 MB): grid and buffers sized as the workload sizes them"""
    from holoagent_amd._lib import sam_postprocess
    logits, iou = CS.seeded_logits(3, 144, 480, 640)
    want = O.postprocess(logits, iou, min_mask_region_area=100)
    assert want["stage"]["after_first_nms"] > want["n"] > 8 and want["stage"]["changed_kept"] > 0
    got = _to_host(sam_postprocess(_dev(logits), _dev(iou), lib_=L, min_mask_region_area=100))
    assert_equal(got, want, "640 x 480, N = 144")


def test_handoff_frame_logits(L):
    """encoder_handoff.handoff_frame_logits (logits -> records on the device -> masks -> encoder inputs -> module ->
    hmsg_add_frame_features_rle) gives the features, frame tables and map of handoff_frame_rle fed the restatement's records and boxes"""
    import torch
    from holoagent_amd.encoder_handoff import handoff_frame_logits, handoff_frame_rle, make_vit_b32
    from holoagent_amd.synth import SceneSpec, SynthScene
    dev = torch.device("cuda", 0)
    spec = SceneSpec(seed=21, rooms_x=1, rooms_z=1, room_size=(3.6, 2.5, 3.2), objects_per_room=4, width=128, height=96, n_frames=2, n_masks=4,
                     feat_dim=64)
    scn = SynthScene(spec)
    frames = [scn.frame(i) for i in range(spec.n_frames)]
    S = PC.stack_frames(frames)
    torch.manual_seed(1)
    enc = make_vit_b32(torch, dim_out=64, width=128, layers=2, heads=4, patch=32, image=224).to(dev).half().eval()
    prm = dict(min_mask_region_area=100)
    maps, n_masks = [], 0
    for route in ("rle", "logits"):
        sc = PC.make_scene(L, frames, dict(feat_dim=64, outlier_nb_points=200))
        sc.add_frames(S["rgb"], S["depth"], S["pose"], S["K"])
        sc.finalize_map()
        feats = []
        for f in range(spec.n_frames):
            seg = S["masks"][f] != 0
            logits = np.where(seg, np.float32(4.0), np.float32(-4.0)).astype(np.float32)
            logits[:, 5:8, 100:103] = 4.0                                  # a speck for the small-region pass
            iou = np.linspace(0.99, 0.9, seg.shape[0]).astype(np.float32)
            image = torch.from_numpy(np.ascontiguousarray(S["rgb"][f])).to(dev)
            want = O.postprocess(logits, iou, **prm)
            n_masks += want["n"]
            if route == "rle":
                f_g, f_masked, f_crop, t_seg = handoff_frame_rle(L, sc, enc, f, image, (want["counts"], want["run_off"]), want["bbox"], torch)
            else:
                f_g, f_masked, f_crop, t_seg, post = handoff_frame_logits(L, sc, enc, f, image, _dev(logits), _dev(iou), torch, **prm)
                assert post["counts"].is_cuda and post["n"] == want["n"]
            assert np.array_equal(t_seg.cpu().numpy(), want["masks"])
            feats.append(torch.cat([f_g, f_masked, f_crop]).cpu().numpy())
        sc.fuse_frames()
        maps.append((feats, sc.map_feats(counter=True), [sc.frame_fp(f) for f in range(spec.n_frames)]))
        sc.close()
    (fa, ma, pa), (fb, mb, pb) = maps
    assert n_masks >= 4
    assert all(np.array_equal(x, y) for x, y in zip(fa, fb)) and all(np.array_equal(x, y) for x, y in zip(pa, pb))
    assert np.array_equal(ma[0], mb[0]) and np.array_equal(ma[1], mb[1]) and np.abs(ma[0]).sum() > 0
