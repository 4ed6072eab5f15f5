"""The encoder hand-off (north_star: "PyTorch-ROCm only for the wrapped vision / CLIP encoders"): what
perception/models/sam_clip_feats_extractor.py:117-158 does per frame around the CLIP image tower -- global feature of the
frame, features of the 2 M crops (masked and plain, utils/sam_utils.py:119-181 -> hmsg_crop_resize_batch on the device) --
with a random-init ViT-B/32-SHAPED PyTorch module (clip_utils.py:63-94 wraps open_clip's ViT-B/32: patch 32, width 768,
12 layers, 12 heads, 512-d projection; open_clip and its weights are not in this image), and the tensors going to the
library BY DEVICE POINTER (`tensor.data_ptr()`), never through the host.

This is a measurement aid (bench.py reports it beside `value`, never as `value`) and the demonstration that the boundary
takes a live PyTorch-ROCm module's outputs as they are: float32, contiguous, on the device."""
from __future__ import annotations

import ctypes as C
import time

import numpy as np


def make_vit_b32(torch, dim_out=512, width=768, layers=12, heads=12, patch=32, image=224):
    nn = torch.nn

    class Block(nn.Module):
        def __init__(self):
            super().__init__()
            self.ln1, self.ln2 = nn.LayerNorm(width), nn.LayerNorm(width)
            self.attn = nn.MultiheadAttention(width, heads, batch_first=True)
            self.mlp = nn.Sequential(nn.Linear(width, 4 * width), nn.GELU(), nn.Linear(4 * width, width))

        def forward(self, x):
            h = self.ln1(x)
            x = x + self.attn(h, h, h, need_weights=False)[0]
            return x + self.mlp(self.ln2(x))

    class ViT(nn.Module):
        def __init__(self):
            super().__init__()
            self.conv = nn.Conv2d(3, width, patch, patch, bias=False)
            self.cls = nn.Parameter(torch.randn(width) * width ** -0.5)
            self.pos = nn.Parameter(torch.randn((image // patch) ** 2 + 1, width) * width ** -0.5)
            self.pre, self.post = nn.LayerNorm(width), nn.LayerNorm(width)
            self.blocks = nn.Sequential(*[Block() for _ in range(layers)])
            self.proj = nn.Parameter(torch.randn(width, dim_out) * width ** -0.5)

        def forward(self, x):                                  # x: [B, 3, image, image]
            x = self.conv(x).flatten(2).transpose(1, 2)
            x = torch.cat([self.cls.expand(x.shape[0], 1, -1), x], 1) + self.pos
            x = self.blocks(self.pre(x))
            return self.post(x[:, 0]) @ self.proj
    return ViT()


def measure(L, scene, inp, device, torch, frames=8, crop=224, feat_dim=512):
    """`frames` frames of the resident stream through crop -> encoder -> hmsg_add_frame_features, everything on the device.
    scene: a Scene with those frames' geometry added and the map final; inp: bench.py's resident inputs.
    Returns a dict of per-frame times and the pointer check."""
    from ._lib import _ptr
    F = min(frames, inp["masks"].shape[0])
    M, H, W = inp["masks"].shape[1:]
    torch.manual_seed(0)
    enc = make_vit_b32(torch, dim_out=feat_dim, image=crop).to(device).half().eval()
    mean = torch.tensor([0.48145466, 0.4578275, 0.40821073], device=device).view(1, 3, 1, 1)     # clip preprocess constants
    std = torch.tensor([0.26862954, 0.26130258, 0.27577711], device=device).view(1, 3, 1, 1)

    def embed(u8_nhwc):
        x = (u8_nhwc.permute(0, 3, 1, 2).float() / 255.0 - mean) / std
        with torch.no_grad():
            f = enc(x.half()).float()
        return torch.nn.functional.normalize(f, dim=-1).contiguous()
    plain = torch.empty((M, crop, crop, 3), dtype=torch.uint8, device=device)
    masked = torch.empty((M, crop, crop, 3), dtype=torch.uint8, device=device)
    t_crop = t_enc = t_hand = 0.0
    on_device = True
    for it in range(-1, F):                                    # (one warm-up pass of frame 0 that is not handed over)
        f = max(it, 0)
        seg = inp["masks"][f]
        # SAM's bbox records (XYWH) of the frame's masks: a few dozen numbers, made on the device, read by the host side of the
        # crop call like the reference's `mask["bbox"]`
        ys = seg.any(dim=2)
        xs = seg.any(dim=1)
        x0 = xs.float().argmax(1)
        x1 = W - 1 - xs.flip(1).float().argmax(1)
        y0 = ys.float().argmax(1)
        y1 = H - 1 - ys.flip(1).float().argmax(1)
        some = xs.any(1)
        bbox = torch.stack([x0, y0, (x1 - x0 + 1).clamp(min=1), (y1 - y0 + 1).clamp(min=1)], 1).double()
        bbox[~some] = torch.tensor([0.0, 0.0, 8.0, 8.0], dtype=torch.float64, device=device)
        bbox_h = np.ascontiguousarray(bbox.cpu().numpy())
        torch.cuda.synchronize(device)
        t0 = time.perf_counter()
        rc = L.c.hmsg_crop_resize_batch(device.index or 0, H, W, _ptr(inp["rgb"][f]), M, _ptr(seg), _ptr(bbox_h), 50.0, crop, _ptr(plain),
                                        _ptr(masked), None)
        assert rc == 0, "hmsg_crop_resize_batch failed (%d)" % rc
        t1 = time.perf_counter()
        whole = torch.nn.functional.interpolate(inp["rgb"][f].permute(2, 0, 1)[None].float(), size=(crop, crop), mode="bilinear",
                                                align_corners=False).clamp(0, 255).permute(0, 2, 3, 1).to(torch.uint8)
        f_g = embed(whole)                                      # [1, D]
        f_masked = embed(masked)                                # [M, D]
        f_crop = embed(plain)
        torch.cuda.synchronize(device)
        t2 = time.perf_counter()
        if it < 0:
            continue
        for t in (f_g, f_masked, f_crop, seg):
            on_device = on_device and t.is_cuda and t.is_contiguous()
        scene.add_frame_features(f, seg[None], f_g, f_masked[None], f_crop[None])
        t3 = time.perf_counter()
        t_crop += t1 - t0
        t_enc += t2 - t1
        t_hand += t3 - t2
    return dict(frames=F, masks=M, crop=crop, encoder="random-init ViT-B/32 shape (12 x 768, patch 32, fp16), PyTorch-ROCm",
                crops_ms_per_frame=round(t_crop / F * 1e3, 3), encoder_ms_per_frame=round(t_enc / F * 1e3, 3),
                handoff_ms_per_frame=round(t_hand / F * 1e3, 3), tensors_on_device=bool(on_device),
                note="hmsg_crop_resize_batch -> torch module -> hmsg_add_frame_features by data_ptr(): no host copy of masks or features")


def embed_frame_reference_inputs(L, enc, image, seg, bbox, torch, bbox_margin=50.0, crop_size=512, size=224, f16=True, mean=None,
                                 std=None):
    """One frame's F_g, F_masked, F_crop from the encoder inputs the reference makes (sam_clip_feats_extractor.py:147-158 with
    clip_utils.py:72-73, 88-89): the frame and its 2 M crops of crop_size, each through open_clip's `preprocess`, bit for bit
    (include/hmsg.h: hmsg_frame_encoder_inputs), as ONE [1 + 2 M, 3, size, size] tensor written by device pointer; the module
    runs once on it.  image u8 [H, W, 3] and seg u8 [M, H, W]: device tensors; bbox: SAM's XYWH records, host, [M, 4].
    Returns (f_g [1, D], f_masked [M, D], f_crop [M, D]), L2-normalised float32 on the device, ready for
    Scene.add_frame_features(f, seg[None], f_g, f_masked[None], f_crop[None])."""
    from ._lib import HmsgError, _clip_params, _ptr
    assert image.dtype == torch.uint8 and image.is_cuda and image.dim() == 3 and image.shape[2] == 3, "image: uint8 [H, W, 3] on the device"
    assert seg.dtype == torch.uint8 and seg.device == image.device and seg.dim() == 3, "seg: uint8 [M, H, W] on the image's device"
    image, seg = image.contiguous(), seg.contiguous()         # (the library reads them by pointer, as dense arrays)
    H, W = image.shape[:2]
    M = int(seg.shape[0])
    assert tuple(seg.shape[1:]) == (H, W)
    bbox = np.ascontiguousarray(bbox, dtype=np.float64).reshape(M, 4)
    x = torch.empty((1 + 2 * M, 3, size, size), dtype=torch.float16 if f16 else torch.float32, device=image.device)
    prm = _clip_params(L, size, f16, mean, std)
    rc = L.c.hmsg_frame_encoder_inputs(image.device.index or 0, C.byref(prm), H, W, _ptr(image), M, _ptr(seg) if M else None,
                                       _ptr(bbox) if M else None, float(bbox_margin), int(crop_size), _ptr(x), None)
    if rc != 0:
        raise HmsgError(f"hmsg_frame_encoder_inputs failed ({rc})")
    with torch.no_grad():
        f = torch.nn.functional.normalize(enc(x).float(), dim=-1)
    return f[:1].contiguous(), f[1:1 + M].contiguous(), f[1 + M:].contiguous()


def handoff_frame_rle(L, scene, enc, frame, image, rles, bbox, torch, bbox_margin=50.0, crop_size=512, size=224, f16=True, mean=None,
                      std=None):
    """The hand-off of one frame whose masks SAM returned run-length coded (output_mode="uncompressed_rle"; holoagent_amd/rle.py):
    hmsg_rle_to_masks expands the records ON THE DEVICE into the uint8 [M, H, W] the crop kernels read, hmsg_frame_encoder_inputs
    makes the 1 + 2 M encoder inputs, the module runs once, and the frame goes to the scene by hmsg_add_frame_features_rle with the
    same records -- no dense mask is built on the host or crosses to the device.  image u8 [H, W, 3]: a device tensor; rles =
    (counts, run_off) of the frame's M masks as rle.pack makes them (numpy arrays: uploaded here, a few KB; or device tensors);
    bbox: SAM's XYWH records, host, [M, 4].  Returns (f_g, f_masked, f_crop, seg): the features handed over and the device masks."""
    from ._lib import rle_to_masks
    H, W = image.shape[:2]
    dev = image.device

    def on_dev(a, np_dtype):
        if hasattr(a, "data_ptr"):
            return a.contiguous()
        a = np.ascontiguousarray(a, dtype=np_dtype)
        return torch.from_numpy(a.view(np.int32) if np_dtype is np.uint32 else a).to(dev)       # (uint32 travels as its bits)
    counts, run_off = on_dev(rles[0], np.uint32), on_dev(rles[1], np.int64)
    M = int(run_off.shape[0]) - 1
    seg = rle_to_masks((counts, run_off), H, W, device_id=dev.index or 0, lib_=L)                # device in, device out
    f_g, f_masked, f_crop = embed_frame_reference_inputs(L, enc, image, seg, bbox, torch, bbox_margin, crop_size, size, f16, mean, std)
    n_masks = torch.tensor([M], dtype=torch.int32, device=dev)
    scene.add_frame_features_rle(frame, (counts, run_off, n_masks), f_g, f_masked[None], f_crop[None])
    return f_g, f_masked, f_crop, seg


def handoff_frame_logits(L, scene, enc, frame, image, logits, iou_preds, torch, sam_params=None, bbox_margin=50.0, crop_size=512, size=224,
                         f16=True, mean=None, std=None, **sam_over):
    """The hand-off of one frame from SAM's mask DECODER on: logits float32 [N, H, W] (or [P, 3, H, W]) and iou_preds of
    predict_torch(..., return_logits=True) as device tensors -> hmsg_sam_postprocess makes the run-length records, boxes and scores on
    the device (everything SamAutomaticMaskGenerator.generate does behind the decoder; include/hmsg.h) -> hmsg_rle_to_masks ->
    hmsg_frame_encoder_inputs -> the module -> hmsg_add_frame_features_rle with the device records.  No mask and no record crosses to
    the host; the boxes do (a few dozen numbers, read by the host side of the crop call like the reference's mask["bbox"]).
    sam_params: an HmsgSamPostParams, or its fields by keyword (config_surface.sam_post_params(cfg)[0]).
    Returns (f_g, f_masked, f_crop, seg, post): the features handed over, the device masks and sam_postprocess' dict."""
    from ._lib import rle_to_masks, sam_postprocess
    assert logits.is_cuda and iou_preds.is_cuda and image.is_cuda, "logits, iou_preds, image: device tensors"
    H, W = image.shape[:2]
    dev = image.device
    post = sam_postprocess(logits, iou_preds, params=sam_params, return_masks=False, lib_=L, **sam_over)
    counts, run_off = post["counts"].contiguous(), post["run_off"].contiguous()
    seg = rle_to_masks((counts, run_off), H, W, device_id=dev.index or 0, lib_=L)
    bbox = post["bbox"].cpu().numpy()
    f_g, f_masked, f_crop = embed_frame_reference_inputs(L, enc, image, seg, bbox, torch, bbox_margin, crop_size, size, f16, mean, std)
    n_masks = torch.tensor([post["n"]], dtype=torch.int32, device=dev)
    scene.add_frame_features_rle(frame, (counts, run_off, n_masks), f_g, f_masked[None], f_crop[None])
    return f_g, f_masked, f_crop, seg, post
