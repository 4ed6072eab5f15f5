"""The CLIP preprocess of one frame's 1 + 2 M encoder inputs on cuda:0, three routes timed in turn in one process, at
configs[1]'s frame (640x480, 32 masks) and at 1280x720 -- everything resident in HBM before and after:
  (a) the only reference-exact route without hmsg_frame_encoder_inputs: 512^2 crops (hmsg_crop_resize_batch) and the frame to
      the host, Pillow's Resize(224, BICUBIC) / CenterCrop / ToTensor / Normalize per image on up to 16 host threads, the float16
      batch uploaded.  Left out, and said so, where Pillow is not importable (the numpy restatement is never timed in its place).
  (b) the hand-off's present INEXACT route (encoder_handoff.measure): crops made at 224 directly + torch ops.  For scale only:
      it computes something else.
  (c) hmsg_frame_encoder_inputs, float16 output, by device pointer: device_ms (HIP events around its three launches) and wall.
Each timing is a host clock around work that ends in a device synchronise; the routes alternate ROUNDS times after a warm-up
pass of each.  Writes profiles/clip_preprocess.json (or the path given) and prints it.
    python scripts/bench_clip_preprocess.py [out.json]"""
import ctypes as C
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from holoagent_amd._lib import _clip_params, _ptr, lib  # noqa: E402
from tests import clip_preprocess_oracle as O  # noqa: E402
from tests.test_crops import _random_frame  # noqa: E402

ROUNDS, REPS_C, S, CS, MARGIN = 7, 5, 224, 512, 50.0
HBM_PEAK = 8.0e12          # bytes / s, the data-sheet figure


def _stats(v):
    return {"median_ms": round(statistics.median(v) * 1e3, 4), "min_ms": round(min(v) * 1e3, 4), "max_ms": round(max(v) * 1e3, 4), "n": len(v)}


def bench_shape(L, H, W, M, pil):
    dev = torch.device("cuda:0")
    image, masks = _random_frame(5, H, W, M)
    t_img = torch.from_numpy(image).to(dev)
    t_seg = torch.from_numpy(np.stack([m["segmentation"] for m in masks]).astype(np.uint8)).to(dev)
    bbox = np.ascontiguousarray([m["bbox"] for m in masks], dtype=np.float64)
    plain = torch.empty((M, CS, CS, 3), dtype=torch.uint8, device=dev)
    masked = torch.empty_like(plain)
    plain_s = torch.empty((M, S, S, 3), dtype=torch.uint8, device=dev)
    masked_s = torch.empty_like(plain_s)
    out_c = torch.empty((1 + 2 * M, 3, S, S), dtype=torch.float16, device=dev)
    prm = _clip_params(L, S, True, None, None)
    mean = torch.tensor(O.MEAN, device=dev).view(1, 3, 1, 1)
    std = torch.tensor(O.STD, device=dev).view(1, 3, 1, 1)
    lut = O.normalize_table()
    pool = ThreadPoolExecutor(16)
    ms = C.c_double(0)

    def one_pil(u8):
        from PIL import Image
        w2, h2 = O.resize_dims(u8.shape[0], u8.shape[1], S)
        im = Image.fromarray(u8)
        if (w2, h2) != im.size:
            im = im.resize((w2, h2), Image.BICUBIC)
        top, left = O.center_crop_offset(h2, S), O.center_crop_offset(w2, S)
        a = np.asarray(im)[top:top + S, left:left + S]
        return np.stack([lut[c][a[:, :, c]] for c in range(3)]).astype(np.float16)

    def route_a():
        rc = L.c.hmsg_crop_resize_batch(0, H, W, _ptr(t_img), M, _ptr(t_seg), _ptr(bbox), MARGIN, CS, _ptr(plain), _ptr(masked), None)
        assert rc == 0
        imgs = [t_img.cpu().numpy()] + list(masked.cpu().numpy()) + list(plain.cpu().numpy())
        x = torch.from_numpy(np.stack(list(pool.map(one_pil, imgs)))).to(dev)
        torch.cuda.synchronize()
        return x

    def route_b():
        rc = L.c.hmsg_crop_resize_batch(0, H, W, _ptr(t_img), M, _ptr(t_seg), _ptr(bbox), MARGIN, S, _ptr(plain_s), _ptr(masked_s), None)
        assert rc == 0
        whole = torch.nn.functional.interpolate(t_img.permute(2, 0, 1)[None].float(), size=(S, S), mode="bilinear",
                                                align_corners=False).clamp(0, 255).permute(0, 2, 3, 1).to(torch.uint8)
        u8 = torch.cat([whole, masked_s, plain_s])
        x = ((u8.permute(0, 3, 1, 2).float() / 255.0 - mean) / std).half()
        torch.cuda.synchronize()
        return x

    def route_c():
        rc = L.c.hmsg_frame_encoder_inputs(0, C.byref(prm), H, W, _ptr(t_img), M, _ptr(t_seg), _ptr(bbox), MARGIN, CS, _ptr(out_c), C.byref(ms))
        assert rc == 0                       # (the call returns after its own stream's synchronise)
        return out_c

    routes = {"b_inexact_crop224_torch": route_b, "c_hmsg_frame_encoder_inputs": route_c}
    if pil:
        routes = dict({"a_host_pillow_16_threads": route_a}, **routes)
    for fn in routes.values():               # warm-up: code objects, allocator, thread pool
        fn()
        fn()
    equal = bool(torch.equal(route_a(), route_c())) if pil else None
    wall = {k: [] for k in routes}
    dev_ms = []
    for _ in range(ROUNDS):
        for k, fn in routes.items():
            reps = REPS_C if k.startswith("c_") else 1
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _r in range(reps):
                fn()
                if k.startswith("c_"):
                    dev_ms.append(ms.value)
            wall[k].append((time.perf_counter() - t0) / reps)
    pool.shutdown()
    # bytes the three launches of (c) have to move: the frame and its masks read, the crops written and read again, the tensor written
    nbytes = H * W * 3 * 2 + M * H * W + 2 * (2 * M * CS * CS * 3) + (1 + 2 * M) * 3 * S * S * 2
    d_med = statistics.median(dev_ms)
    res = {"frame": f"{W}x{H}", "masks": M, "crop_size": CS, "size": S, "output": "float16 [1 + 2 M, 3, 224, 224]",
           "wall_per_frame": {k: _stats(v) for k, v in wall.items()},
           "c_device_ms": {"median": round(d_med, 4), "min": round(min(dev_ms), 4), "max": round(max(dev_ms), 4), "n": len(dev_ms)},
           "c_bytes_per_frame": nbytes,
           "c_bytes_over_device_ms_share_of_hbm_peak": round(nbytes / (d_med * 1e-3) / HBM_PEAK, 4),
           "a_equals_c_bit_for_bit": equal}
    if pil:
        res["slowest_c_under_fastest_a"] = bool(max(wall["c_hmsg_frame_encoder_inputs"]) < min(wall["a_host_pillow_16_threads"]))
    return res


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "clip_preprocess.json")
    try:
        import PIL
        pil = PIL.__version__
    except ImportError:
        pil = None
    L = lib()
    res = {"benchmark": "clip_preprocess", "device": torch.cuda.get_device_name(0), "pillow": pil or "not importable: route (a) not measured",
           "rounds": ROUNDS, "calls_of_c_per_round": REPS_C, "hbm_peak_bytes_per_s": HBM_PEAK,
           "note": "c_bytes_over_device_ms_share_of_hbm_peak = algorithmic bytes of the three launches over the HIP-event time between the first "
                   "and the last, as a share of the HBM data-sheet peak; not a per-kernel figure",
           "shapes": [bench_shape(L, 480, 640, 32, pil), bench_shape(L, 720, 1280, 32, pil)]}
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
