"""Throughput of BackgroundRemoval.remove_background_many against a Python loop of remove_background.

One process, one GPU, 1024 canvas, bf16, synthetic weights.  Both arms run over the same 64 images (the fixture
photo plus deterministic random images of the test shapes scaled x4) and alternate, REPEATS times each:
  (a) loop of remove_background                       -- the baseline, the only way without the batched entry
  (b) remove_background_many at batch_size 4, 8, 16, with return_all_masks True and False
  (c) remove_background_many at batch_size 8 with background=(255, 255, 255), return_masks=False, return_rgba=False
      (only the 3 B/px composite comes back), without and with stats=True
Prints medians and ranges of images/s, the HIP-event time of the batched pre / post kernels against their
single-image counterparts on the fixture's shape, the host wall time per phase of the batched path (stage =
fill the pinned buffer and start the upload, launch, wait = block on the download event, split = copy out of the
pinned buffer) and the bytes that cross PCIe per image.

    python tools/infer_many_bench.py [--repeats 5] [--images 64] [--out FILE]
"""
import argparse
import ctypes
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

SHAPES = [(100, 200), (480, 640), (20, 30), (40, 640), (200, 100), (640, 480), (30, 20), (640, 40), (256, 256), (31, 31),
          (512, 512), (256, 255), (255, 256)]


def build_images(n):
    from PIL import Image
    images = [np.array(Image.open(ROOT / "tests" / "fixture" / "image.jpg").convert("RGB"))]
    rng = np.random.default_rng(0)
    i = 0
    while len(images) < n:
        h, w = SHAPES[i % len(SHAPES)]
        images.append(rng.integers(0, 256, (4 * h, 4 * w, 3), dtype=np.uint8))
        i += 1
    return images


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def event_ms(fn, iters=20, warmup=3):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts)


def kernel_times(br, image, B=8):
    """HIP-event medians (ms per image) of the pre / post entries on one shape, single vs batched."""
    from s3od_amd._lib import lib, stream
    from s3od_amd.infer_many import PostDesc, PreDesc
    from s3od_amd.utils import get_pad_info
    S = br.image_size
    H0, W0 = image.shape[:2]
    info = get_pad_info(image, S)
    nh, nw = info["resized_size"]
    ph, pw = info["height_pad"], info["width_pad"]
    h, w = S - 2 * ph, S - 2 * pw
    n = H0 * W0 * 3
    stride = (n + 15) // 16 * 16
    packed = torch.zeros(B * stride, dtype=torch.uint8, device="cuda")
    img = torch.from_numpy(image).cuda()
    for b in range(B):
        packed[b * stride:b * stride + n] = img.reshape(-1)
    pre, post = (PreDesc * B)(), (PostDesc * B)()
    for b in range(B):
        pre[b] = PreDesc(b * stride, H0, W0, nh, nw, ph, pw)
        post[b] = PostDesc(b * stride, b * 3 * H0 * W0, b * H0 * W0 * 4, b * 3 * h * W0, ph, pw, h, w, H0, W0)
    to_dev = lambda a: torch.from_numpy(np.frombuffer(bytes(a), dtype=np.uint8).copy()).cuda()
    pre_d, post_d = to_dev(pre), to_dev(post)
    x1 = torch.empty((1, 3, S, S), device="cuda")
    xb = torch.empty((B, 3, S, S), device="cuda")
    logits = torch.randn((B, 3, S, S), device="cuda") * 4
    best = torch.zeros(B, dtype=torch.int32, device="cuda")
    tmp = torch.empty((B * 3 * h * W0,), device="cuda")
    masks = torch.empty((B * 3 * H0 * W0,), device="cuda")
    rgba = torch.empty((B * H0 * W0 * 4,), dtype=torch.uint8, device="cuda")
    L = lib()
    out = {"shape": [H0, W0], "batch": B}
    out["pre_single_ms"] = event_ms(lambda: L("s3od_preprocess", img, H0, W0, nh, nw, ph, pw, S, x1, stream()))
    out["pre_batch_ms_per_image"] = event_ms(lambda: L("s3od_preprocess_batch", packed, pre_d, ctypes.addressof(pre), B, S, xb,
                                                       stream())) / B
    out["post_single_ms"] = event_ms(lambda: L("s3od_sigmoid_unpad_resize", logits[0], 3, S, S, ph, pw, h, w, H0, W0, tmp, masks,
                                               stream()))
    for name, allm in (("post_batch_all_ms_per_image", 1), ("post_batch_best_ms_per_image", 0)):
        out[name] = event_ms(lambda: L("s3od_postprocess_batch", logits, B, 3, S, S, best, packed, post_d, ctypes.addressof(post),
                                       allm, masks, rgba, tmp, stream())) / B
    # the composite over white alone (no float plane stored), without and with the mask statistics
    from s3od_amd.infer_many import MODE_RGB_OVER_COLOR, OutDesc
    outd = (OutDesc * B)()
    for b in range(B):
        outd[b] = OutDesc(0, b * stride, b * 288, b * 3 * H0 * W0, MODE_RGB_OVER_COLOR, 0xFFFFFF)
    out_d = to_dev(outd)
    stats = torch.empty(B * 72, dtype=torch.int32, device="cuda")
    for name, st in (("post_batch_white_ms_per_image", None), ("post_batch_white_stats_ms_per_image", stats)):
        out[name] = event_ms(lambda: L("s3od_postprocess_batch_out", logits, B, 3, S, S, best, packed, post_d,
                                       ctypes.addressof(post), out_d, ctypes.addressof(outd), 1, 0, None, rgba, tmp,
                                       masks if st is not None else None, st, 0.5, stream())) / B
    return out


def pcie_bytes(images):
    px = float(np.mean([im.shape[0] * im.shape[1] for im in images]))
    return {"loop": {"h2d": 3 * px, "d2h": 12 * px + 12},
            "many_all_masks": {"h2d": 3 * px + 88, "d2h": 12 * px + 4 * px + 16},
            "many_best_only": {"h2d": 3 * px + 88, "d2h": 4 * px + 4 * px + 16},
            "many_white": {"h2d": 3 * px + 128, "d2h": 3 * px + 16},
            "many_white_stats": {"h2d": 3 * px + 128, "d2h": 3 * px + 16 + 288}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.set_num_threads(min(16, torch.get_num_threads()))
    from s3od import BackgroundRemoval
    br = BackgroundRemoval("synthetic", image_size=1024, compute_dtype="bf16")
    images = build_images(a.images)
    n = len(images)
    arms = {"loop": lambda: [br.remove_background(im) for im in images]}
    for bs in (4, 8, 16):
        for allm in (True, False):
            arms[f"many_bs{bs}_{'all' if allm else 'best'}"] = \
                (lambda bs=bs, allm=allm: br.remove_background_many(images, batch_size=bs, return_all_masks=allm))
    white = dict(batch_size=8, background=(255, 255, 255), return_masks=False, return_rgba=False)
    arms["many_bs8_white"] = lambda: br.remove_background_many(images, **white)
    arms["many_bs8_white_stats"] = lambda: br.remove_background_many(images, stats=True, **white)
    for fn in arms.values():                       # warm-up: allocator, staging buffers, kernel selection
        fn()
    rates = {k: [] for k in arms}
    for _ in range(a.repeats):
        for k, fn in arms.items():                 # alternate the arms inside every repeat
            rates[k].append(n / timed(fn))
    # host wall time per phase of the batched path (one extra pass per mode at batch_size 8, not part of the timings)
    host_ms = {}
    modes = {"all": dict(batch_size=8, return_all_masks=True), "best": dict(batch_size=8, return_all_masks=False),
             "white": white, "white_stats": dict(white, stats=True)}
    for name, kw in modes.items():
        br.remove_background_many(images[:8], **kw)
        br._many.host_seconds = {}
        dt = timed(lambda: br.remove_background_many(images, **kw))
        host_ms[name] = {**{k: 1e3 * v / n for k, v in br._many.host_seconds.items()}, "total": 1e3 * dt / n}
        br._many.host_seconds = None
    rec = {"images": n, "repeats": a.repeats, "canvas": 1024, "dtype": "bf16",
           "images_per_s": {k: {"median": statistics.median(v), "min": min(v), "max": max(v)} for k, v in rates.items()},
           "host_ms_per_image_bs8": host_ms, "kernels_ms": kernel_times(br, images[0]), "pcie_bytes_per_image": pcie_bytes(images)}
    print(f"{'arm':<22}{'median':>10}{'min':>10}{'max':>10}   images/s over {n} images, {a.repeats} repeats")
    for k, v in rec["images_per_s"].items():
        print(f"{k:<22}{v['median']:>10.1f}{v['min']:>10.1f}{v['max']:>10.1f}")
    for k, v in host_ms.items():
        print(f"host ms/image at batch_size 8, {k}: " + ", ".join(f"{p} {ms:.2f}" for p, ms in v.items()))
    print(json.dumps(rec))
    if a.out:
        Path(a.out).write_text(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
