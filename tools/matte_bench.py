"""Times s3od_matte_refine and s3od_matte_foreground on the GPU: HIP events around each call, 5 warm-up calls, then the
median (and the spread) of 30 timed calls per shape and radius.  Beside each time: the bytes the entry's passes move,
counted from the shapes (every plane read and written once, no halo), and the time those bytes take at 6.29 TB/s, the
measured copy rate of the MI355X.  The inputs are tests/_matte_ref.make_case-like: an image with noise and a soft disc.

    python tools/matte_bench.py [--out FILE]
"""
import argparse
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from s3od_amd.matte import estimate_foreground, refine_alpha, workspace_bytes  # noqa: E402

COPY_RATE = 6.29e12
SHAPES = [(1024, 1024), (2048, 2048), (2160, 3840)]
RADII = [16, 64]
# bytes per pixel of the passes.  refine: rows (3 image + 4 mask -> 13 fp32) | columns + solve (13 -> 4 fp32) | rows
# (4 -> 4) | columns + apply (4 fp32 + 3 image -> 1 fp32).  foreground: rows (3 + 4 -> 7 fp32) | columns + estimate
# (7 fp32 + 3 image + 4 alpha -> 3)
REFINE_BPP = (7 + 52) + (52 + 16) + (16 + 16) + (16 + 3 + 4)
FOREGROUND_BPP = (7 + 28) + (28 + 3 + 4 + 3)


def make_inputs(H, W):
    g = torch.Generator(device="cuda").manual_seed(H * 7 + W)
    yy = torch.arange(H, device="cuda", dtype=torch.float32)[:, None]
    xx = torch.arange(W, device="cuda", dtype=torch.float32)[None, :]
    d = ((yy - 0.55 * H) / (0.3 * H)) ** 2 + ((xx - 0.45 * W) / (0.3 * W)) ** 2
    disc = (d <= 1).float()
    img = disc[..., None] * torch.tensor([200.0, 90.0, 60.0], device="cuda") + \
        (1 - disc[..., None]) * torch.tensor([40.0, 110.0, 170.0], device="cuda")
    img = (img + 12 * torch.randn(H, W, 3, device="cuda", generator=g)).round().clamp(0, 255).to(torch.uint8)
    mask = (torch.sigmoid((1 - d) * 8) + 0.05 * torch.randn(H, W, device="cuda", generator=g)).clamp(0, 1)
    return img.contiguous(), mask.contiguous()


def time_call(fn, warmup=5, calls=30):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("matte_bench needs the GPU: there is no time to report without one")
    lines = [f"{torch.cuda.get_device_name(0)}; median of 30 calls after 5 warm-up calls, HIP events; floor = bytes / 6.29 TB/s",
             f"{'entry':<17}{'H x W':>12}{'r':>5}{'median ms':>11}{'min':>8}{'max':>8}{'MB moved':>10}{'floor ms':>10}{'x floor':>9}"]
    for H, W in SHAPES:
        img, mask = make_inputs(H, W)
        out, rgb = torch.empty_like(mask), torch.empty_like(img)
        workspace_bytes(H, W)
        for name, bpp, fn in (("matte_refine", REFINE_BPP, lambda r: refine_alpha(mask, img, r, 1e-4, out=out)),
                              ("matte_foreground", FOREGROUND_BPP, lambda r: estimate_foreground(mask, img, r, out=rgb))):
            for r in RADII:
                med, lo, hi = time_call(lambda: fn(r))
                nbytes = bpp * H * W
                floor = nbytes / COPY_RATE * 1e3
                lines.append(f"{name:<17}{f'{H} x {W}':>12}{r:>5}{med:>11.3f}{lo:>8.3f}{hi:>8.3f}{nbytes / 1e6:>10.1f}{floor:>10.3f}{med / floor:>9.2f}")
                print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text)
    print(text)


if __name__ == "__main__":
    main()
