"""A/B of the flip-consistency scoring paths on the MI355X (dev tool; needs the GPU).

    python tools/flip_scores_ab.py [--out profiles/flip_scores_ab.txt] [--image-size 1024] [--images 32] [--repeats 5]

Per image, bf16, seeded images of mixed sizes with blob ground truths:
  A  the composition of the drop-ins without the mirror-pair path: two SODPredictor.predict calls, the mirror on the
     host, both soft masks uploaded again, three EvaluationMetrics(sm_only=True) steps each read back as eval_sample
     does, and three host IoUs on the binary masks;
  B  FlipScorer.score;
  C  FlipScorer.score_many(batch_size=4).
The three are timed in alternation (A B C, A B C, ...) after one untimed pass of each over every image, a host clock
around work that ends in a device synchronise; median and range over the repeats are reported.

The scoring step alone at S x S: three EvaluationMetrics(sm_only=True) steps + their read-back (X1), the same plus
the two host copies and three host IoUs (X2), against one s3od_flip_scores call + its read-back (Y), on the same
device tensors.
"""
import argparse
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

SHAPES = [(480, 640), (640, 480), (720, 1280), (1024, 1024), (600, 800), (800, 600), (1080, 1920), (333, 500)]


def blob(h, w, r):
    yy, xx = np.mgrid[:h, :w]
    cy, cx = r.uniform(0.3, 0.7) * h, r.uniform(0.3, 0.7) * w
    return ((((yy - cy) / (0.3 * h)) ** 2 + ((xx - cx) / (0.25 * w)) ** 2) < 1).astype(np.float32)


def composed(pred, image, gt, threshold=0.5):
    """Path A -> (s_orig, s_flip, s_cons, iou_orig_gt, iou_flip_gt, iou_orig_flip)."""
    from s3od_amd.filtering import calculate_iou
    from s3od_amd.metrics import EvaluationMetrics
    r1 = pred.predict(image)
    r2 = pred.predict(np.ascontiguousarray(image[:, ::-1]))
    flipped = np.ascontiguousarray(r2.soft_mask[:, ::-1])
    a, b, g = torch.tensor(r1.soft_mask).cuda(), torch.tensor(flipped).cuda(), torch.tensor(gt).cuda()
    em = EvaluationMetrics(device="cuda", sm_only=True)
    s = []
    for p, m in ((a, g), (b, g), (a, b)):
        em.step(p, m)
        s.append(float(em.compute_metrics()["Sm"]))
        em.reset()
    bin_a, bin_b = r1.binary_mask, np.ascontiguousarray(r2.binary_mask[:, ::-1])
    return (*s, calculate_iou(bin_a, gt), calculate_iou(bin_b, gt), calculate_iou(bin_a, bin_b))


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def summary(name, per_image_ms):
    med = statistics.median(per_image_ms)
    return f"{name}: median {med:8.3f} ms/image  range {min(per_image_ms):8.3f} .. {max(per_image_ms):8.3f}  ({len(per_image_ms)} repeats)"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--image-size", type=int, default=1024)
    ap.add_argument("--images", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--step-iters", type=int, default=50)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("flip_scores_ab.py measures on the GPU; no GPU found")
    from s3od_amd.flip_scores import FlipScorer, flip_scores_out
    from s3od_amd.filtering import calculate_iou
    from s3od_amd.metrics import EvaluationMetrics
    from s3od_amd.model import DPTSegmentation
    from s3od_amd.sod_predictor import SODPredictor

    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    S, n = args.image_size, args.images
    pred = SODPredictor(DPTSegmentation(compute_dtype="bf16"), image_size=S)
    scorer = FlipScorer(pred)
    r = np.random.default_rng(7)
    shapes = [SHAPES[i % len(SHAPES)] for i in range(n)]
    images = [r.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in shapes]
    gts = [blob(h, w, r) for h, w in shapes]
    say(f"flip-consistency scoring A/B: {torch.cuda.get_device_name(0)}, image_size {S}, bf16, {n} images of sizes {sorted(set(shapes))}")

    paths = {
        "A composed (2 predict + host mirror + 3 steps + host IoUs)": lambda: [composed(pred, im, g) for im, g in zip(images, gts)],
        "B FlipScorer.score": lambda: [scorer.score(im, g) for im, g in zip(images, gts)],
        "C FlipScorer.score_many(batch_size=4)": lambda: scorer.score_many(images, gts, batch_size=4),
    }
    results = {k: fn() for k, fn in paths.items()}                     # the untimed pass: every shape of every path
    times = {k: [] for k in paths}
    for _ in range(args.repeats):
        for k, fn in paths.items():
            t, _ = timed(fn)
            times[k].append(1e3 * t / n)
    for k in paths:
        say(summary(k, times[k]))
    a_med = statistics.median(times[list(paths)[0]])
    for k in list(paths)[1:]:
        say(f"  speed-up of {k.split()[0]} over A (medians): {a_med / statistics.median(times[k]):.3f}x")
    A = np.array([list(v) for v in results[list(paths)[0]]], np.float64)
    for k in list(paths)[1:]:
        V = np.array([list(v)[:6] for v in results[k]], np.float64)
        ok = ~np.isnan(A) & ~np.isnan(V)
        say(f"  {k.split()[0]} vs A on the same images (bf16, different batching): max |S diff| {np.abs(A - V)[:, :3][ok[:, :3]].max():.3g}, "
            f"max |IoU diff| {np.abs(A - V)[:, 3:][ok[:, 3:]].max():.3g}")

    # ---- the scoring step alone
    g0 = blob(S, S, r)
    a = torch.from_numpy((0.45 * g0 + 0.55 * r.random((S, S))).astype(np.float32)).cuda()
    bm = torch.from_numpy(np.ascontiguousarray((0.4 * g0 + 0.6 * r.random((S, S))).astype(np.float32)[:, ::-1])).cuda()
    gt = torch.from_numpy(g0).cuda()
    em = EvaluationMetrics(device="cuda", sm_only=True)

    def x1():
        b = torch.flip(bm, [1]).contiguous()
        g = gt.clone()
        em.reset()
        em.step(a, g); em.step(b, g); em.step(a, b)
        return em.per_image()[:, 3], b

    def x2():
        s, b = x1()
        ha, hb, hg = a.cpu().numpy(), torch.flip(bm, [1]).cpu().numpy(), g0
        return s, (calculate_iou(ha, hg), calculate_iou(hb, hg), calculate_iou(ha, hb))

    def y():
        return flip_scores_out(a, bm, gt).cpu().numpy()

    steps = {"X1 three s3od_eval_metrics steps + read-back": x1, "X2 X1 + two host copies + three host IoUs": x2,
             "Y  one s3od_flip_scores + read-back": y}
    for fn in steps.values():
        for _ in range(5):
            fn()
    st = {k: [] for k in steps}
    for _ in range(args.repeats):
        for k, fn in steps.items():
            t, _ = timed(lambda: [fn() for _ in range(args.step_iters)])
            st[k].append(1e3 * t / args.step_iters)
    say(f"scoring step alone at {S} x {S} ({args.step_iters} calls per repeat):")
    for k in steps:
        say("  " + summary(k, st[k]).replace("ms/image", "ms/call "))
    sx, sy = x1()[0], y()
    say(f"  S from X1 {np.asarray(sx)} from Y {sy[:3]}")
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
