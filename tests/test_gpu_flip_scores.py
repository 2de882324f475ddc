"""Flip-consistency scoring on the device: s3od_mirror_u8, s3od_flip_scores, FlipScorer (masks / score / score_many)
and the two surfaces on top of it (mining.main, HorizontalFlipConsistencyFilter + DatasetFilter).

Bounds: the mirror is exact; S-measures 2e-6 absolute against the reference golden and against three
EvaluationMetrics(sm_only=True) steps on the same tensors (the S-measure bound of test_gpu_metrics.py), NaN
exactly where they have NaN; IoU counts exact; the mining score 4e-6 * max(1, |score|) (a product of two sums of S
values at 2e-6 each); masks 1e-5 max-rel against SODPredictor.predict (the batched-vs-single bound of
test_gpu_infer_many.py).  Synthetic weights, compute_dtype f32, image_size 256 unless a test says otherwise.
"""
import glob
import json
import math

import numpy as np
import pytest
import torch
from PIL import Image

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

S = 256
G = np.load(GOLDEN / "flip_scores.npz")
NAMES = [str(n) for n in G["names"]]
S_TOL = 2e-6


def rel_max(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-12))


def rand_images(shapes, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in shapes]


def blob_gt(h, w, seed):
    r = np.random.default_rng(seed)
    yy, xx = np.mgrid[:h, :w]
    cy, cx = r.uniform(0.3, 0.7) * h, r.uniform(0.3, 0.7) * w
    return ((((yy - cy) / (0.3 * h)) ** 2 + ((xx - cx) / (0.25 * w)) ** 2) < 1).astype(np.float32)


def same_s(got, want, tol=S_TOL):
    """NaN exactly where `want` has NaN, else within tol absolute."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    if not np.array_equal(np.isnan(got), np.isnan(want)):
        return False
    ok = ~np.isnan(want)
    return bool(np.all(np.abs(got[ok] - want[ok]) <= tol))


def s_err(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    ok = ~np.isnan(want) & ~np.isnan(got)
    return float(np.abs(got[ok] - want[ok]).max()) if ok.any() else 0.0


def existing_path(a, bm, gt, threshold=0.5):
    """The composition that exists without the feature, on device tensors: three EvaluationMetrics(sm_only=True) steps in
    eval_sample's order on the un-mirrored flip and one cloned ground truth (so step 1's in-place binarisation carries
    into step 2), IoU counts from torch boolean ops -> float64 [9] in s3od_flip_scores' order."""
    from s3od_amd.metrics import EvaluationMetrics
    b = torch.flip(bm, [1]).contiguous()
    g = gt.clone()
    ta, tb, tg = a > threshold, b > threshold, gt > 0.5
    counts = [int((p & q).sum()) if k == 0 else int((p | q).sum()) for p, q in ((ta, tg), (tb, tg), (ta, tb)) for k in (0, 1)]
    em = EvaluationMetrics(device="cuda", sm_only=True)
    em.step(a, g)
    em.step(b, g)
    em.step(a, b)
    return np.array(list(em.per_image()[:, 3]) + counts, np.float64)


@pytest.fixture(scope="module")
def pred():
    from s3od_amd.model import DPTSegmentation
    from s3od_amd.sod_predictor import SODPredictor
    return SODPredictor(DPTSegmentation(compute_dtype="f32"), image_size=S)


@pytest.fixture(scope="module")
def scorer(pred):
    from s3od_amd.flip_scores import FlipScorer
    return FlipScorer(pred)


# ---------------------------------------------------------------------------------- 1. s3od_mirror_u8
@pytest.mark.parametrize("shape", [(1, 1, 3), (5, 7, 3), (64, 65, 3), (3, 1, 1), (17, 256, 4), (300, 1023, 3)])
def test_mirror_u8(shape):
    from s3od_amd._lib import lib, stream
    H, W, C = shape
    x = np.random.default_rng(H * 1000 + W).integers(0, 256, shape, dtype=np.uint8)
    src = torch.from_numpy(x).cuda()
    dst = torch.full_like(src, 7)
    lib()("s3od_mirror_u8", src, H, W, C, dst, stream())
    assert np.array_equal(dst.cpu().numpy(), np.flip(x, 1))
    assert np.array_equal(src.cpu().numpy(), x)


def test_mirror_u8_rejects():
    from s3od_amd._lib import lib, stream, HipLibError
    src = torch.zeros(64, dtype=torch.uint8, device="cuda")
    dst = torch.zeros(64, dtype=torch.uint8, device="cuda")
    with pytest.raises(HipLibError):
        lib()("s3od_mirror_u8", src, 4, 0, 3, dst, stream())
    with pytest.raises(HipLibError):
        lib()("s3od_mirror_u8", src, 2, 2, 5, dst, stream())
    with pytest.raises(HipLibError):
        lib()("s3od_mirror_u8", src, 2, 2, 3, src, stream())


# ---------------------------------------------------------------------------------- 2. s3od_flip_scores vs the golden
def _case(name):
    return tuple(torch.from_numpy(G[f"{name}/{k}"]).cuda() for k in ("a", "bm", "gt"))


@pytest.mark.parametrize("name", NAMES)
def test_flip_scores_golden(name):
    from s3od_amd.flip_scores import flip_scores_out, scores_from_out
    a, bm, gt = _case(name)
    keep = [t.clone() for t in (a, bm, gt)]
    v = flip_scores_out(a, bm, gt).cpu().numpy()
    for t, k in zip((a, bm, gt), keep):
        assert torch.equal(t, k), "an input was modified"
    want_s, want_iou = G[f"{name}/s"], G[f"{name}/iou"]
    print(f"{name}: S {v[:3]} golden {want_s[:3]} max err {s_err(v[:3], want_s[:3]):.3g}")
    assert same_s(v[:3], want_s[:3]), (v[:3], want_s[:3])
    assert np.all(v[3:] == np.round(v[3:])) and np.all(v[3:] >= 0)
    r = scores_from_out(v)
    assert [r.iou_orig_gt, r.iou_flip_gt, r.iou_orig_flip] == list(want_iou), (r, want_iou)
    if math.isnan(want_s[3]):
        assert math.isnan(r.score)
    else:
        assert abs(r.score - want_s[3]) <= 4e-6 * max(1.0, abs(want_s[3])), (r.score, want_s[3])


# ---------------------------------------------------------------------------------- 3. vs the existing path
def _big_case(H=1024, W=1000):
    """1024 x 1000: more pixels than 2048 blocks x 256 threads, so the grid-stride loop and every block's atomics run.
    Scaled down: 3 x 85 and 16 x 16 fill one block, 3 x 86 puts two live threads into a second one."""
    r = np.random.default_rng(31)
    g = np.maximum(blob_gt(H, W, 32), blob_gt(H, W, 33))
    a = (0.45 * g + 0.55 * r.random((H, W))).astype(np.float32)
    bm = np.ascontiguousarray((0.4 * g + 0.6 * r.random((H, W))).astype(np.float32)[:, ::-1])
    return tuple(torch.from_numpy(t).cuda() for t in (a, bm, (0.8 * g + 0.1).astype(np.float32)))


SOFT = {"big_1024x1000": (1024, 1000), "soft_3x85": (3, 85), "soft_16x16": (16, 16), "soft_3x86": (3, 86)}


@pytest.mark.parametrize("name", NAMES + list(SOFT))
def test_flip_scores_vs_existing_path(name):
    from s3od_amd.flip_scores import flip_scores_out
    a, bm, gt = _big_case(*SOFT[name]) if name in SOFT else _case(name)
    v = flip_scores_out(a, bm, gt).cpu().numpy()
    want = existing_path(a, bm, gt)
    print(f"{name}: S {v[:3]} existing {want[:3]} max err {s_err(v[:3], want[:3]):.3g}")
    assert same_s(v[:3], want[:3]), (v[:3], want[:3])
    assert np.array_equal(v[3:], want[3:]), (v[3:], want[3:])


def test_flip_scores_repeat_bit_for_bit_in_one_block():
    """16 x 16 is one block: no two partial sums meet in an atomic, so a second call repeats every bit."""
    from s3od_amd.flip_scores import flip_scores_out
    a, bm, gt = _big_case(16, 16)
    v = [flip_scores_out(a.clone(), bm.clone(), gt.clone()).cpu().numpy() for _ in range(2)]
    assert v[0].tobytes() == v[1].tobytes(), v


def test_flip_scores_rejects():
    from s3od_amd._lib import lib, stream, HipLibError
    t = torch.zeros(16, dtype=torch.float32, device="cuda")
    ws = torch.zeros(128, dtype=torch.float64, device="cuda")
    out = torch.zeros(9, dtype=torch.float64, device="cuda")
    with pytest.raises(HipLibError):
        lib()("s3od_flip_scores", t, t, t, 1, 16, 0.5, ws, ws.numel() * 8, out, stream())
    with pytest.raises(HipLibError):
        lib()("s3od_flip_scores", t, t, t, 4, 4, 0.5, ws, 8, out, stream())


# ---------------------------------------------------------------------------------- 4. FlipScorer.masks
def _check_masks(predictor, images):
    from s3od_amd.flip_scores import FlipScorer
    sc = FlipScorer(predictor)
    for im in images:
        a, bm = sc.masks(im)
        assert a.is_cuda and bm.is_cuda and a.dtype == bm.dtype == torch.float32
        assert tuple(a.shape) == tuple(bm.shape) == im.shape[:2]
        ea = rel_max(a.cpu().numpy(), predictor.predict(im).soft_mask)
        eb = rel_max(bm.cpu().numpy(), predictor.predict(np.ascontiguousarray(im[:, ::-1])).soft_mask)
        print(f"masks {im.shape[:2]}: max-rel a {ea:.3g} bm {eb:.3g}")
        assert ea <= 1e-5 and eb <= 1e-5, (im.shape, ea, eb)


def test_masks_dinob(pred):
    _check_masks(pred, rand_images([(100, 200), (200, 101), (31, 31)], 41))


def test_masks_dinol_single_mask():
    from s3od_amd.model import DPTSegmentation
    from s3od_amd.sod_predictor import SODPredictor
    model = DPTSegmentation(compute_dtype="f32", num_classes=1, num_outputs=1,
                            encoder_name="facebook/dinov3-vitl16-pretrain-lvd1689m")
    _check_masks(SODPredictor(model, image_size=224), rand_images([(100, 200)], 42))


# ---------------------------------------------------------------------------------- 5. score / score_many
SHAPES5 = [(100, 200), (200, 101), (31, 31), (256, 256), (64, 300)]


def _inputs5():
    images = rand_images(SHAPES5, 43)
    gts = [blob_gt(h, w, 50 + i) for i, (h, w) in enumerate(SHAPES5)]
    gts[1] = gts[1].astype(np.uint8)                        # {0, 1} uint8, as the filter passes it
    gts[3] = torch.from_numpy(0.9 * gts[3] + 0.05)          # a soft torch ground truth
    return images, gts


def test_score_equals_existing_path(scorer):
    from s3od_amd.flip_scores import scores_from_out
    images, gts = _inputs5()
    for im, gt in zip(images[:3], gts[:3]):
        gt_keep = np.array(gt, copy=True)
        r = scorer.score(im, gt)
        assert np.array_equal(np.asarray(gt), gt_keep), "the caller's ground truth was modified"
        a, bm = scorer.masks(im)
        g = torch.as_tensor(gt).to("cuda", torch.float32)
        want = scores_from_out(existing_path(a, bm, g))
        print(f"score {im.shape[:2]}: {r}  S err {s_err(r[:3], want[:3]):.3g}")
        assert same_s(r[:3], want[:3]), (r, want)
        assert r[3:6] == want[3:6], (r, want)
        assert abs(r.score - want.score) <= 4e-6 * max(1.0, abs(want.score)) or (math.isnan(r.score) and math.isnan(want.score))


def test_score_many_equals_loop(scorer):
    images, gts = _inputs5()
    loop = np.stack([scorer.raw_many([im], [gt], 1)[0] for im, gt in zip(images, gts)])
    # pixels whose soft value lies within 1e-5 of the threshold: only they may change an IoU count between batchings
    near = []
    for im in images:
        a, bm = scorer.masks(im)
        near.append(int(((a - 0.5).abs() <= 1e-5).sum() + ((bm - 0.5).abs() <= 1e-5).sum()))
    print("pixels within 1e-5 of the threshold per image:", near)
    for n, (h, w) in zip(near, SHAPES5):
        assert n <= 1e-4 * h * w, "choose other seeded images: too many pixels sit on the threshold"
    for bs in (1, 3):
        many = scorer.raw_many(images, gts, batch_size=bs)
        assert many.shape == loop.shape
        print(f"score_many(batch_size={bs}) vs loop: max S err {s_err(many[:, :3], loop[:, :3]):.3g}, "
              f"max count difference {np.abs(many[:, 3:] - loop[:, 3:]).max():.0f}")
        assert same_s(many[:, :3], loop[:, :3])
        for i, n in enumerate(near):
            assert np.abs(many[i, 3:] - loop[i, 3:]).max() <= n, (bs, i, many[i], loop[i])
        res = scorer.score_many(images, gts, batch_size=bs)
        assert len(res) == len(images) and all(same_s(r[:3], v[:3]) for r, v in zip(res, many))
    assert scorer.score_many([], []) == []


def test_score_errors_before_the_model_runs(scorer, monkeypatch):
    images, gts = _inputs5()

    def boom(*a, **k):
        raise AssertionError("the model ran before the arguments were validated")
    with monkeypatch.context() as m:
        m.setattr(scorer.predictor.model, "forward", boom)
        with pytest.raises(ValueError):
            scorer.score(images[0], gts[1])
        with pytest.raises(ValueError, match="image 1"):
            scorer.score_many(images[:2], [gts[0], gts[0]], batch_size=2)
        with pytest.raises(ValueError):
            scorer.score_many(images[:1], gts[:1], batch_size=0)
        with pytest.raises(ValueError):
            scorer.score_many(images[:2], gts[:1])


# ---------------------------------------------------------------------------------- 6. end to end on a folder
def _write_folder(root, layout):
    """Six image / mask pairs; layout 'flat' = images/cat_x_i.jpg + masks/cat_x_i.png (mining), 'classes' =
    cat_x/images/i.jpg + cat_x/masks/i.png (the filter framework)."""
    rng = np.random.default_rng(61)
    shapes = [(100, 200), (200, 101), (64, 64), (120, 90), (31, 47), (256, 256)]
    k = 0
    for cat in ("cat_a", "cat_b"):
        for i in range(3):
            h, w = shapes[k]
            img = Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8))
            msk = Image.fromarray((blob_gt(h, w, 70 + k) * 255).astype(np.uint8))
            if layout == "flat":
                di, dm, stem = root / "images", root / "masks", f"{cat}_{i}"
            else:
                di, dm, stem = root / cat / "images", root / cat / "masks", str(i)
            di.mkdir(parents=True, exist_ok=True); dm.mkdir(parents=True, exist_ok=True)
            img.save(di / f"{stem}.jpg", quality=95)
            msk.save(dm / f"{stem}.png")
            k += 1


def test_mining_main(pred, tmp_path):
    from s3od_amd import mining
    _write_folder(tmp_path, "flat")
    out_dir = tmp_path / "results"
    mining.main(str(tmp_path), pred.model, img_size=S, output_dir=str(out_dir))
    files = glob.glob(str(out_dir / "_eval_results_*.json"))
    assert len(files) == 1
    res = json.load(open(files[0]))
    assert set(res) == {"category_scores", "new_samples", "category_sample_scores", "stable_categories", "unstable_categories"}
    assert set(res["category_scores"]) == {"cat_a", "cat_b"}
    for cat in ("cat_a", "cat_b"):
        want = []
        for i in range(3):
            image, gt = mining._load_pair(str(tmp_path / "images" / f"{cat}_{i}.jpg"))
            want.append(mining.eval_sample(pred, image, gt))
        assert not np.isnan(want).any()
        assert len(res["category_sample_scores"][cat]) == 3
        assert abs(res["category_scores"][cat] - np.mean(want)) <= 4e-6 * max(1.0, abs(np.mean(want)))
    assert res["new_samples"] == mining.calculate_new_samples(res["category_scores"], 20, 100)
    assert sorted(res["stable_categories"]) == sorted(res["unstable_categories"]) == ["cat_a", "cat_b"]


def test_consistency_filter_and_dataset_filter(pred, scorer, tmp_path):
    from synth_sod.data_generation.filter_dataset import DatasetFilter, DatasetLoader
    from synth_sod.data_generation.filters import HorizontalFlipConsistencyFilter
    src = tmp_path / "in"
    _write_folder(src, "classes")
    samples = sorted(DatasetLoader(str(src)).load_samples(), key=lambda s: (s.class_name, s.sample_id))
    assert len(samples) == 6
    scores = [scorer.score(s.load_image(), s.load_mask()) for s in samples]
    eps = 1e-9
    s0, r0 = samples[0], scores[0]
    low = min(r0.iou_orig_gt, r0.iou_flip_gt)
    flt = HorizontalFlipConsistencyFilter(pred, threshold=low - eps, consistency_threshold=r0.iou_orig_flip - eps)
    res = flt.filter(s0)
    assert res.passed is True
    assert res.metadata == {"iou_orig_generated": r0.iou_orig_gt, "iou_flipped_generated": r0.iou_flip_gt,
                            "iou_orig_flipped": r0.iou_orig_flip, "avg_iou": (r0.iou_orig_gt + r0.iou_flip_gt) / 2}
    assert res.score == res.metadata["avg_iou"]
    assert HorizontalFlipConsistencyFilter(pred, threshold=low + eps, consistency_threshold=r0.iou_orig_flip - eps).filter(s0).passed is False
    assert HorizontalFlipConsistencyFilter(pred, threshold=low - eps, consistency_threshold=r0.iou_orig_flip + eps).filter(s0).passed is False
    # the dataset run: thresholds at the median sample, so some pass and some do not
    thr = float(np.median([min(r.iou_orig_gt, r.iou_flip_gt) for r in scores]))
    cons = float(np.median([r.iou_orig_flip for r in scores]))
    expect = {f"{s.class_name}_{s.sample_id}" for s, r in zip(samples, scores)
              if r.iou_orig_gt >= thr and r.iou_flip_gt >= thr and r.iou_orig_flip >= cons}
    print("IoUs:", [(round(r.iou_orig_gt, 4), round(r.iou_flip_gt, 4), round(r.iou_orig_flip, 4)) for r in scores], "passing:", sorted(expect))
    f = HorizontalFlipConsistencyFilter(pred, threshold=thr, consistency_threshold=cons)
    dst = tmp_path / "out"
    stats = DatasetFilter([f]).filter_dataset(str(src), str(dst), save_fail_cases=False)
    got_i = {p.stem for p in (dst / "images").glob("*.jpg")} if (dst / "images").exists() else set()
    got_m = {p.stem for p in (dst / "masks").glob("*.png")} if (dst / "masks").exists() else set()
    assert got_i == got_m == expect
    assert stats["total_samples"] == 6 and stats["passed_samples"] == len(expect) and stats["failed_samples"] == 6 - len(expect)
    assert stats["filter_breakdown"][f.name] == {"total_processed": 6, "passed": len(expect), "failed": 6 - len(expect)}
    assert sum(c["passed"] for c in stats["class_stats"].values()) == len(expect)
