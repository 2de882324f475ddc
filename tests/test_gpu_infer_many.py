"""Batched inference over lists of differently sized images: s3od_preprocess_batch, s3od_best_index,
s3od_postprocess_batch, BackgroundRemoval.remove_background_many, SODPredictor.predict_many and
process_dataset(batch_size > 1), against their single-image counterparts.

Bounds: preprocess bit-identical to s3od_preprocess; masks <= 2e-6 against F.interpolate(antialias=True) on the
CPU and against s3od_sigmoid_unpad_resize (bit-identical where the batched two-pass branch runs); alpha, RGB and
best index exact; many-vs-loop 1e-5 max-rel (the batch-invariance bound of test_c2_batch_equals_single_images).
Synthetic weights, image_size 256 unless a test says otherwise.
"""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from PIL import Image

pytestmark = pytest.mark.gpu

S = 256
SHAPES11 = [(100, 200), (480, 640), (20, 30), (40, 640), (200, 100), (640, 480), (30, 20), (640, 40), (256, 256),
            (31, 31), (512, 512)]
QUIRK2 = [(256, 255), (255, 256)]
ODD = [(101, 256), (160, 111)]
# the thirteen non-raising shapes in a fixed shuffled order: ragged last chunk at batch_size 4, Quirk 2 in the middle
SHAPES13 = [(480, 640), (30, 20), (256, 256), (100, 200), (256, 255), (640, 40), (512, 512), (255, 256), (20, 30),
            (200, 100), (40, 640), (31, 31), (640, 480)]


def rel_max(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-12))


def rand_images(shapes, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in shapes]


def _align(n, a=16):
    return (n + a - 1) // a * a


def _dev_bytes(obj):
    return torch.from_numpy(np.frombuffer(bytes(obj), dtype=np.uint8).copy()).cuda()


def pack_images(images):
    offs, off = [], 0
    for im in images:
        offs.append(off)
        off = _align(off + im.size)
    host = np.zeros(off, np.uint8)
    for im, o in zip(images, offs):
        host[o:o + im.size] = im.reshape(-1)
    return torch.from_numpy(host).cuda(), offs


def preprocess_batch(images, size):
    from s3od_amd._lib import lib, stream
    from s3od_amd.infer_many import PreDesc
    from s3od_amd.utils import get_pad_info
    B = len(images)
    dev, offs = pack_images(images)
    descs = (PreDesc * B)()
    for b, im in enumerate(images):
        info = get_pad_info(im, size)
        descs[b] = PreDesc(offs[b], im.shape[0], im.shape[1], *info["resized_size"], info["height_pad"], info["width_pad"])
    out = torch.empty((B, 3, size, size), dtype=torch.float32, device="cuda")
    lib()("s3od_preprocess_batch", dev, _dev_bytes(descs), ctypes.addressof(descs), B, size, out, stream())
    torch.cuda.synchronize()
    return out


def preprocess_single(im, size):
    from s3od_amd._lib import lib, stream
    from s3od_amd.utils import get_pad_info
    info = get_pad_info(im, size)
    x = torch.empty((1, 3, size, size), dtype=torch.float32, device="cuda")
    lib()("s3od_preprocess", torch.from_numpy(im).cuda(), im.shape[0], im.shape[1], *info["resized_size"],
          info["height_pad"], info["width_pad"], size, x, stream())
    torch.cuda.synchronize()
    return x[0]


# ---------------------------------------------------------------------------------- 1. preprocess
@pytest.mark.parametrize("reverse", [False, True])
def test_preprocess_batch_bit_identical(reverse):
    images = rand_images(SHAPES11, 1)
    if reverse:
        images = images[::-1]
    out = preprocess_batch(images, S)
    for b, im in enumerate(images):
        assert torch.equal(out[b], preprocess_single(im, S)), f"image {b} {im.shape[:2]}"


def test_preprocess_batch_unaligned_canvas():
    """a canvas size that is no multiple of 4 takes the scalar stores"""
    images = rand_images([(100, 200), (37, 37)], 2)
    out = preprocess_batch(images, 250)
    for b, im in enumerate(images):
        assert torch.equal(out[b], preprocess_single(im, 250))


# ---------------------------------------------------------------------------------- 2./3. postprocess
def post_geometry(shape, size):
    from s3od_amd.utils import get_pad_info
    info = get_pad_info(np.broadcast_to(np.uint8(0), shape), size)
    ph, pw = info["height_pad"], info["width_pad"]
    return ph, pw, size - 2 * ph, size - 2 * pw


def is_two_pass(h, w, H0, W0):
    return np.float32(h) / np.float32(H0) > 2 or np.float32(w) / np.float32(W0) > 2


def postprocess_batch(logits, iou_logits, images, size, all_masks=True):
    """-> per image (masks [planes,H0,W0], rgba [H0,W0,4]), ious [B,NM], best [B]"""
    from s3od_amd._lib import lib, stream
    from s3od_amd.infer_many import PostDesc
    B, NM = logits.shape[:2]
    planes = NM if all_masks else 1
    dev, offs = pack_images(images)
    descs = (PostDesc * B)()
    mo = ro = to = 0
    for b, im in enumerate(images):
        H0, W0 = im.shape[:2]
        ph, pw, h, w = post_geometry((H0, W0), size)
        descs[b] = PostDesc(offs[b], mo, ro, to, ph, pw, h, w, H0, W0)
        mo += planes * H0 * W0; ro += H0 * W0 * 4; to += planes * h * W0
    masks = torch.full((mo,), -1.0, dtype=torch.float32, device="cuda")
    rgba = torch.zeros((ro,), dtype=torch.uint8, device="cuda")
    tmp = torch.empty((max(to, 4),), dtype=torch.float32, device="cuda")
    ious = torch.empty((B, NM), dtype=torch.float32, device="cuda")
    best = torch.empty((B,), dtype=torch.int32, device="cuda")
    lib()("s3od_best_index", iou_logits, B, NM, ious, best, stream())
    lib()("s3od_postprocess_batch", logits, B, NM, size, size, best, dev, _dev_bytes(descs), ctypes.addressof(descs),
          1 if all_masks else 0, masks, rgba, tmp, stream())
    torch.cuda.synchronize()
    masks, rgba = masks.cpu().numpy(), rgba.cpu().numpy()
    out = []
    for b, im in enumerate(images):
        H0, W0 = im.shape[:2]
        d = descs[b]
        out.append((masks[d.mask_off:d.mask_off + planes * H0 * W0].reshape(planes, H0, W0),
                    rgba[d.rgba_off:d.rgba_off + H0 * W0 * 4].reshape(H0, W0, 4)))
    return out, ious.cpu().numpy(), best.cpu().numpy()


def postprocess_single(logits_b, shape, size):
    from s3od_amd._lib import lib, stream
    NM = logits_b.shape[0]
    H0, W0 = shape
    ph, pw, h, w = post_geometry(shape, size)
    tmp = torch.empty((NM, h, W0), dtype=torch.float32, device="cuda")
    masks = torch.empty((NM, H0, W0), dtype=torch.float32, device="cuda")
    lib()("s3od_sigmoid_unpad_resize", logits_b.contiguous(), NM, size, size, ph, pw, h, w, H0, W0, tmp, masks, stream())
    torch.cuda.synchronize()
    return masks.cpu().numpy()


def cpu_reference(logits_b, shape, size):
    ph, pw, h, w = post_geometry(shape, size)
    crop = torch.sigmoid(logits_b.cpu())[:, ph:ph + h, pw:pw + w]
    return F.interpolate(crop[None], size=shape, mode="bilinear", align_corners=False, antialias=True)[0].numpy()


def _iou_logits(B, seed):
    g = torch.Generator().manual_seed(seed)
    iou = torch.randn((B, 3), generator=g)
    iou[0] = torch.tensor([1.5, 1.5, -1.0])          # two equal maxima: the first index wins
    if B > 1:
        iou[1] = torch.tensor([0.2, 3.0, 3.0])
    return iou.cuda()


@pytest.fixture(scope="module")
def post256():
    g = torch.Generator().manual_seed(3)
    logits = (torch.randn((len(SHAPES11), 3, S, S), generator=g) * 4).cuda()
    images = rand_images(SHAPES11, 4)
    out, ious, best = postprocess_batch(logits, _iou_logits(len(SHAPES11), 5), images, S)
    return dict(logits=logits, images=images, out=out, ious=ious, best=best)


def check_masks(logits, shapes, out, size):
    worst_ref = worst_single = 0.0
    for b, shape in enumerate(shapes):
        masks = out[b][0]
        e_ref = float(np.abs(masks - cpu_reference(logits[b], shape, size)).max())
        single = postprocess_single(logits[b], shape, size)
        e_single = float(np.abs(masks - single).max())
        ph, pw, h, w = post_geometry(shape, size)
        two_pass = is_two_pass(h, w, *shape)
        print(f"post {shape} @ {size}: vs F.interpolate {e_ref:.3g}, vs single-image entry {e_single:.3g}"
              f" ({'two-pass' if two_pass else 'tile'})")
        assert e_ref <= 2e-6 and e_single <= 2e-6, (shape, e_ref, e_single)
        if two_pass:
            assert np.array_equal(masks, single), shape
        worst_ref, worst_single = max(worst_ref, e_ref), max(worst_single, e_single)
    print(f"post @ {size}: worst vs F.interpolate {worst_ref:.3g}, worst vs single-image entry {worst_single:.3g}")


def test_postprocess_batch_masks(post256):
    assert any(is_two_pass(*post_geometry(s, S)[2:], *s) for s in SHAPES11)
    assert any(not is_two_pass(*post_geometry(s, S)[2:], *s) for s in SHAPES11)
    check_masks(post256["logits"], SHAPES11, post256["out"], S)


@pytest.mark.parametrize("shapes", [[(2000, 2000), (40, 4000)], [(40, 30)]], ids=["large", "downscale"])
def test_postprocess_batch_masks_1024(shapes):
    """(2000, 2000) + (40, 4000): the second image's outputs start 12e6 floats in.  (40, 30): a 1024 x 768 crop
    down to 40 x 30, the two-pass branch at the full canvas."""
    g = torch.Generator().manual_seed(6)
    logits = (torch.randn((len(shapes), 3, 1024, 1024), generator=g) * 4).cuda()
    images = rand_images(shapes, 7)
    out, _, best = postprocess_batch(logits, _iou_logits(len(shapes), 8), images, 1024)
    check_masks(logits, shapes, out, 1024)
    for b, im in enumerate(images):
        masks, rgba = out[b]
        assert np.array_equal(rgba[..., :3], im)
        assert np.array_equal(rgba[..., 3], (masks[best[b]] * 255).astype(np.uint8))


def test_postprocess_batch_rgba_and_best(post256):
    ious, best = post256["ious"], post256["best"]
    assert np.array_equal(best, np.argmax(ious, axis=1))
    assert best[0] == 0 and best[1] == 1 and ious[0, 0] == ious[0, 1] and ious[1, 1] == ious[1, 2]
    for b, im in enumerate(post256["images"]):
        masks, rgba = post256["out"][b]
        assert np.array_equal(rgba[..., :3], im)
        assert np.array_equal(rgba[..., 3], (masks[best[b]] * 255).astype(np.uint8)), im.shape


def test_postprocess_batch_best_only(post256):
    out, _, best = postprocess_batch(post256["logits"], _iou_logits(len(SHAPES11), 5), post256["images"], S, all_masks=False)
    assert np.array_equal(best, post256["best"])
    for b in range(len(SHAPES11)):
        assert out[b][0].shape[0] == 1
        assert np.array_equal(out[b][0][0], post256["out"][b][0][best[b]])
        assert np.array_equal(out[b][1], post256["out"][b][1])


def test_postprocess_batch_rejects_bad_descriptor():
    from s3od_amd._lib import HipLibError, lib, stream
    from s3od_amd.infer_many import PostDesc
    descs = (PostDesc * 1)(PostDesc(0, 0, 0, 0, 100, 0, 200, 256, 50, 50))      # pad_h + h > LH
    z = torch.zeros(16, device="cuda")
    with pytest.raises(HipLibError, match="crop outside"):
        lib()("s3od_postprocess_batch", z, 1, 3, 256, 256, z, None, _dev_bytes(descs), ctypes.addressof(descs), 1, z, None, z,
              stream())


# ---------------------------------------------------------------------------------- 4.-6. remove_background_many
@pytest.fixture(scope="module")
def br():
    from s3od import BackgroundRemoval
    return BackgroundRemoval("synthetic", image_size=S, compute_dtype="f32")


def check_against_loop(br, images, many):
    assert len(many) == len(images)
    worst = 0.0
    for i, (im, r) in enumerate(zip(images, many)):
        arr = np.array(im.convert("RGB")) if isinstance(im, Image.Image) else im
        ref = br.remove_background(im)
        assert r.predicted_mask.shape == ref.predicted_mask.shape == arr.shape[:2]       # also: order = input order
        assert r.all_masks.shape == ref.all_masks.shape and r.all_ious.shape == ref.all_ious.shape
        e = max(rel_max(r.all_ious, ref.all_ious), rel_max(r.all_masks, ref.all_masks))
        worst = max(worst, e)
        assert e <= 1e-5, (i, arr.shape, e)
        assert int(r.all_ious.argmax()) == int(ref.all_ious.argmax())
        assert np.array_equal(r.predicted_mask, r.all_masks[r.all_ious.argmax()])
        rgba = np.array(r.rgba_image)
        assert np.array_equal(rgba[..., 3], (r.predicted_mask * 255).astype(np.uint8))
        assert np.array_equal(rgba[..., :3], arr)
        assert r.rgba_image.size == ref.rgba_image.size and r.rgba_image.mode == "RGBA"
    return worst


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_many_equals_loop(br, dtype):
    images = rand_images(SHAPES13, 9)
    br.model.compute_dtype = dtype
    try:
        many = br.remove_background_many(images, batch_size=4)
        worst = check_against_loop(br, images, many)
        print(f"remove_background_many vs loop, {dtype}: worst max-rel {worst:.3g}")
        best_only = br.remove_background_many(images, batch_size=4, return_all_masks=False)
        for r, b in zip(many, best_only):
            assert b.all_masks is None
            assert np.array_equal(b.predicted_mask, r.predicted_mask)
            assert np.array_equal(np.array(b.rgba_image), np.array(r.rgba_image))
    finally:
        br.model.compute_dtype = "f32"


def test_many_accepts_pil(br):
    images = rand_images([(100, 200), (256, 256), (640, 480)], 10)
    images[1] = Image.fromarray(images[1])
    many = br.remove_background_many(images, batch_size=2)
    check_against_loop(br, images, many)


def test_many_errors(br, monkeypatch):
    from s3od import BackgroundRemoval
    images = rand_images(SHAPES13[:2] + [ODD[0]] + SHAPES13[2:] + [ODD[1]], 11)

    def boom(*a, **k):
        raise AssertionError("the model ran before the list was validated")
    with monkeypatch.context() as m:
        m.setattr(br.model, "forward", boom)
        with pytest.raises(ValueError, match="image 2"):
            br.remove_background_many(images, batch_size=4)
    assert br.remove_background_many([]) == []
    with pytest.raises(ValueError):
        br.remove_background_many(images[:1], batch_size=0)
    # without the reference quirks the same list succeeds and every image batches
    free = BackgroundRemoval.__new__(BackgroundRemoval)
    free.__dict__.update(br.__dict__)
    free.exact_reference_quirks, free._many = False, None
    calls = []
    with monkeypatch.context() as m:
        m.setattr(free, "remove_background", lambda *a, **k: calls.append(1))
        res = free.remove_background_many(images, batch_size=4)
    assert not calls and len(res) == 15
    for im, r in zip(images, res):
        ref = free.remove_background(im)
        assert r.all_masks.shape == (3, *im.shape[:2])
        assert max(rel_max(r.all_ious, ref.all_ious), rel_max(r.all_masks, ref.all_masks)) <= 1e-5, im.shape


def test_many_results_own_their_memory(br):
    first = br.remove_background_many(rand_images(SHAPES11[:5], 12), batch_size=2)
    keep = [(r.predicted_mask.copy(), r.all_masks.copy(), r.all_ious.copy(), np.array(r.rgba_image)) for r in first]
    br.remove_background_many(rand_images(SHAPES11[:5], 13), batch_size=2)
    for r, (pm, am, io, rgba) in zip(first, keep):
        assert np.array_equal(r.predicted_mask, pm) and np.array_equal(r.all_masks, am)
        assert np.array_equal(r.all_ious, io) and np.array_equal(np.array(r.rgba_image), rgba)


def test_many_plain_call_equals_old_entry(br):
    """The plain call goes through s3od_postprocess_batch_out with one RGBA row per image; it gives, bit for bit, what
    the same chunks give when driven by hand through s3od_preprocess_batch -> model -> s3od_best_index ->
    s3od_postprocess_batch (the eval forward has no atomics and the two C entries share one implementation)."""
    shapes = [(100, 200), (20, 30), (640, 480), (31, 31)]
    assert {bool(is_two_pass(*post_geometry(s, S)[2:], *s)) for s in shapes} == {True, False}
    images = rand_images(shapes, 17)
    many = br.remove_background_many(images, batch_size=2)
    assert len(many) == len(images)
    for c in range(0, len(images), 2):
        chunk = images[c:c + 2]
        with torch.no_grad():
            out = br.model(preprocess_batch(chunk, S))
        old, ious, best = postprocess_batch(out["pred_masks"].float().contiguous(),
                                            out["pred_iou"].float().reshape(len(chunk), 3).contiguous(), chunk, S)
        for b, (masks, rgba) in enumerate(old):
            r = many[c + b]
            assert np.array_equal(r.all_ious, ious[b]) and int(r.all_ious.argmax()) == best[b], shapes[c + b]
            assert np.array_equal(r.all_masks, masks), shapes[c + b]
            assert np.array_equal(r.predicted_mask, masks[best[b]]), shapes[c + b]
            assert np.array_equal(np.array(r.rgba_image), rgba), shapes[c + b]


# ---------------------------------------------------------------------------------- 7. predict_many
def check_predictions(pred, images, many, threshold=0.5):
    worst = 0.0
    for im, r in zip(images, many):
        ref = pred.predict(im)
        assert r.soft_mask.shape == ref.soft_mask.shape == im.shape[:2]
        e = rel_max(r.soft_mask, ref.soft_mask)
        near = np.abs(ref.soft_mask - threshold) <= 1e-5
        assert np.array_equal(r.binary_mask[~near], ref.binary_mask[~near])
        assert np.array_equal(r.binary_mask, (r.soft_mask > threshold).astype(np.float32))
        if ref.all_masks is None:
            assert r.all_masks is None and r.all_ious is None
        else:
            e = max(e, rel_max(r.all_ious, ref.all_ious))
            assert int(r.all_ious.argmax()) == int(ref.all_ious.argmax())
            assert r.all_masks.shape == ref.all_masks.shape and r.all_masks.dtype == ref.all_masks.dtype
            # predict returns the other masks thresholded only: a pixel can flip only where its soft value lies within
            # 1e-5 of the threshold; with soft values spread over [0, 1] at a density of order 1 that is a fraction
            # of about 2e-5 of the pixels
            assert float(np.mean(r.all_masks != ref.all_masks)) <= 1e-4
        worst = max(worst, e)
        assert e <= 1e-5, (im.shape, e)
    return worst


def test_predict_many_dinob():
    from s3od_amd.model import DPTSegmentation
    from s3od_amd.sod_predictor import SODPredictor
    pred = SODPredictor(DPTSegmentation(compute_dtype="f32"), image_size=840)
    images = rand_images([(480, 640), (640, 480), (300, 300)], 14)
    many = pred.predict_many(images, batch_size=3)
    print(f"predict_many vs loop, dinob @ 840: worst max-rel {check_predictions(pred, images, many):.3g}")


def test_predict_many_dinol():
    from s3od_amd.model import DPTSegmentation
    from s3od_amd.sod_predictor import SODPredictor
    model = DPTSegmentation(compute_dtype="f32", num_classes=1, num_outputs=1,
                            encoder_name="facebook/dinov3-vitl16-pretrain-lvd1689m")
    pred = SODPredictor(model, image_size=224)
    images = rand_images([(100, 200), (224, 224), (300, 150)], 15)
    many = pred.predict_many(images, batch_size=2)
    print(f"predict_many vs loop, dinol @ 224: worst max-rel {check_predictions(pred, images, many):.3g}")


# ---------------------------------------------------------------------------------- 8. process_dataset
def test_process_dataset_batched(tmp_path):
    from s3od_amd.metrics import process_dataset
    from s3od_amd.model import DPTSegmentation
    from s3od_amd.sod_predictor import SODPredictor
    (tmp_path / "images").mkdir(); (tmp_path / "masks").mkdir()
    rng = np.random.default_rng(16)
    for i, (h, w) in enumerate([(100, 200), (200, 100), (256, 256), (31, 31), (480, 640)]):
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(tmp_path / "images" / f"im{i}.png")
        yy, xx = np.mgrid[:h, :w]
        gt = (((yy - h / 2) / (h / 3)) ** 2 + ((xx - w / 2) / (w / 4)) ** 2 <= 1).astype(np.uint8) * 255
        Image.fromarray(gt).save(tmp_path / "masks" / f"im{i}.png")
    pred = SODPredictor(DPTSegmentation(compute_dtype="f32"), image_size=S)
    one = process_dataset(str(tmp_path), pred, compute_best_metrics=True, batch_size=1)
    four = process_dataset(str(tmp_path), pred, compute_best_metrics=True, batch_size=4)
    tol = {"MAE": 1e-9, "Em": 1e-9, "wF": 1e-9, "MaxF": 2e-7, "AvgF": 2e-6, "Sm": 2e-6}      # DESIGN §3, test_gpu_metrics.py
    assert one.keys() == four.keys()
    for part in one:
        assert one[part].keys() == four[part].keys() == tol.keys()
        for k, t in tol.items():
            a, b = float(one[part][k]), float(four[part][k])
            print(f"process_dataset {part}.{k}: batch_size 1 {a:.12g}, 4 {b:.12g}, rel diff {abs(a - b) / max(abs(a), 1e-300):.3g}")
    for part in one:
        for k, t in tol.items():
            a, b = float(one[part][k]), float(four[part][k])
            assert abs(a - b) <= t * max(abs(a), 1e-300), (part, k, a, b)
