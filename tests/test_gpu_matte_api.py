"""``refine=`` of BackgroundRemoval.remove_background / remove_background_many (s3od_amd/matte.py, infer_many.py).

Every comparison is exact: the refined outputs are the device functions ``refine_alpha`` / ``estimate_foreground`` /
``compose`` applied to the unrefined call's best mask (their own parity with float64 is test_gpu_matte.py's), and the
batched call gives the single-image call's bytes.  Synthetic weights, image_size 256.
"""
import numpy as np
import pytest
import torch
from PIL import Image

from test_gpu_infer_many import S, rand_images

pytestmark = pytest.mark.gpu

MODE_RGB_OVER_COLOR, MODE_RGB_OVER_IMAGE = 1, 2
SHAPES = [(100, 200), (256, 255), (300, 200)]       # tile kernel, Quirk 2 (the single-image path), tile kernel


@pytest.fixture(scope="module")
def br():
    from s3od import BackgroundRemoval
    return BackgroundRemoval("synthetic", image_size=S, compute_dtype="f32")


@pytest.fixture(scope="module")
def images():
    return rand_images(SHAPES, 41)


@pytest.fixture(scope="module")
def bgimg():
    return rand_images(SHAPES[:1], 42)[0]


def same_result(a, b, what=""):
    for name in ("predicted_mask", "all_masks", "all_ious"):
        x, y = getattr(a, name), getattr(b, name)
        assert (x is None) == (y is None), (what, name)
        if x is not None:
            assert x.dtype == y.dtype and np.array_equal(x, y), (what, name)
    for name in ("rgba_image", "composite"):
        x, y = getattr(a, name), getattr(b, name)
        assert (x is None) == (y is None), (what, name)
        if x is not None:
            assert x.mode == y.mode and x.size == y.size and np.array_equal(np.array(x), np.array(y)), (what, name)
    assert (a.stats is None) == (b.stats is None), what
    if a.stats is not None:
        assert np.array_equal(a.stats.pair_inter, b.stats.pair_inter) and np.array_equal(a.stats.pair_union, b.stats.pair_union)
        assert a.stats.area == b.stats.area and a.stats.bbox == b.stats.bbox


def test_refine_none_is_the_call_without_it(br, images, bgimg):
    image = images[0]
    for kw in (dict(), dict(background=(9, 200, 30), stats=True), dict(background=bgimg)):
        same_result(br.remove_background(image, 0.4, refine=None, **kw), br.remove_background(image, 0.4, **kw), kw)
    a = br.remove_background_many(images, batch_size=2, background=(1, 2, 3), stats=True, refine=None)
    b = br.remove_background_many(images, batch_size=2, background=(1, 2, 3), stats=True)
    for x, y in zip(a, b):
        same_result(x, y)


@pytest.mark.parametrize("foreground", [True, False])
def test_refined_outputs_are_the_device_functions_of_the_plain_best_mask(br, images, bgimg, foreground):
    from s3od import Refine
    from s3od_amd.compose import compose
    from s3od_amd.matte import estimate_foreground, refine_alpha
    image = images[0]
    rf = Refine(foreground=foreground)
    plain = br.remove_background(image, 0.3, stats=True)
    src = torch.from_numpy(image).cuda()
    refined = refine_alpha(torch.from_numpy(plain.predicted_mask).cuda(), src, rf.radius, rf.eps)
    colors = estimate_foreground(refined, src, rf.fg_radius) if foreground else src
    over_color = br.remove_background(image, 0.3, background=(10, 250, 40), stats=True, refine=rf)
    over_image = br.remove_background(image, 0.3, background=bgimg, refine=rf)
    for r in (over_color, over_image):
        assert r.predicted_mask.dtype == np.float32 and np.array_equal(r.predicted_mask, refined.cpu().numpy())
        assert not np.array_equal(r.predicted_mask, plain.predicted_mask)
        rgba = np.array(r.rgba_image)
        assert r.rgba_image.mode == "RGBA" and np.array_equal(rgba[..., 3], (r.predicted_mask * 255).astype(np.uint8))
        assert np.array_equal(rgba[..., :3], colors.cpu().numpy())
        assert np.array_equal(r.all_masks, plain.all_masks) and np.array_equal(r.all_ious, plain.all_ious)
    if foreground:
        assert not np.array_equal(np.array(over_color.rgba_image)[..., :3], image)
    else:
        assert np.array_equal(np.array(over_color.rgba_image)[..., :3], image)
    want = compose(refined, colors, MODE_RGB_OVER_COLOR, 10 | 250 << 8 | 40 << 16)
    assert np.array_equal(np.array(over_color.composite), want.cpu().numpy())
    want = compose(refined, colors, MODE_RGB_OVER_IMAGE, 0, torch.from_numpy(bgimg).cuda())
    assert np.array_equal(np.array(over_image.composite), want.cpu().numpy())
    same_result(type(plain)(None, None, None, None, None, over_color.stats), type(plain)(None, None, None, None, None, plain.stats))


def test_many_gives_the_single_call_bytes(br, images):
    from s3od import Refine
    rf = Refine(radius=4, fg_radius=8)
    bgs = [(0, 255, 0), rand_images(SHAPES[1:2], 43)[0], None]
    loop = [br.remove_background(im, 0.3, background=bg, stats=True, refine=rf) for im, bg in zip(images, bgs)]
    plain = [br.remove_background(im, 0.3) for im in images]
    for i in range(3):
        assert not np.array_equal(loop[i].predicted_mask, plain[i].predicted_mask)
    many = br.remove_background_many(images, 0.3, batch_size=2, background=bgs, stats=True, refine=rf)
    for i, (r, ref) in enumerate(zip(many, loop)):
        same_result(r, ref, i)
    assert many[2].composite is None and many[0].composite is not None
    # every combination of what is brought back: what remains is what the single call gave
    for return_masks in (True, False):
        for return_all_masks in (True, False):
            for return_rgba in (True, False):
                for use_bg in (True, False):
                    if not (return_masks or return_rgba or use_bg):
                        continue
                    key = dict(return_masks=return_masks, return_all_masks=return_all_masks, return_rgba=return_rgba)
                    got = br.remove_background_many(images, 0.3, batch_size=2, background=bgs if use_bg else None, refine=rf, **key)
                    for i, (r, ref) in enumerate(zip(got, loop)):
                        want = type(ref)(predicted_mask=ref.predicted_mask if return_masks else None,
                                         all_masks=ref.all_masks if return_masks and return_all_masks else None,
                                         all_ious=ref.all_ious, rgba_image=ref.rgba_image if return_rgba else None,
                                         composite=ref.composite if use_bg else None, stats=None)
                        same_result(r, want, (i, key, use_bg))
    # the engine's buffers are reused by an unrefined call after a refined one, and the other way round
    again = br.remove_background_many(images, 0.3, batch_size=2)
    for r, ref in zip(again, plain):
        same_result(r, ref)
    for r, ref in zip(br.remove_background_many(images, 0.3, batch_size=2, background=bgs, stats=True, refine=rf), loop):
        same_result(r, ref)


def test_refine_must_be_a_refine(br, images):
    with pytest.raises(TypeError, match="Refine"):
        br.remove_background(images[0], refine=True)
    with pytest.raises(TypeError, match="Refine"):
        br.remove_background_many(images, refine={"radius": 4})
