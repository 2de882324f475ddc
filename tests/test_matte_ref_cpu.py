"""Pins the float64 reference of the matting kernels (tests/_matte_ref.py) by properties that do not depend on it, and
the parts of the feature that need no GPU: ``Refine``'s validation, the ``refine`` argument of both
``remove_background*`` methods and the three C entries in the header."""
import inspect

import numpy as np
import pytest

import _matte_ref as R


def brute_box_mean(v, r):
    H, W = v.shape
    out = np.zeros((H, W))
    for y in range(H):
        for x in range(W):
            acc, n = 0.0, 0
            for yy in range(y - r, y + r + 1):
                for xx in range(x - r, x + r + 1):
                    if 0 <= yy < H and 0 <= xx < W:
                        acc += v[yy, xx]
                        n += 1
            out[y, x] = acc / n
    return out


@pytest.mark.parametrize("r", [1, 3, 20])
def test_box_mean_is_the_clipped_window_mean(r):
    v = np.random.default_rng(r).normal(size=(9, 11))
    np.testing.assert_allclose(R.box_mean(v, r), brute_box_mean(v, r), rtol=0, atol=1e-13)
    if r == 20:         # the window is the whole image
        np.testing.assert_allclose(R.box_mean(v, r), np.full_like(v, v.mean()), rtol=0, atol=1e-13)


def test_box_mean_keeps_trailing_axes():
    v = np.random.default_rng(0).normal(size=(7, 6, 3))
    for c in range(3):
        np.testing.assert_array_equal(R.box_mean(v, 2)[..., c], R.box_mean(v[..., c], 2))


@pytest.mark.parametrize("eps", [1e-6, 1e-2])
def test_refine_returns_a_constant_mask_unchanged(eps):
    src, _ = R.make_case(23, 31, 0)
    q = R.refine(np.full((23, 31), 0.375, np.float32), src, 4, eps)
    np.testing.assert_allclose(q, 0.375, rtol=0, atol=1e-12)


def test_refine_reproduces_a_mask_that_is_affine_in_the_image():
    rng = np.random.default_rng(1)
    src = rng.integers(0, 256, (21, 26, 3), dtype=np.uint8)     # noise everywhere: Sigma is well away from 0
    w, c = np.array([0.3, -0.2, 0.25]), 0.4
    p = (src / 255.0) @ w + c
    assert p.min() > 0 and p.max() < 1
    np.testing.assert_allclose(R.refine(p, src, 3, 1e-12), p, rtol=0, atol=1e-6)


def test_foreground_is_the_image_where_the_window_is_opaque():
    src, m = R.make_case(40, 50, 2)
    r = 2
    F = R.foreground(m, src, r)
    opaque = R.box_mean((m == 1.0).astype(np.float64), r) == 1.0
    assert opaque.sum() > 10
    np.testing.assert_allclose(F[opaque], (src / 255.0)[opaque], rtol=0, atol=1e-12)
    assert np.array_equal(R.to_bytes(F)[opaque], src[opaque])


def test_make_case_has_its_special_regions():
    src, m = R.make_case(37, 53, 0)
    assert src.dtype == np.uint8 and src.shape == (37, 53, 3) and m.dtype == np.float32 and m.shape == (37, 53)
    assert (src[:9] == 128).all() and src[9:].std() > 10
    assert (m[:, :6] == 0).all() and (m == 1).sum() >= 7 * 10 and 0 < ((m > 0) & (m < 1)).mean()
    src2, m2 = R.make_case(37, 53, 0)
    assert np.array_equal(src, src2) and np.array_equal(m, m2)


# ---------------------------------------------------------------------------------- the feature's CPU-visible parts
def test_refine_validates_like_the_c_entries():
    from s3od_amd import Refine
    import s3od
    assert s3od.Refine is Refine
    d = Refine()
    assert (d.radius, d.eps, d.foreground, d.fg_radius) == (16, 1e-4, True, 64)
    Refine(radius=1, eps=1e-6, fg_radius=256)
    Refine(radius=256, eps=1.0, foreground=False, fg_radius=1)
    for bad in (dict(radius=0), dict(radius=257), dict(radius=2.5), dict(fg_radius=0), dict(fg_radius=257),
                dict(eps=0.0), dict(eps=9e-7), dict(eps=1.5), dict(eps=float("nan")), dict(foreground=1)):
        with pytest.raises(ValueError):
            Refine(**bad)
    with pytest.raises(Exception):      # frozen
        d.radius = 3


def test_remove_background_methods_take_refine():
    from s3od_amd.predictor import BackgroundRemoval
    for fn in (BackgroundRemoval.remove_background, BackgroundRemoval.remove_background_many):
        p = inspect.signature(fn).parameters["refine"]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None


def test_header_declares_the_matte_entries():
    from s3od_amd._lib import parse_header
    decls = parse_header()
    assert decls["s3od_matte_ws"] == ("int", ["int", "int", "long*"])
    assert decls["s3od_matte_refine"] == ("int", ["float*", "void*", "int", "int", "int", "float", "void*", "long", "float*", "void*"])
    assert decls["s3od_matte_foreground"] == ("int", ["float*", "void*", "int", "int", "int", "void*", "long", "void*", "void*"])


def test_plan_keeps_the_unrefined_layout_and_adds_the_refined_plane():
    """``refine`` moves no planned offset of a chunk's host-visible outputs except by the refined planes it adds, tells
    the post-processing kernels to write no row, and keeps one float plane per image on the device."""
    from s3od_amd.image_ops import MODE_NONE, pack_color, reference_geometry
    from s3od_amd.infer_many import Request, plan_chunk
    from s3od_amd.matte import Refine
    shapes = [(40, 64), (64, 48)]
    geoms = [reference_geometry(h, w, 64, False)[0] for h, w in shapes]
    px = [h * w for h, w in shapes]
    for all_masks in (True, False):
        for want_masks in (True, False):
            kw = dict(all_masks=all_masks, want_masks=want_masks, backgrounds=[pack_color((1, 2, 3)), None])
            p0 = plan_chunk(shapes, geoms, 3, 64, 64, Request(**kw))
            p1 = plan_chunk(shapes, geoms, 3, 64, 64, Request(refine=Refine(), **kw))
            assert p0.ref_off is None and p0.dev_bytes == p0.out_bytes and p0.dev_planes == p0.planes
            assert p1.rows == p0.rows and p1.planes == p0.planes and all(o.mode == MODE_NONE for o in p1.outd)
            assert [o.mode for o in p0.outd] == [0, 1, 0, MODE_NONE]
            extra = 4 * sum(px) if (all_masks and want_masks) else 0
            assert p1.outs_off == p0.outs_off + extra and p1.out_bytes == p0.out_bytes + extra
            if want_masks:
                assert p1.masks_off == p0.masks_off and p1.dev_bytes == p1.out_bytes
                first = p1.masks_off + (3 * 4 * sum(px) if all_masks else 0)
                assert first % 4 == 0 and p1.ref_off == [first, first + 4 * px[0]]
            else:       # the plane only the refinement reads lies behind what is downloaded
                assert p1.dev_planes == 1 and p1.masks_off >= p1.out_bytes
                assert p1.ref_off == [p1.masks_off, p1.masks_off + 4 * px[0]]
                assert p1.dev_bytes == p1.masks_off + 4 * sum(px)
