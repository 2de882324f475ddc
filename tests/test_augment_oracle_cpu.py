"""CPU self-check of the geometry / colour restatements in oracle/augment_oracle.py that the device
tests of data_ops.hip compare against (tests/test_gpu_augment_geometry.py, test_gpu_augment.py,
test_gpu_data.py): exact permutations for flips and quarter turns, identities, and the HSV round trip
against the standard library's colorsys."""
import colorsys

import numpy as np
import pytest

from oracle import augment_oracle as AO
from s3od_amd.data import AugParams, letterbox

S = 32


def _params(h0, w0, Minv, S=S):
    p = AugParams()
    for i, v in enumerate(list(Minv[0]) + list(Minv[1])):
        p.A[i] = float(v)
    nh, nw, ph, pw = letterbox(h0, w0, S)
    p.H0, p.W0, p.new_h, p.new_w, p.pad_h, p.pad_w = h0, w0, nh, nw, ph, pw
    p.bright = p.contrast = p.sat = 1.0
    p.mult[0] = p.mult[1] = p.mult[2] = 1.0
    p.raw = 1
    return p


def _sample(h, w, seed=0):
    r = np.random.default_rng(seed)
    return r.integers(0, 256, (h, w, 3), dtype=np.uint8), (r.random((h, w)) > 0.5).astype(np.uint8) * 255


@pytest.mark.parametrize("hw", [(25, 32), (48, 20), (12, 16)])
def test_identity_reproduces_the_canvas(hw):
    img, msk = _sample(*hw)
    p = _params(*hw, np.eye(3))
    canvas, mcan = AO.letterbox_canvas(img, msk, p, S)
    assert canvas.shape == (3, S, S) and 0 <= canvas.min() and canvas.max() <= 1
    assert (canvas[:, :p.pad_h] == 0).all() and (canvas[:, :, :p.pad_w] == 0).all()
    assert set(np.unique(mcan)) <= {0.0, 1.0} and mcan.sum() > 0
    cx, cy, outside = AO.warp_coords(p, S)
    yy, xx = np.mgrid[0:S, 0:S]
    assert np.array_equal(cx, xx) and np.array_equal(cy, yy) and not outside.any()
    oi, om = AO.augment_sample(img, msk, p, S)
    assert np.array_equal(oi, canvas) and np.array_equal(om, mcan)


def test_flip_and_rot90_are_exact_permutations():
    img, msk = _sample(25, 32, 1)
    canvas, mcan = AO.letterbox_canvas(img, msk, _params(25, 32, np.eye(3)), S)
    cases = {
        "hflip": (np.array([[-1, 0, S], [0, 1, 0], [0, 0, 1.0]]), lambda a: a[..., ::-1]),
        "vflip": (np.array([[1, 0, 0], [0, -1, S], [0, 0, 1.0]]), lambda a: a[..., ::-1, :]),
        "rot90": (np.array([[0, -1, S], [1, 0, 0], [0, 0, 1.0]]), lambda a: np.rot90(a, 1, (-2, -1))),   # canvas (S - y, x)
        "rot180": (np.array([[-1, 0, S], [0, -1, S], [0, 0, 1.0]]), lambda a: a[..., ::-1, ::-1]),
    }
    yy, xx = np.mgrid[0:S, 0:S]
    for name, (Minv, perm) in cases.items():
        p = _params(25, 32, Minv)
        cx, cy, _ = AO.warp_coords(p, S)
        assert np.array_equal(cx, perm(xx)) and np.array_equal(cy, perm(yy)), name
        oi, om = AO.augment_sample(img, msk, p, S)
        assert np.array_equal(oi, perm(canvas)) and np.array_equal(om, perm(mcan)), name
        assert not np.array_equal(oi, canvas), name


def test_warp_order_outside_kdist_and_perspective():
    """grid -> elastic -> outside -> kdist -> homography, on values worked by hand."""
    p = _params(32, 32, np.array([[2.0, 0, 1.0], [0, 3.0, -1.0], [0, 0, 1]]))
    p.persp[0], p.persp[1] = 0.5, 0.25
    cx, cy, _ = AO.warp_coords(p, S)
    den = 0.5 * 3.5 + 0.25 * 1.5 + 1
    assert abs(cx[1, 3] - ((2 * 3.5 + 1) / den - 0.5)) < 1e-12 and abs(cy[1, 3] - ((3 * 1.5 - 1) / den - 0.5)) < 1e-12
    p = _params(32, 32, np.eye(3))
    p.kdist = 0.5
    cx, cy, _ = AO.warp_coords(p, S)
    u, v = (3.5 - 16) / 16, (1.5 - 16) / 16
    f = 1 + 0.5 * (u * u + v * v)
    assert abs(cx[1, 3] - (16 + u * f * 16 - 0.5)) < 1e-12 and abs(cy[1, 3] - (16 + v * f * 16 - 0.5)) < 1e-12
    grid = np.stack([np.arange(S) * 1.0, np.arange(S) * 0.5])
    el = np.zeros((2, S, S)); el[0, :, 0] = -2.0; el[1, 5, 5] = 0.25
    cx, cy, outside = AO.warp_coords(_params(32, 32, np.eye(3)), S, grid=grid, elastic=el)
    assert outside[:, 0].all() and not outside[:, 1:].any()
    assert cx[4, 7] == 7.0 and cy[4, 7] == 2.0 and cy[5, 5] == 2.75
    img, msk = _sample(32, 32, 2)
    oi, om = AO.augment_sample(img, msk, _params(32, 32, np.eye(3)), S, grid=grid, elastic=el)
    assert (oi[:, :, 0] == 0).all() and (om[:, 0] == 0).all()


def test_remap_bound_and_ambiguity_helpers():
    canvas = np.zeros((3, S, S)); canvas[1, 10, 10] = 0.8
    cx = np.array([[10.3, 20.0, -40.0]]); cy = np.array([[9.7, 20.0, 5.0]])
    b = AO.remap_bound(canvas, cx, cy, S)
    e = 16 * 2.0 ** -24
    assert np.allclose(b, [1e-5 + 0.8 * e * S, 1e-5, 1e-5], rtol=1e-12, atol=0)
    canvas[:] = 0.5                                       # the zero border counts as a neighbour
    b = AO.remap_bound(canvas, np.array([[0.5, 100.0]]), np.array([[5.0, 5.0]]), S)
    assert np.allclose(b, [1e-5 + 0.5 * e * S, 1e-5], rtol=1e-12, atol=0)
    amb = AO.nearest_ambiguous(np.array([1.4995, 1.2, 3.5004, 2.0]), np.array([0.0, 0.0, 0.0, 7.4999]))
    assert amb.tolist() == [True, False, True, True]


def test_hsv_shift_identity_and_colorsys():
    r = np.random.default_rng(0)
    x = r.random((3, 40, 25))
    x[:, 0, :5] = r.random((1, 5))                        # greys
    x[:, 1, :3] = 0.0; x[:, 1, 3:6] = 1.0                 # black and white
    assert np.abs(AO.hsv_shift(x, 0.0, 0.0, 0.0) - x).max() <= 1e-12
    assert np.abs(AO.hsv_shift(x, 360.0, 0.0, 0.0) - x).max() <= 1e-12
    for dh, ds, dv in [(50.0, 0.0, 0.0), (-50.0, 0.0, 0.0), (0.0, 35 / 255, -30 / 255), (33.0, -0.2, 0.1), (170.0, 0.6, -0.5)]:
        got = AO.hsv_shift(x, dh, ds, dv)
        ref = np.empty_like(x)
        for idx in np.ndindex(x.shape[1:]):
            h, s, v = colorsys.rgb_to_hsv(*x[(slice(None),) + idx])
            ref[(slice(None),) + idx] = colorsys.hsv_to_rgb((h + dh / 360.0) % 1.0, min(max(s + ds, 0.0), 1.0), min(max(v + dv, 0.0), 1.0))
        assert np.abs(got - ref).max() <= 1e-12, (dh, ds, dv, np.abs(got - ref).max())
        assert np.abs(got - x).max() > 0.05


def test_jitter_identity_full_turn_and_stages():
    r = np.random.default_rng(1)
    x = r.random((3, 16, 16))
    assert np.array_equal(AO.jitter(x, 1.0, 1.0, 1.0, 0.0, 0.4), x)
    assert np.abs(AO.jitter(x, 1.0, 1.0, 1.0, 1.0, 0.0) - x).max() <= 1e-12
    assert np.abs(AO.jitter(x, 1.0, 1.0, 1.0, -1.0, 0.0) - x).max() <= 1e-12
    # a third of a turn about the grey axis is the cyclic channel permutation r -> g -> b
    assert np.abs(AO.jitter(x, 1.0, 1.0, 1.0, 1 / 3, 0.0) - x[[2, 0, 1]]).max() <= 1e-12
    assert np.allclose(AO.jitter(x, 1.4, 1.0, 1.0, 0.0, 0.0), np.minimum(x * 1.4, 1), rtol=0, atol=1e-15)
    assert np.allclose(AO.jitter(x, 1.0, 0.6, 1.0, 0.0, 0.37), (x - 0.37) * 0.6 + 0.37, rtol=0, atol=1e-15)
    g = 0.299 * x[0] + 0.587 * x[1] + 0.114 * x[2]
    assert np.allclose(AO.jitter(x, 1.0, 1.0, 0.0, 0.0, 0.0), np.stack([g, g, g]), rtol=0, atol=1e-15)
    # the order is brightness, contrast, saturation, hue, with a clip after each
    y = np.clip(x * 1.4, 0, 1)
    y = np.clip((y - 0.37) * 1.6 + 0.37, 0, 1)
    gy = 0.299 * y[0] + 0.587 * y[1] + 0.114 * y[2]
    y = np.clip((y - gy) * 1.25 + gy, 0, 1)
    y = AO.jitter(y, 1.0, 1.0, 1.0, 0.17, 0.0)
    assert np.abs(AO.jitter(x, 1.4, 1.6, 1.25, 0.17, 0.37) - y).max() <= 1e-15
    assert np.abs(AO.jitter(AO.jitter(x, 1.0, 1.0, 1.0, 0.17, 0.0), 1.0, 1.0, 1.25, 0.0, 0.0) - AO.jitter(x, 1.0, 1.0, 1.25, 0.17, 0.0)).max() > 1e-3


def test_sepia_and_posterize():
    x = np.random.default_rng(2).random((3, 8, 8))
    s = AO.sepia(x)
    assert np.allclose(s[1], np.clip(0.349 * x[0] + 0.686 * x[1] + 0.168 * x[2], 0, 1), rtol=0, atol=1e-15)
    v = np.array([[[0.0, 7 / 255, 7.6 / 255, 8 / 255, 200.4 / 255, 1.0]]])
    assert np.array_equal(AO.posterize(v, 5) * 255, [[[0, 0, 8, 8, 200, 248]]])
    assert np.array_equal(AO.posterize(v, 8) * 255, [[[0, 7, 8, 8, 200, 255]]])
