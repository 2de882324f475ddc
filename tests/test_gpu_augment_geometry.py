"""GPU: s3od_augment_sample (augment_sample_kernel, data_ops.hip) against the float64 restatement
oracle/augment_oracle.py augment_sample, with AugParams filled by hand: every warp is a forward matrix
built here in float64 and inverted here, so no case depends on GpuAugment's draws.  Outputs are
pre-filled with NaN.

Image: per pixel |kernel - reference| <= AO.remap_bound = 1e-5 + G * eps (G: range of the reference
canvas over the 4x4 neighbourhood of the sample point, zero border included; eps = 16 * 2^-24 *
max(S, |cx|, |cy|), sixteen float32 roundings of a coordinate of that size).  At S = 96 that is <= ~1e-4.
Mask: exactly the reference, except where the float64 reference is within 1e-3 of a rounding boundary of
floor(c + 0.5); that share is asserted <= 2 % (the warps are chosen so the reference alone stays below).
Mask sources resize by a ratio that is exact in float32, so the source index has no float32 / float64
ambiguity of its own.
Non-raw tail (jitter, mult, hashed Gaussian, clip, Normalize): 1e-5 + the image bound for the
deterministic members, 1e-4 for the Gaussian member (float32 logf / cosf of Box-Muller, the figure of the
ISONoise test), as an absolute maximum over all pixels.

Every test prints its worst |err| / bound and the excluded mask share (pytest -s).  Measured on an MI355X:
worst |err| / bound (excluded mask share) at S = 96: rotate 0.119 (0.35 %), crop 0.086 (0.00 %), rotate_crop_flip
0.113 (0.35 %), perspective 0.136 (0.38 %), kdist_pos 0.123 (0.17 %), kdist_neg 0.106 (0.17 %), grid_rotate
0.101 (0.33 %), elastic_crop 0.115 (0.35 %), shift_third 0.035 (0.00 %), shrink_four_edges 0.100 (0.00 %); at
S = 264: rotate_crop_flip 0.071 (0.40 %), perspective 0.141 (0.40 %), kdist_pos 0.090 (0.33 %), grid_rotate 0.090
(0.38 %); no mask pixel differed outside the excluded ones.  Tail: brightness 0.139, contrast 0.060, saturation
0.123, hue 0.097, jitter_all 0.099, mult 0.092, gauss 0.082, everything 0.077 (max |err| <= 1.2e-5 throughout).
"""
import ctypes
import math

import numpy as np
import pytest
import torch

from oracle import augment_oracle as AO

pytestmark = pytest.mark.gpu
MEAN = np.array([0.485, 0.456, 0.406])[:, None, None]
STD = np.array([0.229, 0.224, 0.225])[:, None, None]
IMG_SOURCES = [(97, 160), (300, 200), (36, 48)]                 # landscape, portrait, upscaling; pad rows and columns
MASK_SOURCES = [(108, 144), (144, 108), (36, 48), (72, 96)]     # resize ratio exact in float32 at S = 96
BIG_SOURCES = [(198, 264), (99, 132)]                           # ratio 1 and 1/2 at S = 264 (two block columns)


def _T(tx, ty):
    return np.array([[1, 0, tx], [0, 1, ty], [0, 0, 1]], np.float64)


def _about_centre(L, S):
    return _T(S / 2, S / 2) @ L @ _T(-S / 2, -S / 2)


def _rot(deg, S):
    th = math.radians(deg)
    return _about_centre(np.array([[math.cos(th), math.sin(th), 0], [-math.sin(th), math.cos(th), 0], [0, 0, 1]]), S)


def _crop(S):
    """RandomResizedCrop-like: the window at (5, 2) of size (83, 91) * S / 96 stretched to the output."""
    k = S / 96
    return np.diag([96 / 83, 96 / 91, 1.0]) @ _T(-5.0 * k, -2.0 * k)


def _hflip(S):
    return _about_centre(np.diag([-1.0, 1.0, 1.0]), S)


_sources = {}


def _source(h, w):
    if (h, w) not in _sources:
        r = np.random.default_rng(h * 1000 + w)
        img = r.integers(0, 256, (h, w, 3), dtype=np.uint8)
        msk = (r.random((h, w)) > 0.5).astype(np.uint8) * 255
        _sources[(h, w)] = (img, msk, torch.from_numpy(img).cuda(), torch.from_numpy(msk).cuda())
    return _sources[(h, w)]


def _params(h0, w0, S, fwd, persp=(0.0, 0.0), kdist=0.0):
    """AugParams of the forward map `fwd` (canvas -> output, pixel-centre coordinates), inverted here;
    persp: the denominator row applied to the output pixel before the inverse (Perspective)."""
    from s3od_amd.data import AugParams
    p = AugParams.identity(h0, w0, S)
    Tot = np.linalg.inv(fwd) @ np.array([[1, 0, 0], [0, 1, 0], [persp[0], persp[1], 1.0]])
    Tot /= Tot[2, 2]
    for i, v in enumerate(list(Tot[0]) + list(Tot[1])):
        p.A[i] = float(v)
    p.persp[0], p.persp[1] = float(Tot[2, 0]), float(Tot[2, 1])
    p.kdist = kdist
    p.raw = 1
    return p


def _grid(S):
    from s3od_amd.data import grid_distortion_maps
    r = np.random.default_rng(11)
    gx, gy = grid_distortion_maps(S, 1 + r.uniform(-0.3, 0.3, 7), 1 + r.uniform(-0.3, 0.3, 7), 6)
    return np.concatenate([gx, gy]).astype(np.float32)


_fields = {}


def _elastic(S):
    """ElasticTransform displacement (alpha 3, as test_gpu_augment.test_elastic_transform) from the device
    generator, which has its own parity test; the float32 field is the input of both sides here."""
    from s3od_amd._lib import lib, stream
    from s3od_amd.data import elastic_params
    if S not in _fields:
        e = elastic_params(777, alpha=3.0)
        tmp = torch.empty(2, S, S, device="cuda"); fld = torch.empty(2, S, S, device="cuda")
        lib()("s3od_elastic_field", ctypes.addressof(e), S, tmp, fld, stream())
        torch.cuda.synchronize()
        _fields[S] = fld
    return _fields[S]


def _device(src, p, S, grid=None, elastic=None):
    """One launch with NaN pre-filled outputs -> ([3,S,S] in [0,1], [S,S]) as float64."""
    from s3od_amd._lib import lib, stream
    _, _, ti, tm = src
    keep = []
    if grid is not None:
        keep.append(torch.from_numpy(grid).cuda())
        p.grid = keep[-1].data_ptr()
    if elastic is not None:
        p.elastic = elastic.data_ptr()
    oi = torch.full((3, S, S), float("nan"), device="cuda"); om = torch.full((S, S), float("nan"), device="cuda")
    lib()("s3od_augment_sample", ti, tm, ctypes.addressof(p), S, oi, om, stream())
    torch.cuda.synchronize()
    del keep
    oi = oi.cpu().numpy().astype(np.float64)
    return (oi if p.raw else oi * STD + MEAN), om.cpu().numpy().astype(np.float64)


def _check(name, S, sources, img_sources, mask_sources, fwd, persp=(0.0, 0.0), kdist=0.0, grid=False, elastic=False,
           min_outside=0.0):
    g = _grid(S) if grid else None
    e = _elastic(S) if elastic else None
    eh = e.cpu().numpy() if elastic else None
    worst, worst_amb = 0.0, 0.0
    for hw in sources:
        src = _source(*hw)
        p = _params(*hw, S, fwd, persp, kdist)
        got_i, got_m = _device(src, p, S, g, e)
        ref_i, ref_m = AO.augment_sample(src[0], src[1], p, S, grid=g, elastic=eh)
        canvas, _ = AO.letterbox_canvas(src[0], None, p, S)
        cx, cy, outside = AO.warp_coords(p, S, g, eh)
        assert np.isfinite(got_i).all() and np.isfinite(got_m).all(), (name, hw)
        off = outside | (cx < -1) | (cy < -1) | (cx > S) | (cy > S)
        assert off.mean() >= min_outside, (name, off.mean())
        assert np.abs(ref_i - canvas).max() > 0.05                       # the warp moved the picture
        if hw in img_sources:
            ratio = (np.abs(got_i - ref_i) / AO.remap_bound(canvas, cx, cy, S)[None]).max()
            worst = max(worst, ratio)
            assert ratio <= 1.0, (name, hw, ratio)
        if hw in mask_sources:
            amb = AO.nearest_ambiguous(cx, cy)
            worst_amb = max(worst_amb, amb.mean())
            assert amb.mean() <= 0.02, (name, hw, amb.mean())
            bad = (got_m != ref_m) & ~amb
            assert not bad.any(), (name, hw, int(bad.sum()), np.argwhere(bad)[:5])
            assert 0.05 < ref_m.mean() < 0.9
    print(f"\n[{name} S={S}] worst |err|/bound {worst:.3f}, excluded mask share {100 * worst_amb:.2f} %")


def _warps(S):
    third = _T(S / 3 + 0.37, 0.29)                                        # a third of the output leaves the canvas
    shrink = _T(S / 3 + 0.137, 10.3 * S / 96) @ np.diag([0.613, 0.587, 1.0])  # all four canvas edges inside the output
    return {
        "rotate": dict(fwd=_rot(11.3, S)),
        "crop": dict(fwd=_crop(S)),
        "rotate_crop_flip": dict(fwd=_rot(11.3, S) @ _crop(S) @ _hflip(S)),
        "perspective": dict(fwd=_rot(-8.0, S), persp=(1.1e-3, -0.8e-3)),
        "kdist_pos": dict(fwd=np.eye(3), kdist=0.06),
        "kdist_neg": dict(fwd=np.eye(3), kdist=-0.06),
        "grid_rotate": dict(fwd=_rot(11.3, S), grid=True),
        "elastic_crop": dict(fwd=_crop(S), elastic=True),
        "shift_third": dict(fwd=third, min_outside=0.33),
        "shrink_four_edges": dict(fwd=shrink, min_outside=0.6),
    }


@pytest.mark.parametrize("name", sorted(_warps(96)))
def test_warp_matches_float64(name):
    S = 96
    srcs = IMG_SOURCES + [s for s in MASK_SOURCES if s not in IMG_SOURCES]
    _check(name, S, srcs, IMG_SOURCES, MASK_SOURCES, **_warps(S)[name])


@pytest.mark.parametrize("name", ["rotate_crop_flip", "perspective", "kdist_pos", "grid_rotate"])
def test_warp_matches_float64_second_block_column(name):
    """S = 264: the smallest S divisible by 8 whose rows need a second 256-thread block (blockIdx.x = 1)."""
    S = 264
    _check(name, S, BIG_SOURCES, BIG_SOURCES, BIG_SOURCES, **_warps(S)[name])


TAILS = {
    "brightness": dict(bright=1.4),
    "contrast": dict(contrast=0.6, gray_mean=0.37),
    "saturation": dict(sat=1.25),
    "hue": dict(hue=0.17),
    "jitter_all": dict(bright=1.4, contrast=0.6, gray_mean=0.37, sat=1.25, hue=0.17),
    "mult": dict(mult=(0.92, 1.0, 1.08)),
    "gauss": dict(gauss_std=0.44, seed=20240917),
    "everything": dict(bright=1.4, contrast=0.6, gray_mean=0.37, sat=1.25, hue=0.17, mult=(0.92, 1.0, 1.08),
                       gauss_std=0.44, seed=20240917),
}


@pytest.mark.parametrize("name", list(TAILS))
def test_non_raw_tail_matches_float64(name):
    """jitter -> mult -> hashed Gaussian -> clip -> Normalize after one fractional warp (rotation, crop, flip)."""
    S, hw = 96, (97, 160)
    src = _source(*hw)
    p = _params(*hw, S, _rot(11.3, S) @ _crop(S) @ _hflip(S))
    p.raw = 0
    kw = dict(TAILS[name])
    mult = kw.pop("mult", (1.0, 1.0, 1.0))
    for i in range(3):
        p.mult[i] = mult[i]
    for k, v in kw.items():
        setattr(p, k, v)
    got, _ = _device(src, p, S)
    ref, _ = AO.augment_sample(src[0], src[1], p, S)
    assert np.isfinite(got).all()
    p.raw = 1
    plain, _ = AO.augment_sample(src[0], src[1], p, S)
    assert np.abs(ref - plain).max() > 0.02                               # the member did something
    canvas, _ = AO.letterbox_canvas(src[0], None, p, S)
    cx, cy, _ = AO.warp_coords(p, S)
    bound = 1e-4 if "gauss_std" in kw else 1e-5 + AO.remap_bound(canvas, cx, cy, S)[None]
    ratio = (np.abs(got - ref) / bound).max()
    print(f"\n[tail {name}] worst |err|/bound {ratio:.3f}, max |err| {np.abs(got - ref).max():.2e}")
    assert ratio <= 1.0, (name, ratio)
