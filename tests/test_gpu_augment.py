"""GPU: the training-augmentation members built on device (§8(f)3; synth_sod/.../transforms.py:12-224)
against oracle/augment_oracle.py, the numpy restatement of albumentations 2.0.8 / OpenCV 4.12's published
algorithms (neither library is installed: parity with them is unpinned; these tests pin the kernels to
the restated algorithms).  Each member runs alone through the C ABI on a seeded [0,1] image:

* CLAHE (8x8 tiles, clip 2.5): an 8-bit L value on a rounding tie of the LUT interpolation may flip by one
  step (float32 on device, float64 here): <= 1.5 % of pixels beyond 1e-3, max <= 0.02, mean <= 3e-4;
* ISONoise: a Poisson draw on the inversion boundary may flip: <= 0.2 % of pixels beyond 1e-4;
* ImageCompression at quality 30 / 55 / 75 and a canvas that is not a multiple of the 16-pixel MCU: a
  coefficient whose quantisation rounds the other way (float32 DCT on device, float64 here) moves its
  8x8 block, so <= 3 % of pixels may be more than one 8-bit step away, mean |d| <= 1e-3;
* ZoomBlur (+ Sharpen composed), Downscale + RandomBrightnessContrast, RandomShadow, RandomSnow,
  RandomRain, GridDistortion, ElasticTransform: <= 1e-4 (shadow / snow: <= 0.1 % of pixels on a
  polygon edge / threshold may differ);
* the regular chain's Sharpen -> ISONoise order;
* HueSaturationValue, ColorJitter through the colour group, GaussNoise / MultiplicativeNoise, ToSepia, the
  colour space -> Posterize -> RandomSnow order, non-symmetric filters up to 15x15, Downscale + filter and the
  regular chain's filter -> colour -> noise order, per pixel against float64 (second half of this file)."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import augment_oracle as AO

pytestmark = pytest.mark.gpu
MEAN = np.array([0.485, 0.456, 0.406])[:, None, None]
STD = np.array([0.229, 0.224, 0.225])[:, None, None]


def _img(S, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.rand(3, S // 4, S // 4, device="cuda", generator=g)[None]
    x = torch.nn.functional.interpolate(x, size=(S, S), mode="bilinear", align_corners=False)[0]
    return (x + 0.15 * torch.rand(3, S, S, device="cuda", generator=g)).clamp(0, 1).contiguous()


def _run(raw, q, kw=None, ws=True):
    from s3od_amd._lib import lib, stream
    from s3od_amd.data import augment_ws_floats
    S = raw.shape[-1]
    keep = None
    if ws:
        keep = torch.empty(augment_ws_floats(S), device="cuda")
        q.ws = keep.data_ptr()
    out = torch.empty(3, S, S, device="cuda")
    src = raw.clone()
    lib()("s3od_augment_synthetic", src, ctypes.addressof(q), kw, S, out, stream())
    torch.cuda.synchronize()
    return out.cpu().numpy().astype(np.float64) * STD + MEAN


def _frac(a, b, tol):
    return float((np.abs(a - b) > tol).mean())


@pytest.mark.parametrize("S", [64, 96])
def test_clahe(S):
    from s3od_amd.data import SynthParams
    x = _img(S, 1)
    q = SynthParams.identity()
    q.clahe_clip = 2.5
    got = _run(x, q)
    ref = AO.clahe(x.cpu().numpy().astype(np.float64), 2.5)
    # float32 Lab round trip on device (~1e-4 near black) vs float64 here; an 8-bit L value whose LUT
    # interpolation lands on a rounding tie (common with 12-pixel tiles) may flip by one step (<= 2.5/255 in RGB)
    d = np.abs(got - ref)
    assert _frac(got, ref, 1e-3) <= 1.5e-2 and d.max() < 0.02 and d.mean() < 3e-4, (_frac(got, ref, 1e-3), d.max(), d.mean())
    assert np.abs(got - x.cpu().numpy()).mean() > 1e-3          # the member did something


def test_iso_noise():
    from s3od_amd.data import SynthParams
    S = 96
    x = _img(S, 2)
    q = SynthParams.identity()
    q.iso_intensity, q.iso_color_shift, q.seed = 0.3, 0.03, 1234
    got = _run(x, q)
    ref = AO.iso_noise(x.cpu().numpy().astype(np.float64), 0.3, 0.03, 1234)
    f = _frac(got, ref, 1e-4)
    assert f <= 2e-3, f
    assert np.abs(got - x.cpu().numpy()).mean() > 1e-3


@pytest.mark.parametrize("S,quality", [(64, 30), (72, 75), (96, 55)])
def test_jpeg(S, quality):
    from s3od_amd.data import SynthParams
    x = _img(S, 3)
    q = SynthParams.identity()
    q.jpeg_quality = quality
    got = _run(x, q)
    ref = AO.jpeg(x.cpu().numpy().astype(np.float64), quality)
    f = _frac(got, ref, 1.5 / 255)
    assert f <= 3e-2 and np.abs(got - ref).mean() <= 1e-3, (f, np.abs(got - ref).mean())
    assert np.abs(got - x.cpu().numpy()).mean() > 1e-3


@pytest.mark.parametrize("with_sharpen", [False, True])
def test_zoom_blur(with_sharpen):
    from s3od_amd.data import SynthParams, _sharpen_kernel
    S = 96
    x = _img(S, 4)
    q = SynthParams.identity()
    zs = [1.0, 1.01, 1.02]
    q.zoom_n = 3
    for i, z in enumerate(zs):
        q.zoom[i] = z
    kw, ker = None, None
    if with_sharpen:
        ker = _sharpen_kernel(0.4, 0.8)
        q.ksize = 3
        kw = torch.tensor(ker.reshape(-1), dtype=torch.float32, device="cuda")
    got = _run(x, q, kw, ws=False)
    v = AO.zoom_blur(x.cpu().numpy().astype(np.float64), np.float32(zs))
    ref = AO.filter2d(v, ker) if with_sharpen else np.clip(v, 0, 1)
    assert np.abs(got - ref).max() <= 1e-4


def test_downscale_brightness_contrast():
    from s3od_amd.data import SynthParams
    S = 96
    x = _img(S, 5)
    q = SynthParams.identity()
    q.down, q.rbc_alpha, q.rbc_beta = 0.55, 1.3, -0.1
    got = _run(x, q, ws=False)
    ref = AO.lit(x.cpu().numpy().astype(np.float64), down=0.55, rbc=(1.3, -0.1))
    assert np.abs(got - ref).max() <= 1e-4


def test_random_shadow_pentagons():
    from s3od_amd.data import SynthParams
    S = 96
    x = _img(S, 6)
    r = np.random.default_rng(0)
    q = SynthParams.identity()
    polys = [r.integers(0, S, 10).astype(float) for _ in range(3)]
    q.n_shadow, q.shadow_dim = 3, 0.5
    for t, pv in enumerate(polys):
        for i, v in enumerate(pv):
            q.shadow[t][i] = float(v)
    got = _run(x, q, ws=False)
    ref = AO.lit(x.cpu().numpy().astype(np.float64), shadows=polys, shadow_dim=0.5)
    assert _frac(got, ref, 1e-4) <= 1e-3
    assert np.abs(got - x.cpu().numpy()).max() > 0.05


def test_snow_bleach():
    from s3od_amd.data import SynthParams
    S = 64
    x = _img(S, 7)
    q = SynthParams.identity()
    q.snow_point, q.snow_coeff = 0.2, 2.5
    got = _run(x, q, ws=False)
    ref = AO.snow_bleach(x.cpu().numpy().astype(np.float64), 0.2, 2.5)
    assert _frac(got, ref, 1e-4) <= 1e-3


@pytest.mark.parametrize("slant", [-7, 0, 9])
def test_rain(slant):
    from s3od_amd.data import SynthParams
    S = 96
    x = _img(S, 8)
    r = np.random.default_rng(slant + 20)
    n = S * S // 600
    lo, hi = (-slant, S) if slant < 0 else (0, S - slant)
    drops = np.stack([r.integers(lo, hi, n), r.integers(0, S - 20, n)], 1).astype(np.int32)
    dr = torch.from_numpy(drops).cuda()
    q = SynthParams.identity()
    q.rain_n, q.rain_slant, q.rain_len, q.rain_blur, q.rain_color, q.rain_bright = n, slant, 20, 7, 200 / 255, 0.7
    q.rain_drops = dr.data_ptr()
    got = _run(x, q)
    ref = AO.rain(x.cpu().numpy().astype(np.float64), drops, slant)
    assert np.abs(got - ref).max() <= 1e-4


def _geometry(S, p_mod):
    """test-mode letterbox of a seeded uint8 image, then the distortion member through the geometry pass
    (raw [0,1] output) vs cv2.remap of the undistorted canvas."""
    from s3od_amd._lib import lib, stream
    from s3od_amd.data import GpuAugment
    r = np.random.default_rng(3)
    img = r.integers(0, 256, (S - 10, S, 3), dtype=np.uint8)
    msk = (r.random((S - 10, S)) > 0.5).astype(np.uint8) * 255
    aug = GpuAugment(S, mode="test")
    p = aug.draw(S - 10, S).geometry
    p.raw = 1
    ti, tm = torch.from_numpy(img).cuda(), torch.from_numpy(msk).cuda()
    base = torch.empty(3, S, S, device="cuda"); bm = torch.empty(S, S, device="cuda")
    lib()("s3od_augment_sample", ti, tm, ctypes.addressof(p), S, base, bm, stream())
    keep = p_mod(p)
    out = torch.empty(3, S, S, device="cuda"); om = torch.empty(S, S, device="cuda")
    lib()("s3od_augment_sample", ti, tm, ctypes.addressof(p), S, out, om, stream())
    torch.cuda.synchronize()
    del keep
    return base.cpu().numpy().astype(np.float64), out.cpu().numpy().astype(np.float64), om.cpu().numpy()


def test_grid_distortion():
    from s3od_amd.data import grid_distortion_maps
    S = 96
    r = np.random.default_rng(11)
    gx, gy = grid_distortion_maps(S, 1 + r.uniform(-0.3, 0.3, 7), 1 + r.uniform(-0.3, 0.3, 7), 6)
    assert abs(float(gx[-1]) - S) < 1e-3 and gx[0] == 0 and np.all(np.diff(gx) >= 0)

    def mod(p):
        g = torch.from_numpy(np.concatenate([gx, gy]).astype(np.float32)).cuda()
        p.grid = g.data_ptr()
        return g
    base, out, om = _geometry(S, mod)
    ref = AO.remap_bilinear(base, gx[None, :].astype(np.float64) + 0 * gy[:, None], gy[:, None].astype(np.float64) + 0 * gx[None, :])
    assert np.abs(out - ref).max() <= 1e-4
    assert np.abs(out - base).max() > 0.05


def test_elastic_transform():
    from s3od_amd._lib import lib, stream
    from s3od_amd.data import elastic_params
    S = 96
    e = elastic_params(777, alpha=3.0)                 # alpha raised so the warp is visible in the check
    tmp = torch.empty(2, S, S, device="cuda"); fld = torch.empty(2, S, S, device="cuda")
    lib()("s3od_elastic_field", ctypes.addressof(e), S, tmp, fld, stream())
    torch.cuda.synchronize()
    dx, dy = AO.elastic_field(S, 777, alpha=3.0)
    f = fld.cpu().numpy()
    assert np.abs(f[0] - dx).max() <= 1e-5 * max(1.0, np.abs(dx).max()) and np.abs(f[1] - dy).max() <= 1e-5 * max(1.0, np.abs(dy).max())

    def mod(p):
        p.elastic = fld.data_ptr()
        return fld
    base, out, om = _geometry(S, mod)
    yy, xx = np.mgrid[0:S, 0:S].astype(np.float64)
    ref = AO.remap_bilinear(base, xx + f[0], yy + f[1])
    assert np.abs(out - ref).max() <= 1e-4


def test_regular_chain_sharpen_then_iso():
    """transforms.py:44-62 order: Sharpen (colour OneOf) before ISONoise (noise OneOf), then Normalize."""
    from s3od_amd.data import SynthParams, _sharpen_kernel
    S = 64
    x = _img(S, 9)
    ker = _sharpen_kernel(0.35, 0.7)
    q = SynthParams.identity()
    q.order, q.ksize = 1, 3
    q.iso_intensity, q.iso_color_shift, q.seed = 0.4, 0.04, 99
    kw = torch.tensor(ker.reshape(-1), dtype=torch.float32, device="cuda")
    got = _run(x, q, kw)
    ref = AO.iso_noise(AO.filter2d(x.cpu().numpy().astype(np.float64), ker), 0.4, 0.04, 99)
    assert _frac(got, ref, 1e-4) <= 2e-3


@pytest.mark.parametrize("mode", ["regular", "synthetic"])
def test_modes_draw_every_member(mode, monkeypatch):
    """Every member of the mode is reachable through GpuAugment's draws: run enough samples that each
    OneOf group draws each member, check the outputs are finite, in range and reproducible."""
    from s3od_amd import data as D
    seen = set()
    real_one_of = D._one_of

    def spy(r, p, weights):
        g = real_one_of(r, p, weights)
        seen.add((len(weights), tuple(weights), g))
        return g
    monkeypatch.setattr(D, "_one_of", spy)
    r = np.random.default_rng(1)
    smps = [{"image": r.integers(0, 256, (70 + i % 9, 64, 3), dtype=np.uint8),
             "mask": (r.random((70 + i % 9, 64)) > 0.5).astype(np.uint8) * 255} for i in range(16)]
    a = D.GpuAugment(64, mode=mode, seed=3)
    outs = [a(smps[i:i + 4]) for i in range(0, 16, 4) for _ in range(12)]
    torch.cuda.synchronize()
    for o in outs:
        assert torch.isfinite(o["images"]).all()
        lo = torch.tensor(((0 - MEAN) / STD).ravel(), dtype=torch.float32).view(1, 3, 1, 1).cuda()
        hi = torch.tensor(((1 - MEAN) / STD).ravel(), dtype=torch.float32).view(1, 3, 1, 1).cuda()
        assert (o["images"] >= lo - 1e-4).all() and (o["images"] <= hi + 1e-4).all()
    groups = {}
    for n, w, g in seen:
        groups.setdefault((n, w), set()).add(g)
    for (n, w), gs in groups.items():
        assert set(range(n)) <= gs, (w, gs)


# ------------------------------------------------------------------ photometric members against float64, per pixel
# Each test prints its worst |err| / bound and the share of pixels it excludes (pytest -s).  Measured on an MI355X:
# worst |err| / bound: hsv_shift 0.007 .. 0.010 (no pixel excluded); colour_group brightness 0.006, contrast 0.004,
# saturation 0.007, hue 0.015, all 0.016; noise gauss 0.062, mult 0.001, gauss_mult 0.062, jitter_gauss_mult 0.063;
# sepia 0.010; sepia -> posterize -> snow 0.015 (0.52 % excluded); filters motion7 0.011 (S = 264: 0.012), emboss3
# 0.010, disk6_emboss15 0.022; downscale -> gaussian 0.021; order 1 jitter_iso / jitter_gauss_sharpen: no pixel
# beyond 1e-4 (max |err| 5.8e-7 / 9.2e-7); jitter + gauss at S = 264 0.122.
JITTERS = {
    "brightness": dict(bright=1.4),
    "contrast": dict(contrast=0.6, gray_mean=0.37),
    "saturation": dict(sat=1.25),
    "hue": dict(hue=0.17),
    "all": dict(bright=1.4, contrast=0.6, gray_mean=0.37, sat=1.25, hue=0.17),
}
MULT = (0.92, 1.0, 1.08)


def _q(**kw):
    from s3od_amd.data import SynthParams
    q = SynthParams.identity()
    mult = kw.pop("mult", None)
    if mult is not None:
        for i in range(3):
            q.mult[i] = mult[i]
    for k, v in kw.items():
        setattr(q, k, v)
    return q


def _np(x):
    return x.cpu().numpy().astype(np.float64)


def _report(name, got, ref, bound, excluded=None, cap=0.02):
    """max |got - ref| / bound over the pixels that are not excluded; the excluded share is capped."""
    share = 0.0
    err = np.abs(got - ref) / bound
    if excluded is not None:
        share = float(excluded.mean())
        assert share <= cap, (name, share)
        err = np.where(excluded[None], 0.0, err)
    print(f"\n[{name}] worst |err|/bound {err.max():.3f}, excluded {100 * share:.3f} %")
    assert err.max() <= 1.0, (name, err.max())


def _filter_bound(ker):
    """float32 accumulation of n_taps products of values in [0, 1]."""
    return 1e-5 + ker.size * 2.0 ** -24 * np.abs(ker).sum()


@pytest.mark.parametrize("shift", [(50.0, 0.0, 0.0), (-50.0, 0.0, 0.0), (0.0, 35 / 255, -30 / 255), (50.0, 35 / 255, -30 / 255)])
def test_hsv_shift(shift):
    """HueSaturationValue: hue is ill-conditioned where max - min over RGB is tiny, so those reference pixels
    (below 1e-3) are left out, at most 2 % of them."""
    S = 96
    x = _img(S, 10)
    q = _q(hsv_h=shift[0], hsv_s=shift[1], hsv_v=shift[2])
    got = _run(x, q, ws=False)
    xr = _np(x)
    ref = AO.hsv_shift(xr, *shift)
    assert np.abs(ref - xr).max() > 0.05
    _report(f"hsv_shift {shift}", got, ref, 1e-4, excluded=(xr.max(0) - xr.min(0)) < 1e-3)


@pytest.mark.parametrize("name", list(JITTERS))
def test_colour_jitter_through_colour_group(name):
    S = 96
    x = _img(S, 11)
    q = _q(**JITTERS[name])
    got = _run(x, q, ws=False)
    xr = _np(x)
    ref = AO.jitter(xr, q.bright, q.contrast, q.sat, q.hue, q.gray_mean)
    assert np.abs(ref - xr).max() > 0.02
    _report(f"colour_group {name}", got, ref, 1e-5)


@pytest.mark.parametrize("name", ["gauss", "mult", "gauss_mult", "jitter_gauss_mult"])
def test_gauss_and_mult_noise(name):
    """GaussNoise / MultiplicativeNoise against gauss_mult_noise; with ColorJitter: colour -> mult -> noise -> clip."""
    S = 96
    x = _img(S, 12)
    kw = dict(seed=4321)
    if "gauss" in name:
        kw["gauss_std"] = 0.6
    if "mult" in name:
        kw["mult"] = MULT
    if "jitter" in name:
        kw.update(JITTERS["all"])
    q = _q(**kw)
    got = _run(x, q, ws=False)
    xr = _np(x)
    ref = AO.gauss_mult_noise(AO.jitter(xr, q.bright, q.contrast, q.sat, q.hue, q.gray_mean), q.gauss_std, MULT if "mult" in name else (1, 1, 1), 4321)
    assert np.abs(ref - xr).max() > 0.05
    if name == "jitter_gauss_mult":       # the order is visible: the noise is not multiplied, the jitter sees no noise
        wrong = AO.jitter(AO.gauss_mult_noise(xr, q.gauss_std, MULT, 4321), q.bright, q.contrast, q.sat, q.hue, q.gray_mean)
        assert np.abs(ref - wrong).mean() > 1e-2
    _report(f"noise {name}", got, ref, 1e-4)


def test_sepia():
    S = 96
    x = _img(S, 13)
    got = _run(x, _q(color_op=1), ws=False)
    ref = AO.sepia(_np(x))
    assert np.abs(ref[0] - ref[2]).max() > 0.05
    _report("sepia", got, ref, 1e-5)


def test_sepia_then_posterize_then_snow():
    """The filter pass's order colour space -> Posterize -> RandomSnow.  Posterize and the snow threshold are
    discontinuous: a pixel is left out when a reference channel's v * 255 + 0.5 (after sepia) is within 1e-3
    of an integer, or its lightness (after posterize) within 1e-4 of the snow threshold; at most 2 %.  Posterize
    snaps to k / 255, so the sepia bound 1e-5 holds for the whole composition."""
    S = 96
    x = _img(S, 14)
    snow_point = 0.25
    got = _run(x, _q(color_op=1, post_bits=5, snow_point=snow_point, snow_coeff=2.5), ws=False)
    xr = _np(x)
    sep = AO.sepia(xr)
    post = AO.posterize(sep, 5)
    ref = AO.snow_bleach(post, snow_point, 2.5)
    t = sep * 255.0 + 0.5
    near_int = (np.abs(t - np.rint(t)) < 1e-3).any(0)
    _, l, _ = AO.rgb2hls(post)
    near_thr = np.abs(l - (snow_point * 0.5 + 1.0 / 3.0)) < 1e-4
    for other in (AO.posterize(AO.snow_bleach(sep, snow_point, 2.5), 5), AO.snow_bleach(AO.sepia(AO.posterize(xr, 5)), snow_point, 2.5)):
        assert (np.abs(ref - other).max(0) > 1e-3).mean() > 0.05           # another order is another picture
    assert 0.05 < (l < snow_point * 0.5 + 1.0 / 3.0).mean() < 0.95         # both sides of the threshold
    _report("sepia -> posterize -> snow", got, ref, 1e-5, excluded=near_int | near_thr)


def _filter_kernels():
    from s3od_amd.data import _disk_kernel, _emboss_kernel, _conv_full
    k, th, c = 7, 0.6, 3.0
    motion = np.zeros((k, k))
    for t in np.linspace(-c, c, 4 * k):
        motion[int(round(c + t * np.sin(th))), int(round(c + t * np.cos(th)))] = 1.0
    motion /= motion.sum()
    emboss = _emboss_kernel(0.35, 0.4)
    return {"motion7": motion, "emboss3": emboss, "disk6_emboss15": _conv_full(_disk_kernel(6, 0.2), emboss)}


@pytest.mark.parametrize("name,S", [("motion7", 96), ("emboss3", 96), ("disk6_emboss15", 96), ("motion7", 264)])
def test_filter_orientation_and_border(name, S):
    """Non-symmetric kernels on a non-constant image against filter2d (correlation, BORDER_REFLECT_101): a
    transposed or flipped read of the taps fails; radius 7 reflects on all four borders.  S = 264: second
    block column."""
    ker = _filter_kernels()[name]
    assert ker.shape[0] == {"motion7": 7, "emboss3": 3, "disk6_emboss15": 15}[name]
    variants = [v for v in (ker.T, ker[::-1], ker[:, ::-1], ker[::-1, ::-1]) if np.abs(ker - v).max() > 1e-3]
    # a centred line is its own 180-degree turn and Emboss its own transpose: motion7 sees a transposed read and
    # a mirrored one, the emboss kernels a mirrored and a turned one
    assert len(variants) >= 3 and (name != "motion7" or np.abs(ker - ker.T).max() > 1e-3)
    x = _img(S, 15)
    kw = torch.tensor(ker.reshape(-1), dtype=torch.float32, device="cuda")
    got = _run(x, _q(ksize=ker.shape[0]), kw, ws=False)
    xr = _np(x)
    ref = AO.filter2d(xr, kw.cpu().numpy().astype(np.float64).reshape(ker.shape))
    for other in variants:
        assert np.abs(ref - AO.filter2d(xr, other)).max() > 1e-3 > 10 * _filter_bound(ker)
    _report(f"filter {name} S={S}", got, ref, _filter_bound(ker))


def test_downscale_then_gaussian_filter():
    from s3od_amd.data import _gauss_kernel
    S = 96
    x = _img(S, 16)
    ker = _gauss_kernel(5)
    kw = torch.tensor(ker.reshape(-1), dtype=torch.float32, device="cuda")
    got = _run(x, _q(down=0.55, ksize=5), kw, ws=False)
    xr = _np(x)
    ref = AO.filter2d(AO.lit(xr, down=0.55), kw.cpu().numpy().astype(np.float64).reshape(5, 5))
    assert np.abs(ref - AO.filter2d(xr, ker)).max() > 0.05
    _report("downscale -> gaussian 5x5", got, ref, _filter_bound(ker))


@pytest.mark.parametrize("name", ["jitter_iso", "jitter_gauss_sharpen"])
def test_regular_chain_colour_and_noise_order(name):
    """order 1: the filter first, then ColorJitter, then the noise; ISONoise takes its lightness statistics
    after the colour group.  The ISONoise test's criterion: <= 0.2 % of pixels beyond 1e-4 (a Poisson draw
    on an inversion boundary)."""
    from s3od_amd.data import _sharpen_kernel
    S = 96
    x = _img(S, 17)
    xr = _np(x)
    jit = JITTERS["all"]
    if name == "jitter_iso":
        q = _q(order=1, iso_intensity=0.4, iso_color_shift=0.04, seed=77, **jit)
        got = _run(x, q)
        col = AO.jitter(xr, q.bright, q.contrast, q.sat, q.hue, q.gray_mean)
        ref = AO.iso_noise(col, 0.4, 0.04, 77)
        # statistics of the input instead of the colour group's output: another Poisson rate, another picture
        h, l, s = AO.rgb2hls(col)
        sd_in = float(np.std(AO.rgb2hls(xr)[1]))
        assert abs(sd_in - float(np.std(l))) * 0.4 * 255 > 0.5
    else:
        ker = _sharpen_kernel(0.35, 0.7)
        kw = torch.tensor(ker.reshape(-1), dtype=torch.float32, device="cuda")
        q = _q(order=1, ksize=3, gauss_std=0.3, seed=78, **jit)
        got = _run(x, q, kw)
        jn = lambda v: AO.gauss_mult_noise(AO.jitter(v, q.bright, q.contrast, q.sat, q.hue, q.gray_mean), q.gauss_std, (1, 1, 1), 78)
        ref = jn(AO.filter2d(xr, ker))
        assert (np.abs(ref - AO.filter2d(jn(xr), ker)) > 1e-2).mean() > 0.2          # the filter last is another picture
    f = _frac(got, ref, 1e-4)
    print(f"\n[order 1 {name}] share of pixels beyond 1e-4: {100 * f:.4f} %, max |err| {np.abs(got - ref).max():.2e}")
    assert f <= 2e-3, f


def test_jitter_gauss_second_block_column():
    S = 264
    x = _img(S, 18)
    q = _q(gauss_std=0.6, seed=99, **JITTERS["all"])
    got = _run(x, q, ws=False)
    xr = _np(x)
    ref = AO.gauss_mult_noise(AO.jitter(xr, q.bright, q.contrast, q.sat, q.hue, q.gray_mean), q.gauss_std, (1, 1, 1), 99)
    _report("jitter + gauss S=264", got, ref, 1e-4)
