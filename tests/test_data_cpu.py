"""MaskDataset file discovery and train/val split (synth_sod/.../dataset.py:34-106) on CPU."""
import math
import random

import numpy as np
import pytest
from PIL import Image

from s3od_amd.data import MaskDataset, letterbox


def _make(root, names, mask_ext=".png", skip_mask=()):
    (root / "images").mkdir()
    (root / "masks").mkdir()
    for n in names:
        Image.fromarray(np.full((6, 8, 3), 7, np.uint8)).save(root / "images" / n)
        stem = n.rsplit(".", 1)[0]
        if stem not in skip_mask:
            Image.fromarray(np.full((6, 8), 255, np.uint8)).save(root / "masks" / (stem + mask_ext))


def test_split_matches_reference_rule(tmp_path):
    names = [f"img_{i:03d}.jpg" for i in range(37)] + ["x.png", "notes.txt"]
    _make(tmp_path, [n for n in names if not n.endswith(".txt")], skip_mask=("img_005",))
    (tmp_path / "images" / "notes.txt").write_text("not an image")
    tr = MaskDataset(str(tmp_path), 64, split="train", val_split=0.2, seed=42)
    va = MaskDataset(str(tmp_path), 64, split="val", val_split=0.2, seed=42)
    # restated reference rule: valid = sorted(images with a mask); random.seed(seed); shuffle; val first
    valid = sorted(n for n in names if not n.endswith(".txt") and not n.startswith("img_005"))
    random.seed(42)
    random.shuffle(valid)
    nv = int(len(valid) * 0.2)
    assert va.files == valid[:nv] and tr.files == valid[nv:]
    item = tr[0]
    assert item["image"].shape == (6, 8, 3) and item["image"].dtype == np.uint8 and item["mask"].shape == (6, 8)
    sub = MaskDataset(str(tmp_path), 64, split="train", val_split=0.2, seed=42, debug_subset_fraction=0.5)
    assert sub.files == tr.files[:int(len(tr.files) * 0.5)]


def test_letterbox_geometry():
    assert letterbox(480, 640, 1024) == (768, 1024, 128, 0)
    assert letterbox(1024, 1024, 1024) == (1024, 1024, 0, 0)
    nh, nw, ph, pw = letterbox(300, 1000, 512)
    assert nw == 512 and nh == 154 and ph == (512 - 154) // 2 and pw == 0


def test_synthetic_params_host_logic():
    """Host half of mode="synthetic": every draw is inside the kernel's contract (odd filter <= 15,
    normalised blur taps, valid colour op / posterize / downscale), and the perspective branch gives
    a finite projective map with the same geometry as the mask (one AugParams drives both)."""
    from s3od_amd.data import GpuAugment
    aug = GpuAugment(128, mode="synthetic", device="cpu", seed=3)
    img = np.random.default_rng(0).integers(0, 256, (90, 140, 3), dtype=np.uint8)
    seen_k, seen_op, persp = set(), set(), 0
    seen = set()
    for _ in range(400):
        drawn = aug.draw(90, 140, img)
        q, kw, dr, p = drawn.chain, drawn.kernel, drawn.drops, drawn.geometry
        assert q.clahe_clip == 0 or 1.0 <= q.clahe_clip <= 4.0
        assert q.jpeg_quality == 0 or 30 <= q.jpeg_quality <= 80
        assert 0 <= q.zoom_n <= 3 and (q.zoom_n == 0 or (q.zoom[0] == 1.0 and all(1.0 <= q.zoom[i] < 1.03 for i in range(q.zoom_n))))
        assert q.snow_point == 0 or 0.1 <= q.snow_point <= 0.3
        assert (dr is None) == (q.rain_n == 0)
        if dr is not None:                                   # drops stay on the canvas (x + slant too)
            d = dr
            assert d.shape == (128 * 128 // 600, 2) and -10 < q.rain_slant < 10
            assert (d[:, 0] + min(q.rain_slant, 0) >= 0).all() and (d[:, 0] + max(q.rain_slant, 0) < 128).all()
            assert (d[:, 1] >= 0).all() and (d[:, 1] + 20 < 128).all()
        seen.update(k for k, on in (("clahe", q.clahe_clip > 0), ("iso", q.iso_intensity > 0), ("jpeg", q.jpeg_quality > 0),
                                    ("zoom", q.zoom_n > 0), ("snow", q.snow_point > 0), ("rain", q.rain_n > 0),
                                    ("shadow", q.n_shadow > 0)) if on)
        assert q.ksize % 2 == 1 and 1 <= q.ksize <= 15
        assert (kw is None) == (q.ksize == 1)
        if kw is not None:
            assert kw.size == q.ksize ** 2 and kw.dtype == np.float32 and np.isfinite(kw).all() and float(kw.sum()) > 0.3
        assert 0 <= q.color_op <= 3 and sorted(q.perm) == [0, 1, 2]
        assert q.post_bits in (5, 8) and 0.4 <= q.down <= 1.0 and 0 <= q.n_shadow <= 3
        assert 0.0 <= q.gray_mean <= 1.0
        seen_k.add(q.ksize); seen_op.add(q.color_op)
        assert p.raw == 1 and all(np.isfinite(list(p.A))) and np.isfinite(p.persp[0]) and np.isfinite(p.persp[1])
        persp += p.persp[0] != 0 or p.persp[1] != 0
    assert len(seen_k) >= 4 and len(seen_op) >= 2 and persp > 0
    assert seen == {"clahe", "iso", "jpeg", "zoom", "snow", "rain", "shadow"}, seen
    # reproducible from the seed
    a = GpuAugment(128, mode="synthetic", device="cpu", seed=11)
    b = GpuAugment(128, mode="synthetic", device="cpu", seed=11)
    for _ in range(20):
        da, db = a.draw(90, 140, img), b.draw(90, 140, img)
        assert bytes(da.chain) == bytes(db.chain) and bytes(da.geometry) == bytes(db.geometry)


def test_synthetic_mode_rejects_sizes_clahe_cannot_tile():
    """CLAHE's 8x8 tile grid needs S % 8 == 0: the synthetic pipeline fails when built, not at the random
    step that first draws CLAHE."""
    import pytest
    from s3od_amd.data import GpuAugment
    with pytest.raises(ValueError, match="divisible by 8"):
        GpuAugment(100, mode="synthetic", device="cpu", seed=1)
    GpuAugment(100, mode="regular", device="cpu", seed=1)     # regular mode draws no CLAHE


def test_multiplicative_noise_draws_one_multiplier_per_channel():
    """albumentations 2.x MultiplicativeNoise samples shape [num_channels] (per_channel deprecated)."""
    from s3od_amd.data import GpuAugment
    aug = GpuAugment(64, mode="synthetic", device="cpu", seed=7)
    img = np.zeros((64, 64, 3), np.uint8)
    seen = 0
    for _ in range(300):
        m = list(aug.draw(64, 64, img).chain.mult)
        if m != [1.0, 1.0, 1.0]:
            assert len(set(m)) == 3 and all(0.9 <= v <= 1.1 for v in m)
            seen += 1
    assert seen > 0


def test_grid_distortion_maps_cover_the_image():
    """GridDistortion(num_steps=6) normalised steps: the source maps start at 0, increase, and end at the
    image width (so the distorted grid never leaves the image), for sizes that are not multiples of 6."""
    from s3od_amd.data import grid_distortion_maps
    r = np.random.default_rng(0)
    for S in (64, 100, 1024):
        for _ in range(5):
            gx, gy = grid_distortion_maps(S, 1 + r.uniform(-0.3, 0.3, 7), 1 + r.uniform(-0.3, 0.3, 7), 6)
            for g in (gx, gy):
                assert g.shape == (S,) and g[0] == 0 and np.all(np.diff(g) >= 0)      # segment ends repeat (linspace endpoints)
                assert abs(float(g[-1]) - S) < 1e-3 * S


def test_regular_mode_draws_sharpen_and_iso_chain():
    """mode="regular": Sharpen (OneOf weight 0.3 of p 0.5) and ISONoise (1/3 of p 0.3) are drawn at their
    reference rates and route the sample through the two-stage chain (raw geometry + order-1 chain)."""
    from s3od_amd.data import GpuAugment
    aug = GpuAugment(64, mode="regular", device="cpu", seed=5)
    n, sharpen, iso = 4000, 0, 0
    for _ in range(n):
        d = aug.draw(50, 60)
        p, q = d.geometry, d.chain
        if q is not None:
            assert p.raw == 1 and q.order == 1
            sharpen += q.ksize == 3
            iso += q.iso_intensity > 0
            assert (d.kernel is None) == (q.ksize == 1)
            if q.ksize == 3:
                assert d.kernel.shape == (3, 3)
            if q.iso_intensity > 0:
                assert 0.1 <= q.iso_intensity <= 0.5 and 0.01 <= q.iso_color_shift <= 0.05
        else:
            assert p.raw == 0
    assert abs(sharpen / n - 0.5 * 0.3) < 0.025 and abs(iso / n - 0.3 / 3) < 0.02, (sharpen / n, iso / n)


@pytest.mark.parametrize("mode", ["regular", "synthetic"])
def test_draw_stream_matches_recorded_draws(mode):
    """GpuAugment.draw reproduces, byte for byte, the draws recorded in tests/golden/augment_draws.npz at commit
    2bb4301 (the last one with the (AugParams, extra) / (q, kw, dr) draw API; recorded with its _draw and
    synth_params in __call__'s order): GpuAugment(96, mode, device="cpu", seed=s), four samples per seed of one
    72x96 image from np.random.RandomState(0), regular seeds 0..7, synthetic seeds 0..15.  Per sample: the raw
    bytes of AugParams and SynthParams (pointer fields zero), the float32 filter kernel, the rain drops, the
    GridDistortion maps and the ElasticTransform seed.  Each member the file must exercise occurs at least twice."""
    import ctypes
    from pathlib import Path
    from s3od_amd.data import AugParams, GpuAugment, SynthParams
    G = np.load(Path(__file__).parent / "golden" / "augment_draws.npz")
    k = mode[:3]
    img = np.random.RandomState(0).randint(0, 256, (72, 96, 3)).astype(np.uint8)
    seen = {}
    count = lambda **kw: seen.update({n: seen.get(n, 0) + bool(on) for n, on in kw.items()})
    i = 0
    for seed in range(8 if mode == "regular" else 16):
        aug = GpuAugment(96, mode, device="cpu", seed=seed)
        for _ in range(4):
            d = aug.draw(72, 96, img)
            tag = f"{mode} seed {seed} record {i}"
            assert bytes(d.geometry) == G[f"{k}_aug"][i].tobytes(), tag
            assert (d.chain is not None) == bool(G[f"{k}_has_chain"][i]), tag
            if d.chain is not None:
                assert bytes(d.chain) == G[f"{k}_chain"][i].tobytes(), tag
            ker = G[f"{k}_kernel"][G[f"{k}_kernel_off"][i]:G[f"{k}_kernel_off"][i + 1]]
            assert (d.kernel is None) == (ker.size == 0), tag
            if d.kernel is not None:
                assert d.kernel.dtype == np.float32 and d.kernel.tobytes() == ker.tobytes(), tag
            drops = G[f"{k}_drops"][G[f"{k}_drops_off"][i]:G[f"{k}_drops_off"][i + 1]]
            assert (d.drops is None) == (len(drops) == 0), tag
            if d.drops is not None:
                assert d.drops.dtype == np.int32 and d.drops.tobytes() == drops.tobytes(), tag
            assert (d.grid is not None) == bool(G[f"{k}_has_grid"][i]), tag
            if d.grid is not None:
                assert d.grid.dtype == np.float32 and d.grid.tobytes() == G[f"{k}_grid"][i].tobytes(), tag
            assert (-1 if d.elastic is None else d.elastic) == int(G[f"{k}_elastic"][i]), tag
            p, q = d.geometry, d.chain
            if mode == "synthetic":
                count(perspective=p.persp[0] != 0 or p.persp[1] != 0, kdist=p.kdist != 0, grid=d.grid is not None,
                      elastic=d.elastic is not None, clahe=q.clahe_clip > 0, hsv=q.hsv_h != 0, iso=q.iso_intensity > 0,
                      jpeg=q.jpeg_quality > 0, downscale=q.down < 1, shadow=q.n_shadow > 0, rbc=q.rbc_alpha != 1,
                      zoom=q.zoom_n > 0, colour_op=q.color_op > 0, posterize=q.post_bits < 8, snow=q.snow_point > 0,
                      rain=q.rain_n > 0, filter13=q.ksize >= 13)
            else:
                count(sharpen_chain=q is not None and q.ksize == 3, iso_chain=q is not None and q.iso_intensity > 0,
                      one_pass_jitter=q is None and p.bright != 1, one_pass_gauss=q is None and p.gauss_std > 0)
            i += 1
    assert i == len(G[f"{k}_aug"]) and ctypes.sizeof(AugParams) == G[f"{k}_aug"].shape[1] and ctypes.sizeof(SynthParams) == G[f"{k}_chain"].shape[1]
    assert all(n >= 2 for n in seen.values()), seen


def test_jpeg_restatement_matches_libjpeg():
    """The ImageCompression restatement (oracle/augment_oracle.py jpeg, which the device kernels are
    tested against) vs a real libjpeg encode/decode (PIL, quality q, 4:2:0): the same codec family
    cv2.imencode / imdecode use.  Differences come from libjpeg's integer DCT and fixed-point colour
    conversion: mean <= 1 8-bit step, and the restatement's loss vs the input within 5 % of libjpeg's."""
    import io
    from PIL import Image
    from oracle import augment_oracle as AO
    r = np.random.default_rng(0)
    for S in (64, 72):
        yy, xx = np.mgrid[0:S, 0:S] / S
        x = np.clip(np.stack([xx, yy, 0.5 + 0.3 * np.sin(6 * xx)]) + 0.15 * r.random((3, S, S)), 0, 1)
        for q in (30, 55, 80):
            u8 = np.rint(x * 255).astype(np.uint8).transpose(1, 2, 0)
            buf = io.BytesIO()
            Image.fromarray(u8).save(buf, format="JPEG", quality=q, subsampling=2)
            lj = np.asarray(Image.open(io.BytesIO(buf.getvalue())).convert("RGB")).transpose(2, 0, 1) / 255.0
            o = AO.jpeg(x, q)
            assert np.abs(o - lj).mean() * 255 <= 1.0, (S, q, np.abs(o - lj).mean() * 255)
            lo, ll = np.abs(o - u8.transpose(2, 0, 1) / 255.0).mean(), np.abs(lj - u8.transpose(2, 0, 1) / 255.0).mean()
            assert abs(lo - ll) <= 0.05 * ll, (S, q, lo, ll)


# ------------------------------------------------------------------ host composition of the warp (GpuAugment._geometry / draw)
class _Script:
    """random.Random stand-in: every draw returns the next scripted value, whatever its distribution, so a
    test walks one branch of the host code at a time."""

    def __init__(self, values):
        self.values = list(values)

    def _next(self, lo=None, hi=None):
        v = self.values.pop(0)
        assert lo is None or lo <= v <= hi, (v, lo, hi)
        return v

    def random(self):
        return self._next(0.0, 1.0)

    def uniform(self, a, b):
        return self._next(min(a, b), max(a, b))

    def randint(self, a, b):
        return int(self._next(a, b))

    def gauss(self, mu, sigma):
        return mu + sigma * self._next()

    def getrandbits(self, n):
        return int(self._next()) & ((1 << n) - 1)


_NO = 0.95                       # a gate draw that takes no branch
_S = 96


def _geo(script):
    from s3od_amd.data import GpuAugment
    aug = GpuAugment(_S, mode="regular", device="cpu", seed=0)
    aug.rng = _Script(script)
    M = aug._geometry(np.eye(3))
    assert not aug.rng.values
    return M


def _draw_A(script, mode="regular"):
    from s3od_amd.data import GpuAugment
    aug = GpuAugment(_S, mode=mode, device="cpu", seed=0)
    if mode == "synthetic":                          # the photometric groups follow: eight OneOf gates taken by none, the chain's seed
        script = script + [_NO] * 8 + [4321]
    aug.rng = _Script(script)
    d = aug.draw(72, 96)
    assert not aug.rng.values
    return d.geometry


def _apply(M, pts):
    q = (M @ np.concatenate([np.asarray(pts, np.float64), np.ones((len(pts), 1))], 1).T).T
    return q[:, :2] / q[:, 2:]


_PTS = [(0.0, 0.0), (10.0, 3.5), (95.5, 40.25), (96.0, 96.0)]
_CORNERS = [(0.0, 0.0), (_S, 0.0), (_S, _S), (0.0, _S)]
_GEO_SCRIPTS = {
    "hflip": [0.0, _NO, _NO, _NO, _NO],
    "vflip": [_NO, 0.0, _NO, _NO, _NO],
    "rot90_1": [_NO, _NO, 0.0, 1, _NO, _NO],
    "crop": [_NO, _NO, _NO, 0.0, 0.9, 0.05, 2, 5, _NO],
    "rotate": [_NO, _NO, _NO, _NO, 0.0, 10.0],
    "all": [0.0, 0.0, 0.0, 3, 0.0, 0.9, 0.05, 2, 5, 0.0, -7.5],
}


def test_geometry_flips_map_points():
    x, y = np.array(_PTS).T
    assert np.array_equal(_apply(_geo(_GEO_SCRIPTS["hflip"]), _PTS), np.stack([_S - x, y], 1))
    assert np.array_equal(_apply(_geo(_GEO_SCRIPTS["vflip"]), _PTS), np.stack([x, _S - y], 1))
    assert np.array_equal(_geo([_NO] * 5), np.eye(3))


def test_geometry_rot90_lands_corners_on_corners():
    perms = []
    for k in range(4):
        got = _apply(_geo([_NO, _NO, 0.0, k, _NO, _NO]), _CORNERS)
        idx = [_CORNERS.index((float(a), float(b))) for a, b in got]        # exact, or .index raises
        assert sorted(idx) == [0, 1, 2, 3]
        assert idx == [(i + idx[0]) % 4 for i in range(4)]                  # a rotation: cyclic order kept
        perms.append(idx[0])
    assert perms[0] == 0 and sorted(perms) == [0, 1, 2, 3]                  # k = 0 is the identity, every k differs
    assert (perms[1] + perms[3]) % 4 == 0 and perms[2] == 2                 # k and 4 - k undo each other


def test_geometry_resized_crop_maps_the_crop_to_the_output():
    M = _geo(_GEO_SCRIPTS["crop"])
    area, ar = _S * _S * 0.9, math.exp(0.05)
    cw, ch = int(round(math.sqrt(area * ar))), int(round(math.sqrt(area / ar)))
    assert (cw, ch) == (93, 89)
    got = _apply(M, [(2.0, 5.0), (2.0 + cw, 5.0 + ch)])
    assert np.abs(got - [[0, 0], [_S, _S]]).max() < 1e-12


def test_geometry_rotate_convention():
    """Rotate(limit 15) = cv2.getRotationMatrix2D(centre, angle, 1): [[cos, sin], [-sin, cos]] about the centre,
    so a positive angle moves the point right of the centre upwards (y down: counter-clockwise on screen)."""
    M = _geo(_GEO_SCRIPTS["rotate"])
    c, th = _S / 2, math.radians(10.0)
    assert np.abs(_apply(M, [(c, c)]) - [[c, c]]).max() < 1e-12
    L = M[:2, :2]
    assert np.abs(L @ L.T - np.eye(2)).max() < 1e-12 and abs(np.linalg.det(L) - 1) < 1e-12
    assert np.abs(_apply(M, [(c + 20, c)]) - [[c + 20 * math.cos(th), c - 20 * math.sin(th)]]).max() < 1e-12
    assert np.abs(M[2] - [0, 0, 1]).max() == 0


@pytest.mark.parametrize("name", sorted(_GEO_SCRIPTS))
def test_draw_packs_the_inverse_of_the_forward_matrix(name):
    """AugParams.A is the float32 cast of inv(M) (output pixel centre -> canvas), rows 0 and 1; the affine
    branches leave persp at 0."""
    script = _GEO_SCRIPTS[name]
    M = _geo(script)
    p = _draw_A(script + [_NO, _NO, 1234])          # no colour member, no noise member, the sample seed
    Minv = np.linalg.inv(M)
    A = np.array(list(p.A)).reshape(2, 3)
    assert np.abs(A - Minv[:2]).max() <= 1e-6 * np.abs(Minv[:2]).max(), (A, Minv)
    assert np.abs(_apply(np.vstack([A, [0, 0, 1]]) @ M, _PTS) - _PTS).max() < 1e-4      # and it undoes M
    assert p.persp[0] == 0 and p.persp[1] == 0 and p.kdist == 0 and p.seed == 1234
    if name != "all":
        assert np.abs(A - np.eye(3)[:2]).max() > 1e-3


def test_homography_maps_its_point_pairs():
    from s3od_amd.data import _homography
    src = np.array(_CORNERS)
    dst = src + np.array([[4.0, -6.5], [-7.25, 3.0], [5.5, 8.0], [-3.0, -9.0]])
    H = _homography(dst, src)
    assert np.abs(_apply(H, dst) - src).max() < 1e-9
    assert np.abs(_apply(_homography(src, dst), src) - dst).max() < 1e-9
    assert abs(H[2, 2] - 1) < 1e-12 and np.abs(H[2, :2]).max() > 1e-5          # genuinely projective


def test_perspective_composes_homography_then_inverse_geometry():
    """Perspective draw: output pixel -> H (jittered corners -> the square's corners) -> inv(M) -> canvas.
    With a non-trivial M (flip, crop, rotation) the swapped product inv(M)-then-H lands pixels away."""
    from s3od_amd.data import _homography
    geo = _GEO_SCRIPTS["all"]
    jit = [0.4, -0.65, -0.7, 0.3, 0.55, 0.8, -0.3, -0.9]                        # standard-normal draws, scale 0.07 * S
    p = _draw_A(geo + [0.0, 0.99, 0.07] + jit, mode="synthetic")                # distortion OneOf: member 3, Perspective
    M = _geo(geo)
    src = np.array(_CORNERS)
    dst = src + 0.07 * _S * np.array(jit).reshape(4, 2)
    Tot = np.array([list(p.A)[:3], list(p.A)[3:], [p.persp[0], p.persp[1], 1.0]])
    Mi = np.linalg.inv(M)
    assert p.raw == 1 and p.kdist == 0 and abs(p.persp[0]) > 1e-5
    assert np.abs(_apply(Tot, dst) - _apply(Mi, src)).max() < 5e-4              # float32 parameters on ~1e2 coordinates
    H = _homography(dst, src)
    assert np.abs(_apply(Tot, src) - _apply(Mi, _apply(H, src))).max() < 5e-4
    assert np.abs(_apply(Tot, src) - _apply(H, _apply(Mi, src))).max() > 1.0    # the swapped order is pixels away
