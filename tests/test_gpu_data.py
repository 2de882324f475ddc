"""Device batch construction (s3od_augment_sample via GpuAugment).  "test" mode against a numpy
restatement of LongestMaxSize + centred PadIfNeeded + Normalize (bilinear, half-pixel, edge
replicate; masks nearest) to 1e-5; geometric augmentations checked as exact pixel permutations;
reproducibility from the seed; the drawn "regular" and "synthetic" batches against the float64 oracle
applied to the replayed draws (test_drawn_batch_matches_oracle).  Parity with albumentations itself is
unpinned (not installed)."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import augment_oracle as AO

pytestmark = pytest.mark.gpu
MEAN = np.array([0.485, 0.456, 0.406])
STD = np.array([0.229, 0.224, 0.225])


def _sample(h, w, seed=0):
    r = np.random.default_rng(seed)
    img = r.integers(0, 256, (h, w, 3), dtype=np.uint8)
    mask = (r.random((h, w)) > 0.5).astype(np.uint8) * 255
    return {"image": img, "mask": mask}


def _ref_test_mode(smp, S):
    from s3od_amd.data import AugParams
    p = AugParams.identity(*smp["mask"].shape, S)
    canvas, mcan = AO.letterbox_canvas(smp["image"], smp["mask"], p, S)
    return (canvas - MEAN[:, None, None]) / STD[:, None, None], mcan


@pytest.mark.parametrize("hw", [(300, 200), (97, 160), (128, 128)])
def test_test_mode_matches_restatement(hw):
    from s3od_amd.data import GpuAugment
    smp = _sample(*hw)
    out = GpuAugment(128, mode="test")([smp])
    torch.cuda.synchronize()
    ri, rm = _ref_test_mode(smp, 128)
    assert np.abs(out["images"][0].cpu().numpy() - ri).max() < 1e-4
    assert np.array_equal(out["masks"][0].cpu().numpy(), rm)


def test_flip_and_rot90_are_exact_permutations():
    from s3od_amd.data import GpuAugment, AugParams
    from s3od_amd._lib import lib, stream
    S = 64
    smp = _sample(50, 64, 3)
    aug = GpuAugment(S, mode="test")
    base = aug([smp])
    img = torch.from_numpy(smp["image"]).cuda()
    msk = torch.from_numpy(smp["mask"]).cuda()

    def run(Minv):
        p = aug.draw(50, 64).geometry
        for i, v in enumerate(list(Minv[0]) + list(Minv[1])):
            p.A[i] = float(v)
        oi = torch.empty((3, S, S), device="cuda"); om = torch.empty((S, S), device="cuda")
        lib()("s3od_augment_sample", img, msk, ctypes.addressof(p), S, oi, om, stream())
        torch.cuda.synchronize()
        return oi.cpu(), om.cpu()

    fl = np.array([[-1, 0, S], [0, 1, 0], [0, 0, 1]], np.float64)        # x -> S - x (its own inverse)
    oi, om = run(fl)
    assert torch.equal(oi, base["images"][0].cpu().flip(-1)) and torch.equal(om, base["masks"][0].cpu().flip(-1))
    r90 = np.array([[0, -1, S], [1, 0, 0], [0, 0, 1]], np.float64)      # output (x,y) <- canvas (S-y, x)
    oi, om = run(r90)
    assert torch.equal(oi, torch.rot90(base["images"][0].cpu(), 1, (1, 2)))
    assert torch.equal(om, torch.rot90(base["masks"][0].cpu(), 1, (0, 1)))


def test_regular_mode_reproducible_and_sane():
    from s3od_amd.data import GpuAugment
    smps = [_sample(120 + 7 * i, 90 + 11 * i, i) for i in range(6)]
    a = GpuAugment(96, mode="regular", seed=5)(smps)
    b = GpuAugment(96, mode="regular", seed=5)(smps)
    torch.cuda.synchronize()
    assert torch.equal(a["images"], b["images"]) and torch.equal(a["masks"], b["masks"])
    assert torch.isfinite(a["images"]).all()
    lo = torch.tensor(((0 - MEAN) / STD), dtype=torch.float32).view(1, 3, 1, 1).cuda()
    hi = torch.tensor(((1 - MEAN) / STD), dtype=torch.float32).view(1, 3, 1, 1).cuda()
    assert (a["images"] >= lo - 1e-5).all() and (a["images"] <= hi + 1e-5).all()
    assert set(torch.unique(a["masks"]).tolist()) <= {0.0, 1.0}


def _denorm(t):
    return t.cpu().numpy() * STD[:, None, None] + MEAN[:, None, None]


def test_synthetic_identity_chain_equals_test_mode():
    """raw geometry pass + the synthetic photometric passes with every effect at identity == the
    test-mode (letterbox + Normalize) output: the plumbing of the three-pass pipeline is exact."""
    from s3od_amd.data import GpuAugment, SynthParams
    from s3od_amd._lib import lib, stream
    S = 96
    smp = _sample(80, 120, 4)
    base = GpuAugment(S, mode="test")([smp])
    aug = GpuAugment(S, mode="test")
    p = aug.draw(80, 120, smp["image"]).geometry
    p.raw = 1
    img = torch.from_numpy(smp["image"]).cuda(); msk = torch.from_numpy(smp["mask"]).cuda()
    raw = torch.empty(3, S, S, device="cuda"); om = torch.empty(S, S, device="cuda"); out = torch.empty(3, S, S, device="cuda")
    lib()("s3od_augment_sample", img, msk, ctypes.addressof(p), S, raw, om, stream())
    q = SynthParams.identity()
    lib()("s3od_augment_synthetic", raw, ctypes.addressof(q), None, S, out, stream())
    torch.cuda.synchronize()
    assert float((out - base["images"][0]).abs().max()) < 1e-5
    assert torch.equal(om, base["masks"][0])


@pytest.mark.parametrize("what", ["gray", "posterize", "blur_const", "shuffle"])
def test_synthetic_effects_exact_properties(what):
    from s3od_amd.data import SynthParams
    from s3od_amd._lib import lib, stream
    S = 64
    g = torch.Generator(device="cuda").manual_seed(1)
    raw = torch.rand(3, S, S, device="cuda", generator=g)
    if what == "blur_const":
        raw = torch.full((3, S, S), 0.3, device="cuda")
    ref = raw.clone()
    q = SynthParams.identity()
    kw = None
    if what == "gray":
        q.color_op = 2
    elif what == "posterize":
        q.post_bits = 5
    elif what == "blur_const":
        q.ksize = 5
        kw = torch.full((25,), 1 / 25, device="cuda")
    elif what == "shuffle":
        q.color_op = 3
        q.perm[0], q.perm[1], q.perm[2] = 2, 0, 1
    out = torch.empty(3, S, S, device="cuda")
    lib()("s3od_augment_synthetic", raw, ctypes.addressof(q), kw, S, out, stream())
    torch.cuda.synchronize()
    v = _denorm(out)
    r = ref.cpu().numpy()
    if what == "gray":
        assert np.abs(v[0] - v[1]).max() < 1e-5 and np.abs(v[1] - v[2]).max() < 1e-5
        assert np.abs(v[0] - (0.299 * r[0] + 0.587 * r[1] + 0.114 * r[2])).max() < 1e-5
    elif what == "posterize":
        q8 = np.round(v * 255)
        assert np.abs(v * 255 - q8).max() < 1e-3 and (q8.astype(int) % 8 == 0).all()
    elif what == "blur_const":
        assert np.abs(v - 0.3).max() < 1e-5
    elif what == "shuffle":
        assert np.abs(v - r[[2, 0, 1]]).max() < 1e-5


def test_synthetic_mode_reproducible_and_sane():
    from s3od_amd.data import GpuAugment
    smps = [_sample(120 + 7 * i, 90 + 11 * i, i) for i in range(8)]
    a = GpuAugment(96, mode="synthetic", seed=9)(smps)
    b = GpuAugment(96, mode="synthetic", seed=9)(smps)
    torch.cuda.synchronize()
    assert torch.equal(a["images"], b["images"]) and torch.equal(a["masks"], b["masks"])
    lo = torch.tensor(((0 - MEAN) / STD), dtype=torch.float32).view(1, 3, 1, 1).cuda()
    hi = torch.tensor(((1 - MEAN) / STD), dtype=torch.float32).view(1, 3, 1, 1).cuda()
    assert torch.isfinite(a["images"]).all()
    assert (a["images"] >= lo - 1e-5).all() and (a["images"] <= hi + 1e-5).all()
    assert set(torch.unique(a["masks"]).tolist()) <= {0.0, 1.0}
    assert a["masks"].sum() > 0


# ------------------------------------------------------------------ end to end: the drawn batch against the oracle
# Sources whose letterbox ratio at S = 96 is exact in float32 (the mask's source index has no rounding ambiguity).
E2E_SOURCES = [(108, 144), (144, 108), (36, 48), (72, 96)]
E2E_SEEDS = {"regular": (0, 1, 2), "synthetic": (12, 19, 38)}       # chosen on the CPU: see _drawn and the test's last asserts


def _replay(mode, seed, smps, S=96, device="cpu"):
    """The draws of GpuAugment(S, mode, seed) for these samples, from a second instance: draw is host-only
    and __call__ makes exactly one per sample, in order."""
    from s3od_amd.data import GpuAugment
    rep = GpuAugment(S, mode=mode, device=device, seed=seed)
    return rep, [rep.draw(*smp["image"].shape[:2], smp["image"]) for smp in smps]


def _drawn(draws):
    """Which of the members the end-to-end test must see were drawn."""
    seen = set()
    for d in draws:
        p, q = d.geometry, d.chain
        A = np.array(list(p.A))
        if np.abs(A - np.rint(A)).max() > 1e-3:
            seen.add("fractional_affine")
        if p.persp[0] != 0 or p.persp[1] != 0:
            seen.add("perspective")
        if p.kdist != 0:
            seen.add("kdist")
        if p.bright != 1 or (q is not None and q.bright != 1):
            seen.add("colour_jitter")
    return seen


def _jitter_gain(b):
    """Lipschitz constant (max norm) of ColorJitter + mult: how far an input error can grow through them."""
    th = 2 * np.pi * b.hue
    cs, a, s = np.cos(th), (1 - np.cos(th)) / 3, np.sin(th) / np.sqrt(3.0)
    return (max(1.0, b.bright) * max(1.0, b.contrast) * (b.sat + abs(1 - b.sat)) * (abs(cs + a) + abs(a - s) + abs(a + s))
            * max(list(b.mult)))


def _chain_tol(q, ker):
    """Tolerance of the photometric chain on an exact input, from the figures of the member tests: 1e-5 per
    pixel (1e-4 with a hashed Gaussian, ISONoise, an HSV shift or ZoomBlur), the filter's float32 accumulation
    n_taps * 2^-24 * sum|w|, and the gains of what follows a stage (the filter's sum|w| and the contrast of
    RandomBrightnessContrast after the per-pixel stage, sepia's largest row sum 1.351 and the snow coefficient
    after the filter; in the regular chain the jitter follows the filter)."""
    pix = 1e-4 if (q.gauss_std > 0 or q.iso_intensity > 0 or q.hsv_h != 0 or q.hsv_s != 0 or q.hsv_v != 0 or q.zoom_n) else 1e-5
    sw = float(np.abs(ker).sum()) if ker is not None else 1.0
    filt = (ker.size if ker is not None else 1) * 2.0 ** -24 * sw
    if q.order == 1:
        return pix + (1e-5 + filt) * _jitter_gain(q)
    post = (1.351 if q.color_op == 1 else 1.0) * (q.snow_coeff if q.snow_point > 0 else 1.0)
    return (pix * max(1.0, sw) * max(1.0, q.rbc_alpha) + filt) * post


@pytest.mark.parametrize("mode", ["regular", "synthetic"])
def test_drawn_batch_matches_oracle(mode):
    """GpuAugment end to end for three seeds of four samples: the device batch equals the oracle applied to
    the replayed draws, so the host composition (matrix order, inverse, perspective product, packing, the
    chain's parameters) is compared with something.  Masks: exact outside the reference's ambiguous pixels
    (<= 2 %).  Images: one-pass regular samples under the geometry test's bound (1e-5 + remap_bound, 1e-4 with
    Gaussian noise).  Samples with a second stage (synthetic, or Sharpen / ISONoise in regular mode): the
    geometry pass is launched again with the replayed parameters and checked under remap_bound, and the
    batch image must equal the oracle's chain of that raw picture within _chain_tol; the chain has
    discontinuous members (Poisson inversion, polygon edges, Posterize steps, the snow threshold), so at most
    0.2 % of pixels may be beyond it, as in the ISONoise test.  CLAHE / ImageCompression / RandomRain draws
    keep their own tests: for them only the geometry pass and the mask are compared.
    Measured on an MI355X: masks: no mismatch, excluded share <= 1.04 % (regular <= 0.48 %); one-pass regular
    samples worst |err| / bound 0.053; geometry of the two-stage samples worst 0.111; chains: max |err| 7.4e-6 at
    tolerances of 1.3e-5 .. 2.3e-4, no pixel beyond; 2 of the 12 synthetic samples drew CLAHE / JPEG / rain."""
    from s3od_amd.data import GpuAugment, elastic_params
    from s3od_amd._lib import lib, stream
    S = 96
    smps = [_sample(h, w, 10 + i) for i, (h, w) in enumerate(E2E_SOURCES)]
    seen, fails, full = set(), [], 0
    for seed in E2E_SEEDS[mode]:
        out = GpuAugment(S, mode=mode, seed=seed)(smps)
        torch.cuda.synchronize()
        _, draws = _replay(mode, seed, smps)
        seen |= _drawn(draws)
        for b, (smp, d) in enumerate(zip(smps, draws)):
            tag = f"{mode} seed {seed} sample {b}"
            p, q = d.geometry, d.chain
            ker = d.kernel.astype(np.float64) if d.kernel is not None else None
            grid = d.grid
            keep, fld = [], None
            if d.elastic is not None:                   # the device generator's field (it has its own parity test)
                e = elastic_params(d.elastic)
                tmp = torch.empty(2, S, S, device="cuda"); fld = torch.empty(2, S, S, device="cuda")
                lib()("s3od_elastic_field", ctypes.addressof(e), S, tmp, fld, stream())
                torch.cuda.synchronize()
            eh = fld.cpu().numpy() if fld is not None else None
            ref_i, ref_m = AO.augment_sample(smp["image"], smp["mask"], p, S, grid=grid, elastic=eh)
            canvas, _ = AO.letterbox_canvas(smp["image"], None, p, S)
            cx, cy, _ = AO.warp_coords(p, S, grid, eh)
            geo = AO.remap_bound(canvas, cx, cy, S)[None]
            amb = AO.nearest_ambiguous(cx, cy)
            got_m = out["masks"][b].cpu().numpy().astype(np.float64)
            bad = int(((got_m != ref_m) & ~amb).sum())
            got = _denorm(out["images"][b]).astype(np.float64)
            line = f"[{tag}] excluded mask share {100 * amb.mean():.2f} %, mask mismatches {bad}"
            if amb.mean() > 0.02 or bad:
                fails.append(line)
            if not p.raw:                               # one-pass regular sample
                bound = 1e-4 if p.gauss_std > 0 else 1e-5 + geo
                ratio = (np.abs(got - ref_i) / bound).max()
                line += f", one pass worst |err|/bound {ratio:.3f}"
                if ratio > 1:
                    fails.append(line)
                print("\n" + line)
                full += 1
                continue
            if grid is not None:
                keep.append(torch.from_numpy(grid).cuda())
                p.grid = keep[-1].data_ptr()
            if fld is not None:
                p.elastic = fld.data_ptr()
            raw = torch.full((3, S, S), float("nan"), device="cuda")
            ti, tm = torch.from_numpy(smp["image"]).cuda(), torch.from_numpy(smp["mask"]).cuda()
            om = torch.empty(S, S, device="cuda")
            lib()("s3od_augment_sample", ti, tm, ctypes.addressof(p), S, raw, om, stream())
            torch.cuda.synchronize()
            raw = raw.cpu().numpy().astype(np.float64)
            ratio = (np.abs(raw - ref_i) / geo).max()
            line += f", geometry worst |err|/bound {ratio:.3f}"
            if not ratio <= 1:
                fails.append(line)
            if q.clahe_clip > 0 or q.jpeg_quality > 0 or q.rain_n > 0:
                print("\n" + line + ", photometric chain not compared (CLAHE / JPEG / rain)")
                continue
            ref = AO.synthetic_chain(raw, q, ker)
            tol = _chain_tol(q, ker)
            f = float((np.abs(got - ref).max(0) > tol).mean())
            line += f", chain tol {tol:.2e}: max |err| {np.abs(got - ref).max():.2e}, share beyond {100 * f:.3f} %"
            if f > 2e-3:
                fails.append(line)
            print("\n" + line)
            full += 1
    want = {"fractional_affine", "colour_jitter"} | ({"perspective", "kdist"} if mode == "synthetic" else set())
    assert want <= seen, (want - seen)
    assert full >= 6, full                              # most samples are compared through to the batch image
    assert not fails, "\n".join(fails)


def test_batch_equals_launch_of_replayed_draws():
    """__call__ is the loop around draw and launch, and nothing else: for one regular and one synthetic seed
    (chosen on the CPU: a Sharpen chain, an ISONoise chain, one-pass samples; rain, an elastic field, 3x3 and 7x7
    filters), launch of the replayed draws into fresh NaN-filled buffers, one sample at a time, gives the
    batch's images and masks bit for bit.  ISONoise samples are left out: their float64 lightness sums go through
    atomics whose order varies from run to run (test_drawn_batch_matches_oracle covers them)."""
    S = 96
    smps = [_sample(h, w, 10 + i) for i, (h, w) in enumerate(E2E_SOURCES)]
    compared = 0
    for mode, seed in (("regular", E2E_SEEDS["regular"][1]), ("synthetic", E2E_SEEDS["synthetic"][2])):
        from s3od_amd.data import GpuAugment
        out = GpuAugment(S, mode=mode, seed=seed)(smps)
        torch.cuda.synchronize()
        rep, draws = _replay(mode, seed, smps, device="cuda")
        for b, (smp, d) in enumerate(zip(smps, draws)):
            if d.chain is not None and d.chain.iso_intensity > 0:
                continue
            oi = torch.full((3, S, S), float("nan"), device="cuda"); om = torch.full((S, S), float("nan"), device="cuda")
            keep = rep.launch(d, torch.from_numpy(smp["image"]).cuda(), torch.from_numpy(smp["mask"]).cuda(), oi, om)
            torch.cuda.synchronize()
            del keep
            assert torch.equal(oi, out["images"][b]) and torch.equal(om, out["masks"][b]), f"{mode} seed {seed} sample {b}"
            compared += 1
    assert compared >= 6, compared
