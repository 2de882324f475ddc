"""Device-side compositing, output formats and mask statistics: s3od_compose, s3od_mask_stats,
s3od_postprocess_batch_out, the ``background`` / ``stats`` / ``return_masks`` / ``return_rgba`` arguments of
BackgroundRemoval and s3od.visualizer.

Every comparison is exact.  The oracle of the blend is the reference's numpy formula (src/s3od/visualizer.py:17-21),
restated here and applied to the mask the call was given or returned; the counters are integers.  The one float bound,
1e-5 max-rel between a batched and a single-image forward, is that of test_gpu_infer_many.py and applies to masks only.
Synthetic weights, image_size 256.
"""
import ctypes

import numpy as np
import pytest
import torch
from PIL import Image

from test_gpu_infer_many import (S, SHAPES11, _align, _dev_bytes, _iou_logits, check_masks, is_two_pass, post_geometry,
                                 postprocess_batch, rand_images, rel_max)

pytestmark = pytest.mark.gpu

RGBA, OVER_COLOR, OVER_IMAGE, MASK_U8, NONE = range(5)
BPP = (4, 3, 3, 1, 0)


# ---------------------------------------------------------------------------------- oracles
def blend(mask, image, background):
    """src/s3od/visualizer.py:17-21: float32 products, a float32 1 - m, one add, truncation."""
    mask = mask[..., None]
    return (mask * image + (1 - mask) * background).astype(np.uint8)


def blend_contracted(mask, image, background, fuse_first):
    """The blend as a compiler that contracts a * b + c * d evaluates it: one product rounded to float32, the other
    exact inside the fused multiply-add (float64 holds the 24 x 8 bit product and the sum exactly), one rounding."""
    mask = mask[..., None]
    fg, rest = mask.astype(np.float64) * image, (1 - mask).astype(np.float64) * background
    if fuse_first:
        rest = rest.astype(np.float32).astype(np.float64)
    else:
        fg = fg.astype(np.float32).astype(np.float64)
    return (fg + rest).astype(np.float32).astype(np.uint8)


def expected(mode, mask, image, color=None, bg=None):
    if mode == RGBA:
        return np.dstack([image, (mask * 255).astype(np.uint8)])
    if mode == MASK_U8:
        return (mask * 255).astype(np.uint8)[..., None]
    return blend(mask, image, np.full_like(image, color) if mode == OVER_COLOR else bg)


def pack(color):
    return color[0] | color[1] << 8 | color[2] << 16


def numpy_stats(masks, best, thr):
    """demo/app.py:38-42 counts for every pair + area / bounding box of masks[best] > thr."""
    n = len(masks)
    inter, union = np.zeros((n, n), np.int64), np.zeros((n, n), np.int64)
    for i in range(n):
        for j in range(i, n):
            inter[i, j] = inter[j, i] = np.logical_and(masks[i] > 0.5, masks[j] > 0.5).sum()
            union[i, j] = union[j, i] = np.logical_or(masks[i] > 0.5, masks[j] > 0.5).sum()
    on = masks[best] > thr
    ys, xs = np.nonzero(on)
    bbox = (int(xs.min()), int(ys.min()), int(xs.max()) + 1, int(ys.max()) + 1) if on.any() else None
    return inter, union, int(on.sum()), bbox


def demo_is_ambiguous(all_masks, threshold=0.8):
    """demo/app.py:45-56"""
    for i in range(len(all_masks)):
        for j in range(i + 1, len(all_masks)):
            inter = np.logical_and(all_masks[i] > 0.5, all_masks[j] > 0.5).sum()
            union = np.logical_or(all_masks[i] > 0.5, all_masks[j] > 0.5).sum()
            if inter / (union + 1e-6) < threshold:
                return True
    return False


def assert_stats(st, masks, best, thr):
    inter, union, area, bbox = numpy_stats(masks, best, thr)
    assert np.array_equal(st.pair_inter, inter) and np.array_equal(st.pair_union, union)
    assert np.array_equal(st.pair_ious, inter / (union + 1e-6)) and st.pair_ious.dtype == np.float64
    assert st.area == area and st.bbox == bbox
    assert st.is_ambiguous() == demo_is_ambiguous(masks)


def compose_dev(mask, image, mode, color=(0, 0, 0), bg=None):
    from s3od_amd.compose import compose
    out = compose(torch.from_numpy(np.ascontiguousarray(mask)).cuda(), torch.from_numpy(image).cuda(), mode, pack(color),
                  None if bg is None else torch.from_numpy(bg).cuda())
    torch.cuda.synchronize()
    return out.cpu().numpy().reshape(*mask.shape, BPP[mode])


# ---------------------------------------------------------------------------------- 1. blend exactness
@pytest.fixture(scope="module")
def triples():
    """1000 x 700 pixels x 3 channels = 2.1 M (m, s, bg) triples with m = k / 255 as float32; the first pixels carry
    m = 0, 1 and two values slightly above 1."""
    rng = np.random.default_rng(0)
    H, W = 1000, 700
    m = (rng.integers(0, 256, (H, W)) / 255).astype(np.float32)
    m[0, :4] = [0.0, 1.0, np.nextafter(np.float32(1), np.float32(2)), np.float32(1) + np.float32(2.0 ** -21)]
    return m, rng.integers(0, 256, (H, W, 3), dtype=np.uint8), rng.integers(0, 256, (H, W, 3), dtype=np.uint8)


@pytest.mark.parametrize("background", ["colour", "image"])
def test_blend_is_numpy_float32_byte_for_byte(triples, background):
    m, s, bgimg = triples
    color = (201, 37, 119)
    bg = np.full_like(s, color) if background == "colour" else bgimg
    want = blend(m, s, bg)
    # the inputs tell a contracted evaluation from the reference's: either fused form changes >= 100 bytes
    for fuse_first in (True, False):
        n = int((blend_contracted(m, s, bg, fuse_first) != want).sum())
        print(f"{background}: contracted form (fma on the {'first' if fuse_first else 'second'} product) differs on {n} bytes")
        assert n >= 100
    lerp = (bg + m[..., None] * (s.astype(np.float32) - bg)).astype(np.uint8)
    assert int((lerp != want).sum()) >= 100
    got = compose_dev(m, s, OVER_COLOR, color) if background == "colour" else compose_dev(m, s, OVER_IMAGE, bg=bg)
    assert int((got != want).sum()) == 0
    assert np.array_equal(got[0, :4], want[0, :4])               # m = 0, 1 and just above 1


def test_blend_over_white_and_other_modes(triples):
    m, s, _ = triples
    m, s = m[:64], s[:64]
    assert np.array_equal(compose_dev(m, s, OVER_COLOR, (255, 255, 255)), blend(m, s, np.full_like(s, 255)))
    assert np.array_equal(compose_dev(m, s, RGBA), expected(RGBA, m, s))
    assert np.array_equal(compose_dev(m, s, MASK_U8), expected(MASK_U8, m, s))


# ---------------------------------------------------------------------------------- 2. geometry
@pytest.mark.parametrize("H", [1, 17])
@pytest.mark.parametrize("W", [1, 3, 31, 64, 111, 257])
def test_compose_geometry(W, H):
    """every mode, dense and with a pitch wider than the row (the bytes between rows stay), output offset by 1 byte"""
    from s3od_amd.compose import compose
    rng = np.random.default_rng(W * 100 + H)
    m = (rng.integers(0, 256, (H, W)) / 255).astype(np.float32)
    s = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    bg = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    color = (12, 200, 99)
    md, sd, bd = torch.from_numpy(m).cuda(), torch.from_numpy(s).cuda(), torch.from_numpy(bg).cuda()
    for mode in (RGBA, OVER_COLOR, OVER_IMAGE, MASK_U8):
        want = expected(mode, m, s, color, bg)
        assert np.array_equal(compose_dev(m, s, mode, color, bg if mode == OVER_IMAGE else None), want), mode
        row = W * BPP[mode]
        for offset, pitch in ((0, row + 5), (1, row + 8), (1, row)):
            buf = torch.full((offset + H * pitch + 7,), 0xA5, dtype=torch.uint8, device="cuda")
            compose(md, sd, mode, pack(color), bd, out=buf, out_offset=offset, pitch=pitch)
            torch.cuda.synchronize()
            host = buf.cpu().numpy()
            touched = np.zeros(host.shape, bool)
            for y in range(H):
                a = offset + y * pitch
                assert np.array_equal(host[a:a + row], want[y].reshape(-1)), (mode, offset, pitch, y)
                touched[a:a + row] = True
            assert (host[~touched] == 0xA5).all(), (mode, offset, pitch)


def test_compose_rejects_bad_arguments():
    from s3od_amd._lib import HipLibError, lib, stream
    z = torch.zeros(64, device="cuda")
    u = torch.zeros(64, dtype=torch.uint8, device="cuda")
    for args in [(z, u, 2, 2, 7, 0, None, u, 8),       # unknown mode
                 (z, u, 2, 2, OVER_IMAGE, 0, None, u, 6),   # mode 2 without an image
                 (z, u, 2, 2, OVER_COLOR, 0, u, u, 6),      # an image with another mode
                 (z, u, 2, 2, OVER_COLOR, 0, None, u, 5),   # pitch shorter than the row
                 (z, None, 2, 2, RGBA, 0, None, u, 8)]:     # no source
        with pytest.raises(HipLibError, match="compose"):
            lib()("s3od_compose", *args, stream())


# ---------------------------------------------------------------------------------- 3. mask statistics
def run_stats(masks, best, thr):
    from s3od_amd.compose import mask_stats
    st = mask_stats(torch.from_numpy(np.ascontiguousarray(masks)).cuda(), best, thr)
    return st


def levels(rng, shape):
    """values around and exactly at the 0.5 threshold"""
    return rng.choice(np.array([0.0, 0.25, 0.5, np.nextafter(np.float32(0.5), np.float32(1)), 0.75, 1.0], np.float32), size=shape)


@pytest.mark.parametrize("shape", [(3, 31, 31), (3, 1, 65), (3, 17, 257), (8, 37, 53), (1, 9, 9), (2, 5, 300)])
def test_mask_stats_against_numpy(shape):
    rng = np.random.default_rng(sum(shape))
    masks = levels(rng, shape)
    assert (masks == 0.5).any()
    for best, thr in ((0, 0.5), (shape[0] - 1, 0.3), (shape[0] // 2, 0.8)):
        assert_stats(run_stats(masks, best, thr), masks, best, thr)


def test_mask_stats_half_does_not_count():
    masks = np.full((3, 31, 31), 0.5, np.float32)
    st = run_stats(masks, 1, 0.5)
    assert not st.pair_inter.any() and not st.pair_union.any() and st.area == 0 and st.bbox is None
    assert run_stats(masks, 1, 0.49).area == 31 * 31


def test_mask_stats_crafted_planes():
    H, W = 31, 31
    zeros = np.zeros((3, H, W), np.float32)
    st = run_stats(zeros, 0, 0.5)
    assert not st.pair_union.any() and (st.pair_ious == 0).all() and st.bbox is None and st.area == 0
    assert st.is_ambiguous()
    ones = np.ones((3, H, W), np.float32)
    st = run_stats(ones, 2, 0.5)
    off = ~np.eye(3, dtype=bool)
    assert (st.pair_inter[off] == H * W).all() and (st.pair_union[off] == H * W).all()
    assert st.area == H * W and st.bbox == (0, 0, W, H) and not st.is_ambiguous()
    single = zeros.copy()
    single[:, H - 1, W - 1] = 1.0
    st = run_stats(single, 1, 0.5)
    assert (st.pair_inter[off] == 1).all() and st.area == 1 and st.bbox == (W - 1, H - 1, W, H)
    assert_stats(st, single, 1, 0.5)


def test_mask_stats_large_counts_and_repeatable():
    """2048 x 2048: block partials and atomics carry counts in the millions; two runs give the same block"""
    from s3od_amd.compose import MaskStats, mask_stats_words
    g = torch.Generator(device="cuda").manual_seed(1)
    masks = torch.rand((3, 2048, 2048), device="cuda", generator=g)
    masks[:, :5] = 0.0
    masks[:, :, :7] = 0.0
    masks[1] = (masks[0] + masks[1]) / 2
    w1 = mask_stats_words(masks, 2, 0.999).cpu().numpy()
    w2 = mask_stats_words(masks, 2, 0.999).cpu().numpy()
    assert np.array_equal(w1, w2)
    host = masks.cpu().numpy()
    st = MaskStats.from_words(w1.view(np.uint32), 3)
    assert_stats(st, host, 2, 0.999)
    assert st.pair_union[0, 2] > 3_000_000 and st.bbox[0] >= 7 and st.bbox[1] >= 5


def test_mask_stats_refuses_nine_masks():
    from s3od_amd._lib import HipLibError, lib, stream
    masks = torch.ones((9, 4, 4), device="cuda")
    words = torch.full((72,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    with pytest.raises(HipLibError, match="mask count 9"):
        lib()("s3od_mask_stats", masks, 9, 4, 4, 0, 0.5, words, stream())
    torch.cuda.synchronize()
    assert (words.cpu().numpy() == 0x5A5A5A5A).all()             # nothing was launched: the block is untouched


# ---------------------------------------------------------------------------------- 4. the batched entry
COLORS = [(255, 255, 255), (0, 255, 0), (201, 37, 119)]


def out_rows(b):
    """two outputs per image, mixed over the batch; every mode appears in both rows, some images get mode NONE"""
    first = (RGBA, OVER_COLOR, OVER_IMAGE, MASK_U8)[b % 4]
    second = (OVER_IMAGE, NONE, OVER_COLOR, RGBA, MASK_U8)[b % 5]
    return first, second


def postprocess_batch_out(logits, iou_logits, images, bgs, size, all_masks, want_masks, want_stats, thr=0.3):
    """-> per image (masks or None, [row outputs], counter words or None), best"""
    from s3od_amd._lib import lib, stream
    from s3od_amd.infer_many import OutDesc, PostDesc
    B, NM = logits.shape[:2]
    n_out = 2
    planes = (NM if all_masks else 1) if want_masks else 0
    lplanes = NM if (all_masks or want_stats) else 1
    offs, off = [], 0
    for im in images:
        offs.append(off)
        off = _align(off + im.size)
    bg_offs = []
    for bg in bgs:
        bg_offs.append(off)
        off = _align(off + bg.size)
    host = np.zeros(off, np.uint8)
    for im, o in zip(list(images) + list(bgs), offs + bg_offs):
        host[o:o + im.size] = im.reshape(-1)
    dev = torch.from_numpy(host).cuda()
    descs, odescs = (PostDesc * B)(), (OutDesc * (B * n_out))()
    mo = oo = to = so = 0
    for b, im in enumerate(images):
        H0, W0 = im.shape[:2]
        ph, pw, h, w = post_geometry((H0, W0), size)
        descs[b] = PostDesc(offs[b], mo, 0, to, ph, pw, h, w, H0, W0)
        for k, mode in enumerate(out_rows(b)):
            odescs[b * n_out + k] = OutDesc(bg_offs[b], oo, b * 288 if want_stats else -1, so, mode, pack(COLORS[b % 3]))
            oo = _align(oo + H0 * W0 * BPP[mode], 4)
        mo += planes * H0 * W0; to += lplanes * h * W0; so += NM * H0 * W0
    masks = torch.full((max(mo, 1),), -1.0, dtype=torch.float32, device="cuda")
    out = torch.full((oo,), 0xA5, dtype=torch.uint8, device="cuda")
    tmp = torch.empty((max(to, 4),), dtype=torch.float32, device="cuda")
    scratch = torch.empty((so,), dtype=torch.float32, device="cuda")
    stats = torch.full((B * 72,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    ious = torch.empty((B, NM), dtype=torch.float32, device="cuda")
    best = torch.empty((B,), dtype=torch.int32, device="cuda")
    lib()("s3od_best_index", iou_logits, B, NM, ious, best, stream())
    lib()("s3od_postprocess_batch_out", logits, B, NM, size, size, best, dev, _dev_bytes(descs), ctypes.addressof(descs),
          _dev_bytes(odescs), ctypes.addressof(odescs), n_out, 1 if all_masks else 0, masks if want_masks else None, out, tmp,
          scratch if want_stats and not (all_masks and want_masks) else None, stats if want_stats else None, thr, stream())
    torch.cuda.synchronize()
    masks, out, stats = masks.cpu().numpy(), out.cpu().numpy(), stats.cpu().numpy().view(np.uint32)
    res = []
    for b, im in enumerate(images):
        H0, W0 = im.shape[:2]
        d = descs[b]
        rows = []
        for k, mode in enumerate(out_rows(b)):
            o = odescs[b * n_out + k]
            rows.append(out[o.out_off:o.out_off + H0 * W0 * BPP[mode]].reshape(H0, W0, BPP[mode]))
        res.append((masks[d.mask_off:d.mask_off + planes * H0 * W0].reshape(planes, H0, W0) if planes else None, rows,
                    stats[b * 72:(b + 1) * 72] if want_stats else None))
    return res, best.cpu().numpy()


@pytest.fixture(scope="module")
def batch11():
    g = torch.Generator().manual_seed(3)
    logits = (torch.randn((len(SHAPES11), 3, S, S), generator=g) * 4).cuda()
    images = rand_images(SHAPES11, 4)
    bgs = rand_images(SHAPES11, 21)
    iou = _iou_logits(len(SHAPES11), 5)
    old, ious, best = postprocess_batch(logits, iou, images, S)
    return dict(logits=logits, images=images, bgs=bgs, iou=iou, old=old, best=best)


def test_old_entry_outputs_unchanged(batch11):
    """s3od_postprocess_batch forwards to the new code: its masks still match s3od_sigmoid_unpad_resize (bit-identical
    on the two-pass branch, 2e-6 on the tile branch, the bounds of test_gpu_infer_many.py) and its RGBA is the source
    plus the host's alpha of those masks"""
    assert any(is_two_pass(*post_geometry(s, S)[2:], *s) for s in SHAPES11)
    assert any(not is_two_pass(*post_geometry(s, S)[2:], *s) for s in SHAPES11)
    check_masks(batch11["logits"], SHAPES11, batch11["old"], S)
    for b, im in enumerate(batch11["images"]):
        masks, rgba = batch11["old"][b]
        assert np.array_equal(rgba, expected(RGBA, masks[batch11["best"][b]], im))


@pytest.mark.parametrize("variant", ["all_masks", "best_mask", "no_masks"])
def test_batched_outputs_equal_standalone_compose(batch11, variant):
    from s3od_amd.compose import MaskStats
    all_masks, want_masks = variant == "all_masks", variant != "no_masks"
    res, best = postprocess_batch_out(batch11["logits"], batch11["iou"], batch11["images"], batch11["bgs"], S, all_masks,
                                      want_masks, want_stats=True, thr=0.3)
    assert np.array_equal(best, batch11["best"])
    for b, (im, bg) in enumerate(zip(batch11["images"], batch11["bgs"])):
        old_masks = batch11["old"][b][0]
        masks, rows, words = res[b]
        if variant == "all_masks":
            assert np.array_equal(masks, old_masks), SHAPES11[b]
        elif variant == "best_mask":
            assert masks.shape[0] == 1 and np.array_equal(masks[0], old_masks[best[b]]), SHAPES11[b]
        else:
            assert masks is None
        m = old_masks[best[b]]
        for mode, got in zip(out_rows(b), rows):
            if mode == NONE:
                continue
            want = compose_dev(m, im, mode, COLORS[b % 3], bg if mode == OVER_IMAGE else None)
            assert np.array_equal(got, want), (SHAPES11[b], mode)
            assert np.array_equal(got, expected(mode, m, im, COLORS[b % 3], bg)), (SHAPES11[b], mode)
        assert_stats(MaskStats.from_words(words, 3), old_masks, best[b], 0.3)


def test_batched_without_stats_or_scratch(batch11):
    """no statistics: only the best plane is resampled, nothing touches the counter buffer; bytes are the same"""
    res, best = postprocess_batch_out(batch11["logits"], batch11["iou"], batch11["images"], batch11["bgs"], S, False, False,
                                      want_stats=False)
    for b, (im, bg) in enumerate(zip(batch11["images"], batch11["bgs"])):
        m = batch11["old"][b][0][best[b]]
        for mode, got in zip(out_rows(b), res[b][1]):
            if mode != NONE:
                assert np.array_equal(got, expected(mode, m, im, COLORS[b % 3], bg)), (SHAPES11[b], mode)


def test_batched_entry_rejects_bad_tables():
    from s3od_amd._lib import HipLibError, lib, stream
    from s3od_amd.infer_many import OutDesc, PostDesc
    descs = (PostDesc * 1)(PostDesc(0, 0, 0, 0, 0, 0, 256, 256, 50, 50))
    z = torch.zeros(50 * 50 * 12, device="cuda")
    u = torch.zeros(50 * 50 * 4, dtype=torch.uint8, device="cuda")
    best = torch.zeros(1, dtype=torch.int32, device="cuda")

    def call(od, n_out=1, out=u, scratch=None, stats=None, NM=3):
        lib()("s3od_postprocess_batch_out", z, 1, NM, 256, 256, best, u, _dev_bytes(descs), ctypes.addressof(descs),
              _dev_bytes(od), ctypes.addressof(od), n_out, 0, None, out, z, scratch, stats, 0.5, stream())
    with pytest.raises(HipLibError, match="unknown output mode"):
        call((OutDesc * 1)(OutDesc(0, 0, -1, 0, 9, 0)))
    with pytest.raises(HipLibError, match="output offset"):
        call((OutDesc * 1)(OutDesc(0, 2, -1, 0, RGBA, 0)))             # RGBA needs 4-byte alignment
    with pytest.raises(HipLibError, match="output buffer missing"):
        call((OutDesc * 1)(OutDesc(0, 0, -1, 0, OVER_COLOR, 0)), out=None)
    with pytest.raises(HipLibError, match="row count"):
        call((OutDesc * 1)(OutDesc(0, 0, -1, 0, NONE, 0)), n_out=0)
    with pytest.raises(HipLibError, match="every plane"):
        call((OutDesc * 1)(OutDesc(0, 0, 0, 0, NONE, 0)), stats=torch.zeros(72, dtype=torch.int32, device="cuda"))


# ---------------------------------------------------------------------------------- 5. API
@pytest.fixture(scope="module")
def br():
    from s3od import BackgroundRemoval
    return BackgroundRemoval("synthetic", image_size=S, compute_dtype="f32")


API_SHAPES = [(100, 200), (20, 30), (256, 255), (31, 31), (300, 200)]       # tile, two-pass, Quirk 2, two-pass, tile


def check_result(r, image, bg, thr, *, masks=True, all_masks=True, rgba=True, stats=True):
    """a result against the formulas applied to the masks it returned"""
    if masks:
        assert r.predicted_mask.shape == image.shape[:2]
        if all_masks:
            assert np.array_equal(r.predicted_mask, r.all_masks[r.all_ious.argmax()])
    else:
        assert r.predicted_mask is None and r.all_masks is None
    if not all_masks:
        assert r.all_masks is None
    if rgba:
        assert r.rgba_image.mode == "RGBA" and r.rgba_image.size == (image.shape[1], image.shape[0])
        if masks:
            assert np.array_equal(np.array(r.rgba_image), expected(RGBA, r.predicted_mask, image))
    else:
        assert r.rgba_image is None
    if bg is None:
        assert r.composite is None
    else:
        assert r.composite.mode == "RGB" and r.composite.size == (image.shape[1], image.shape[0])
        if masks:
            full = np.full_like(image, bg) if isinstance(bg, tuple) else bg
            assert np.array_equal(np.array(r.composite), blend(r.predicted_mask, image, full))
    if stats and masks and all_masks:
        assert_stats(r.stats, r.all_masks, int(r.all_ious.argmax()), thr)
    assert (r.stats is not None) == stats


@pytest.mark.parametrize("shape", [(100, 200), (20, 30), (256, 255)])
def test_remove_background_composite_and_stats(br, shape):
    image = rand_images([shape], 30)[0]
    bgimg = rand_images([shape], 31)[0]
    plain = br.remove_background(image)
    assert plain.composite is None and plain.stats is None
    for bg in [(255, 255, 255), (201, 37, 119), bgimg, Image.fromarray(bgimg)]:
        r = br.remove_background(image, 0.3, background=bg, stats=True)
        check_result(r, image, bgimg if isinstance(bg, Image.Image) else bg, 0.3)
        assert np.array_equal(r.all_masks, plain.all_masks) and np.array_equal(r.all_ious, plain.all_ious)
        assert np.array_equal(np.array(r.rgba_image), np.array(plain.rgba_image))
        assert r.stats.is_ambiguous() == demo_is_ambiguous(r.all_masks)
    # the threshold moves area and bbox and nothing else
    lo, hi = br.remove_background(image, 0.1, stats=True), br.remove_background(image, 0.9, stats=True)
    assert np.array_equal(lo.stats.pair_inter, hi.stats.pair_inter) and np.array_equal(lo.all_masks, hi.all_masks)
    assert lo.stats.area == int((lo.predicted_mask > 0.1).sum()) and hi.stats.area == int((hi.predicted_mask > 0.9).sum())


@pytest.fixture(scope="module")
def many_setup(br):
    images = rand_images(API_SHAPES, 32)
    bgimgs = rand_images(API_SHAPES, 33)
    backgrounds = {"none": None, "colour": (255, 255, 255),
                   "list": [(0, 255, 0), bgimgs[1], None, Image.fromarray(bgimgs[3]), bgimgs[4]]}
    per_image = {"none": [None] * 5, "colour": [(255, 255, 255)] * 5, "list": [(0, 255, 0), bgimgs[1], None, bgimgs[3], bgimgs[4]]}
    loops = {k: [br.remove_background(im, 0.3, background=bg, stats=True) for im, bg in zip(images, per_image[k])]
             for k in backgrounds}
    return images, backgrounds, per_image, loops


@pytest.mark.parametrize("background", ["none", "colour", "list"])
def test_many_equals_loop_for_every_combination(br, many_setup, background):
    images, backgrounds, per_image, loops = many_setup
    loop = loops[background]
    full = {}
    for stats in (True, False):
        for return_all_masks in (True, False):
            for return_masks in (True, False):
                for return_rgba in (True, False):
                    if not (return_masks or return_rgba or stats or background != "none"):
                        continue
                    key = dict(stats=stats, return_all_masks=return_all_masks, return_masks=return_masks, return_rgba=return_rgba)
                    many = br.remove_background_many(images, 0.3, batch_size=2, background=backgrounds[background], **key)
                    assert len(many) == len(images)
                    for i, (im, r, ref) in enumerate(zip(images, many, loop)):
                        check_result(r, im, per_image[background][i], 0.3, masks=return_masks, all_masks=return_all_masks,
                                     rgba=return_rgba, stats=stats)
                        assert rel_max(r.all_ious, ref.all_ious) <= 1e-5
                        if return_masks:
                            assert rel_max(r.predicted_mask, ref.predicted_mask) <= 1e-5, (i, key)
                        if API_SHAPES[i] == (256, 255):          # Quirk 2: the single-image path itself, bit for bit
                            if r.composite is not None:
                                assert np.array_equal(np.array(r.composite), np.array(ref.composite))
                            if stats:
                                assert np.array_equal(r.stats.pair_inter, ref.stats.pair_inter)
                                assert np.array_equal(r.stats.pair_union, ref.stats.pair_union)
                                assert r.stats.area == ref.stats.area and r.stats.bbox == ref.stats.bbox
                    if stats and return_all_masks and return_masks and return_rgba:
                        full = many
                    elif full:
                        # whatever is left out, what remains is what the full call gave: same composite, same counters
                        for r, f in zip(many, full):
                            if r.composite is not None:
                                assert np.array_equal(np.array(r.composite), np.array(f.composite)), key
                            if return_rgba:
                                assert np.array_equal(np.array(r.rgba_image), np.array(f.rgba_image)), key
                            if return_masks:
                                assert np.array_equal(r.predicted_mask, f.predicted_mask), key
                            if stats:
                                assert np.array_equal(r.stats.pair_inter, f.stats.pair_inter), key
                                assert np.array_equal(r.stats.pair_union, f.stats.pair_union), key
                                assert r.stats.area == f.stats.area and r.stats.bbox == f.stats.bbox, key
    assert full


def test_many_default_call_is_unchanged(br, many_setup):
    images = many_setup[0]
    a = br.remove_background_many(images, batch_size=2)
    b = br.remove_background_many(images, batch_size=2, stats=True, background=(1, 2, 3))
    for x, y in zip(a, b):
        assert x.composite is None and x.stats is None
        assert np.array_equal(x.all_masks, y.all_masks) and np.array_equal(x.all_ious, y.all_ious)
        assert np.array_equal(np.array(x.rgba_image), np.array(y.rgba_image))


def test_api_errors_come_before_gpu_work(br, monkeypatch):
    images = rand_images(API_SHAPES[:2], 34)

    def boom(*a, **k):
        raise AssertionError("the model ran before the arguments were validated")
    with monkeypatch.context() as m:
        m.setattr(br.model, "forward", boom)
        with pytest.raises(ValueError, match="background image has the size of its image"):
            br.remove_background(images[0], background=np.zeros((200, 100, 3), np.uint8))
        with pytest.raises(ValueError, match="image 1"):
            br.remove_background_many(images, background=np.zeros((100, 200, 3), np.uint8))
        with pytest.raises(ValueError, match="nothing requested"):
            br.remove_background_many(images, return_masks=False, return_rgba=False)
        with pytest.raises(ValueError, match="1 values for 2 images"):
            br.remove_background_many(images, background=[(1, 2, 3)])


# ---------------------------------------------------------------------------------- visualizer
class _Result:
    def __init__(self, masks, best=0):
        self.all_masks, self.predicted_mask = masks, masks[best]


@pytest.mark.parametrize("shape,n", [((37, 53), 3), ((64, 64), 5), ((9, 111), 1), ((20, 31), 8)])
def test_visualizer_equals_reference_formulas(shape, n):
    from s3od.visualizer import visualize_all_masks, visualize_removal
    rng = np.random.default_rng(n)
    image = rng.integers(0, 256, (*shape, 3), dtype=np.uint8)
    masks = (rng.integers(0, 256, (n, *shape)) / 255).astype(np.float32)
    res = _Result(masks, best=n - 1)
    for img in (image, Image.fromarray(image)):
        for color in ((0, 255, 0), (255, 255, 255), (201, 37, 119)):
            got = visualize_removal(img, res, background_color=color)
            assert isinstance(got, Image.Image) and got.mode == "RGB"
            assert np.array_equal(np.array(got), blend(res.predicted_mask, image, np.full_like(image, color)))
        assert np.array_equal(np.array(visualize_removal(img, res)), blend(res.predicted_mask, image, np.full_like(image, (0, 255, 0))))
        # src/s3od/visualizer.py:33-48
        h, w = shape
        gw = min(n, 4)
        gh = (n + gw - 1) // gw
        grid = np.zeros((h * gh, w * gw, 3), np.uint8)
        for idx, mask in enumerate(masks):
            r, c = idx // gw, idx % gw
            grid[r * h:(r + 1) * h, c * w:(c + 1) * w] = (mask[..., None] * image).astype(np.uint8)
        got = visualize_all_masks(img, res)
        assert isinstance(got, Image.Image) and got.size == (w * gw, h * gh)
        assert np.array_equal(np.array(got), grid)


def test_visualizer_on_a_real_result(br):
    from s3od.visualizer import visualize_all_masks, visualize_removal
    image = rand_images([(100, 200)], 35)[0]
    r = br.remove_background(image, background=(0, 255, 0), stats=True)
    assert np.array_equal(np.array(visualize_removal(image, r)), np.array(r.composite))
    assert visualize_all_masks(image, r).size == (600, 100)
    assert demo_is_ambiguous(r.all_masks) == r.stats.is_ambiguous()


def test_many_composites_own_their_memory(br, many_setup):
    images = many_setup[0]
    only = dict(batch_size=2, return_masks=False, return_rgba=False)
    first = br.remove_background_many(images, background=(255, 255, 255), stats=True, **only)
    keep = [(np.array(r.composite), r.stats.pair_inter.copy(), r.all_ious.copy()) for r in first]
    br.remove_background_many(rand_images(API_SHAPES, 36), background=(0, 0, 0), stats=True, **only)
    for r, (comp, inter, ious) in zip(first, keep):
        assert np.array_equal(np.array(r.composite), comp) and np.array_equal(r.stats.pair_inter, inter)
        assert np.array_equal(r.all_ious, ious)
