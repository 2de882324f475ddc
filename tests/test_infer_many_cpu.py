"""CPU checks of the batched inference plumbing: the ctypes descriptor mirrors against the layout
include/s3od_hip.h states (sizes and @offset comments), the pre-flight geometry classifier and the byte
layout ``plan_chunk`` gives a chunk for every kind of request."""
import ctypes
import itertools
import re

import numpy as np
import pytest

from conftest import REPO

from s3od_amd.infer_many import (MODE_NONE, MODE_RGB_OVER_COLOR, MODE_RGB_OVER_IMAGE, MODE_RGBA, STATS_WORDS, PostDesc, PreDesc,
                                 Request, classify_geometry, plan_chunk)

CT = {"long": ctypes.c_long, "int": ctypes.c_int}


def header_struct(name):
    """-> (sizeof, [(field, ctype, offset)]) as the header states them"""
    text = (REPO / "include" / "s3od_hip.h").read_text()
    m = re.search(r"struct %s \{\s*/\* (\d+) bytes \*/\n(.*?)\n\};" % name, text, re.S)
    assert m, f"struct {name} not in the header"
    fields = re.findall(r"^\s+(long|int) (\w+);\s*/\* @(\d+) ", m.group(2), re.M)
    assert len(fields) == len(m.group(2).splitlines())
    return int(m.group(1)), [(f, CT[t], int(o)) for t, f, o in fields]


@pytest.mark.parametrize("name,mirror", [("S3odPreDesc", PreDesc), ("S3odPostDesc", PostDesc)])
def test_descriptor_mirrors_header(name, mirror):
    size, fields = header_struct(name)
    assert ctypes.sizeof(mirror) == size
    assert [f for f, _ in mirror._fields_] == [f for f, _, _ in fields]
    for (fname, ctype), (_, htype, off) in zip(mirror._fields_, fields):
        assert ctype is htype, fname
        assert getattr(mirror, fname).offset == off, fname
    # a packed array: the stride is the size
    assert ctypes.sizeof(mirror * 3) == 3 * size


def test_header_declares_batched_entries():
    text = (REPO / "include" / "s3od_hip.h").read_text()
    for fn in ("s3od_preprocess_batch", "s3od_best_index", "s3od_postprocess_batch"):
        assert re.search(r"^int %s\(" % fn, text, re.M), fn


def test_batched_image_kernels_do_not_spill(tmp_path):
    """Resource audit of the built gfx950 code object of image_ops.hip: the batched kernels have no private segment
    and no register spills (read from build/image_ops.o as test_kernel_resources_cpu.py reads its kernels)."""
    import subprocess
    from test_kernel_resources_cpu import LLVM, TOOLS
    from pathlib import Path
    obj = REPO / "build" / "image_ops.o"
    if not all(t and Path(t).exists() for t in TOOLS):
        pytest.skip("objcopy / clang-offload-bundler / llvm-readelf / c++filt not available")
    if not obj.exists():
        pytest.skip("build/image_ops.o absent: run make (or __graft_entry__.build()) first")
    fat, co = tmp_path / "image_ops.fatbin", tmp_path / "image_ops.co"
    subprocess.run([TOOLS[0], "-O", "binary", "--only-section=.hip_fatbin", str(obj), str(fat)], check=True)
    subprocess.run([str(LLVM / "clang-offload-bundler"), "--unbundle", "--type=o", f"--input={fat}",
                    "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}"], check=True, capture_output=True)
    notes = subprocess.run([str(LLVM / "llvm-readelf"), "--notes", str(co)], check=True, capture_output=True, text=True).stdout
    found, cur = {}, None
    for line in notes.splitlines():
        m = re.match(r"\s+\.(name|private_segment_fixed_size|sgpr_spill_count|vgpr_spill_count):\s+(\S+)", line)
        if m and m.group(1) == "name":
            cur = m.group(2)
        elif m and cur:
            found.setdefault(cur, {})[m.group(1)] = int(m.group(2))
    want = ["preprocess_batch_kernel", "post_tile_kernel", "post_h_batch_kernel", "post_v_batch_kernel", "best_index_kernel"]
    for k in want:
        hits = [v for n, v in found.items() if k in n]
        assert hits, f"{k} not in the build"
        for v in hits:
            assert v == {"private_segment_fixed_size": 0, "sgpr_spill_count": 0, "vgpr_spill_count": 0}, (k, v)


BATCHED = [(100, 200), (480, 640), (20, 30), (40, 640), (200, 100), (640, 480), (30, 20), (640, 40), (256, 256), (31, 31),
           (512, 512)]
SINGLE = [(256, 255), (255, 256)]
RAISES = [(101, 256), (160, 111)]


@pytest.mark.parametrize("shape", BATCHED)
def test_classifier_batched(shape):
    assert classify_geometry(*shape, 256) == "batched"


@pytest.mark.parametrize("shape", SINGLE)
def test_classifier_quirk2_single(shape):
    assert classify_geometry(*shape, 256) == "single"


@pytest.mark.parametrize("shape", RAISES)
def test_classifier_odd_padding_raises(shape):
    with pytest.raises(ValueError, match="image 7: could not broadcast"):
        classify_geometry(*shape, 256, index=7)


@pytest.mark.parametrize("shape", BATCHED + SINGLE + RAISES)
def test_classifier_without_quirks_batches_everything(shape):
    assert classify_geometry(*shape, 256, exact_reference_quirks=False) == "batched"


# ---------------------------------------------------------------------------------- the chunk planner
PLAN_SHAPES = [(100, 200), (20, 30), (640, 480), (31, 31)]
PLAN_S = 256
FLAGS = list(itertools.product([True, False], repeat=4))       # all_masks, want_masks, want_rgba, want_stats


def plan_backgrounds(kind):
    """-> per-image normalised backgrounds: none, one colour, or colour / image / None / image"""
    if kind == "none":
        return None
    if kind == "colour":
        return [0xFFFFFF] * len(PLAN_SHAPES)
    return [0x00FF00, np.full((20, 30, 3), 7, np.uint8), None, np.full((31, 31, 3), 9, np.uint8)]


def assert_disjoint_inside(regions, total, what):
    regions = sorted(regions)
    assert regions[0][0] >= 0 and regions[-1][1] <= total, (what, regions, total)
    for (a0, a1), (b0, b1) in zip(regions, regions[1:]):
        assert a0 < a1 <= b0, (what, regions)
    assert regions[-1][0] < regions[-1][1], (what, regions)


@pytest.mark.parametrize("background", ["none", "colour", "mixed"])
@pytest.mark.parametrize("NM", [1, 3])
def test_plan_chunk_layout(NM, background):
    from s3od_amd.image_ops import reference_geometry
    geoms = [reference_geometry(h, w, PLAN_S)[0] for h, w in PLAN_SHAPES]
    bgs = plan_backgrounds(background)
    per_image = bgs if bgs is not None else [None] * len(PLAN_SHAPES)
    B, LH, LW = len(PLAN_SHAPES), PLAN_S, PLAN_S
    for all_masks, want_masks, want_rgba, want_stats in FLAGS:
        key = (NM, background, all_masks, want_masks, want_rgba, want_stats)
        p = plan_chunk(PLAN_SHAPES, geoms, NM, LH, LW, Request(all_masks=all_masks, want_masks=want_masks, want_rgba=want_rgba,
                                                               backgrounds=bgs, want_stats=want_stats, threshold=0.3))
        assert p.shapes == PLAN_SHAPES and p.threshold == 0.3
        assert p.all_masks == (all_masks and want_masks), key
        assert p.planes == ((NM if all_masks else 1) if want_masks else 0), key
        assert p.n_out == max(1, int(want_rgba) + int(any(bg is not None for bg in per_image))), key
        assert len(p.pre) == len(p.post) == B and len(p.outd) == B * p.n_out, key
        # ---- inputs: the three tables, every source and every background image
        regions = [(off, off + ctypes.sizeof(t)) for off, t in ((p.pre_off, p.pre), (p.post_off, p.post), (p.out_desc_off, p.outd))]
        for b, (H0, W0) in enumerate(PLAN_SHAPES):
            assert p.post[b].img_off == p.pre[b].img_off
            assert (p.pre[b].H0, p.pre[b].W0, p.pre[b].new_h, p.pre[b].new_w, p.pre[b].pad_h, p.pre[b].pad_w) == (H0, W0, *geoms[b][:4])
            assert (p.post[b].pad_h, p.post[b].pad_w, p.post[b].h, p.post[b].w, p.post[b].H0, p.post[b].W0) == \
                (*geoms[b][4:], LH - 2 * geoms[b][4], LW - 2 * geoms[b][5], H0, W0)
            regions.append((p.pre[b].img_off, p.pre[b].img_off + H0 * W0 * 3))
        regions += [(off, off + bg.size) for off, bg in p.bg_copies]
        assert all(a % 16 == 0 for a, _ in regions), key
        assert_disjoint_inside(regions, p.in_bytes, key)
        # ---- the output table: an RGBA row when wanted, then the image's composite row, NONE where it has nothing
        bg_regions = dict((off, bg) for off, bg in p.bg_copies)
        for b, bg in enumerate(per_image):
            rows = [p.outd[b * p.n_out + k] for k in range(p.n_out)]
            want = [MODE_RGBA] if want_rgba else []
            if bg is not None:
                want.append(MODE_RGB_OVER_COLOR if isinstance(bg, int) else MODE_RGB_OVER_IMAGE)
            assert [r.mode for r in rows if r.mode != MODE_NONE] == want, (key, b)
            for r in rows:
                assert r.stats_off == (b * STATS_WORDS * 4 if want_stats else -1), (key, b)
                if r.mode == MODE_RGB_OVER_COLOR:
                    assert r.color == bg
                if r.mode == MODE_RGB_OVER_IMAGE:
                    assert bg_regions[r.bg_off] is bg
        assert len(p.bg_copies) == sum(isinstance(bg, np.ndarray) for bg in per_image)
        # ---- outputs: IoUs | best | float masks | outputs | counter blocks
        assert (p.stats_off is not None) == want_stats, key
        out = [(p.ious_off, p.ious_off + B * NM * 4), (p.best_off, p.best_off + B * 4)]
        for b, (H0, W0) in enumerate(PLAN_SHAPES):
            if p.planes:
                m0 = p.masks_off + p.post[b].mask_off * 4
                assert m0 % 4 == 0
                out.append((m0, m0 + p.planes * H0 * W0 * 4))
            for k in range(p.n_out):
                r = p.outd[b * p.n_out + k]
                if r.mode != MODE_NONE:
                    r0 = p.outs_off + r.out_off
                    assert r.mode != MODE_RGBA or r0 % 4 == 0, (key, b)
                    out.append((r0, r0 + H0 * W0 * (4, 3, 3, 1)[r.mode]))
            if want_stats:
                s0 = p.stats_off + p.outd[b * p.n_out].stats_off
                assert s0 % 4 == 0, (key, b)
                out.append((s0, s0 + STATS_WORDS * 4))
        assert_disjoint_inside(out, p.out_bytes, key)
        assert p.ious_off < p.best_off < p.masks_off <= p.outs_off <= (p.stats_off if want_stats else p.out_bytes), key
        # ---- tmp: NM planes of h x W0 with statistics, otherwise the planes the kernels resample
        resampled = NM if (want_stats or p.all_masks) else 1
        ends = [p.post[b + 1].tmp_off for b in range(B - 1)] + [p.tmp_bytes // 4]
        for b, (H0, W0) in enumerate(PLAN_SHAPES):
            assert p.post[b].tmp_off >= 0 and ends[b] - p.post[b].tmp_off >= resampled * p.post[b].h * W0, (key, b)
        # ---- scratch: exactly when the statistics need planes that are not all kept
        assert (p.scratch_bytes > 0) == (want_stats and not (all_masks and want_masks)), key
        if p.scratch_bytes:
            assert_disjoint_inside([(p.outd[b * p.n_out].scratch_off * 4, (p.outd[b * p.n_out].scratch_off + NM * H0 * W0) * 4)
                                    for b, (H0, W0) in enumerate(PLAN_SHAPES)], p.scratch_bytes, key)


@pytest.mark.parametrize("NM", [1, 3])
def test_plan_chunk_plain_request_has_one_rgba_row_per_image(NM):
    from s3od_amd.image_ops import reference_geometry
    geoms = [reference_geometry(h, w, PLAN_S)[0] for h, w in PLAN_SHAPES]
    p = plan_chunk(PLAN_SHAPES, geoms, NM, PLAN_S, PLAN_S, Request())
    assert p.n_out == 1 and len(p.outd) == len(PLAN_SHAPES) and all(o.mode == MODE_RGBA for o in p.outd)
    assert p.all_masks and p.planes == NM and p.stats_off is None and p.scratch_bytes == 0 and not p.bg_copies
