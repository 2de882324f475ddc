"""CPU checks of the compositing / mask-statistics surface: the alias module, RemovalResult's construction, the header
and library symbols of the new entries, the S3odOutDesc mirror, MaskStats decoding, background-argument normalisation
and the register audit of the new kernels (read from build/image_ops.o as test_kernel_resources_cpu.py reads its own)."""
import ctypes
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest
from PIL import Image

from conftest import REPO

NEW_ENTRIES = ("s3od_compose", "s3od_mask_stats", "s3od_postprocess_batch_out")


def test_visualizer_alias_imports():
    import s3od.visualizer as v
    import s3od_amd.visualizer as va
    assert v.visualize_removal is va.visualize_removal and v.visualize_all_masks is va.visualize_all_masks
    from s3od.visualizer import visualize_removal, visualize_all_masks  # noqa: F401  (the demo's import)
    import inspect
    sig = inspect.signature(visualize_removal)
    assert list(sig.parameters) == ["image", "result", "background_color"]
    assert sig.parameters["background_color"].default == (0, 255, 0)
    assert list(inspect.signature(visualize_all_masks).parameters) == ["image", "result"]


def test_removal_result_positional_construction():
    from s3od import RemovalResult
    a, b, c, d = np.zeros((2, 2)), np.zeros((3, 2, 2)), np.zeros(3), Image.new("RGBA", (2, 2))
    r = RemovalResult(a, b, c, d)
    assert r.predicted_mask is a and r.all_masks is b and r.all_ious is c and r.rgba_image is d
    assert r.composite is None and r.stats is None
    r = RemovalResult(a, b, c, d, "comp", "stats")
    assert r.composite == "comp" and r.stats == "stats"


def test_api_signatures():
    import inspect
    from s3od import BackgroundRemoval
    one = inspect.signature(BackgroundRemoval.remove_background).parameters
    assert list(one)[:3] == ["self", "image", "threshold"] and one["threshold"].default == 0.5
    assert one["background"].kind is inspect.Parameter.KEYWORD_ONLY and one["background"].default is None
    assert one["stats"].kind is inspect.Parameter.KEYWORD_ONLY and one["stats"].default is False
    many = inspect.signature(BackgroundRemoval.remove_background_many).parameters
    assert list(many)[:5] == ["self", "images", "threshold", "batch_size", "return_all_masks"]
    assert (many["background"].default, many["stats"].default, many["return_masks"].default, many["return_rgba"].default) == \
        (None, False, True, True)


def test_header_declares_new_entries_and_abi_stays_2():
    text = (REPO / "include" / "s3od_hip.h").read_text()
    for fn in NEW_ENTRIES:
        assert re.search(r"^int %s\(" % fn, text, re.M), fn
    from s3od_amd._lib import parse_header
    decls = parse_header()
    assert decls["s3od_compose"][1] == ["float*", "void*", "int", "int", "int", "int", "void*", "void*", "long", "void*"]
    assert decls["s3od_mask_stats"][1] == ["float*", "int", "int", "int", "int", "float", "void*", "void*"]
    # the old entry keeps its signature
    assert len(decls["s3od_postprocess_batch"][1]) == 14 and len(decls["s3od_postprocess_batch_out"][1]) == 20
    src = (REPO / "s3od_amd" / "csrc" / "runtime.hip").read_text()
    m = re.search(r"s3od_abi_version\((?:void)?\)\s*\{\s*return (\d+);", src)
    assert m and int(m.group(1)) == 2


def test_library_exports_new_entries():
    lib = REPO / "s3od_amd" / "libs3od_hip.so"
    if not lib.exists():
        pytest.skip("libs3od_hip.so absent: run make (or __graft_entry__.build()) first")
    syms = subprocess.run(["nm", "-D", "--defined-only", str(lib)], check=True, capture_output=True, text=True).stdout
    for fn in NEW_ENTRIES + ("s3od_postprocess_batch",):
        assert re.search(r" T %s$" % fn, syms, re.M), fn


def test_out_descriptor_mirrors_header():
    from test_infer_many_cpu import header_struct
    from s3od_amd.infer_many import OutDesc
    size, fields = header_struct("S3odOutDesc")
    assert ctypes.sizeof(OutDesc) == size == 40
    assert [f for f, _ in OutDesc._fields_] == [f for f, _, _ in fields]
    for (fname, ctype), (_, htype, off) in zip(OutDesc._fields_, fields):
        assert ctype is htype and getattr(OutDesc, fname).offset == off, fname
    assert ctypes.sizeof(OutDesc * 3) == 3 * size


# ---------------------------------------------------------------------------------- background arguments
def test_background_colour():
    from s3od_amd.infer_many import normalize_background, normalize_backgrounds, pack_color
    assert pack_color((1, 2, 3)) == 1 | 2 << 8 | 3 << 16
    assert normalize_background((255, 255, 255), (4, 5)) == 0xFFFFFF
    assert normalize_background([0, 255, 0], (4, 5)) == 0x00FF00
    assert normalize_background(None, (4, 5)) is None
    assert normalize_backgrounds((9, 8, 7), [(4, 5), (2, 2)]) == [9 | 8 << 8 | 7 << 16] * 2
    assert normalize_backgrounds(None, [(4, 5), (2, 2)]) == [None, None]
    for bad in [(1, 2), (1, 2, 256), (-1, 0, 0), (0.5, 0, 0), "red", 7]:
        with pytest.raises(ValueError):
            normalize_background(bad, (4, 5))


def test_background_list_and_wrong_length():
    from s3od_amd.infer_many import normalize_backgrounds
    shapes = [(4, 5), (2, 3), (6, 6), (1, 1)]
    img = np.full((2, 3, 3), 7, np.uint8)
    out = normalize_backgrounds([(1, 2, 3), img, None, Image.new("RGB", (1, 1), (4, 5, 6))], shapes)
    assert out[0] == 1 | 2 << 8 | 3 << 16 and out[2] is None
    assert np.array_equal(out[1], img) and out[1].flags.c_contiguous
    assert np.array_equal(out[3], np.array([[[4, 5, 6]]], np.uint8))
    with pytest.raises(ValueError, match="3 values for 4 images"):
        normalize_backgrounds([None, None, None], shapes)
    # three per-image colours for three images are not one colour
    assert normalize_backgrounds([(1, 1, 1), (2, 2, 2), (3, 3, 3)], shapes[:3]) == [0x010101, 0x020202, 0x030303]


def test_background_wrong_dtype_and_size():
    from s3od_amd.infer_many import normalize_background, normalize_backgrounds
    with pytest.raises(ValueError, match="uint8"):
        normalize_background(np.zeros((4, 5, 3), np.float32), (4, 5))
    with pytest.raises(ValueError, match="4 x 5 x 3"):
        normalize_background(np.zeros((5, 4, 3), np.uint8), (4, 5))
    with pytest.raises(ValueError):
        normalize_background(np.zeros((4, 5), np.uint8), (4, 5))
    with pytest.raises(ValueError, match="image 1"):
        normalize_backgrounds(np.zeros((4, 5, 3), np.uint8), [(4, 5), (4, 6)])
    # a strided view is made contiguous
    v = np.zeros((4, 10, 3), np.uint8)[:, ::2]
    assert normalize_background(v, (4, 5)).flags.c_contiguous


# ---------------------------------------------------------------------------------- MaskStats
def demo_is_ambiguous(all_masks, threshold=0.8):
    """demo/app.py:38-56 restated."""
    for i in range(len(all_masks)):
        for j in range(i + 1, len(all_masks)):
            inter = np.logical_and(all_masks[i] > 0.5, all_masks[j] > 0.5).sum()
            union = np.logical_or(all_masks[i] > 0.5, all_masks[j] > 0.5).sum()
            if inter / (union + 1e-6) < threshold:
                return True
    return False


def test_mask_stats_decoding():
    from s3od_amd.compose import MaskStats
    words = np.zeros(72, np.uint32)
    # slots of the pairs (0,1), (0,2), (1,2) among the 28 pairs of 8 planes: 0, 1, 7
    words[[0, 1, 7]] = [10, 20, 30]
    words[[28, 29, 35]] = [40, 20, 4000000000]
    words[56:59] = [25, 25, 35]                                   # the planes' own counts: the diagonals
    words[64:69] = [5, 1, 2, 3, 4]
    s = MaskStats.from_words(words, 3)
    assert s.pair_inter.dtype.kind == "i" and s.pair_inter.shape == s.pair_union.shape == s.pair_ious.shape == (3, 3)
    assert s.pair_inter[0, 1] == s.pair_inter[1, 0] == 10 and s.pair_inter[0, 2] == 20 and s.pair_inter[1, 2] == 30
    assert s.pair_union[1, 2] == 4000000000 and s.pair_ious.dtype == np.float64
    assert s.pair_ious[0, 1] == 10 / (40 + 1e-6) and s.pair_ious[0, 2] == 20 / (20 + 1e-6)
    assert s.area == 5 and s.bbox == (1, 2, 3, 4)
    assert list(np.diag(s.pair_inter)) == list(np.diag(s.pair_union)) == [25, 25, 35]
    assert s.is_ambiguous() and s.is_ambiguous(0.8) and not s.is_ambiguous(1e-9)
    words[64] = 0
    words[65:69] = [0x7FFFFFFF, 0x7FFFFFFF, 0, 0]
    e = MaskStats.from_words(words, 3)
    assert e.area == 0 and e.bbox is None
    z = MaskStats.from_words(np.zeros(72, np.uint32), 3)
    assert z.pair_ious[0, 1] == 0.0 and z.is_ambiguous()          # union 0 -> IoU 0 < 0.8, as in the demo
    assert not MaskStats.from_words(np.zeros(72, np.uint32), 1).is_ambiguous()
    assert demo_is_ambiguous(np.zeros((3, 2, 2), np.float32)) and not demo_is_ambiguous(np.zeros((1, 2, 2), np.float32))


def test_nothing_requested_raises_before_any_gpu_work():
    from s3od import BackgroundRemoval
    br = BackgroundRemoval.__new__(BackgroundRemoval)         # no model, no device: the check comes first
    with pytest.raises(ValueError, match="nothing requested"):
        br.remove_background_many([np.zeros((4, 4, 3), np.uint8)], return_masks=False, return_rgba=False)


def test_non_uint8_image_raises_before_any_gpu_work():
    from s3od import BackgroundRemoval
    br = BackgroundRemoval.__new__(BackgroundRemoval)         # no model, no device: the check comes first
    for dtype in (np.float32, np.float64, np.int32):
        with pytest.raises(TypeError, match="uint8"):
            br.remove_background(np.zeros((4, 4, 3), dtype))


# ---------------------------------------------------------------------------------- kernel resources
def test_new_kernels_have_no_private_segment_and_no_spills(tmp_path):
    from test_kernel_resources_cpu import LLVM, TOOLS
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
    want = ["compose_kernel", "mask_stats_kernel", "mask_stats_batch_kernel", "stats_init_kernel", "stats_init_batch_kernel",
            "post_tile_kernel", "post_v_batch_kernel"]
    for k in want:
        hits = [v for n, v in found.items() if re.search(r"\d%s[A-Z]" % k, n)]
        assert hits, f"{k} not in the build"
        for v in hits:
            assert v == {"private_segment_fixed_size": 0, "sgpr_spill_count": 0, "vgpr_spill_count": 0}, (k, v)
