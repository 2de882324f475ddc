"""CPU checks of the batched inference plumbing: the ctypes descriptor mirrors against the layout
include/s3od_hip.h states (sizes and @offset comments), and the pre-flight geometry classifier."""
import ctypes
import re

import pytest

from conftest import REPO

from s3od_amd.infer_many import PostDesc, PreDesc, classify_geometry

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
