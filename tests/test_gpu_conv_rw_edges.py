"""GPU: the persistent register-weight conv kernels of csrc/gemm_ops.hip -- conv3x3_c64_rw_kernel (forward, the masked
data gradient, the fused mask heads), convT4s2_rw_kernel and conv4s2_rw_kernel -- per element against a float64
reference of the same bf16 operands, through the C entry points, in two data modes (tests/_gemm_ref.py):

  exact    integer operands ({-1, 0, 1} activations, 1/8-dense {-1, 0, 1} weights, small-integer biases / w2 / b2): every
           partial sum is an integer below 2^24 and every bf16 output is at most 256 (asserted on the reference), so the
           kernel must EQUAL the reference whatever its summation order.  One wrong halo pixel is a mismatch.
  random   randn operands at the scales of test_gpu_conv_halo.py, judged by ref_conv / finish / check: finite from
           NaN-prefilled outputs, |err| / cap <= 1, at most 1 % ReLU-kink skips; the f32 logits also against the
           sequential-f32 emulation where that is affordable (the one-tile classes; printed where skipped).

These kernels launch nwg = min(max(T, 8), CUs) workgroups over T tiles; XCD x owns the tile range [T x / 8, T (x + 1) / 8)
and its workgroups stride through it with a 3-deep LDS-DMA ring issued two tiles ahead.  The shapes are derived from the
device's CU count C so that every class of the schedule runs:

  partial  T = 1, an image smaller than a tile          dummy pieces only, 7 workgroups with empty ranges
  whole    T = 1, exactly one tile                      no partial edges
  few      2 <= T <= 7                                  nwg = 8 > T: XCD ranges of 0 and 1 tiles
  uneven   8 < T <= C, T % 8 != 0                       unequal XCD ranges (an XCD with fewer workgroups than tiles)
  ring2    T ~ 1.5 C                                    first reuse of a ring slot
  ring3    T ~ 2.5 C                                    ring full, wrap-around
  ring5    T ~ 4.5 C                                    steady state, every workgroup >= 4 tiles

The ring classes use B = 3 images of 5 x ty tiles, ragged at the right and bottom, with an image boundary strictly
inside some workgroup's tile sequence (asserted from a restatement of the schedule: the buffer descriptor is rebased
there).  Every case asserts from a restatement of the host predicate which kernel its shape selects, gives poisoned
inputs (a read outside an image that the buffer range check does not zero turns the output NaN) and NaN-prefilled
outputs with guard rows, and runs once more with the path's knob off: the implicit GEMM must meet the same check.

ring2 / ring3 / ring5 of the 64 -> 64 forward subsume test_gpu_conv_halo.py::test_conv_fwd_64_relu and the forward part
of test_rw_grouped_epilogue_bit_identical (whose largest case, 45 tiles, is one tile per workgroup on 256 CUs)."""
import os

import pytest
import torch

import _gemm_ref as R

pytestmark = pytest.mark.gpu
BF16 = 1
CLASSES = ["partial", "whole", "few", "uneven", "ring2", "ring3", "ring5"]
RINGS = {"ring2": 1.5, "ring3": 2.5, "ring5": 4.5}


def _lib():
    from s3od_amd._lib import lib, stream
    return lib(), stream()


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def shape_of(cls, TH, TW):
    """(B, H, W) in tile-grid pixels for a class, from the device's CU count"""
    C = _cus()
    if cls == "partial":
        return 1, 3, 5
    if cls == "whole":
        return 1, TH, TW
    if cls == "few":
        return 2, 3 * TH - 3, TW - 9                       # 2 x 1 x 3 = 6 tiles
    if cls == "uneven":
        B, tx = 2, 3
        ty = C // (B * tx)
        while (B * tx * ty) % 8 == 0 or ty in (B, tx):
            ty -= 1
        assert B * tx * ty > 8
        return B, TH * ty - 3, (tx - 1) * TW + 7
    B, tx = 3, 5
    ty = max(4, round(RINGS[cls] * C / (B * tx)))
    while ty in (B, tx):
        ty += 1
    return B, TH * ty - 3, (tx - 1) * TW + 7


def check_class(cls, B, H, W, TH, TW):
    """the class's claims about the schedule, from a restatement of the kernels' tile split"""
    C = _cus()
    tx, ty = -(-W // TW), -(-H // TH)
    T = B * tx * ty
    sched = R.rw_schedule(T, C)
    per = [len(s) for s in sched]
    assert sorted(t for s in sched for t in s) == list(range(T))
    if cls in ("partial", "whole"):
        assert T == 1 and len(sched) == 8 and sorted(per) == [0] * 7 + [1]
        assert (H < TH and W < TW) if cls == "partial" else (H == TH and W == TW)
    elif cls == "few":
        assert 2 <= T <= 7 and len(sched) == 8 and set(per) == {0, 1}
    elif cls == "uneven":
        assert 8 < T <= C and T % 8 and len({T * (x + 1) // 8 - T * x // 8 for x in range(8)}) == 2 and max(per) <= 2
    else:
        assert len({B, tx, ty}) == 3 and B >= 2 and tx >= 2 and ty >= 3 and H % TH and W % TW
        assert R.crosses_image(sched, tx * ty), "no workgroup's tiles span an image boundary"
        lo = {"ring2": (1, 2), "ring3": (2, 3), "ring5": (4, 5)}[cls]
        assert lo[0] <= min(per) and max(per) <= lo[1] + 1 and max(per) >= lo[1], (cls, min(per), max(per))
    return T


class knob:
    """an S3OD_* dispatch knob for the calls inside (read per call under S3OD_AB=1, tests/conftest.py)"""

    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        os.environ.update(self.kv)

    def __exit__(self, *a):
        for k in self.kv:
            os.environ.pop(k, None)


def rw_ok(B, H, W, off=False):                 # gemm_ops.hip rw_ok (bf16)
    return not off and H * W * 192 < 2 ** 31 and B > 0


def convt_rw_ok(B, H, W, off=False):           # gemm_ops.hip convt_rw_ok (bf16)
    return not off and B > 0 and 4 * H * W * 128 < 2 ** 31


def _acts(mode, shape, seed):
    """NHWC bf16 activations in a poisoned buffer: NaN for more than a row of pixels before and after, so a halo row
    read above the first or below the last image that the buffer range check does not zero is NaN"""
    if mode == "exact":
        v = R.ints(shape, seed)
    else:
        v = torch.randn(shape, device=R.DEVICE, generator=torch.Generator(device=R.DEVICE).manual_seed(seed)).bfloat16()
    return R.poisoned_from(v, slack=shape[2] + 8)


def _weights(mode, shape, seed, scale):
    """conv-view weights [Cout, Cin, KH, KW], bf16"""
    if mode == "exact":
        return R.ints(shape, seed, 0.125)
    return (torch.randn(shape, device=R.DEVICE, generator=torch.Generator(device=R.DEVICE).manual_seed(seed)) * scale).bfloat16()


def _vec(mode, n, seed, scale, lo=-3, hi=3):
    if mode == "exact":
        return R.poisoned_from(R.small_ints((n,), seed, lo, hi))
    return R.poisoned_from(torch.randn(n, device=R.DEVICE, generator=torch.Generator(device=R.DEVICE).manual_seed(seed)) * scale)


def _nchw64(t):
    return R.wide(t, R.DEVICE).permute(0, 3, 1, 2)


def _rows64(t):
    return R.wide(t, R.DEVICE).reshape(-1, t.shape[-1])


def _judge(mode, got, ref, t, skip, label, emu=None):
    if mode == "exact":
        R.check_exact(got, ref, label)
    else:
        R.check(got, ref, t, emu, skip, label=label)
    assert R.guards_intact(got), f"{label}: a guard row was written"


def _colsum_judge(mode, cs, r, cs0, label):
    ref, t = R.colsum_ref(r, R.wide(cs0, R.DEVICE))
    if mode == "exact":
        R.assert_exact_domain([r.out.abs().sum(0) + R.wide(cs0, R.DEVICE).abs()])
    _judge(mode, cs, ref, t, None, label)


# ------------------------------------------------------------------------------------------------ 3x3 64 -> 64 forward
@pytest.mark.parametrize("mode", ["exact", "random"])
@pytest.mark.parametrize("cls", CLASSES)
def test_conv3x3_rw_fwd(cls, mode):
    """s3od_conv_fwd bf16 64 -> 64 3x3 s1: ReLU / none x bias / null bias, each on the grouped epilogue (S3OD_RW_GB
    default 2), on S3OD_RW_GB=0 (bit-identical to the grouped one in both modes: the same MFMA chain per accumulator)
    and on the implicit GEMM (S3OD_CONV_RW=0)."""
    L, st = _lib()
    B, H, W = shape_of(cls, 8, 32)
    T = check_class(cls, B, H, W, 8, 32)
    assert rw_ok(B, H, W) and not rw_ok(B, H, W, off=True)
    x = _acts(mode, (B, H, W, 64), 11)
    w = _weights(mode, (64, 64, 3, 3), 12, 0.06)
    bias = _vec(mode, 64, 13, 0.1)
    wp = R.poisoned_from(w.permute(0, 2, 3, 1).contiguous())
    x64, w64 = _nchw64(x), R.wide(w, R.DEVICE)
    for act in (R.ACT_RELU, R.ACT_NONE):
        for bv in (bias, None):
            r = R.ref_conv("fwd", x64, w64, stride=1, pad=1, dtype="bf16", bias=R.wide(bv, R.DEVICE), act=act)
            if mode == "exact":
                R.assert_exact_domain([r.S + (0 if bv is None else R.wide(bv, R.DEVICE).abs())], [r.out])
            outs = {}
            for name, kv in (("gb2", {}), ("gb0", {"S3OD_RW_GB": "0"}), ("igemm", {"S3OD_CONV_RW": "0"})):
                out = R.poisoned((B, H, W, 64), None, torch.bfloat16)
                with knob(**kv):
                    L("s3od_conv_fwd", BF16, B, H, W, 64, H, W, 64, 3, 3, 1, 1, x, 0, wp, bv, None, None, act, None, None, out,
                      None, None, None, st)
                    torch.cuda.synchronize()
                _judge(mode, out.view(-1, 64), r.out, r.t_out, r.skip,
                       f"rw fwd {cls} T={T} {B}x{H}x{W} act{act} bias{int(bv is not None)} {name} {mode}")
                outs[name] = out
            assert torch.equal(outs["gb2"], outs["gb0"]), "grouped and ungrouped epilogue differ"


# ------------------------------------------------------------------------------------------------ masked data gradient
@pytest.mark.parametrize("mode", ["exact", "random"])
@pytest.mark.parametrize("cout", [64, 96])
@pytest.mark.parametrize("cls", ["few", "uneven", "ring3", "ring5"])
def test_conv3x3_rw_dgrad_masked(cls, cout, mode):
    """s3od_conv_dgrad with wT, ACT_RELU_BWD and res1 (kernel mode 1): dy has 64 channels (8 x 32 tiles) or the mask
    heads' 96 (8 x 16 tiles); column sums null and added onto a non-zero start; S3OD_CONV_RW=0 is the per-class
    implicit GEMM."""
    L, st = _lib()
    TW = 32 if cout == 64 else 16
    B, H, W = shape_of(cls, 8, TW)
    T = check_class(cls, B, H, W, 8, TW)
    assert rw_ok(B, H, W)
    dy = _acts(mode, (B, H, W, cout), 21 + cout)
    res1 = _acts(mode, (B, H, W, 64), 22 + cout)
    w = _weights(mode, (cout, 64, 3, 3), 23 + cout, 0.06)
    wp = R.poisoned_from(w.permute(0, 2, 3, 1).contiguous())
    wT = R.poisoned_from(w.flip(2, 3).permute(1, 2, 3, 0).contiguous())
    cs0 = _vec(mode, 64, 24, 1.0)
    r = R.ref_conv("dgrad", None, R.wide(w, R.DEVICE), dy=_nchw64(dy), stride=1, pad=1, hw=(H, W), dtype="bf16",
                   act=R.ACT_RELU_BWD, res1=_rows64(res1))
    if mode == "exact":
        R.assert_exact_domain([r.S], [r.out])
    for name, kv in (("rw", {}), ("igemm", {"S3OD_CONV_RW": "0"})):
        for with_cs in (False, True):
            dx = R.poisoned((B, H, W, 64), None, torch.bfloat16)
            cs = R.poisoned_from(cs0.clone()) if with_cs else None
            with knob(**kv):
                L("s3od_conv_dgrad", BF16, B, H, W, 64, H, W, cout, 3, 3, 1, 1, dy, wp, None, None, None, R.ACT_RELU_BWD, res1,
                  None, dx, None, None, cs, wT, st)
                torch.cuda.synchronize()
            label = f"rw dgrad {cls} T={T} {B}x{H}x{W} {cout}->64 {name} cs{int(with_cs)} {mode}"
            _judge(mode, dx.view(-1, 64), r.out, r.t_out, r.skip, label)
            if with_cs:
                _colsum_judge(mode, cs, r, cs0, label + " colsum")


# ------------------------------------------------------------------------------------------------ fused mask heads
def _heads_emu(x, w1, b1, w2, b2):
    """sequential-f32 emulation of the logits: the conv as a k-ordered f32 chain, then the head sums in f32"""
    B, _, H, W = x.shape
    acc = R.chain(R.conv_cols(x.cpu(), 3, 3, 1, 1), w1.cpu().permute(2, 3, 1, 0).reshape(-1, w1.shape[0]))
    h = (acc + b1.cpu().float()).clamp_min(0).view(B, H, W, 3, 32)
    lg = b2.cpu().float().expand(B, H, W, 3).clone()
    for j in range(32):
        lg = lg + h[..., j] * w2.cpu().float()[:, j]
    return lg.permute(0, 3, 1, 2)


@pytest.mark.parametrize("mode", ["exact", "random"])
@pytest.mark.parametrize("cls", ["partial", "uneven", "ring3", "ring5"])
def test_mask_heads_rw(cls, mode):
    """s3od_mask_heads_fwd, NM = 3 (kernel mode 3): hsave given and null; f32 logits against the cap of
    _gemm_ref.ref_heads (random |w2|, |b2| ~ 1: head 1's odd-wave partial, ~16 terms of h w2, is far above it) or equal
    (exact); S3OD_CONV_RW=0 is the implicit GEMM with the EpiHeads epilogue."""
    L, st = _lib()
    B, H, W = shape_of(cls, 8, 32)
    T = check_class(cls, B, H, W, 8, 32)
    assert rw_ok(B, H, W) and 3 * H * W * 4 < 2 ** 31
    feat = _acts(mode, (B, H, W, 64), 31)
    w1 = _weights(mode, (96, 64, 3, 3), 32, 0.06)
    b1 = _vec(mode, 96, 33, 0.1)
    w2 = _vec(mode, 96, 34, 1.0, -2, 2).view(3, 32)
    b2 = _vec(mode, 3, 35, 1.0)
    w1p = R.poisoned_from(w1.permute(0, 2, 3, 1).contiguous())
    dev = lambda t: R.wide(t, R.DEVICE)
    rh, logit, t = R.ref_heads(_nchw64(feat), dev(w1), dev(b1), dev(w2), dev(b2))
    if mode == "exact":
        R.assert_exact_domain([rh.S + dev(b1).abs(), (rh.out.view(-1, 3, 32) * dev(w2)).abs().sum(-1) + dev(b2).abs()], [rh.out])
    emu = None
    if mode == "random":
        if B * H * W * 96 * 576 <= 2e9:
            emu = _heads_emu(_nchw64(feat), dev(w1), dev(b1), dev(w2), dev(b2))
        else:
            print(f"[heads {cls}] emulation skipped ({B * H * W} pixels x 96 x 576); the exact mode carries this case")
    for name, kv in (("rw", {}), ("igemm", {"S3OD_CONV_RW": "0"})):
        for with_h in (True, False):
            logits = R.poisoned((B, 3, H, W), None, torch.float32)
            hsave = R.poisoned((B * H * W, 96), None, torch.bfloat16) if with_h else None
            with knob(**kv):
                L("s3od_mask_heads_fwd", BF16, B, H, W, 3, feat, w1p, b1, w2, b2, logits, hsave, st)
                torch.cuda.synchronize()
            label = f"heads {cls} T={T} {B}x{H}x{W} {name} hsave{int(with_h)} {mode}"
            _judge(mode, logits, logit, t, None, label + " logits", emu)
            if with_h:
                _judge(mode, hsave, rh.out, rh.t_out, rh.skip, label + " hsave")


# ------------------------------------------------------------------------------------------------ ConvTranspose 4x4 s2
@pytest.mark.parametrize("mode", ["exact", "random"])
@pytest.mark.parametrize("cls", CLASSES)
def test_convT4s2_rw(cls, mode):
    """ConvTranspose2d(128, 64, 4, 2, 1) + bias (+ ReLU) through s3od_conv_dgrad with the un-flipped wT
    (convT4s2_rw_kernel, tiles of 8 x 16 INPUT pixels; the ragged classes have odd input sizes); S3OD_CONVT_RW=0 is one
    implicit GEMM per output parity class."""
    L, st = _lib()
    B, H, W = shape_of(cls, 8, 16)
    T = check_class(cls, B, H, W, 8, 16)
    assert convt_rw_ok(B, H, W)
    x = _acts(mode, (B, H, W, 128), 41)
    w = _weights(mode, (128, 64, 4, 4), 42, 0.03)                  # ConvTranspose weight = the conv view [128][64][4][4]
    bias = _vec(mode, 64, 43, 0.1)
    wp = R.poisoned_from(w.permute(0, 2, 3, 1).contiguous())
    wT = R.poisoned_from(w.permute(1, 2, 3, 0).contiguous())
    x64, w64 = _nchw64(x), R.wide(w, R.DEVICE)
    for act in (R.ACT_RELU, R.ACT_NONE):
        r = R.ref_conv("dgrad", None, w64, dy=x64, stride=2, pad=1, hw=(2 * H, 2 * W), dtype="bf16", bias=R.wide(bias, R.DEVICE),
                       act=act)
        if mode == "exact":
            R.assert_exact_domain([r.S + R.wide(bias, R.DEVICE).abs()], [r.out])
        for name, kv in (("rw", {}), ("igemm", {"S3OD_CONVT_RW": "0"})):
            out = R.poisoned((B, 2 * H, 2 * W, 64), None, torch.bfloat16)
            with knob(**kv):
                L("s3od_conv_dgrad", BF16, B, 2 * H, 2 * W, 64, H, W, 128, 4, 4, 2, 1, x, wp, bias, None, None, act, None, None,
                  out, None, None, None, wT, st)
                torch.cuda.synchronize()
            _judge(mode, out.view(-1, 64), r.out, r.t_out, r.skip, f"convT {cls} T={T} {B}x{H}x{W} act{act} {name} {mode}")


# ------------------------------------------------------------------------------------------------ conv 4x4 s2 + colsum
@pytest.mark.parametrize("mode", ["exact", "random"])
@pytest.mark.parametrize("cls", CLASSES)
def test_conv4s2_rw(cls, mode):
    """Conv2d(64, 128, 4, 2, 1) of a 2 OH x 2 OW map with the column sums added onto a non-zero start, through
    s3od_conv_fwd (conv4s2_rw_kernel, tiles of 4 x 16 OUTPUT pixels; the ragged classes have odd output sizes);
    S3OD_CONVT_RW=0 is the implicit GEMM."""
    L, st = _lib()
    B, OH, OW = shape_of(cls, 4, 16)
    T = check_class(cls, B, OH, OW, 4, 16)
    assert convt_rw_ok(B, OH, OW)
    x = _acts(mode, (B, 2 * OH, 2 * OW, 64), 51)
    w = _weights(mode, (128, 64, 4, 4), 52, 0.03)
    wp = R.poisoned_from(w.permute(0, 2, 3, 1).contiguous())
    cs0 = _vec(mode, 128, 53, 1.0)
    r = R.ref_conv("fwd", _nchw64(x), R.wide(w, R.DEVICE), stride=2, pad=1, dtype="bf16")
    if mode == "exact":
        R.assert_exact_domain([r.S], [r.out])
    for name, kv in (("rw", {}), ("igemm", {"S3OD_CONVT_RW": "0"})):
        out = R.poisoned((B, OH, OW, 128), None, torch.bfloat16)
        cs = R.poisoned_from(cs0.clone())
        with knob(**kv):
            L("s3od_conv_fwd", BF16, B, 2 * OH, 2 * OW, 64, OH, OW, 128, 4, 4, 2, 1, x, 0, wp, None, None, None, R.ACT_NONE, None,
              None, out, None, None, cs, st)
            torch.cuda.synchronize()
        label = f"conv4s2 {cls} T={T} {B}x{OH}x{OW} {name} {mode}"
        _judge(mode, out.view(-1, 128), r.out, r.t_out, r.skip, label)
        _colsum_judge(mode, cs, r, cs0, label + " colsum")
