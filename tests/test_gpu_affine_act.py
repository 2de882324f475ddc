"""GPU: s3od_affine_act (BatchNorm apply + ReLU + up to two residual adds, the forward of every ResidualConvUnit in
train mode: src/s3od/model.py:334-345, 383-393), called through its entry point on a NaN-filled output and compared
per element with a float64 restatement on the CPU,

    y = act(x * scale[c] + shift[c]) + r1 + r2,    act = identity (0) or ReLU (1), r1 / r2 optional,

for every combination of act, r1 and r2 (the engine runs act = 0 with both residuals), in both dtypes.

Allowed error, from the operation count: the kernel does one fma and up to two additions in f32, and every
intermediate is at most M = |x scale| + |shift| + |r1| + |r2| in magnitude, so |got - ref| <= 3 * 2^-24 M; a bf16
output adds the one rounding of the store, 2^-8 |ref|.

Shapes (npix, C): (1, 8) one thread; (3, 8) and (257, 8) a ragged last block (256 threads of 8 channels: 257 * 8 / 8
= one block and one thread); (7, 304) C not a power of two, so the channel phase c = i % C wraps inside a block at a
different place in every row; (33, 256); (1, 2048) one pixel of the widest layer; (2049, 16) several blocks.  A quarter
of x sits on the ReLU threshold -shift/scale or one ulp of its dtype to either side, as in test_gpu_bn_relu.py.
Measured on the MI355X: worst ratio 0.66 (f32) and 0.996 (bf16, the store's rounding); with the ReLU moved after the
residual adds all 42 cases with act = 1 and a residual fail, at ratios up to 5.6e6.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

NAN = float("nan")
DT = {"f32": (torch.float32, 0, torch.int32), "bf16": (torch.bfloat16, 1, torch.int16)}
SHAPES = [(1, 8), (3, 8), (257, 8), (7, 304), (33, 256), (1, 2048), (2049, 16)]


def _inputs(dtype, npix, C):
    dt, _, bits = DT[dtype]
    gen = torch.Generator().manual_seed(npix * 4099 + C)
    sign = torch.where(torch.rand(C, generator=gen) < 0.25, -1.0, 1.0)          # BatchNorm weights may be negative
    scale = (torch.rand(C, generator=gen) + 0.5) * sign
    shift = torch.randn(C, generator=gen) * 0.3 + 0.05
    x = torch.randn(npix, C, generator=gen) * 1.7 + 0.2
    # a quarter of the elements on the threshold x = -shift/scale, rounded to the dtype, or one ulp beside it
    thr = (-shift / scale).expand(npix, C).to(dt)
    step = torch.randint(-1, 2, (npix, C), generator=gen).to(bits)
    near = (thr.contiguous().view(bits) + step).view(dt)
    x = torch.where(torch.rand(npix, C, generator=gen) < 0.25, near, x.to(dt)).contiguous()
    r1, r2 = (torch.randn(npix, C, generator=gen).to(dt) for _ in range(2))
    return x, scale, shift, r1, r2


@pytest.mark.parametrize("has_r2", [False, True], ids=["nor2", "r2"])
@pytest.mark.parametrize("has_r1", [False, True], ids=["nor1", "r1"])
@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("npix,C", SHAPES)
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_affine_act(dtype, npix, C, act, has_r1, has_r2):
    """Per element against float64 under the bound of the module docstring.  With act = 1 and no residual, y == 0
    exactly where the f32 fma(x, scale, shift) <= 0 and y > 0 elsewhere: the BatchNorm backward that recomputes its
    ReLU mask from z relies on this.  (The sign of the f32 fma is the sign of the exact x scale + shift, which float64
    holds: the product is exact in 48 bits, the sum rounds once and cannot cross zero.)  With act = 1 and residuals,
    y - r1 - r2 >= -bound everywhere: ReLU is applied before the adds, not after."""
    from s3od_amd._lib import lib, stream
    dt, code, _ = DT[dtype]
    x, scale, shift, r1, r2 = _inputs(dtype, npix, C)
    r1 = r1 if has_r1 else None
    r2 = r2 if has_r2 else None
    d = lambda t: t.double()
    pre = d(x) * d(scale) + d(shift)
    res = (d(r1) if has_r1 else 0.0) + (d(r2) if has_r2 else 0.0)
    ref = (pre.clamp_min(0) if act else pre) + res
    M = (d(x) * d(scale)).abs() + d(shift).abs() + (d(r1).abs() if has_r1 else 0.0) + (d(r2).abs() if has_r2 else 0.0)
    tol = 3 * 2.0 ** -24 * M + (2.0 ** -8 * ref.abs() if dtype == "bf16" else 0.0)
    cu = lambda t: None if t is None else t.cuda()
    y = torch.full((npix, C), NAN, device="cuda", dtype=dt)
    lib()("s3od_affine_act", code, cu(x), cu(scale), cu(shift), act, cu(r1), cu(r2), y, npix * C, C, stream())
    torch.cuda.synchronize()
    got = y.double().cpu()
    r = float(torch.nan_to_num((got - ref).abs() / tol, nan=float("inf")).max())
    print(f"\n[affine_act {dtype} npix{npix} C{C} act{act} r1 {int(has_r1)} r2 {int(has_r2)}] worst |err| / allowed {r:.3f}")
    assert torch.isfinite(got).all(), "every y element must be written"
    assert r <= 1.0, r
    if act == 1 and not has_r1 and not has_r2:
        assert torch.equal(got == 0, pre <= 0), "y == 0 exactly where fma(x, scale, shift) <= 0"
        if npix * C >= 2048:          # the threshold elements do fall on both sides
            edge = pre.abs() <= 2.0 ** -6 * d(shift).abs()
            assert int((edge & (pre <= 0)).sum()) > 0 and int((edge & (pre > 0)).sum()) > 0
    if act == 1 and (has_r1 or has_r2):
        assert bool((got - res >= -tol).all()), "ReLU must come before the residual adds"
