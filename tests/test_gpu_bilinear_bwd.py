"""GPU: s3od_bilinear_bwd (the backward of F.interpolate(bilinear, align_corners=False), src/s3od/model.py:395-403)
against torch autograd of the fp32 interpolate, on the exact-2x path (its own gather with all 16 candidate rows loaded
together) and on the generic path (a non-multiple size), odd sizes and the broadcast term included (bf16 tolerance).

test_bilinear_bwd_per_element compares every element, in both dtypes, with a float64 restatement built from the
interpolation matrices, under a bound derived from the kernel's operation count (its docstring), at the exact-2x
ratio, generic up-scales, one axis at 2x only, the identity, 1-pixel axes, large ratios and down-scales: a rel-L2
of 1e-2 over the tensor passes with a whole border row wrong."""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("B,IH,IW,OH,OW,C,bc", [(2, 16, 16, 32, 32, 64, False), (2, 15, 13, 30, 26, 32, True),
                                               (1, 7, 9, 14, 18, 16, True), (2, 12, 10, 25, 17, 32, True)])
def test_bilinear_bwd_vs_torch_autograd(B, IH, IW, OH, OW, C, bc):
    from s3od_amd._lib import lib, stream, BF16
    g = torch.Generator(device="cuda").manual_seed(IH * 100 + IW)
    dy = torch.randn(B, OH, OW, C, device="cuda", generator=g).bfloat16()
    bcast = torch.randn(B, C, device="cuda", generator=g) if bc else None
    dx = torch.full((B, IH, IW, C), float("nan"), device="cuda", dtype=torch.bfloat16)
    lib()("s3od_bilinear_bwd", BF16, dy, bcast, dx, B, IH, IW, OH, OW, C, stream())
    torch.cuda.synchronize()
    x = torch.zeros(B, C, IH, IW, device="cuda", requires_grad=True)
    y = F.interpolate(x, size=(OH, OW), mode="bilinear", align_corners=False)
    gy = dy.float().permute(0, 3, 1, 2)
    if bc:
        gy = gy + bcast[:, :, None, None]
    y.backward(gy)
    ref = x.grad.permute(0, 2, 3, 1)
    got = dx.float()
    assert torch.isfinite(got).all()
    assert float((got - ref).norm() / ref.norm()) < 1e-2


# ------------------------------------------------------------------------------------------------ per element
NAN = float("nan")
DT = {"f32": (torch.float32, 0), "bf16": (torch.bfloat16, 1)}
SHAPES = {
    "up2": [(1, 1, 2, 2), (1, 5, 2, 10), (5, 1, 10, 2), (7, 9, 14, 18), (16, 16, 32, 32)],
    "up": [(12, 10, 25, 17), (7, 9, 15, 18), (3, 4, 12, 4), (13, 11, 14, 12), (24, 24, 37, 37)],
    "one_axis_2x": [(7, 9, 14, 17)],
    "identity": [(5, 5, 5, 5)],
    "pixel_or_large": [(1, 1, 7, 5), (1, 6, 9, 6), (2, 3, 37, 41), (3, 3, 100, 7)],
    "down": [(25, 17, 12, 10), (9, 8, 3, 3), (8, 8, 4, 4), (7, 5, 1, 1)],
}


@functools.lru_cache(maxsize=None)
def interp_matrix(n_in, n_out):
    """[n_out, n_in] float64 matrix of one axis of F.interpolate(bilinear, align_corners=False):
    src = max(0, (o + .5) in/out - .5), i0 = min(int(src), in - 1), i1 = min(i0 + 1, in - 1), weights 1 - w1 and w1,
    accumulated where the clamp makes i0 == i1."""
    W = torch.zeros(n_out, n_in, dtype=torch.float64)
    for o in range(n_out):
        src = max(0.0, (o + 0.5) * n_in / n_out - 0.5)
        i0 = min(int(src), n_in - 1)
        i1 = min(i0 + 1, n_in - 1)
        w1 = src - i0
        W[o, i0] += 1.0 - w1
        W[o, i1] += w1
    return W


def _sandwich(Wy, g, Wx):
    return torch.einsum("oi,bopc,pj->bijc", Wy, g, Wx)


@pytest.mark.parametrize("bc", [False, True], ids=["nobcast", "bcast"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("C", [8, 64])
@pytest.mark.parametrize("IH,IW,OH,OW", [s for grp in SHAPES.values() for s in grp])
def test_bilinear_bwd_per_element(IH, IW, OH, OW, C, dtype, bc):
    """dx = Wy^T (dy + bcast) Wx per (b, c) in float64 (NHWC), with Wy, Wx the interpolation matrices above; the same
    test ties them to torch: float64 autograd of F.interpolate agrees to 1e-12 (of the largest |dx|, which reaches
    several hundred where 37x41 outputs fold into 2x3 inputs).

    Allowed error, from the kernel's arithmetic and not from its output.  With g = dy + bcast, mag = |Wy|^T |g| |Wx|,
    S = By^T |g| Bx for By = (Wy != 0), Bx = (Wx != 0), and n = colsum(By) (x) colsum(Bx) the number of terms the
    kernel adds into one input pixel:
        f32   |got - ref| <= 2^-24 ((n + 3) mag + S)
        bf16  that + 2^-8 |ref| (the one rounding of the store).
    n accumulating additions, and per term the rounding of g, of the product of the two weights and of the product with
    g give (n + 3) mag; S covers w0 = 1 - w1, whose rounding is absolute (2^-25), not relative to a small w0: without
    it 25x17 -> 12x10 would exceed a purely relative bound.  An emulation of the kernel's f32 arithmetic in numpy
    (same candidate ranges, visit order, both paths) over these shapes and 150 random ones stayed at <= 0.50 of the f32
    bound and visited exactly the n non-zero taps; the rest is room for FMA contraction.
    A missed tap, a dropped clamped tap (i0 == i1 at the border) or a weight taken from the wrong axis shows as a
    ratio in the millions: with bil_weight_on keeping only its a0 term 144 of these cases fail (3.3e6 at
    25x17 -> 12x10).  The candidate range itself has room to spare: the outputs that reach row iy are the o < B,
    B = (iy + 1.5) / sy - 0.5, so oy_hi = ceil(B) already covers them and the kernel's ceil(B) + 1 is margin; the
    range first loses a tap at ceil(B) - 2, and then 104 cases fail (3.4e6 at 7x5 -> 1x1)."""
    from s3od_amd._lib import lib, stream
    dt, code = DT[dtype]
    B = 2
    torch.manual_seed(((IH * 101 + IW) * 103 + OH) * 107 + OW + C + bc)
    dy = torch.randn(B, OH, OW, C).to(dt)
    bcast = torch.randn(B, C) if bc else None
    Wy, Wx = interp_matrix(IH, OH), interp_matrix(IW, OW)
    g = dy.double() + (bcast.double()[:, None, None, :] if bc else 0.0)
    ref = _sandwich(Wy, g, Wx)
    # the matrices are torch's: float64 autograd of the interpolation gives the same gradient
    x = torch.zeros(B, C, IH, IW, dtype=torch.float64, requires_grad=True)
    F.interpolate(x, size=(OH, OW), mode="bilinear", align_corners=False).backward(g.permute(0, 3, 1, 2))
    assert float((x.grad.permute(0, 2, 3, 1) - ref).abs().max()) <= 1e-12 * max(1.0, float(ref.abs().max()))
    By, Bx = (Wy != 0).double(), (Wx != 0).double()
    n = (By.sum(0)[:, None] * Bx.sum(0)[None, :])[None, :, :, None]
    tol = 2.0 ** -24 * ((n + 3) * _sandwich(Wy.abs(), g.abs(), Wx.abs()) + _sandwich(By, g.abs(), Bx))
    if dtype == "bf16":
        tol = tol + 2.0 ** -8 * ref.abs()
    dx = torch.full((B, IH, IW, C), NAN, device="cuda", dtype=dt)
    lib()("s3od_bilinear_bwd", code, dy.cuda(), bcast.cuda() if bc else None, dx, B, IH, IW, OH, OW, C, stream())
    torch.cuda.synchronize()
    got = dx.double().cpu()
    err = (got - ref).abs()
    # an input pixel that no output reaches (down-scales) has ref = 0 and bound 0: it must hold an exact zero
    r = float(torch.nan_to_num(torch.where(tol > 0, err / tol, torch.where(err == 0, 0.0, float("inf"))), nan=float("inf")).max())
    path = "up2" if (OH, OW) == (2 * IH, 2 * IW) else "generic"
    print(f"\n[bilinear_bwd {path} {dtype} C{C} {IH}x{IW}->{OH}x{OW} {'bcast' if bc else 'nobcast'}] "
          f"n <= {int(n.max())}  worst |err| / allowed {r:.3f}")
    assert torch.isfinite(got).all(), "every dx element must be written"
    assert r <= 1.0, r
