"""GPU: BatchNorm2d + ReLU backward with the ReLU mask recomputed from z (s3od_bn_relu_bwd) is
bit-identical to the backward that reads the stored activation y = relu(bn(z)) (s3od_bn_bwd with
y_relu), for both dtypes, on a ragged pixel count and with z placed so that many y sit at or next
to the ReLU threshold.  The forward y comes from s3od_affine_act, as in the engine's train-mode
ResidualConvUnit (src/s3od/model.py:334-345).  Also checked against a float64 restatement of
the BatchNorm backward computed on the CPU from the same inputs (rel-L2 <= 1e-5 f32 / 1e-2 bf16).

The kernels split a 256-thread block into C/8 column groups x rows = 256/(C/8) row phases, read
pixels in batches of 4 * rows and reduce the row phases in LDS, so the shapes below are the ones at
which that decomposition changes: one group (C = 8) to 256 groups of one phase (C = 2048, the largest
C the entry admits), fewer pixels than phases, exactly one batch plus a one-row tail.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _lib():
    from s3od_amd._lib import lib, stream
    return lib(), stream()


def _rel(got, ref):
    """rel-L2; against an all-zero reference the error itself has to meet the bound"""
    den = float(ref.norm())
    err = float((got.double().cpu() - ref).norm())
    return err / den if den > 0 else err


def _case(dtype, C, npix):
    L, st = _lib()
    torch.manual_seed(7)
    dt, code = (torch.float32, 0) if dtype == "f32" else (torch.bfloat16, 1)
    dev = "cuda"
    w = torch.rand(C, device=dev) + 0.5
    b = torch.randn(C, device=dev) * 0.3
    zf = torch.randn(npix, C, device=dev) * 1.7 + 0.2
    mean = zf.mean(0)
    var = zf.var(0, unbiased=False)
    rstd = (var + 1e-5).rsqrt()
    scale = (w * rstd).contiguous()
    shift = (b - mean * w * rstd).contiguous()
    # a quarter of the rows sit exactly on (or one ulp around) the ReLU threshold z = -shift/scale
    thr = -shift / scale
    zf[: npix // 4] = thr + torch.randint(-1, 2, (npix // 4, C), device=dev).float() * thr.abs() * 2 ** -20
    z = zf.to(dt).contiguous()
    y = torch.empty_like(z)
    L("s3od_affine_act", code, z, scale, shift, 1, None, None, y, y.numel(), C, st)
    dy = torch.randn(npix, C, device=dev).to(dt)

    outs = {}
    for with_dcb in (True, False):
        for mode in ("stored", "recompute"):
            sums = torch.zeros(32 * 3 * C, dtype=torch.float64, device=dev)     # all zero on entry, left all zero
            dz = torch.empty_like(z)
            dw, db = (torch.zeros(C, device=dev) for _ in range(2))
            dcb = torch.zeros(C, device=dev) if with_dcb else None
            if mode == "stored":
                L("s3od_bn_bwd", code, dy, z, y, mean, rstd, w, sums, dz, dw, db, dcb, npix, C, st)
            else:
                L("s3od_bn_relu_bwd", code, dy, z, scale, shift, mean, rstd, w, sums, dz, dw, db, dcb, npix, C, st)
            torch.cuda.synchronize()
            assert int((sums != 0).sum()) == 0, "bn backward must leave its workspace all zero"
            outs[with_dcb, mode] = (dz, dw, db) + ((dcb,) if with_dcb else ())
        for a, c in zip(outs[with_dcb, "stored"], outs[with_dcb, "recompute"]):
            assert torch.equal(a, c)
    # dz, dw and db do not depend on whether the conv-bias gradient is asked for
    for a, c in zip(outs[True, "recompute"][:3], outs[False, "recompute"]):
        assert torch.equal(a, c)
    if npix >= 4:
        n_edge = int(((y[: npix // 4].float() == 0) & (z[: npix // 4].float() * scale + shift >= -1e-3)).sum())
        assert n_edge > 0

    # float64 reference of the BatchNorm backward given the forward's statistics (mean, rstd):
    # dz = w*rstd*(dy' - mean(dy') - xhat*mean(dy'*xhat)), dy' = dy*(y > 0); dw = sum(dy'*xhat), db = sum(dy');
    # dcb = sum(dz)
    d64 = lambda t: t.double().cpu()
    dyp = d64(dy) * (d64(y) > 0)
    xh = (d64(z) - d64(mean)) * d64(rstd)
    dz_ref = d64(w) * d64(rstd) * (dyp - dyp.mean(0) - xh * (dyp * xh).mean(0))
    tol = 1e-5 if dtype == "f32" else 1e-2
    dz, dw, db, dcb = outs[True, "recompute"]
    for name, got, ref in (("dz", dz, dz_ref), ("dw", dw, (dyp * xh).sum(0)), ("db", db, dyp.sum(0))):
        rel = _rel(got, ref)
        print(f"bn_bwd {dtype} C={C} npix={npix} {name}: rel {rel:.3e}")
        assert rel <= tol, (name, rel)
    # dcb is a sum of dz whose terms cancel (they sum to ~0 when mean is the mean of z): like every summation
    # error, its error is measured against the sum of the magnitudes
    rel = float((d64(dcb) - dz_ref.sum(0)).norm() / dz_ref.abs().sum(0).norm().clamp_min(1e-300))
    print(f"bn_bwd {dtype} C={C} npix={npix} dcb: rel (to sum |dz|) {rel:.3e}")
    assert rel <= tol, ("dcb", rel)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_bn_relu_bwd_matches_stored_mask(dtype):
    _case(dtype, 256, 3 * 1000 + 17)


def _edge_shapes():
    out = []
    for C in (8, 64, 256, 2048):
        rows = 256 // (C // 8)
        for npix in dict.fromkeys((1, rows - 1, 4 * rows + 1, 3017)):
            if npix > 0 and (C, npix) != (256, 3017):         # (256, 3017) is the test above
                out.append((C, npix))
    return out


@pytest.mark.parametrize("C,npix", _edge_shapes())
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_bn_bwd_edge_shapes(dtype, C, npix):
    """What test_bn_relu_bwd_matches_stored_mask asserts (stored mask == recomputed mask bit for bit, workspace left
    all zero, float64 parity of dz / dw / db, with and without the conv-bias gradient) at the shapes where the
    block decomposition changes: C = 8 (one column group, 256 row phases) .. 2048 (256 groups, one phase), and with
    rows = 256/(C/8): npix = 1 (fewer pixels than phases), rows - 1, 4*rows + 1 (one 4-row batch, then a one-row
    tail), 3017.  Before this only C = 256, npix = 3017 ran."""
    _case(dtype, C, npix)
