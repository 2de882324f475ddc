"""s3od_matte_refine and s3od_matte_foreground (csrc/matte.hip) against the float64 reference of tests/_matte_ref.py.

Float output: max |q - q64| <= 1/510, half an 8-bit alpha step, the precision at which the product emits alpha.  The
margin: an fp32 restatement with whole-image running sums (the worst summation order a reasonable kernel could use) and
a float64 solve stays within 2.6e-4 on a 300 x 400 case, direct fp32 sums within 3e-6, so the bound is at least 7 x what
fp32 needs; the kernels sum in float64 and keep float32 between their passes (a numpy restatement of exactly that
arithmetic is within 1.3e-6 on these cases).  Bytes (the alpha byte trunc(q 255), the foreground bytes): at most one
level from the reference's bytes, on at most 1 % of a case's bytes (a byte differs only where the float64 value lies
within the float error of a rounding boundary).  The measured maxima are printed.

Shapes: no side is a multiple of the 256-column tile or of a row strip; (5, 301) and (129, 257) span two tiles,
(130, 7) is narrower than a tile and than 2 r + 1, every row of every case starts at another byte alignment (3 W is
odd), and radius 256 exceeds every image.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import _matte_ref as R

pytestmark = pytest.mark.gpu

SHAPES = [(37, 53), (64, 200), (5, 301), (130, 7), (129, 257)]
RADII = [1, 8, 40, 256]
EPS = [1e-6, 1e-4, 1e-2]
FG_RADII = [1, 8, 90]
Q_BOUND = 1.0 / 510.0
BYTE_SHARE = 0.01


@functools.lru_cache(maxsize=None)
def case(shape):
    src, m = R.make_case(*shape, seed=shape[0] * 1000 + shape[1])
    src.setflags(write=False)
    m.setflags(write=False)
    return src, m


@functools.lru_cache(maxsize=None)
def ref_refine(shape, r, eps):
    q = R.refine(case(shape)[1], case(shape)[0], r, eps)
    q.setflags(write=False)
    return q


@functools.lru_cache(maxsize=None)
def ref_foreground(shape, r):
    f = R.to_bytes(R.foreground(case(shape)[1], case(shape)[0], r))
    f.setflags(write=False)
    return f


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()       # a writable copy


def check_bytes(got, ref, what):
    d = np.abs(got.astype(np.int32) - ref.astype(np.int32))
    share = float((d != 0).mean())
    assert d.max() <= 1, f"{what}: a byte is {d.max()} levels off"
    assert share <= BYTE_SHARE, f"{what}: {share:.4%} of the bytes differ"
    return share


@pytest.mark.parametrize("shape", SHAPES)
def test_refine_matches_the_float64_reference(shape):
    from s3od_amd.matte import refine_alpha
    src, m = case(shape)
    src_d, m_d = dev(src), dev(m)
    worst = worst_share = 0.0
    for r in RADII:
        for eps in EPS:
            out = torch.full_like(m_d, float("nan"))
            assert refine_alpha(m_d, src_d, r, eps, out=out) is out
            q, q64 = out.cpu().numpy(), ref_refine(shape, r, eps)
            assert np.isfinite(q).all() and q.min() >= 0.0 and q.max() <= 1.0
            err = float(np.abs(q - q64).max())
            worst = max(worst, err)
            assert err <= Q_BOUND, (shape, r, eps, err)
            share = check_bytes((q * 255).astype(np.uint8), R.alpha_bytes(q64), f"alpha {shape} r {r} eps {eps}")
            worst_share = max(worst_share, share)
    print(f"matte_refine {shape}: max |q - q64| {worst:.3g} (bound {Q_BOUND:.3g}), differing alpha bytes <= {worst_share:.4%}")


@pytest.mark.parametrize("shape", SHAPES)
def test_foreground_matches_the_float64_reference(shape):
    from s3od_amd.matte import estimate_foreground
    src, m = case(shape)
    src_d, m_d = dev(src), dev(m)
    worst_share = 0.0
    for r in FG_RADII:
        out = torch.full_like(src_d, 77)
        assert estimate_foreground(m_d, src_d, r, out=out) is out
        worst_share = max(worst_share, check_bytes(out.cpu().numpy(), ref_foreground(shape, r), f"foreground {shape} r {r}"))
    print(f"matte_foreground {shape}: differing bytes <= {worst_share:.4%}")


def test_source_at_an_odd_address():
    """The image may start at any byte: the same result from a copy one byte into its buffer."""
    from s3od_amd.matte import estimate_foreground, refine_alpha
    src, m = case((37, 53))
    m_d, base = dev(m), torch.zeros(src.size + 1, dtype=torch.uint8, device="cuda")
    base[1:] = dev(src).reshape(-1)
    odd = base[1:].view(37, 53, 3)
    assert odd.data_ptr() % 2 == 1
    assert torch.equal(refine_alpha(m_d, odd, 8, 1e-4), refine_alpha(m_d, dev(src), 8, 1e-4))
    assert torch.equal(estimate_foreground(m_d, odd, 8), estimate_foreground(m_d, dev(src), 8))


def test_repeated_and_aliased_calls_give_the_same_bits():
    from s3od_amd.matte import estimate_foreground, refine_alpha
    src, m = case((129, 257))
    src_d, m_d = dev(src), dev(m)
    for r, eps in ((8, 1e-6), (256, 1e-4)):
        first = refine_alpha(m_d, src_d, r, eps)
        assert torch.equal(refine_alpha(m_d, src_d, r, eps), first)
        alias = m_d.clone()
        assert refine_alpha(alias, src_d, r, eps, out=alias) is alias
        assert torch.equal(alias, first)
        assert torch.equal(m_d, dev(m))                     # an input that is not the output is left alone
    f = estimate_foreground(m_d, src_d, 8)
    assert torch.equal(estimate_foreground(m_d, src_d, 8), f)


def test_bad_arguments_are_rejected_on_the_host():
    """Every check precedes the first launch: the poisoned output is untouched."""
    from s3od_amd._lib import HipLibError, lib, stream
    from s3od_amd.matte import workspace_bytes
    H, W = 16, 20
    need = workspace_bytes(H, W)
    assert need >= 13 * H * W * 4
    mask = torch.rand(H, W, device="cuda")
    src = torch.zeros(H, W, 3, dtype=torch.uint8, device="cuda")
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    out = torch.full((H, W), float("nan"), device="cuda")
    rgb = torch.full((H, W, 3), 77, dtype=torch.uint8, device="cuda")
    L = lib()

    def refine(mask=mask, src=src, H=H, W=W, r=4, eps=1e-4, ws=ws, nbytes=need, out=out):
        L("s3od_matte_refine", mask, src, H, W, r, eps, ws, nbytes, out, stream())

    def fg(H=H, W=W, r=4, ws=ws, nbytes=need, out=rgb):
        L("s3od_matte_foreground", mask, src, H, W, r, ws, nbytes, out, stream())

    for kw, match in ((dict(r=0), "radius"), (dict(r=257), "radius"), (dict(eps=0.0), "eps"), (dict(eps=2.0), "eps"),
                      (dict(nbytes=need - 1), "workspace"), (dict(H=1), "outside"), (dict(W=32769), "outside"),
                      (dict(mask=None), "missing"), (dict(src=None), "missing"), (dict(ws=None), "missing"),
                      (dict(out=None), "missing")):
        with pytest.raises(HipLibError, match=match):
            refine(**kw)
    for kw, match in ((dict(r=0), "radius"), (dict(r=257), "radius"), (dict(nbytes=need - 1), "workspace"),
                      (dict(H=1), "outside"), (dict(out=None), "missing")):
        with pytest.raises(HipLibError, match=match):
            fg(**kw)
    n = ctypes.c_long(-1)
    with pytest.raises(HipLibError, match="outside"):
        L("s3od_matte_ws", 1, W, ctypes.addressof(n))
    with pytest.raises(HipLibError, match="missing"):
        L("s3od_matte_ws", H, W, None)
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and (rgb == 77).all()
    refine()                                                # the same arguments, valid: it runs
    fg()
    torch.cuda.synchronize()
    assert not torch.isnan(out).any()
