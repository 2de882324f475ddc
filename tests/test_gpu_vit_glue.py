"""GPU: the small ViT glue kernels of csrc/vit_ops.hip that only the whole-model goldens reached, each called
through its entry point on NaN-filled outputs and compared with a float64 restatement on the CPU:
s3od_layernorm_fwd, s3od_rope_table, s3od_patch_im2col, s3od_token_prefix, s3od_token_prefix_bwd, s3od_cast_tap.
Copies and casts must be exact (bf16: torch's round-to-nearest-even cast).  Each test prints its worst error
(pytest -s).
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

NAN = float("nan")
DT = {"f32": (torch.float32, 0), "bf16": (torch.bfloat16, 1)}
U = 2.0 ** -24            # unit roundoff of f32


def _lib():
    from s3od_amd._lib import lib, stream
    return lib(), stream()


def worst_ratio(got, ref, tol):
    got, ref = got.detach().double().cpu(), ref.double()
    r = (got - ref).abs() / tol
    return float(torch.nan_to_num(r, nan=float("inf")).max())


# ------------------------------------------------------------------------------------------------ LayerNorm forward
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("offset", [0.0, 1000.0])
@pytest.mark.parametrize("M", [1, 3, 5, 4101])
@pytest.mark.parametrize("D", [768, 1024])
def test_layernorm_fwd(dtype, offset, M, D):
    """One wave per row, four rows per block: M = 1, 3, 5, 4101 leave 1, 3, 1, 1 live rows in the last block.
    x = offset + randn: the two-pass variance must survive an offset of 1000.  Also y = None (statistics only).

    Bounds against float64, from the f32 arithmetic of a correct kernel (u = 2^-24):
      mean   a lane adds D/64 values, the wave reduces in 6 butterfly steps, then one product with 1/D (itself
             rounded): every input goes through at most L = D/64 + 6 + 2 roundings, so
             |d mean| <= L u mean|x|  =: tm.
      rstd   d = x - mean_kernel is exact or one rounding; sum((x - m')^2)/D = var + (m' - mean)^2, so the
             variance is relatively off by at most (L + 3) u + tm^2 / var, rstd by half of that plus the
             roundings of sqrt and the division:  |d rstd| / rstd <= ((L + 3) / 2 + 3) u + tm^2 / (2 var)  =: tr.
      y      (x - m') rstd w + b:  |d y| <= |w| rstd tm + (tr + 4 u) |xhat w| + u |y|;  bf16 adds the single
             rounding of the store, 2^-8 |y| in the project's convention.
    """
    L_, st = _lib()
    dt, code = DT[dtype]
    torch.manual_seed(M + D)
    eps = 1e-6
    x = torch.randn(M, D) + offset
    w, b = torch.rand(D) + 0.5, torch.randn(D) * 0.3
    xd = x.double()
    mean, var = xd.mean(1), xd.var(1, unbiased=False)
    rstd = 1 / torch.sqrt(var + eps)
    xhat_w = (xd - mean[:, None]) * rstd[:, None] * w.double()
    y_ref = xhat_w + b.double()
    chain = D // 64 + 6 + 2
    tm = chain * U * xd.abs().mean(1)
    tr = ((chain + 3) / 2 + 3) * U + tm ** 2 / (2 * var)
    ty = w.double().abs() * (rstd * tm)[:, None] + (tr[:, None] + 4 * U) * xhat_w.abs() + U * y_ref.abs()
    if dtype == "bf16":
        ty = ty + 2.0 ** -8 * y_ref.abs()
    xg, wg, bg = x.cuda(), w.cuda(), b.cuda()
    res = {}
    for with_y in (True, False):
        y = torch.full((M, D), NAN, device="cuda", dtype=dt) if with_y else None
        mo, ro = (torch.full((M,), NAN, device="cuda") for _ in range(2))
        L_("s3od_layernorm_fwd", code, xg, wg, bg, y, mo, ro, M, D, eps, st)
        torch.cuda.synchronize()
        res[with_y] = (y, mo, ro)
    y, mo, ro = res[True]
    rm, rr, ry = worst_ratio(mo, mean, tm), worst_ratio(ro, rstd, tr * rstd), worst_ratio(y, y_ref, ty)
    print(f"\n[layernorm_fwd {dtype} D{D} M{M} offset {offset:g}] worst |err| / allowed: mean {rm:.3f}  rstd {rr:.3f}  y {ry:.3f}")
    assert torch.equal(res[False][1], mo) and torch.equal(res[False][2], ro), "y = None must still write the same statistics"
    assert rm <= 1.0 and rr <= 1.0 and ry <= 1.0, (rm, rr, ry)


# ------------------------------------------------------------------------------------------------ RoPE table
def _rope_f64(ph, pw, rescale):
    """oracle.s3od_oracle.rope_cos_sin restated with every intermediate in float64 (the oracle pins float32)."""
    from oracle.s3od_oracle import ROPE_THETA, HEAD_DIM
    import math
    inv_freq = 1.0 / ROPE_THETA ** torch.arange(0, 1, 4 / HEAD_DIM, dtype=torch.float64)
    ch = torch.arange(0.5, ph, dtype=torch.float64) / ph
    cw = torch.arange(0.5, pw, dtype=torch.float64) / pw
    coords = 2.0 * torch.stack(torch.meshgrid(ch, cw, indexing="ij"), dim=-1).flatten(0, 1) - 1.0
    if rescale is not None:
        coords = coords * rescale
    ang = (2 * math.pi * coords[:, :, None] * inv_freq[None, None, :]).flatten(1, 2).tile(2)
    return torch.cos(ang), torch.sin(ang)


@pytest.mark.parametrize("rescale", [0.0, 0.8, 1.25])
@pytest.mark.parametrize("ph,pw", [(1, 1), (10, 16), (14, 14), (64, 64)])
def test_rope_table(ph, pw, rescale):
    """cos / sin [P, 64] against the oracle's rope_cos_sin in float64; rescale 0 means none.  Absolute tolerance
    2e-6: the arguments reach |2 pi 1.25| = 7.9, where f32 rounding of the argument alone is about 4e-7."""
    from oracle.s3od_oracle import rope_cos_sin
    L_, st = _lib()
    rs = None if rescale == 0.0 else rescale
    cos_ref, sin_ref = _rope_f64(ph, pw, rs)
    oc, os_ = rope_cos_sin(ph, pw, rs)
    assert float((oc.double() - cos_ref).abs().max()) <= 2e-6 and float((os_.double() - sin_ref).abs().max()) <= 2e-6, \
        "the float64 restatement must be the oracle's function"
    P = ph * pw
    cs, sn = (torch.full((P, 64), NAN, device="cuda") for _ in range(2))
    L_("s3od_rope_table", cs, sn, ph, pw, rescale, st)
    torch.cuda.synchronize()
    ec, es = float((cs.cpu().double() - cos_ref).abs().max()), float((sn.cpu().double() - sin_ref).abs().max())
    print(f"\n[rope_table {ph}x{pw} rescale {rescale:g}] max |err| cos {ec:.2e}  sin {es:.2e}")
    assert ec <= 2e-6 and es <= 2e-6, (ec, es)


# ------------------------------------------------------------------------------------------------ patch im2col
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("B,H,W", [(1, 16, 16), (2, 32, 48), (1, 48, 36), (1, 40, 52)])
def test_patch_im2col(dtype, B, H, W):
    """unfold(16, 16) in the c*256 + kh*16 + kw order.  36 = 2*16 + 4, 40 = 2*16 + 8, 52 = 3*16 + 4: the
    remainder columns / rows are ignored, and a patch row never reads across image rows."""
    import torch.nn.functional as F
    L_, st = _lib()
    dt, code = DT[dtype]
    torch.manual_seed(H + W)
    x = torch.randn(B, 3, H, W)
    P = (H // 16) * (W // 16)
    ref = F.unfold(x.double(), kernel_size=16, stride=16).transpose(1, 2).reshape(B * P, 768)
    cols = torch.full((B * P, 768), NAN, device="cuda", dtype=dt)
    L_("s3od_patch_im2col", code, x.cuda(), cols, B, H, W, st)
    torch.cuda.synchronize()
    want = ref.float().to(dt)            # f32: the values themselves; bf16: torch's round-to-nearest-even cast
    bad = int((cols.cpu() != want).sum())
    print(f"\n[patch_im2col {dtype} {B}x{H}x{W}] mismatching elements {bad} of {want.numel()}")
    assert bad == 0


# ------------------------------------------------------------------------------------------------ token prefix / tap cast
@pytest.mark.parametrize("D", [768, 1024])
@pytest.mark.parametrize("P", [1, 140])
@pytest.mark.parametrize("B", [1, 3])
def test_token_prefix_fwd_bwd(B, P, D):
    """rows 0..4 of each image = cls + 4 register tokens, every other row untouched; the backward accumulates
    the batch sums of those rows into pre-filled dcls / dreg."""
    L_, st = _lib()
    torch.manual_seed(B + P + D)
    Ntok = 5 + P
    cls, reg = torch.randn(D), torch.randn(4, D)
    x0 = torch.randn(B, Ntok, D)
    x = x0.cuda()
    L_("s3od_token_prefix", x, cls.cuda(), reg.cuda(), B, Ntok, D, st)
    dx = torch.randn(B, Ntok, D)
    dcls0, dreg0 = torch.randn(D), torch.randn(4, D)
    dcls, dreg = dcls0.cuda(), dreg0.cuda()
    L_("s3od_token_prefix_bwd", dx.cuda(), dcls, dreg, B, Ntok, D, st)
    torch.cuda.synchronize()
    want = x0.clone()
    want[:, 0], want[:, 1:5] = cls, reg
    assert torch.equal(x.cpu(), want), "prefix rows are copies; patch rows are untouched"
    ref = torch.cat([dcls0[None], dreg0]).double() + dx[:, :5].double().sum(0)
    got = torch.cat([dcls[None], dreg]).cpu().double()
    # B + 1 f32 additions per element
    r = worst_ratio(got, ref, (B + 1) * U * (torch.cat([dcls0[None], dreg0]).double().abs() + dx[:, :5].double().abs().sum(0)))
    print(f"\n[token_prefix B{B} P{P} D{D}] fwd exact; bwd worst |err| / allowed {r:.3f}")
    assert r <= 1.0, r


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("D", [768, 1024])
@pytest.mark.parametrize("P", [1, 140])
@pytest.mark.parametrize("B", [1, 3])
def test_cast_tap(dtype, B, P, D):
    """x f32 [B, 5 + P, D] -> T [B, P, D]: drops exactly the five prefix rows of every image."""
    L_, st = _lib()
    dt, code = DT[dtype]
    torch.manual_seed(B * 3 + P + D)
    Ntok = 5 + P
    x = torch.randn(B, Ntok, D)
    y = torch.full((B, P, D), NAN, device="cuda", dtype=dt)
    L_("s3od_cast_tap", code, x.cuda(), y, B, Ntok, P, D, st)
    torch.cuda.synchronize()
    want = x[:, 5:].to(dt)
    bad = int((y.cpu() != want).sum())
    print(f"\n[cast_tap {dtype} B{B} P{P} D{D}] mismatching elements {bad} of {want.numel()}")
    assert bad == 0
