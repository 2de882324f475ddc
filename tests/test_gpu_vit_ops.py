"""GPU: the fused LayerNorm + LayerScale backward (s3od_layernorm_ls_bwd, csrc/vit_ops.hip ln_bwd_kernel<..., LS>)
against the unfused pair it replaces (s3od_layernorm_bwd, then s3od_layerscale_bwd on its dx) and against fp32 torch
autograd of y = x + lam * u and LayerNorm (tf:modeling_dinov3_vit.py:419-445).  dx and du are the same arithmetic in
both paths (bit-identical); the parameter gradients differ only in fp32 summation order (rel 1e-5)."""
import pytest
import torch

pytestmark = pytest.mark.gpu
F32, BF16 = 0, 1


@pytest.mark.parametrize("dtype", [BF16, F32])
def test_layernorm_ls_bwd_matches_pair(dtype):
    from s3od_amd._lib import lib, stream
    L, st = lib(), stream()
    torch.manual_seed(dtype)
    M, D = 2 * 4101, 768
    T = torch.bfloat16 if dtype == BF16 else torch.float32
    x = torch.randn(M, D, device="cuda")
    w, b = torch.randn(D, device="cuda"), torch.randn(D, device="cuda")
    mean, rstd = x.mean(1), torch.rsqrt(x.var(1, unbiased=False) + 1e-5)
    dy = torch.randn(M, D, device="cuda").to(T)
    dres = torch.randn(M, D, device="cuda")
    u = torch.randn(M, D, device="cuda").to(T)
    lam = torch.rand(D, device="cuda") + 0.1
    ws, ws2 = torch.zeros(32 * 2 * D, device="cuda"), torch.zeros(32 * 2 * D, device="cuda")
    out = {}
    for fused in (True, False):
        dx = torch.empty(M, D, device="cuda")
        du = torch.empty(M, D, device="cuda", dtype=T)
        g = [torch.zeros(D, device="cuda") for _ in range(4)]     # dw, db, dlam, dbias
        if fused:
            L("s3od_layernorm_ls_bwd", dtype, dy, x, mean, rstd, w, dres, dx, g[0], g[1], ws, u, lam, du, g[2], g[3], ws2,
              M, D, st)
        else:
            L("s3od_layernorm_bwd", dtype, dy, x, mean, rstd, w, dres, dx, g[0], g[1], ws, M, D, st)
            L("s3od_layerscale_bwd", dtype, dx, u, lam, du, g[2], g[3], ws2, M, D, st)
        torch.cuda.synchronize()
        out[fused] = (dx, du, g)
    assert torch.equal(out[True][0], out[False][0])
    assert torch.equal(out[True][1], out[False][1])
    for a, c in zip(out[True][2], out[False][2]):
        assert float((a - c).norm() / c.norm()) < 1e-5
    assert float(ws.abs().max()) == 0.0 and float(ws2.abs().max()) == 0.0
    # fp32 autograd reference of the same maths
    xr = x.clone().requires_grad_(True)
    wr, br = w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    y = torch.nn.functional.layer_norm(xr, (D,), wr, br, 1e-5)
    gx, gw, gb = torch.autograd.grad(y, (xr, wr, br), dy.float())
    dx_ref = gx + dres
    dx, du, g = out[True]
    assert float((dx - dx_ref).norm() / dx_ref.norm()) < 1e-5
    assert float((g[0] - gw).norm() / gw.norm()) < 1e-4 and float((g[1] - gb).norm() / gb.norm()) < 1e-4
    assert float((g[2] - (dx_ref * u.float()).sum(0)).norm() / (dx_ref * u.float()).sum(0).norm()) < 1e-4
    assert float((g[3] - (dx_ref * lam).sum(0)).norm() / (dx_ref * lam).sum(0).norm()) < 1e-4


@pytest.mark.parametrize("with_dres", [True, False])
@pytest.mark.parametrize("D", [768, 1024])
@pytest.mark.parametrize("M", [1, 3, 5, 33, 65, 8202])
@pytest.mark.parametrize("dtype", [BF16, F32])
def test_layernorm_ls_bwd_edge_shapes(dtype, M, D, with_dres):
    """The fused kernel, s3od_layernorm_bwd and s3od_layerscale_bwd away from the one shape (M 8202, D 768, dres
    given) the test above runs: blocks take 32 rows (64 fused), 4 waves at a time, so M = 33 / 65 is one full block
    plus one row and M = 1 / 3 / 5 leaves waves idle (LayerNorm) or row phases empty (LayerScale); D = 1024 is the
    other built width; dres = None is the other residual branch.  Every output of BOTH paths -- the unfused pair's
    own parameter gradients included, which nothing compared to a reference before -- against a float64
    restatement on the CPU; fused == pair bit for bit on dx and du; workspaces left all zero.
    Bounds: 1e-5 on dx (and du in f32), 1e-4 on parameter gradients, as above; du in bf16 is one round-to-nearest
    of an f32 product, 2^-9 relative per element, so 2^-8 bounds its rel-L2."""
    from s3od_amd._lib import lib, stream
    L, st = lib(), stream()
    torch.manual_seed(1000 * dtype + M + D)
    T = torch.bfloat16 if dtype == BF16 else torch.float32
    x = torch.randn(M, D, device="cuda")
    w = torch.randn(D, device="cuda")
    mean, rstd = x.mean(1), torch.rsqrt(x.var(1, unbiased=False) + 1e-5)
    dy = torch.randn(M, D, device="cuda").to(T)
    dres = torch.randn(M, D, device="cuda") if with_dres else None
    u = torch.randn(M, D, device="cuda").to(T)
    lam = torch.rand(D, device="cuda") + 0.1
    ws, ws2 = torch.zeros(32 * 2 * D, device="cuda"), torch.zeros(32 * 2 * D, device="cuda")
    out = {}
    for fused in (True, False):
        dx = torch.empty(M, D, device="cuda")
        du = torch.empty(M, D, device="cuda", dtype=T)
        g = [torch.zeros(D, device="cuda") for _ in range(4)]     # dw, db, dlam, dbias
        if fused:
            L("s3od_layernorm_ls_bwd", dtype, dy, x, mean, rstd, w, dres, dx, g[0], g[1], ws, u, lam, du, g[2], g[3], ws2,
              M, D, st)
        else:
            L("s3od_layernorm_bwd", dtype, dy, x, mean, rstd, w, dres, dx, g[0], g[1], ws, M, D, st)
            L("s3od_layerscale_bwd", dtype, dx, u, lam, du, g[2], g[3], ws2, M, D, st)
        torch.cuda.synchronize()
        assert float(ws.abs().max()) == 0.0 and float(ws2.abs().max()) == 0.0
        out[fused] = (dx, du, g)
    assert torch.equal(out[True][0], out[False][0])
    assert torch.equal(out[True][1], out[False][1])
    # float64: dx = dres + rstd (g - mean(g) - xhat mean(g xhat)), g = dy w; dw = sum dy xhat, db = sum dy;
    # du = dx lam, dlam = sum dx u, dbias = sum dx lam
    d64 = lambda t: t.double().cpu()
    xh = (d64(x) - d64(mean)[:, None]) * d64(rstd)[:, None]
    gg = d64(dy) * d64(w)
    dx_ref = d64(rstd)[:, None] * (gg - gg.mean(1, keepdim=True) - xh * (gg * xh).mean(1, keepdim=True))
    if with_dres:
        dx_ref = dx_ref + d64(dres)
    du_ref = dx_ref * d64(lam)
    refs = [(d64(dy) * xh).sum(0), d64(dy).sum(0), (dx_ref * d64(u)).sum(0), du_ref.sum(0)]
    rel = lambda a, r: float((d64(a) - r).norm() / r.norm())
    for fused in (True, False):
        dx, du, g = out[fused]
        figs = [rel(dx, dx_ref), rel(du, du_ref)] + [rel(a, r) for a, r in zip(g, refs)]
        print(f"dtype {dtype} M {M} D {D} dres {with_dres} fused {fused}: dx {figs[0]:.2e} du {figs[1]:.2e} "
              f"dw {figs[2]:.2e} db {figs[3]:.2e} dlam {figs[4]:.2e} dbias {figs[5]:.2e}")
        assert figs[0] < 1e-5
        assert figs[1] < (1e-5 if dtype == F32 else 2.0 ** -8)
        assert all(f < 1e-4 for f in figs[2:]), figs
