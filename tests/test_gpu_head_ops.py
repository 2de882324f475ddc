"""GPU: the decoder-head kernels of csrc/decoder_ops.hip that only the whole-model goldens reached, each called
through its entry point on NaN-filled outputs and compared with a float64 restatement on the CPU:
s3od_avgpool, s3od_iou_head_fwd / _bwd, s3od_mask_heads_bwd, s3od_bilinear_fwd (exact-2x and generic kernel),
s3od_bn_finalize and s3od_bn_fold.

Tolerances (the convention of tests/test_gpu_bn_relu.py): f32 results rel-L2 <= 1e-5 against float64; bf16
outputs per element, |got - ref| <= 2^-8 |ref| + 1e-6 max|input| (computed in f32, rounded once), because a
rel-L2 of 1e-2 over a tensor can hide one wrong border row.  Each test prints its worst error (pytest -s).
"""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

NAN = float("nan")
DT = {"f32": (torch.float32, 0), "bf16": (torch.bfloat16, 1)}
TOL_F32 = 1e-5


def _lib():
    from s3od_amd._lib import lib, stream
    return lib(), stream()


def rel_l2(got, ref):
    got, ref = got.detach().double().cpu(), ref.double()
    return float((got - ref).norm() / ref.norm())


def worst_ratio(got, ref, tol):
    """max over elements of |got - ref| / tol (tol a tensor or a number); <= 1 passes.  NaN counts as a miss."""
    got, ref = got.detach().double().cpu(), ref.double()
    r = (got - ref).abs() / tol
    return float(torch.nan_to_num(r, nan=float("inf")).max())


def bf16_tol(ref, max_in):
    return 2.0 ** -8 * ref.double().abs() + 1e-6 * float(max_in)


# ------------------------------------------------------------------------------------------------ avgpool
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("C", [256, 64])
@pytest.mark.parametrize("HW", [1, 7, 1023, 1024, 1025, 2 * 1024 + 5])
@pytest.mark.parametrize("B", [1, 3])
def test_avgpool(dtype, C, HW, B):
    """mean over pixels of the (already rounded) input.  Allowed error per output: 2^-24 * L * mean_p |x|, with L
    the longest chain of f32 operations one input goes through: a thread adds ceil(min(HW, 1024) / rows) terms
    (rows = 256 / (C/8) row phases per block), thread 0 of a column adds the `rows` phase partials, the fold
    adds the nk = ceil(HW / 1024) block partials.  Counting terms, not additions, leaves three units, which
    cover the rounded 1/HW and the final product:  L = ceil(min(HW, 1024) / rows) + rows + nk."""
    L_, st = _lib()
    dt, code = DT[dtype]
    torch.manual_seed(HW * 7 + C + B)
    x = (torch.randn(B, HW, C) + 0.25).to(dt)
    rows, nk = 256 // (C // 8), -(-HW // 1024)
    chain = -(-min(HW, 1024) // rows) + rows + nk
    ref = x.double().mean(1)
    tol = 2.0 ** -24 * chain * x.double().abs().mean(1)
    xg = x.cuda()
    ws = torch.full((B, nk, C), NAN, device="cuda")
    outs = []
    for _ in range(2):
        out = torch.full((B, C), NAN, device="cuda")
        L_("s3od_avgpool", code, xg, out, ws, B, HW, C, st)     # second call: ws holds the first call's partials
        torch.cuda.synchronize()
        outs.append(out)
    r = worst_ratio(outs[0], ref, tol)
    print(f"\n[avgpool {dtype} B{B} HW{HW} C{C}] L {chain}  worst |err| / allowed {r:.3f}")
    assert torch.isfinite(outs[0]).all(), "NaN from the workspace or an unwritten output"
    assert torch.equal(outs[0], outs[1]), "two calls on the same input must be bit-identical"
    assert r <= 1.0, r


# ------------------------------------------------------------------------------------------------ IoU head
@pytest.mark.parametrize("NM", [1, 3])
@pytest.mark.parametrize("B", [1, 3, 22])
def test_iou_head_fwd_bwd(B, NM):
    """Linear(256,64) -> ReLU -> Linear(64,NM) and its backward (accumulating weight gradients, dpix = dpooled / HW).
    Hidden units 0..7 are dead for every image (bias -50), so relu' = 0 is exercised on whole columns."""
    L_, st = _lib()
    torch.manual_seed(B * 10 + NM)
    HW, DEAD = 37 * 41, 8
    pooled, w1, b1 = torch.randn(B, 256), torch.randn(64, 256) / 16, torch.randn(64) * 0.1
    b1[:DEAD] = -50.0
    w2, b2, dout = torch.randn(NM, 64) / 8, torch.randn(NM), torch.randn(B, NM)
    pre = {n: torch.randn(s) * 0.1 for n, s in (("dw1", (64, 256)), ("db1", (64,)), ("dw2", (NM, 64)), ("db2", (NM,)))}
    # float64 reference
    P = {n: v.double().requires_grad_(True) for n, v in (("pooled", pooled), ("w1", w1), ("b1", b1), ("w2", w2), ("b2", b2))}
    hid_ref = F.relu(F.linear(P["pooled"], P["w1"], P["b1"]))
    out_ref = F.linear(hid_ref, P["w2"], P["b2"])
    out_ref.backward(dout.double())
    assert (hid_ref[:, :DEAD] == 0).all() and (hid_ref[:, DEAD:] > 0).any()
    g = {n: v.cuda() for n, v in (("pooled", pooled), ("w1", w1), ("b1", b1), ("w2", w2), ("b2", b2), ("dout", dout))}
    hid = torch.full((B, 64), NAN, device="cuda")
    out = torch.full((B, NM), NAN, device="cuda")
    L_("s3od_iou_head_fwd", g["pooled"], g["w1"], g["b1"], g["w2"], g["b2"], hid, out, B, NM, st)
    acc = {n: v.cuda() for n, v in pre.items()}
    dpix = torch.full((B, 256), NAN, device="cuda")
    L_("s3od_iou_head_bwd", g["pooled"], hid, g["w1"], g["w2"], g["dout"], acc["dw1"], acc["db1"], acc["dw2"], acc["db2"],
       dpix, B, HW, NM, st)
    torch.cuda.synchronize()
    errs = {"out": rel_l2(out, out_ref.detach()), "hid": rel_l2(hid, hid_ref.detach()),
            "dpix": rel_l2(dpix, P["pooled"].grad / HW)}
    for n, p in (("dw1", "w1"), ("db1", "b1"), ("dw2", "w2"), ("db2", "b2")):
        errs[n] = rel_l2(acc[n], pre[n].double() + P[p].grad)
    print(f"\n[iou_head B{B} NM{NM}] " + "  ".join(f"{n} {e:.2e}" for n, e in errs.items()))
    assert (hid[:, :DEAD] == 0).all(), "dead hidden units must store exact zeros"
    assert torch.equal(acc["dw1"][:DEAD].cpu(), pre["dw1"][:DEAD]) and torch.equal(acc["db1"][:DEAD].cpu(), pre["db1"][:DEAD]), \
        "dead units add exactly nothing to the accumulators"
    for n, e in errs.items():
        assert e <= TOL_F32, (n, e)


# ------------------------------------------------------------------------------------------------ mask heads backward
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("NM", [1, 3])
@pytest.mark.parametrize("B,HW", [(1, 5), (2, 33 * 31), (1, 181 * 182)])
def test_mask_heads_bwd(dtype, NM, B, HW):
    """(1, 5): fewer rows than one block's 32.  (2, 1023): the image boundary falls inside a block.  (1, 32942):
    more than 1024 * 32 rows, so the grid-stride loop takes a second trip with a ragged tail.  h = relu(randn)
    stored in T: about half of its entries are exact zeros."""
    L_, st = _lib()
    dt, code = DT[dtype]
    torch.manual_seed(HW + NM)
    M, C = B * HW, 32 * NM
    h = F.relu(torch.randn(M, C)).to(dt)
    dlog, w2 = torch.randn(B, NM, HW), torch.randn(NM, 32)
    pre = {"dw2": torch.randn(NM, 32), "db2": torch.randn(NM), "db1": torch.randn(C)}
    assert 0.4 < float((h == 0).float().mean()) < 0.6
    # float64: dh = (h > 0) dl_k w2, dw2 = sum dl h, db2 = sum dl, db1 = sum dh
    dlm = dlog.double().permute(0, 2, 1).reshape(M, NM)
    dlc = dlm.repeat_interleave(32, dim=1)
    dh_ref = (h > 0).double() * dlc * w2.double().reshape(1, C)
    ref = {"dw2": pre["dw2"].double() + (dlc * h.double()).sum(0).view(NM, 32), "db2": pre["db2"].double() + dlm.sum(0),
           "db1": pre["db1"].double() + dh_ref.sum(0)}
    dh = torch.full((M, C), NAN, device="cuda", dtype=dt)
    acc = {n: v.cuda() for n, v in pre.items()}
    L_("s3od_mask_heads_bwd", code, dlog.cuda(), h.cuda(), w2.cuda(), dh, acc["dw2"], acc["db2"], acc["db1"], B, HW, NM, st)
    torch.cuda.synchronize()
    errs = {n: rel_l2(acc[n], ref[n]) for n in ref}
    if dtype == "f32":
        errs["dh"] = rel_l2(dh, dh_ref)
        dh_ratio = 0.0
    else:
        dh_ratio = worst_ratio(dh, dh_ref, bf16_tol(dh_ref, dlog.abs().max()))
    print(f"\n[mask_heads_bwd {dtype} NM{NM} B{B} HW{HW}] " + "  ".join(f"{n} {e:.2e}" for n, e in errs.items())
          + (f"  dh worst |err| / allowed {dh_ratio:.3f}" if dtype == "bf16" else ""))
    assert torch.isfinite(dh.float()).all(), "every dh row must be written"
    assert ((dh.float().cpu() == 0) == (h == 0)).all(), "relu' must zero exactly the entries where h is zero"
    assert dh_ratio <= 1.0, dh_ratio
    for n, e in errs.items():
        assert e <= TOL_F32, (n, e)


# ------------------------------------------------------------------------------------------------ bilinear forward
UP2 = [(ih, iw, 2 * ih, 2 * iw) for ih, iw in [(1, 1), (1, 5), (5, 1), (7, 9), (16, 16)]]
GENERIC = [(12, 10, 25, 17), (7, 9, 15, 18), (5, 5, 5, 5), (3, 4, 12, 4),
           (1, 1, 7, 5), (1, 6, 9, 6), (2, 3, 37, 41), (3, 3, 100, 7),          # a 1-pixel axis, large ratios
           (25, 17, 12, 10), (9, 8, 3, 3), (8, 8, 4, 4), (7, 5, 1, 1)]          # down-scales


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("C", [8, 64])
@pytest.mark.parametrize("IH,IW,OH,OW", UP2 + GENERIC)
def test_bilinear_fwd(dtype, C, IH, IW, OH, OW):
    """F.interpolate(bilinear, align_corners=False) in float64, NHWC.  OH == 2 IH and OW == 2 IW takes the
    exact-2x kernel (clamped 3x3 neighbourhood), anything else the generic one.  Per element, so that a single
    wrong border pixel cannot hide: f32 |got - ref| <= 2^-22 max|x|, bf16 as stated in the module docstring.
    With the source coordinate formed in f32 (scale = in/out, then a product) the generic kernel measured 3.06x
    the f32 bound at 12x10 -> 25x17 and 1.06x at 7x9 -> 15x18; it takes the coordinate exactly now (bil_coef_exact)."""
    L_, st = _lib()
    dt, code = DT[dtype]
    B = 2
    torch.manual_seed(IH * 100 + IW + C)
    x = torch.randn(B, IH, IW, C).to(dt)
    ref = F.interpolate(x.double().permute(0, 3, 1, 2), size=(OH, OW), mode="bilinear", align_corners=False).permute(0, 2, 3, 1)
    y = torch.full((B, OH, OW, C), NAN, device="cuda", dtype=dt)
    L_("s3od_bilinear_fwd", code, x.cuda(), y, B, IH, IW, OH, OW, C, st)
    torch.cuda.synchronize()
    mx = float(x.double().abs().max())
    tol = 2.0 ** -22 * mx if dtype == "f32" else bf16_tol(ref, mx)
    r = worst_ratio(y, ref, tol)
    kern = "up2" if (OH, OW) == (2 * IH, 2 * IW) else "generic"
    print(f"\n[bilinear_fwd {kern} {dtype} C{C} {IH}x{IW}->{OH}x{OW}] worst |err| / allowed {r:.3f}")
    assert r <= 1.0, r


# ------------------------------------------------------------------------------------------------ BatchNorm finalize / fold
EPS, MOM = 1e-5, 0.1
CONST_CH, CONST_V = 3, 1000.25


def _split_replicas(tot, nrep, gen):
    """[2][C] totals -> [nrep][2][C] float64 replicas with very uneven shares (some empty, some negative)."""
    share = torch.rand(nrep, 1, tot.shape[1], dtype=torch.float64, generator=gen) ** 4
    share[torch.rand(nrep, generator=gen) < 0.3] = 0.0
    share[1] = -0.5
    rep = share * tot
    rep[0] += tot - rep.sum(0)
    rep[:, :, CONST_CH] = 0.0
    rep[5, :, CONST_CH] = tot[:, CONST_CH]           # one replica holds this channel whole: its fold is exact
    return rep.contiguous()


@pytest.mark.parametrize("case", ["running", "count1", "no_running"])
@pytest.mark.parametrize("C", [8, 256, 304])
def test_bn_finalize(C, case):
    """(sum z, sum z^2) in float64, split unevenly over the NREP replicas -> mean, rstd, scale, shift and the
    running statistics (momentum 0.1, unbiased variance); the workspace is left all zero.  C = 304 needs a
    second block.  Channel 3 is constant at 1000.25 with its sum of squares a few ulps low, as accumulated
    rounding leaves it: the variance comes out negative and must clamp to 0 (rstd = 1/sqrt(eps)).
    count1: one value per channel, so the unbiased factor n/(n-1) must not be formed."""
    from s3od_amd._lib import NREP
    L_, st = _lib()
    gen = torch.Generator().manual_seed(C + len(case))
    n = 1 if case == "count1" else 3017
    z = (torch.randn(n, C, generator=gen) * 1.7 + 0.3).double()
    z[:, CONST_CH] = CONST_V
    tot = torch.stack([z.sum(0), (z * z).sum(0)])
    if n > 1:
        tot[1, CONST_CH] *= 1 - 2.0 ** -48
    w, b = torch.rand(C, generator=gen) + 0.5, torch.randn(C, generator=gen) * 0.3
    rm0, rv0 = torch.randn(C, generator=gen), torch.rand(C, generator=gen) + 0.5
    # float64 reference from the unsplit totals
    mean = tot[0] / n
    var = (tot[1] / n - mean * mean).clamp_min(0)
    if n > 1:
        assert float(tot[1, CONST_CH] / n - mean[CONST_CH] ** 2) < 0 and var[CONST_CH] == 0
    rstd = 1 / torch.sqrt(var + EPS)
    unb = var * n / (n - 1) if n > 1 else var
    ref = {"mean": mean, "rstd": rstd, "scale": w.double() * rstd, "shift": b.double() - mean * w.double() * rstd,
           "rm": (1 - MOM) * rm0.double() + MOM * mean, "rv": (1 - MOM) * rv0.double() + MOM * unb}
    stats = _split_replicas(tot, NREP, gen).cuda()
    out = {k: torch.full((C,), NAN, device="cuda") for k in ("mean", "rstd", "scale", "shift")}
    rm, rv = (rm0.cuda(), rv0.cuda()) if case != "no_running" else (None, None)
    L_("s3od_bn_finalize", stats, n, w.cuda(), b.cuda(), rm, rv, MOM, EPS, out["mean"], out["rstd"], out["scale"], out["shift"], C, st)
    torch.cuda.synchronize()
    if rm is not None:
        out.update(rm=rm, rv=rv)
    keep = torch.ones(C, dtype=torch.bool)
    keep[CONST_CH] = False                  # rstd = 316 there would dominate a norm over the channels
    errs = {k: rel_l2(v.cpu()[keep], ref[k][keep]) for k, v in out.items()}
    const = {k: abs(float(v[CONST_CH]) - float(ref[k][CONST_CH])) / abs(float(ref[k][CONST_CH])) for k, v in out.items()}
    print(f"\n[bn_finalize C{C} {case}] " + "  ".join(f"{k} {e:.2e}" for k, e in errs.items())
          + f"  constant channel worst rel {max(const.values()):.2e}")
    assert int((stats != 0).sum()) == 0, "bn_finalize must leave its workspace all zero"
    for k, e in errs.items():
        assert e <= TOL_F32, (k, e)
    for k, e in const.items():              # without the clamp rstd is off by 1.8e-4 here
        assert e <= TOL_F32, ("constant channel", k, e)
    assert abs(float(out["rstd"][CONST_CH]) * math.sqrt(EPS) - 1) <= 1e-6


@pytest.mark.parametrize("C", [8, 256, 304])
def test_bn_fold(C):
    """eval fold: scale = w / sqrt(rv + eps), shift = b - rm * scale."""
    L_, st = _lib()
    gen = torch.Generator().manual_seed(C)
    w, b = torch.rand(C, generator=gen) + 0.5, torch.randn(C, generator=gen) * 0.3
    rm, rv = torch.randn(C, generator=gen), torch.rand(C, generator=gen) * 2 + 1e-3
    scale, shift = (torch.full((C,), NAN, device="cuda") for _ in range(2))
    L_("s3od_bn_fold", w.cuda(), b.cuda(), rm.cuda(), rv.cuda(), EPS, scale, shift, C, st)
    torch.cuda.synchronize()
    s_ref = w.double() / torch.sqrt(rv.double() + EPS)
    e1, e2 = rel_l2(scale, s_ref), rel_l2(shift, b.double() - rm.double() * s_ref)
    print(f"\n[bn_fold C{C}] scale {e1:.2e}  shift {e2:.2e}")
    assert e1 <= TOL_F32 and e2 <= TOL_F32, (e1, e2)
