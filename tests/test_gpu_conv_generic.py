"""GPU: the generic implicit-GEMM conv path of csrc/conv_ops.hip -- s3od_conv_fwd / _dgrad / _wgrad on the gathers of
csrc/gemm.hpp (ConvFwdA, ConvDgradA / ConvDgradB, WgradB) -- element by element against float64 CPU convolutions, in
both compute dtypes, NHWC, weights repacked as the entries document, on tiny maps: the decoder's other geometries
(ConvTranspose 4x4 s4 p0 and 2x2 s2 p0, Conv 3x3 s2 p1) besides 1x1 and 3x3 s1 p1, the parity-class data gradient at
odd map sizes (classes with 1 or 2 taps per axis and unequal row counts), input channels that are no multiple of the
K tile (a K tile spanning two taps: 96 in bf16, 40 in f32 -- and three with 40 channels in bf16, which the gathers
got wrong until these tests: DESIGN.md section 6), output channels 8 / 72 / 136 / 264 (all three
column-tile widths, each with an N tail), and both pixel walkers of the weight gradient.  f32 takes the generic path
at every shape; the bf16 shapes are ones the specialised kernels decline (conv_ops.hip's routing conditions; the 4x4
s2 p1 weight gradient through the S3OD_WGRAD_DMA=0 hook).

Outputs are NaN-poisoned with 64 NaN slack rows around them ("every pixel written": no NaN survives; nothing outside
is touched).  References, caps and the f32 emulation: tests/_gemm_ref.py.  Worst ratios are printed (pytest -s)."""
import pytest
import torch

import _gemm_ref as R

pytestmark = pytest.mark.gpu
NAN = R.NAN


def _lib():
    from s3od_amd._lib import lib, stream
    return lib(), stream()


def _rand(g, *shape, dt=torch.float32, scale=1.0):
    return (torch.randn(*shape, generator=g) * scale).to(dt)


def _nhwc(t):
    """NCHW CPU values -> NHWC rows in a poisoned buffer"""
    return None if t is None else R.poisoned_from(t.permute(0, 2, 3, 1).contiguous())


def _rows(t):
    """NCHW CPU values -> float64 NHWC rows [B H W, C] (the layout of the references' epilogue tensors)"""
    return None if t is None else R.wide(t).permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def _vec(t):
    return None if t is None else R.poisoned_from(t)


def _out_hw(H, W, k, s, p):
    return (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1


_REFS = {}


def _shared(key, make):
    if key not in _REFS:
        _REFS[key] = make()
    return _REFS[key]


def _epi(g, dtype, rows_shape, C, form):
    """the epilogue tensors of one form, CPU: per-channel f32 vectors, residuals in the compute dtype (NCHW)"""
    dt = R.DT[dtype][0]
    B, H, W = rows_shape
    e = dict(bias=None, scale=None, shift=None, res1=None, res2=None)
    if "bias" in form:
        e["bias"] = _rand(g, C, scale=0.5)
    if "affine" in form:
        e["scale"], e["shift"] = torch.rand(C, generator=g) + 0.5, _rand(g, C, scale=0.3)
    if "res1" in form or "mask" in form:
        e["res1"] = _rand(g, B, C, H, W, dt=dt)
    if "res2" in form:
        e["res2"] = _rand(g, B, C, H, W, dt=dt)
    return e


def _epi_ref(e):
    return dict(bias=R.wide(e["bias"]), scale=R.wide(e["scale"]), shift=R.wide(e["shift"]), res1=_rows(e["res1"]), res2=_rows(e["res2"]))


def _check_sums(r, label, cs=None, cs0=None, stats=None):
    if cs is not None:
        R.check(cs, *R.colsum_ref(r, cs0), label=f"{label} colsum")
        assert R.guards_intact(cs)
    if stats is not None:
        from s3od_amd._lib import NREP
        C = r.out.shape[1]
        R.check(stats.view(NREP, 2, C).sum(0), *R.stats_ref(r), label=f"{label} stats")
        assert R.guards_intact(stats)


# ------------------------------------------------------------------------------------------------ s3od_conv_fwd
#   k  s  p   B  H   W  Cin Cout  form (bias / affine = scale + shift / relu / relu_in / res1 / res2 / pre / stats / colsum)
FWD = [
    (3, 2, 1, 2, 7, 9, 64, 72, "bias affine relu"),
    (3, 2, 1, 3, 8, 8, 96, 136, "res1 res2"),
    (4, 4, 0, 2, 8, 12, 40, 8, "bias pre"),
    (2, 2, 0, 2, 6, 10, 64, 264, "relu_in bias"),
    (1, 1, 0, 3, 5, 7, 96, 72, "bias colsum"),
    (1, 1, 0, 2, 5, 7, 40, 264, "relu_in pre"),
    (3, 1, 1, 2, 1, 1, 40, 136, "bias stats"),
    (3, 1, 1, 2, 5, 7, 64, 8, "relu_in res1 pre"),
    (3, 1, 1, 3, 16, 33, 96, 264, "bias affine relu stats colsum"),
    (3, 1, 1, 2, 16, 33, 40, 72, "pre res2"),
    (3, 1, 1, 1, 5, 7, 96, 72, "bias relu pre stats"),
]


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("k,s,p,B,H,W,Cin,Cout,form", FWD, ids=[f"k{c[0]}s{c[1]}p{c[2]}-{c[3]}x{c[4]}x{c[5]}-{c[6]}to{c[7]}" for c in FWD])
def test_conv_fwd(dtype, k, s, p, B, H, W, Cin, Cout, form):
    L, st = _lib()
    dt, code = R.DT[dtype]
    OH, OW = _out_hw(H, W, k, s, p)
    g = torch.Generator().manual_seed(k * 1000 + H * 37 + W + Cin + Cout)
    x, w = _rand(g, B, Cin, H, W, dt=dt), _rand(g, Cout, Cin, k, k, dt=dt, scale=(k * k * Cin) ** -0.5)
    e = _epi(g, dtype, (B, OH, OW), Cout, form)
    act = R.ACT_RELU if "relu" in form.replace("relu_in", "") else R.ACT_NONE
    r = R.ref_conv("fwd", R.wide(x), R.wide(w), stride=s, pad=p, relu_in="relu_in" in form, dtype=dtype, emu=dtype == "f32",
                   act=act, **_epi_ref(e))
    label = f"conv_fwd {dtype} {k}x{k} s{s} p{p} {B}x{H}x{W} {Cin}->{Cout} [{form}]"
    out = R.poisoned((B, OH, OW, Cout), None, dt)
    pre = R.poisoned((B, OH, OW, Cout), None, dt) if "pre" in form else None
    from s3od_amd._lib import NREP
    stats = R.poisoned_from(torch.zeros(NREP * 2 * Cout, dtype=torch.float64)) if "stats" in form else None
    cs0 = _rand(g, Cout) if "colsum" in form else None
    cs = _vec(cs0)
    L("s3od_conv_fwd", code, B, H, W, Cin, OH, OW, Cout, k, k, s, p, _nhwc(x), int("relu_in" in form),
      R.poisoned_from(w.permute(0, 2, 3, 1).contiguous()), _vec(e["bias"]), _vec(e["scale"]), _vec(e["shift"]), act,
      _nhwc(e["res1"]), _nhwc(e["res2"]), out, pre, stats, cs, st)
    torch.cuda.synchronize()
    f32 = dtype == "f32"
    R.check(out.view(-1, Cout), r.out, r.t_out, r.emu_out if f32 else None, r.skip, label=f"{label} out")
    if pre is not None:
        R.check(pre.view(-1, Cout), r.pre, r.t_pre, r.emu_pre if f32 else None, label=f"{label} pre")
    assert R.guards_intact(out) and (pre is None or R.guards_intact(pre))
    _check_sums(r, label, cs, cs0, stats)


# ------------------------------------------------------------------------------------------------ s3od_conv_dgrad
# conv view: the forward conv maps [B, H, W, Cin] -> [B, OH, OW, Cout]; the data gradient (= ConvTranspose2d forward)
# maps dy [B, OH, OW, Cout] -> dx [B, H, W, Cin]
#   k  s  p   B  H   W  Cin Cout  form (+ "wT": the transposed tap-reversed weight is passed)
DGRAD = [
    (4, 4, 0, 2, 12, 20, 72, 96, "bias"),                    # ConvTranspose 4x4 s4 p0
    (2, 2, 0, 3, 10, 14, 136, 40, "bias"),                   # ConvTranspose 2x2 s2 p0
    (3, 2, 1, 2, 7, 9, 40, 64, ""),                           # classes of 4x5, 4x4, 3x5, 3x4 rows; 2 or 1 taps
    (3, 2, 1, 2, 8, 8, 264, 96, ""),
    (3, 2, 1, 3, 7, 9, 72, 40, "bias relu"),
    (3, 1, 1, 2, 5, 7, 72, 40, ""),                          # 3x3 s1 p1 without wT: the transposed-conv gather
    (3, 1, 1, 2, 16, 33, 96, 136, "wT mask res2 colsum"),    # with wT: a forward conv of dy
    (4, 2, 1, 2, 10, 12, 64, 128, "bias relu"),              # the up-sampler (128 -> 64) on the generic path
]


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("k,s,p,B,H,W,Cin,Cout,form", DGRAD, ids=[f"k{c[0]}s{c[1]}p{c[2]}-{c[3]}x{c[4]}x{c[5]}-{c[6]}from{c[7]}" for c in DGRAD])
def test_conv_dgrad(dtype, k, s, p, B, H, W, Cin, Cout, form):
    L, st = _lib()
    dt, code = R.DT[dtype]
    OH, OW = _out_hw(H, W, k, s, p)
    g = torch.Generator().manual_seed(k * 1000 + H * 37 + W + Cin + Cout + 1)
    dy, w = _rand(g, B, Cout, OH, OW, dt=dt), _rand(g, Cout, Cin, k, k, dt=dt, scale=(k * k * Cout / (s * s)) ** -0.5)
    e = _epi(g, dtype, (B, H, W), Cin, form)
    act = R.ACT_RELU_BWD if "mask" in form else R.ACT_RELU if "relu" in form else R.ACT_NONE
    r = R.ref_conv("dgrad", None, R.wide(w), dy=R.wide(dy), stride=s, pad=p, hw=(H, W), dtype=dtype, emu=dtype == "f32",
                   act=act, **_epi_ref(e))
    label = f"conv_dgrad {dtype} {k}x{k} s{s} p{p} -> {B}x{H}x{W} {Cin}<-{Cout} [{form}]"
    dx = R.poisoned((B, H, W, Cin), None, dt)
    cs0 = _rand(g, Cin) if "colsum" in form else None
    cs = _vec(cs0)
    wp = R.poisoned_from(w.permute(0, 2, 3, 1).contiguous())                              # [Cout][KH][KW][Cin]
    wT = R.poisoned_from(w.flip(2, 3).permute(1, 2, 3, 0).contiguous()) if "wT" in form else None   # [Cin][3][3][Cout], taps reversed
    L("s3od_conv_dgrad", code, B, H, W, Cin, OH, OW, Cout, k, k, s, p, _nhwc(dy), wp, _vec(e["bias"]), _vec(e["scale"]),
      _vec(e["shift"]), act, _nhwc(e["res1"]), _nhwc(e["res2"]), dx, None, None, cs, wT, st)
    torch.cuda.synchronize()
    R.check(dx.view(-1, Cin), r.out, r.t_out, r.emu_out if dtype == "f32" else None, r.skip, label=f"{label} dx")
    assert R.guards_intact(dx)
    _check_sums(r, label, cs, cs0)


# ------------------------------------------------------------------------------------------------ s3od_conv_wgrad
#   k  s  p   B  H   W(bf16, f32)  Cin Cout relu_x
WGRAD = [
    (4, 4, 0, 2, 8, (12, 12), 64, 72, False),
    (2, 2, 0, 2, 6, (10, 10), 96, 136, True),
    (3, 2, 1, 2, 7, (9, 9), 40, 8, False),
    (3, 2, 1, 2, 8, (8, 8), 64, 264, True),
    (4, 2, 1, 2, 10, (12, 12), 64, 128, False),        # bf16 with ws: the LDS-DMA kernel's shape, switched off below
    (3, 1, 1, 2, 5, (7, 7), 40, 72, False),
    (3, 1, 1, 3, 16, (33, 33), 96, 136, True),         # ragged width: the per-lane pixel walker
    (3, 1, 1, 2, 3, (64, 32), 64, 72, False),          # output width = one K tile: the uniform walker, image-border tiles
    (2, 2, 0, 2, 4, (128, 64), 40, 136, True),         # the same walker, interior tiles (no bounds test per lane)
]


def _wg_case(dtype, k, s, p, B, H, W, Cin, Cout, relu_x, split):
    def make():
        dt = R.DT[dtype][0]
        OH, OW = _out_hw(H, W, k, s, p)
        g = torch.Generator().manual_seed(k * 1000 + H * 37 + W + Cin + Cout + 2)
        c = dict(x=_rand(g, B, Cin, H, W, dt=dt), dy=_rand(g, B, Cout, OH, OW, dt=dt), dw0=_rand(g, Cout, Cin, k, k))
        # Kc = pixels; one more f32 addition per split (atomics), one for the workspace pass, one into dw
        c["ref"] = R.ref_conv("wgrad", R.wide(c["x"]), torch.empty(Cout, Cin, k, k), dy=R.wide(c["dy"]), stride=s, pad=p,
                              relu_in=relu_x, dw0=R.wide(c["dw0"]), emu=True, extra=split + 2)
        return c
    return _shared((dtype, k, s, p, B, H, W, Cin, Cout, relu_x, split), make)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("with_ws", [False, True])
@pytest.mark.parametrize("split", [1, 3])
@pytest.mark.parametrize("k,s,p,B,H,Ws,Cin,Cout,relu_x", WGRAD, ids=[f"k{c[0]}s{c[1]}p{c[2]}-{c[3]}x{c[4]}x{c[5][0]}-{c[6]}to{c[7]}" for c in WGRAD])
def test_conv_wgrad(monkeypatch, dtype, with_ws, split, k, s, p, B, H, Ws, Cin, Cout, relu_x):
    """dw [Cout][Cin][KH][KW] = dw0 + conv2d_weight(relu?(x), dy) from a non-zero dw0, split-K forced to 1 and 3;
    without ws the atomics go straight into dw's layout, with it they go through the [Cout][tap][Cin] workspace,
    which enters all zero and must leave all zero."""
    L, st = _lib()
    dt, code = R.DT[dtype]
    W = Ws[0] if dtype == "bf16" else Ws[1]
    OH, OW = _out_hw(H, W, k, s, p)
    if (k, s, p) == (4, 2, 1):
        monkeypatch.setenv("S3OD_WGRAD_DMA", "0")
    c = _wg_case(dtype, k, s, p, B, H, W, Cin, Cout, relu_x, split)
    r = c["ref"]
    dw = R.poisoned_from(c["dw0"])
    ws = R.poisoned_from(torch.zeros(Cout * k * k * Cin)) if with_ws else None
    L("s3od_conv_wgrad", code, B, H, W, Cin, OH, OW, Cout, k, k, s, p, _nhwc(c["dy"]), _nhwc(c["x"]), int(relu_x), dw, ws,
      split, None, 0, st)
    torch.cuda.synchronize()
    R.check(dw.view(Cout, -1), r.out, r.t_out, r.emu_out,
            label=f"conv_wgrad {dtype} {k}x{k} s{s} p{p} {B}x{H}x{W} {Cin}->{Cout} relu_x {int(relu_x)} split {split} ws {int(with_ws)}")
    assert R.guards_intact(dw)
    if ws is not None:
        assert int((ws != 0).sum()) == 0 and R.guards_intact(ws), "the workspace must be left all zero"


# ------------------------------------------------------------------------------------------------ rejection
@pytest.mark.parametrize("dtype,Cin", [("bf16", 8), ("bf16", 16), ("f32", 8)])
def test_narrow_conv_is_rejected(dtype, Cin):
    """2 Cin < BK (bf16: K tiles of 64, f32: of 32): a K tile would span more than two taps, which the gathers do
    not walk.  Forward, data gradient and weight gradient all refuse on the host and leave their outputs alone."""
    from s3od_amd._lib import HipLibError
    L, st = _lib()
    dt, code = R.DT[dtype]
    B, H, W, Cout, k = 2, 5, 7, 72, 3
    g = torch.Generator().manual_seed(Cin)
    x, dy = _nhwc(_rand(g, B, Cin, H, W, dt=dt)), _nhwc(_rand(g, B, Cout, H, W, dt=dt))
    wp = R.poisoned_from(_rand(g, Cout, k, k, Cin, dt=dt))
    out, dx, dw = R.poisoned((B, H, W, Cout), None, dt), R.poisoned((B, H, W, Cin), None, dt), R.poisoned((Cout, Cin, k, k), None)
    with pytest.raises(HipLibError):
        L("s3od_conv_fwd", code, B, H, W, Cin, H, W, Cout, k, k, 1, 1, x, 0, wp, None, None, None, R.ACT_NONE, None, None,
          out, None, None, None, st)
    with pytest.raises(HipLibError):
        L("s3od_conv_dgrad", code, B, H, W, Cin, H, W, Cout, k, k, 1, 1, dy, wp, None, None, None, R.ACT_NONE, None, None,
          dx, None, None, None, None, st)
    with pytest.raises(HipLibError):
        L("s3od_conv_wgrad", code, B, H, W, Cin, H, W, Cout, k, k, 1, 1, dy, x, 0, dw, None, 0, None, 0, st)
    torch.cuda.synchronize()
    for name, t in (("out", out), ("dx", dx), ("dw", dw)):
        assert bool(torch.isnan(t).all()) and R.guards_intact(t), f"{name} was written by a rejected call"
