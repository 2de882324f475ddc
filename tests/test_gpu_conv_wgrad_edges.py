"""GPU: the hand-pipelined weight-gradient kernels -- the register-staged halo kernel and the 4x4 s2 LDS-DMA kernel of
csrc/gemm_ops.hip, the LDS-DMA 3x3 kernel of csrc/wgrad_dma.hip, the ping-pong Wgrad3B instance -- and the ping-pong
Conv3A forward / data-gradient-as-forward instance, per element against a float64 reference of the same bf16 operands
computed on the device, through s3od_conv_wgrad / s3od_conv_fwd / s3od_conv_dgrad, in the two data modes of
tests/_gemm_ref.py (see test_gpu_conv_rw_edges.py).

Exact mode is the discriminating one here: the random mode's cap (K + 8 + extra) 2^-23 S has K = the pixel count and is
far wider than one missing product at any useful size, while with integer operands one missing or doubled product of
one tile is a mismatch.  In random mode `extra` counts the f32 additions outside the MFMA chain from a restatement of
the launcher: the wpc atomic flushes onto one element (or the split-K slabs), the permute add and the += dw0; the f32
chain emulation runs over a slice of output channels where pixels x slice x taps x Cin stays affordable, and the test
prints where it is skipped.

The weight-gradient launchers give each of the nblk 64 x 64 channel blocks wpc = max(1, min(T, C / nblk)) workgroups
with contiguous tile ranges [T wi / wpc, T (wi + 1) / wpc), double-buffered (two-slot loops with an odd tail).  Shapes
are derived from the CU count C so that the workgroups own 1 tile, 2 and 3, and 5 and 6 tiles (odd and even counts),
by choosing channel blocks rather than large maps; the multi-tile shapes have B, tiles_x, tiles_y all different, and an
image boundary strictly inside some workgroup's range (asserted from the restated schedule).  Every case asserts the
route from a restatement of conv_wgrad_route / conv_pp_ok, poisons dw's and ws's surroundings and the inputs (except
the dy of the 96-channel LDS-DMA case, whose padded second block legitimately reads the next pixel's channels), and
requires the workspace to be left all zero.

The exact 1 x 512 x 520 128 -> 192 case subsumes that case of test_gpu_conv_halo.py::
test_conv_wgrad_halo_channel_blocks; the ping-pong cases subsume test_gpu_conv_pp.py (same 4 x 61 x 269 shape)."""
import ctypes

import pytest
import torch

import _gemm_ref as R
from test_gpu_conv_rw_edges import BF16, _acts, _cus, _lib, _nchw64, _rows64, _vec, _weights, knob

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ host predicates
def wgrad_route(B, H, W, Cin, OH, OW, Cout, KH, KW, stride, pad, relu_x, dma_on=True, pp_on=True, slab_on=True, split=0):
    """conv_wgrad_route of csrc/conv_ops.hip for bf16 with a workspace: (path, split)"""
    if KH == 4 and KW == 4 and stride == 2 and pad == 1 and H == 2 * OH and W == 2 * OW and Cin % 64 == 0 and Cout % 64 == 0 \
            and not relu_x and H * W * Cin * 2 < 2 ** 31 and OH * OW * Cout * 2 < 2 ** 31 and dma_on:
        return "Dma4s2", 0
    if not (KH == 3 and KW == 3 and stride == 1 and pad == 1 and OH == H and OW == W):
        return "Igemm", 0
    blocks = Cin % 64 == 0 and (Cout % 64 == 0 or (Cout == 96 and Cin == 64))
    if blocks and H % 8 == 0 and W % 32 == 0 and H * W * max(Cin, Cout) * 2 < 2 ** 31 and dma_on:
        return "Dma3x3", 0
    if Cin % 64 == 0 and (Cout % 64 == 0 or Cout == 96) and (Cin == 64 or H * W >= 512 * 512):
        return "Halo", 0
    if W % 64 == 0 and Cin % 256 == 0 and Cout % 256 == 0 and (H * W >= 128 * 128 or Cin >= 512) and pp_on:
        ktiles, tiles = B * OH * OW // 64, (Cout // 256) * (9 * Cin // 256)
        sp = split if split > 0 else max(1, min(256 // tiles, ktiles // 8))
        return ("PpSlab" if slab_on and sp > 1 else "PpAtomic"), sp
    return "Igemm", 0


def nblk_of(path, Cin, Cout):
    """channel blocks per launcher: the halo kernel runs Cout 96 as one block, the LDS-DMA one as two"""
    if path == "Halo":
        return (Cout // (64 if Cout % 64 == 0 else 96)) * (Cin // 64)
    return -(-Cout // 64) * (Cin // 64)


def conv_pp_ok(B, H, W, SC, N, stats, on=True):
    """conv_pp_ok of csrc/conv_ops.hip for a 3x3 s1 p1 bf16 conv of SC input channels to N outputs"""
    M, nch = B * H * W, SC // 64
    tiles = (M // 256) * (N // 256)
    rounds = tiles >= 2048 or SC >= 512 or (tiles >= 512 and not stats)
    t2 = (M // 256) * -(-N // 256)
    pays = t2 >= 256 and t2 / (-(-t2 // 256) * 256) >= 0.95
    return SC >= 256 and SC % 64 == 0 and nch & (nch - 1) == 0 and N % 256 == 0 and pays and rounds and on


def tiles_shape(nblk, want, TH, TW, whole):
    """(B, H, W, wpc): a map of TH x TW tiles whose workgroups own exactly the tile counts `want`, with an image boundary
    strictly inside some workgroup's range where a range has more than one tile.  First choice: the smallest with B >= 2,
    tiles_x >= 2, tiles_y >= 3 all different; where wpc is too small for that (32 channel blocks on 256 CUs leave 8
    workgroups per block: 8 or fewer tiles for one each) the largest map that has no other counts, B >= 2 if it can."""
    C = _cus()

    def fits(T, strict):
        wpc, sched = R.wgrad_schedule(T, C, nblk)
        if not ({len(s) for s in sched} == set(want) if strict else {len(s) for s in sched} <= set(want)):
            return None
        for B in (2, 3) if strict else (2, 3, 1):
            for tx in (2, 3, 4, 5, 7) if strict else (3, 2, 1):
                ty = T // (B * tx)
                if B * tx * ty != T or ty < (3 if strict else 1) or (strict and len({B, tx, ty}) != 3):
                    continue
                if max(want) > 1 and not R.crosses_image(sched, tx * ty):
                    continue
                return B, (TH * ty if whole else TH * ty - 3), (TW * tx if whole else TW * (tx - 1) + 7), wpc
        return None

    for strict, order in ((True, range(1, 8 * C)), (False, range(8 * C, 0, -1))):
        for T in order:
            got = fits(T, strict)
            if got:
                return got
    raise AssertionError(f"no shape for nblk {nblk} with {want} tiles per workgroup on {C} CUs")


COUNTS = {"one": (1,), "two3": (2, 3), "five6": (5, 6)}


def _wgrad_emu(dy, x, dw0, k, stride, pad, relu_x, taps_cin, budget=6e8):
    """f32 chain over the pixels for the first output channels that fit the budget: (emulation [n, Cin k k], n) or None"""
    npix, Cout = dy.shape[0] * dy.shape[1] * dy.shape[2], dy.shape[3]
    n = int(min(Cout, budget // (npix * taps_cin)))
    if n < 4 or npix * taps_cin > 6e7:
        return None, 0
    xc = x.detach().cpu().float().permute(0, 3, 1, 2)
    cols = R.conv_cols(xc.clamp_min(0) if relu_x else xc, k, k, stride, pad)
    e = R.chain(dy.detach().cpu().float().reshape(npix, Cout)[:, :n].T.contiguous(), cols)
    Cin = x.shape[3]
    return e.view(n, k * k, Cin).permute(0, 2, 1).reshape(n, -1) + dw0.detach().cpu().reshape(Cout, -1)[:n].float(), n


def _run_wgrad(mode, label, B, H, W, Cin, OH, OW, Cout, k, stride, pad, relu_x, path, extra, seed, knobs=None, slab=None,
               slab_bytes=0, share=None):
    """one s3od_conv_wgrad call against its reference; share: a dict that keeps the operands and the reference"""
    L, st = _lib()
    if share is None or "r" not in share:
        dy = _acts(mode, (B, OH, OW, Cout), seed)
        if path == "Dma3x3" and Cout == 96:
            dy = dy.clone()                                # dense and finite: the padded block reads the next pixel's channels
        x = _acts(mode, (B, H, W, Cin), seed + 1)
        dw0 = R.small_ints((Cout, Cin, k, k), seed + 2) if mode == "exact" else \
            torch.randn(Cout, Cin, k, k, device=R.DEVICE, generator=torch.Generator(device=R.DEVICE).manual_seed(seed + 2))
        r = R.ref_conv("wgrad", _nchw64(x), torch.empty(Cout, Cin, k, k), dy=_nchw64(dy), stride=stride, pad=pad,
                       relu_in=bool(relu_x), dw0=R.wide(dw0, R.DEVICE), extra=extra)
        if mode == "exact":
            R.assert_exact_domain([r.S + R.wide(dw0, R.DEVICE).abs().reshape(Cout, -1)])
        emu, n = (None, 0)
        if mode == "random":
            emu, n = _wgrad_emu(dy, x, dw0, k, stride, pad, relu_x, k * k * Cin)
            if emu is None:
                print(f"[{label}] emulation skipped ({B * OH * OW} pixels x {k * k * Cin}); the exact mode carries this case")
        s = dict(dy=dy, x=x, dw0=dw0, r=r, emu=emu, n=n)
        if share is not None:
            share.update(s)
    else:
        s = share
    dw = R.poisoned_from(s["dw0"])
    ws = R.poisoned_from(torch.zeros(Cout * k * k * Cin, device=R.DEVICE))
    with knob(**(knobs or {})):
        L("s3od_conv_wgrad", BF16, B, H, W, Cin, OH, OW, Cout, k, k, stride, pad, s["dy"], s["x"], int(relu_x), dw, ws, 0, slab,
          slab_bytes, st)
        torch.cuda.synchronize()
    r = s["r"]
    if mode == "exact":
        R.check_exact(dw.view(Cout, -1), r.out, label)
    else:
        R.check(dw.view(Cout, -1), r.out, r.t_out, label=label)
        if s["emu"] is not None:
            n = s["n"]
            R.check(dw.view(Cout, -1)[:n], r.out[:n], r.t_out[:n], s["emu"], label=f"{label} [{n} channels vs emulation]")
    assert R.guards_intact(dw) and R.guards_intact(ws), f"{label}: a guard row was written"
    assert int((ws != 0).sum()) == 0, f"{label}: the workspace is not left all zero"
    return dw


# ------------------------------------------------------------------------------------------------ 3x3: halo and LDS-DMA
#        path     Cin Cout relu  shape: (B, H, W) or the tile counts per workgroup
W3 = [("Halo", 64, 64, 0, (1, 5, 19)), ("Halo", 64, 64, 1, "one"), ("Halo", 64, 96, 1, (2, 19, 45)), ("Halo", 64, 96, 0, "one"),
      ("Halo", 64, 512, 0, "one"), ("Halo", 64, 512, 1, "two3"), ("Halo", 64, 512, 0, "five6"),
      ("Dma3x3", 64, 64, 1, (1, 8, 32)), ("Dma3x3", 64, 64, 0, "one"), ("Dma3x3", 64, 96, 0, (2, 8, 32)), ("Dma3x3", 64, 96, 1, "one"),
      ("Dma3x3", 512, 256, 1, "one"), ("Dma3x3", 512, 256, 0, "two3"), ("Dma3x3", 512, 256, 1, "five6")]


@pytest.mark.parametrize("mode", ["exact", "random"])
@pytest.mark.parametrize("path,Cin,Cout,relu,shape", W3, ids=[f"{c[0]}-{c[1]}to{c[2]}-relu{c[3]}-{c[4] if isinstance(c[4], str) else 'x'.join(map(str, c[4]))}" for c in W3])
def test_wgrad3x3(path, Cin, Cout, relu, shape, mode):
    """3x3 s1 p1 weight gradients added onto an existing gradient: the register-staged halo kernel on ragged maps (one
    image smaller than a tile, Cout 96 as one block, 64 -> 512 as 8 blocks) and the LDS-DMA kernel on whole tiles (a
    one-tile image, Cout 96 as a padded second block, 512 -> 256 as 32 blocks)."""
    C = _cus()
    nblk = nblk_of(path, Cin, Cout)
    if isinstance(shape, str):
        B, H, W, wpc = tiles_shape(nblk, COUNTS[shape], 8, 32, path == "Dma3x3")
    else:
        B, H, W = shape
        wpc = R.wgrad_schedule(B * -(-H // 8) * -(-W // 32), C, nblk)[0]
    assert wgrad_route(B, H, W, Cin, H, W, Cout, 3, 3, 1, 1, relu)[0] == path
    label = f"wgrad {path} {Cin}->{Cout} relu{relu} {B}x{H}x{W} wpc={wpc} {mode}"
    _run_wgrad(mode, label, B, H, W, Cin, H, W, Cout, 3, 1, 1, relu, path, wpc + 2, 100 + Cin + Cout + relu)


def test_wgrad_halo_512sq_channel_blocks_exact():
    """1 x 512 x 520, 128 -> 192 with a ReLU'd input in exact mode: the halo kernel over 6 channel blocks, 25 / 26 tiles
    per workgroup on 256 CUs (the random-mode cap at 266 240 pixels is ~3 % of S: blind to a missing tile)."""
    B, H, W, Cin, Cout = 1, 512, 520, 128, 192
    assert wgrad_route(B, H, W, Cin, H, W, Cout, 3, 3, 1, 1, 1)[0] == "Halo"
    wpc = R.wgrad_schedule(64 * 17, _cus(), nblk_of("Halo", Cin, Cout))[0]
    _run_wgrad("exact", f"wgrad Halo {Cin}->{Cout} relu1 {B}x{H}x{W} wpc={wpc} exact", B, H, W, Cin, H, W, Cout, 3, 1, 1, 1, "Halo",
               wpc + 2, 7)


# ------------------------------------------------------------------------------------------------ 4x4 s2 LDS-DMA
@pytest.mark.parametrize("mode", ["exact", "random"])
@pytest.mark.parametrize("shape", [(1, 1, 19), "one", "two3", "five6"], ids=["1x1x19", "one", "two3", "five6"])
def test_wgrad4s2_dma(shape, mode):
    """the 4x4 s2 p1 conv view of upsample_2x.0 (x 64 channels on 2 OH x 2 OW, dy 128 on OH x OW; dy tiles of 2 x 32):
    one image of a single partial tile, then odd OH and OW % 32 != 0 at 1, 2-3 and 5-6 tiles per workgroup."""
    C = _cus()
    if isinstance(shape, str):
        B, OH, OW, wpc = tiles_shape(2, COUNTS[shape], 2, 32, False)
        OH += 2                                            # 2 ty - 3 + 2: odd, the same tile rows
    else:
        B, OH, OW = shape
        wpc = R.wgrad_schedule(B * -(-OH // 2) * -(-OW // 32), C, 2)[0]
    assert OH % 2 == 1 and OW % 32
    assert wgrad_route(B, 2 * OH, 2 * OW, 64, OH, OW, 128, 4, 4, 2, 1, 0)[0] == "Dma4s2"
    label = f"wgrad Dma4s2 64->128 {B}x{OH}x{OW} wpc={wpc} {mode}"
    _run_wgrad(mode, label, B, 2 * OH, 2 * OW, 64, OH, OW, 128, 4, 2, 1, 0, "Dma4s2", wpc + 2, 300 + OH)


# ------------------------------------------------------------------------------------------------ ping-pong Wgrad3B
@pytest.mark.parametrize("mode", ["exact", "random"])
@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("B,H,W", [(3, 7, 64), (3, 20, 64)])
def test_wgrad_pp(B, H, W, relu, mode):
    """512 -> 256 on maps the route sends to the ping-pong kernel (odd or non-multiple-of-8 H: no LDS-DMA; Cin >= 512):
    split-K 2 and 7, into a poisoned caller slab (wholly written: no NaN reaches dw, none is left in the slab) and by
    atomics into ws (no slab given); S3OD_WGRAD_PP=0 is the 128x128 implicit GEMM on the same check."""
    L, st = _lib()
    Cin, Cout = 512, 256
    path, sp = wgrad_route(B, H, W, Cin, H, W, Cout, 3, 3, 1, 1, relu)
    assert path == "PpSlab" and sp == {21: 2, 60: 7}[B * H]
    nb = ctypes.c_long(-1)
    L("s3od_conv_wgrad_ws", BF16, B, H, W, Cin, H, W, Cout, 3, 3, 1, 1, 0, ctypes.addressof(nb))
    assert nb.value == 4 * sp * Cout * 9 * Cin
    share = {}
    label = f"wgrad pp {Cin}->{Cout} relu{relu} {B}x{H}x{W} split {sp} {mode}"
    slab = R.poisoned((nb.value // 4,), None, torch.float32)
    _run_wgrad(mode, label + " slab", B, H, W, Cin, H, W, Cout, 3, 1, 1, relu, path, sp + 2, 400 + H + relu, None, slab, nb.value, share)
    assert bool(torch.isfinite(slab).all()) and R.guards_intact(slab), "the slab was not wholly written"
    _run_wgrad(mode, label + " atomic", B, H, W, Cin, H, W, Cout, 3, 1, 1, relu, path, sp + 2, 0, None, None, 0, share)
    assert wgrad_route(B, H, W, Cin, H, W, Cout, 3, 3, 1, 1, relu, pp_on=False)[0] == "Igemm"
    # the implicit GEMM chooses its own split-K (wgrad_split: at most a quarter of the 64-pixel K tiles): its cap takes
    # that many partials; the same seeds give the same operands
    _run_wgrad(mode, label + " igemm", B, H, W, Cin, H, W, Cout, 3, 1, 1, relu, path, -(-B * H * W // 64) // 4 + 2, 400 + H + relu,
               {"S3OD_WGRAD_PP": "0"})


# ------------------------------------------------------------------------------------------------ ping-pong Conv3A
PP_SHAPE = (4, 61, 269)          # M = 65636 = 256 panels of 256 rows + a 100-row tail: the smallest shape conv_pp_ok takes
_PP = {}


def _pp_case(mode, relu_in):
    """operands and the float64 contraction of the 512 -> 256 conv at PP_SHAPE (155 GFLOP each for the sum and its
    absolute twin, on the device), shared by the variants and left unchanged"""
    key = (mode, relu_in)
    if key not in _PP:
        if any(k[1] != relu_in for k in _PP):
            _PP.clear()                                    # the two modes of one input form resident at a time
        B, H, W = PP_SHAPE
        x = _acts(mode, (B, H, W, 512), 61)
        w = _weights(mode, (256, 512, 3, 3), 62, 0.02)
        x64 = _nchw64(x).clamp_min(0) if relu_in else _nchw64(x)
        acc = R._nhwc2d(R.conv2d64(x64, R.wide(w, R.DEVICE), 1, 1))
        S = R._nhwc2d(R.conv2d64(x64.abs(), R.wide(w, R.DEVICE).abs(), 1, 1))
        _PP[key] = (x, w, acc, S)
    return _PP[key]


@pytest.mark.parametrize("mode", ["exact", "random"])
@pytest.mark.parametrize("form", ["relu_in bias stats", "bias res1 res2", "dgrad mask res2 colsum"])
def test_conv3a_pp(form, mode):
    """The 256x256 ping-pong kernel with the Conv3A loader at its smallest shape, 4 x 61 x 269, K = 9 x 512, N = 256, with
    the M tail: forward with a ReLU'd input + bias + BN statistics (float64, the 32 replicas summed), forward with both
    residual adds, and the data-gradient form (s3od_conv_dgrad with wT: a forward conv of a 512-channel dy) with the ReLU'
    mask, the residual gradient and column sums.  S3OD_CONV_PP=0 is the 128x128 implicit GEMM on the same check."""
    from s3od_amd._lib import NREP
    L, st = _lib()
    B, H, W = PP_SHAPE
    relu_in, dgrad = "relu_in" in form, "dgrad" in form
    stats_on = "stats" in form
    assert conv_pp_ok(B, H, W, 512, 256, stats_on) and not conv_pp_ok(B, H, W, 512, 256, stats_on, on=False)
    assert (B * H * W) % 256 == 100
    x, w, acc, S = _pp_case(mode, relu_in)                 # dgrad form: x is dy, w = the forward conv of dy's weight
    bias = None if dgrad else _vec(mode, 256, 63, 0.1)
    res1 = _acts(mode, (B, H, W, 256), 64) if ("res1" in form or "mask" in form) else None
    res2 = _acts(mode, (B, H, W, 256), 65) if "res2" in form else None
    act = R.ACT_RELU_BWD if dgrad else R.ACT_NONE
    r = R.finish(acc, S, 9 * 512, "bf16", bias=R.wide(bias, R.DEVICE), act=act, res1=None if res1 is None else _rows64(res1),
                 res2=None if res2 is None else _rows64(res2))
    if mode == "exact":
        R.assert_exact_domain([S + (0 if bias is None else R.wide(bias, R.DEVICE).abs()) + 2], [r.out])
    print(f"[conv3a {form} {mode}] f32 emulation skipped (65636 x 256 outputs x K 4608; bf16 outputs); the exact mode carries it")
    wp = R.poisoned_from(w.permute(0, 2, 3, 1).contiguous())         # [256][3][3][512]: the forward pack, or wT of the dgrad form
    cs0 = _vec(mode, 256, 66, 1.0) if "colsum" in form else None
    for name, kv in (("pp", {}), ("igemm", {"S3OD_CONV_PP": "0"})):
        out = R.poisoned((B, H, W, 256), None, torch.bfloat16)
        stats = R.poisoned_from(torch.zeros(NREP * 2 * 256, dtype=torch.float64, device=R.DEVICE)) if stats_on else None
        cs = None if cs0 is None else R.poisoned_from(cs0.clone())
        with knob(**kv):
            if dgrad:
                # the conv whose data gradient this is has 256 input and 512 output channels; its own pack (only read by
                # the transposed-conv gather, which a call with wT never takes) is wT transposed back with the taps reversed
                wfwd = R.poisoned_from(w.flip(2, 3).permute(1, 2, 3, 0).contiguous())          # [512][3][3][256]
                L("s3od_conv_dgrad", BF16, B, H, W, 256, H, W, 512, 3, 3, 1, 1, x, wfwd, None, None, None, act, res1, res2, out,
                  None, None, cs, wp, st)
            else:
                L("s3od_conv_fwd", BF16, B, H, W, 512, H, W, 256, 3, 3, 1, 1, x, int(relu_in), wp, bias, None, None, act, res1,
                  res2, out, None, stats, cs, st)
            torch.cuda.synchronize()
        label = f"conv3a {form} {name} {mode}"
        if mode == "exact":
            R.check_exact(out.view(-1, 256), r.out, label)
        else:
            R.check(out.view(-1, 256), r.out, r.t_out, None, r.skip, label=label)
        assert R.guards_intact(out)
        if stats is not None:
            got, (sref, st_t) = stats.view(NREP, 2, 256).sum(0), R.stats_ref(r)
            if mode == "exact":
                R.check_exact(got, sref, label + " stats")
            else:
                R.check(got, sref, st_t, label=label + " stats")
            assert R.guards_intact(stats)
        if cs is not None:
            cref, ct = R.colsum_ref(r, R.wide(cs0, R.DEVICE))
            if mode == "exact":
                R.assert_exact_domain([r.out.abs().sum(0) + R.wide(cs0, R.DEVICE).abs()])
                R.check_exact(cs, cref, label + " colsum")
            else:
                R.check(cs, cref, ct, label=label + " colsum")
            assert R.guards_intact(cs)
