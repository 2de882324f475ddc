"""CPU: the float64 reference, cap and emulation of tests/_gemm_ref.py have teeth.  f32 stand-ins for the kernel
(torch's f32 matmul / conv, and the sequential chain itself) must pass check(); each planted error -- the ways a GEMM
or implicit-GEMM kernel goes subtly wrong -- must fail it.  A planted error need not exceed the cap in every element
(a dropped 32-deep k-step exceeds it in 100 % / 99 % / 89 % of the elements at K = 72 / 776 / 3072 with bf16 operands):
the assertion is that check() fails, i.e. that some element does."""
import pytest
import torch
import torch.nn.functional as F

import _gemm_ref as R

SHAPES = [(130, 96, 72), (130, 96, 776), (130, 96, 3072)]


def _operands(M, N, K, bf16=True):
    g = torch.Generator().manual_seed(M + N + K)
    x, w = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g)
    bias = 2 * torch.randn(N, generator=g)
    if bf16:
        x, w = x.bfloat16().float(), w.bfloat16().float()
    return x, w, bias


_CACHE = {}


def _case(M, N, K, bf16=True):
    """(x, w, bias, Ref with the chain emulation): computed once per shape and left unchanged"""
    key = (M, N, K, bf16)
    if key not in _CACHE:
        x, w, bias = _operands(M, N, K, bf16)
        _CACHE[key] = (x, w, bias, R.ref_linear(x.double(), w.double().T, "f32", emu=True, bias=bias.double()))
    return _CACHE[key]


@pytest.mark.parametrize("bf16", [True, False])
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_standins_pass(M, N, K, bf16):
    x, w, bias, r = _case(M, N, K, bf16)
    R.check(x @ w.T + bias, r.out, r.t_out, r.emu_out, label=f"matmul {M}x{N}x{K}")
    R.check(r.emu_out, r.out, r.t_out, r.emu_out, label=f"chain {M}x{N}x{K}")
    # a bf16 store of the same values passes the bf16 cap
    rb = R.ref_linear(x.double(), w.double().T, "bf16", bias=bias.double())
    R.check((x @ w.T + bias).bfloat16(), rb.out, rb.t_out, label=f"matmul -> bf16 {M}x{N}x{K}")


def _fails(got, r, match=None, **kw):
    with pytest.raises(AssertionError, match=match):
        R.check(got, r.out, r.t_out, r.emu_out, **kw)


@pytest.mark.parametrize("M,N,K", SHAPES)
def test_dropped_k_step(M, N, K):
    x, w, bias, r = _case(M, N, K)
    xd = x.clone()
    xd[:, 32:64] = 0
    _fails(xd @ w.T + bias, r, match="cap", label="k-step dropped")


@pytest.mark.parametrize("M,N,K", SHAPES)
def test_dropped_k_element(M, N, K):
    """one k of 3072 with |x| ~ 0.1 moves an element by ~1e-4 of S: inside the cap, but far outside what f32
    accumulation does -- the comparison with the emulation catches it"""
    x, w, bias, r = _case(M, N, K)
    xd = x.clone()
    k = int((x[57].abs() - 0.1).abs().argmin())
    xd[57, k] = 0
    _fails(xd @ w.T + bias, r, match="emulation" if K == 3072 else None, label="k element dropped")


@pytest.mark.parametrize("M,N,K", SHAPES)
def test_segment_from_neighbouring_row(M, N, K):
    x, w, bias, r = _case(M, N, K)
    o = x @ w.T + bias
    o[57, 40:48] = o[58, 40:48]
    _fails(o, r, label="segment of the next row")


@pytest.mark.parametrize("M,N,K", SHAPES)
def test_bias_of_column_plus_8(M, N, K):
    x, w, bias, r = _case(M, N, K)
    _fails(x @ w.T + bias.roll(-8), r, label="bias[n + 8]")


@pytest.mark.parametrize("M,N,K", SHAPES)
def test_unwritten_element_and_relu_share(M, N, K):
    x, w, bias, r = _case(M, N, K)
    o = x @ w.T + bias
    o[M - 1, N - 1] = R.NAN
    _fails(o, r, match="not finite", label="tail element never written")
    # a ReLU case whose reference sits on the kink too often is refused, not skipped through
    rr = R.ref_linear(x.double(), torch.zeros_like(w).double().T, "f32", act=R.ACT_RELU)
    with pytest.raises(AssertionError, match="kink"):
        R.check(torch.zeros(M, N), rr.out, rr.t_out, skip=rr.skip, label="all on the kink")


def test_rope_partner_sign():
    B, Ntok, P, H = 2, 9, 4, 1
    D = 64 * H
    g = torch.Generator().manual_seed(3)
    x, w = torch.randn(B * Ntok, D, generator=g).bfloat16().double(), torch.randn(3 * D, D, generator=g).bfloat16().double()
    bias = torch.randn(3 * D, generator=g).double()
    ang = torch.rand(P, 64, generator=g).double() * 6.28
    ref = R.ref_qkv_rope(x, w, bias, ang.cos(), ang.sin(), B, Ntok, P, H, "f32")

    def standin(sign):
        a = (x.float() @ w.float().T + bias.float()).view(B, Ntok, 3, H, 64)
        out = []
        for i in range(3):
            t = a[:, :, i].clone()
            if i < 2:
                rot = torch.cat([-sign * t[..., 32:], sign * t[..., :32]], -1)
                t[:, Ntok - P:] = t[:, Ntok - P:] * ang.cos().float().view(1, P, 1, 64) + rot[:, Ntok - P:] * ang.sin().float().view(1, P, 1, 64)
            if i == 0:
                t = t * R.QSCALE
            out.append(t.permute(0, 2, 1, 3))
        return out
    for name, got in zip("qkv", standin(1.0)):
        R.check(got, *ref[name], label=f"rope {name}")
    bad = standin(-1.0)
    for i, name in enumerate("qk"):
        with pytest.raises(AssertionError):
            R.check(bad[i], *ref[name], label=f"rope {name}, partner sign flipped")
    # prefix tokens are not rotated: the flipped sign leaves them right
    R.check(bad[0][:, :, :Ntok - P], ref["q"][0][:, :, :Ntok - P], ref["q"][1][:, :, :Ntok - P], label="rope q prefix rows")


def test_prefix_offset_off_by_one():
    B, P, prefix, N, K = 3, 7, 5, 16, 40
    g = torch.Generator().manual_seed(4)
    x, w = torch.randn(B * P, K, generator=g), torch.randn(N, K, generator=g)
    r = R.ref_linear(x.double(), w.double().T, "f32", emu=True)
    o = x @ w.T
    for off, ok in ((0, True), (-1, False), (1, False)):
        full = torch.full((B * (P + prefix), N), R.NAN)
        rows = R.token_rows(B, P, prefix) + off
        full[rows[rows < full.shape[0]]] = o[rows < full.shape[0]]
        if ok:
            R.check_token_rows(full, r.out, r.t_out, B, P, prefix, r.emu_out, label="token rows")
        else:
            with pytest.raises(AssertionError):
                R.check_token_rows(full, r.out, r.t_out, B, P, prefix, r.emu_out, label=f"token rows off by {off}")


def _conv_operands(B, Cin, Cout, H, W, KH, KW, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, Cin, H, W, generator=g).bfloat16().float(),
            (torch.randn(Cout, Cin, KH, KW, generator=g) * 0.1).bfloat16().float())


def test_dgrad_parity_class_shifted():
    """3x3 s2 p1 data gradient onto 7 x 9: class (1, 0) moved one pixel along x"""
    B, Cin, Cout, H, W = 2, 16, 24, 7, 9
    _, w = _conv_operands(B, Cin, Cout, H, W, 3, 3, 5)
    dy = torch.randn(B, Cout, 4, 5, generator=torch.Generator().manual_seed(6)).bfloat16().float()
    r = R.ref_conv("dgrad", None, w.double(), dy=dy.double(), stride=2, pad=1, hw=(H, W), emu=True)
    o = F.conv_transpose2d(dy, w, stride=2, padding=1)
    assert o.shape[2:] == (H, W)
    R.check(o.permute(0, 2, 3, 1).reshape(-1, Cin), r.out, r.t_out, r.emu_out, label="dgrad 3x3 s2")
    o[:, :, 1::2, 0::2] = o[:, :, 1::2, 0::2].roll(1, 3)
    _fails(o.permute(0, 2, 3, 1).reshape(-1, Cin), r, label="dgrad class (1, 0) shifted")


def test_conv_tap_uses_next_taps_weights():
    B, Cin, Cout, H, W = 2, 16, 24, 5, 7
    x, w = _conv_operands(B, Cin, Cout, H, W, 3, 3, 7)
    r = R.ref_conv("fwd", x.double(), w.double(), stride=1, pad=1, emu=True)
    R.check(F.conv2d(x, w, padding=1).permute(0, 2, 3, 1).reshape(-1, Cout), r.out, r.t_out, r.emu_out, label="conv 3x3")
    wb = w.clone()
    wb[:, :, 1, 1] = w[:, :, 1, 2]
    _fails(F.conv2d(x, wb, padding=1).permute(0, 2, 3, 1).reshape(-1, Cout), r, label="tap (1, 1) with the weights of (1, 2)")
    # the weight gradient reference and its chain agree with torch's f32 one
    dy = torch.randn(B, Cout, H, W, generator=torch.Generator().manual_seed(8)).bfloat16().float()
    dw0 = torch.randn(Cout, Cin, 3, 3, generator=torch.Generator().manual_seed(9))
    rw = R.ref_conv("wgrad", x.double(), w.double(), dy=dy.double(), stride=1, pad=1, dw0=dw0.double(), emu=True)
    got = dw0 + torch.nn.grad.conv2d_weight(x, w.shape, dy, padding=1)
    R.check(got.reshape(Cout, -1), rw.out, rw.t_out, rw.emu_out, label="conv wgrad")
    _fails(got.roll(1, 3).reshape(Cout, -1), rw, label="conv wgrad, taps rolled")


# ------------------------------------------------------------------------------------------------ hand-pipelined convs
# The ways the persistent LDS-DMA kernels (gemm_ops.hip, wgrad_dma.hip) go wrong, planted into a correct result, in the
# two data modes of test_gpu_conv_rw_edges.py / test_gpu_conv_wgrad_edges.py: "random" (randn operands, the per-element
# cap of check()) and "exact" (integer operands, equality).  64 -> 64 3x3 + bias + ReLU on 2 x 19 x 45: 2 x 3 tiles of
# 8 x 32 per image, ragged at the right and bottom.
HP = dict(B=2, H=19, W=45, C=64)


def _hp_operands(mode, cout=64):
    B, H, W, C = HP["B"], HP["H"], HP["W"], HP["C"]
    if mode == "exact":
        return (R.ints((B, C, H, W), 1, device="cpu").double(), R.ints((cout, C, 3, 3), 2, 0.125, device="cpu").double(),
                R.small_ints((cout,), 3, device="cpu").double())
    g = torch.Generator().manual_seed(19 * 45)
    x = torch.randn(B, C, H, W, generator=g).bfloat16().double()
    w = (torch.randn(cout, C, 3, 3, generator=g) * 0.06).bfloat16().double()      # the scale of test_gpu_conv_halo.py
    return x, w, (torch.randn(cout, generator=g) * 0.1).double()


def _hp_judge(mode, got_pre, r, caught, label):
    """got_pre: float64 accumulators [B, C, H, W] of a stand-in kernel -> bias + ReLU -> bf16, judged by the mode"""
    got = (got_pre.permute(0, 2, 3, 1).reshape(-1, got_pre.shape[1]) + r.bias_rows).clamp_min(0).float().bfloat16()
    judge = (lambda: R.check_exact(got, r.out, label)) if mode == "exact" else \
            (lambda: R.check(got, r.out, r.t_out, skip=r.skip, label=label))
    if caught:
        with pytest.raises(AssertionError):
            judge()
    else:
        judge()
    return got


def _hp_ref(mode):
    key = ("hp", mode)
    if key not in _CACHE:
        x, w, bias = _hp_operands(mode)
        r = R.ref_conv("fwd", x, w, stride=1, pad=1, dtype="bf16", bias=bias, act=R.ACT_RELU)
        r.bias_rows = bias.expand_as(r.out)
        if mode == "exact":
            R.assert_exact_domain([r.S + bias.abs()], [r.out])
        _CACHE[key] = (x, w, bias, r, F.conv2d(x, w, padding=1))
    return _CACHE[key]


@pytest.mark.parametrize("mode", ["random", "exact"])
def test_hp_clean_standin_passes(mode):
    x, w, bias, r, acc = _hp_ref(mode)
    _hp_judge(mode, acc, r, False, f"{mode}: clean")
    if mode == "random":      # the numbers of the issue: bf16 rounding against the cap, and the ReLU-kink share
        got = r.out.float().bfloat16()
        print("bf16 rounding / cap", float(R.ratio(got, r.out, r.t_out, r.skip).max()), "kink share", float(r.skip.double().mean()))
        assert float(r.skip.double().mean()) <= R.MAX_SKIP


@pytest.mark.parametrize("mode", ["random", "exact"])
def test_hp_dropped_tap_product_at_corner(mode):
    """a. ONE product x[ci] w[co][tap][ci] missing at the corner pixel (0, 0) of image 1.  In random mode the dropped
    product is the largest one that still passes the criterion the existing GPU test applies, max |err| / max |ref| <=
    2e-2 (asserted: that criterion does not see it); the per-element cap fails it.  In exact mode any non-zero one."""
    x, w, bias, r, acc = _hp_ref(mode)
    B, H, W, C = HP["B"], HP["H"], HP["W"], HP["C"]
    scale = float(r.out.abs().max())
    pre = r.pre_lin.view(B, H, W, C)[1, 0, 0]                           # [co]
    best = None
    for kh in (1, 2):                                                    # the taps inside the image at the corner
        for kw in (1, 2):
            p = w[:, :, kh, kw] * x[1, :, kh - 1, kw - 1]                # [co, ci]
            ok = (p.abs() <= (2e-2 * scale if mode == "random" else 1.0)) & (pre[:, None] > p.abs()) & (pre[:, None] - p > 0) & (p != 0)
            v, i = (p.abs() * ok).flatten().max(0)
            if best is None or float(v) > best[0]:
                best = (float(v), int(i) // C, float(p.flatten()[i]))
    size, co, prod = best
    assert size > 0
    bad = acc.clone()
    bad[1, co, 0, 0] -= prod
    got = _hp_judge(mode, bad, r, True, f"{mode}: one product dropped at a corner")
    if mode == "random":
        old = float((got.double() - r.out).abs().max() / scale)
        at = (1 * H * W, co)
        print(f"dropped product {prod:.4f}: old criterion {old:.3e} (limit 2e-2); |err| / cap "
              f"{float(R.ratio(got, r.out, r.t_out, r.skip)[at]):.1f}")
        assert 5e-3 < old <= 2e-2, old


@pytest.mark.parametrize("mode", ["random", "exact"])
def test_hp_halo_row_from_previous_image(mode):
    """b. the halo row above image 1 read from the last row of image 0 (the buffer range check did not zero it)"""
    x, w, bias, r, acc = _hp_ref(mode)
    bad = acc.clone()
    bad[1:2, :, 0:1] += F.conv2d(x[0:1, :, -1:], w[:, :, 0:1, :], padding=(0, 1))
    _hp_judge(mode, bad, r, True, f"{mode}: halo row of the previous image")


@pytest.mark.parametrize("mode", ["random", "exact"])
def test_hp_tile_from_stale_ring_slot(mode):
    """c. one 8 x 32 tile computed from the halo of the tile three earlier (the 3-deep ring's slot was not refilled)"""
    x, w, bias, r, acc = _hp_ref(mode)
    B, H, W = HP["B"], HP["H"], HP["W"]
    tx, ty = -(-W // 32), -(-H // 8)
    xp = F.pad(x, (1, 32 * tx - W + 1, 1, 8 * ty - H + 1))
    halo = lambda t: xp[t // (tx * ty), :, 8 * (t // tx % ty):8 * (t // tx % ty) + 10, 32 * (t % tx):32 * (t % tx) + 34]
    t = 4                                                                # image 0, tile row 2, column 0; t - 3 = (0, 1)
    y0, x0 = 8 * (t // tx % ty), 32 * (t % tx)
    stale = F.conv2d(halo(t - 3)[None], w)[0]                            # [C, 8, 32]
    bad = acc.clone()
    hh, ww = min(8, H - y0), min(32, W - x0)
    bad[t // (tx * ty), :, y0:y0 + hh, x0:x0 + ww] = stale[:, :hh, :ww]
    assert torch.equal(F.conv2d(halo(t)[None], w)[0][:, :hh, :ww], acc[0, :, y0:y0 + hh, x0:x0 + ww])    # the plant's own tiling
    _hp_judge(mode, bad, r, True, f"{mode}: stale ring slot")


@pytest.mark.parametrize("mode", ["random", "exact"])
def test_hp_mask_heads_odd_wave_partial_missing(mode):
    """d. head 1 = channels 32..63 straddles the two waves of a row group; the odd wave's part (48..63) goes through LDS.
    That part missing from the logit."""
    x, w1, b1 = _hp_operands(mode, cout=96)
    if mode == "exact":
        w2, b2 = R.small_ints((3, 32), 4, -2, 2, device="cpu").double(), R.small_ints((3,), 5, device="cpu").double()
    else:
        g = torch.Generator().manual_seed(7)
        w2, b2 = torch.randn(3, 32, generator=g).double(), torch.randn(3, generator=g).double()
    rh, logit, t = R.ref_heads(x, w1, b1, w2, b2)
    if mode == "exact":
        R.assert_exact_domain([rh.S + b1.abs(), (rh.out.view(-1, 3, 32) * w2).abs().sum(-1) + b2.abs()], [rh.out])
    h32 = rh.out.float()                                                 # a stand-in: f32 h, f32 head sums
    B, H, W = HP["B"], HP["H"], HP["W"]
    good = ((h32.view(B, H, W, 3, 32) * w2.float()).sum(-1) + b2.float()).permute(0, 3, 1, 2)
    bad = good.clone()
    bad[:, 1] -= (h32.view(B, H, W, 96)[..., 48:64] * w2.float().flatten()[48:64]).sum(-1)
    for got, caught in ((good, False), (bad, True)):
        judge = (lambda: R.check_exact(got, logit, f"{mode}: logits")) if mode == "exact" else \
                (lambda: R.check(got, logit, t, label=f"{mode}: logits"))
        if caught:
            with pytest.raises(AssertionError):
                judge()
        else:
            judge()


@pytest.mark.parametrize("plant", ["missing", "twice"])
def test_hp_wgrad_tile_missing_or_twice(plant):
    """e. weight gradient with one 8 x 32 tile's pixels left out, or added twice (a workgroup range off by one).  The
    worst-case cap of the random mode grows with the pixel count and may cover this; exact mode must catch it."""
    x, _, _ = _hp_operands("exact")
    B, H, W, C = HP["B"], HP["H"], HP["W"], HP["C"]
    dy = R.ints((B, C, H, W), 6, device="cpu").double()
    dw0 = R.small_ints((C, C, 3, 3), 7, device="cpu").double()
    r = R.ref_conv("wgrad", x, torch.empty(C, C, 3, 3), dy=dy, stride=1, pad=1, dw0=dw0, extra=3)
    R.assert_exact_domain([r.S + dw0.abs().reshape(C, -1)])
    good = dw0 + torch.nn.grad.conv2d_weight(x, (C, C, 3, 3), dy, padding=1)
    R.check_exact(good.float().reshape(C, -1), r.out, "wgrad clean")
    one = torch.zeros_like(dy)
    one[1, :, 8:16, 32:45] = dy[1, :, 8:16, 32:45]                      # image 1, tile row 1, the ragged right column
    part = torch.nn.grad.conv2d_weight(x, (C, C, 3, 3), one, padding=1)
    bad = good - part if plant == "missing" else good + part
    with pytest.raises(AssertionError):
        R.check_exact(bad.float().reshape(C, -1), r.out, f"wgrad tile {plant}")


@pytest.mark.parametrize("k,s,p,H,W", [(3, 1, 1, 7, 9), (4, 2, 1, 10, 14), (4, 2, 1, 6, 8), (3, 2, 1, 7, 9)])
def test_per_tap_contractions_equal_torch(monkeypatch, k, s, p, H, W):
    """the per-tap float64 matmul forms the references use on the device (no float64 convolution there) are the same
    contractions as torch's conv2d / conv_transpose2d / conv2d_weight"""
    g = torch.Generator().manual_seed(k + s + H)
    x, w = torch.randn(2, 5, H, W, generator=g).double(), torch.randn(6, 5, k, k, generator=g).double()
    y = F.conv2d(x, w, stride=s, padding=p)
    dy = torch.randn(y.shape, generator=g).double()
    ref = (y, R.conv_transpose2d64(dy, w, s, p, (H, W)), R.conv2d_weight64(x, w.shape, dy, s, p))
    monkeypatch.setattr(R, "PER_TAP", True)
    got = (R.conv2d64(x, w, s, p), R.conv_transpose2d64(dy, w, s, p, (H, W)), R.conv2d_weight64(x, w.shape, dy, s, p))
    for a, b in zip(got, ref):
        assert a.shape == b.shape and float((a - b).abs().max()) <= 1e-12 * float(b.abs().max())
