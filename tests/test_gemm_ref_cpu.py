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
