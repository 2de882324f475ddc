"""Shared by test_gemm_ref_cpu.py, test_gpu_linear_edges.py, test_gpu_conv_generic.py, test_gpu_conv_rw_edges.py and
test_gpu_conv_wgrad_edges.py: float64 references of the GEMM and conv entry points (csrc/gemm.hpp through linear_ops.hip
/ conv_ops.hip, and the hand-pipelined kernels of gemm_ops.hip / wgrad_dma.hip they route to), a per-element error cap
derived from the arithmetic, an f32 emulation of the most error-prone correct kernel, NaN-poisoned buffers, and (at the
end) the exact integer mode and the tile schedules of the persistent kernels.  The references compute on the device of
their inputs (wide(t, device)); check() compares where the reference lives.

Reference.  The operands are the values the kernel saw (bf16 or f32, widened to double).  The epilogue restates EpiStd:
    pre = acc + bias ;  v = pre * scale + shift ;  out = act(v) (+ res1) (+ res2)
    act 3 (GELU_BWD): out = v * gelu'(res1)      act 4 (RELU_BWD): out = v * (res1 > 0)      act 6 (MUL): out = v * res1
    act 5 (GELU_SG):  out = gelu(v) and `pre` receives gelu'(v)

Cap.  S = the same contraction over absolute values.  Kc terms accumulated in f32 in any order: every addition
contributes at most 2^-23 relative (round-to-nearest or truncation inside the matrix unit), bf16 x bf16 products are
exact in f32 and an f32 product is one more rounding, so |acc - ref| <= (Kc + 8) 2^-23 S.  Through the epilogue:
    t = (Kc + 8) 2^-23 S |scale|  +  2^-23 (|bias scale| + |shift| + |v|)        -- the f32 arithmetic that forms v
    f32 store:  + 2^-23 (|res1| + |res2| + |out|)        bf16 store:  + 2^-8 |out|   (the project's convention)
    GELU / GELU': t of v times the Lipschitz constant 1.13, plus the error of the erf: bf16 mode (branch-free
        Abramowitz-Stegun, csrc/common.hpp) 1.5e-7 absolute, times |v| for the derivative forms; f32 mode (erff,
        __expf: 16 ulp by the OpenCL bound ocml is built to) 16 * 2^-24 * |v| / 2, times (1 + |res1|) |v| for gelu'.
    ReLU: elements whose reference v lies within t of zero are skipped (either branch is right); at most 1 %.
    column sums (f32 atomics of the unrounded outputs): sum_m t + (M + 8) 2^-23 sum_m |o|
    BN statistics (f64 sums of the f32 pre): sum_m t_pre ; squares: sum_m (2 |pre| t_pre + t_pre^2)

check() asserts: all finite (NaN-poisoned outputs: everything was written); max |got - ref| / t <= 1; and for f32
outputs that the same ratio is <= 4 x that of the emulation -- an f32 chain adding the K products one at a time in k
order, the most error-prone order a correct kernel could use (the margin of test_gpu_attention_edges.py).
"""
import math

import torch
import torch.nn.functional as F

NAN = float("nan")
U = 2.0 ** -23
BF = 2.0 ** -8
ERF_FAST = 1.5e-7             # |erf error| of the branch-free bf16-mode erf (csrc/common.hpp)
ERF_F32 = 16 * 2.0 ** -24     # erff / __expf of the f32 mode: 16 ulp
GELU_LIP = 1.13               # max |gelu'| (and > max |gelu''| = 0.80)
MARGIN = 4
MAX_SKIP = 0.01
ACT_NONE, ACT_RELU, ACT_GELU, ACT_GELU_BWD, ACT_RELU_BWD, ACT_GELU_SG, ACT_MUL = range(7)
DT = {"f32": (torch.float32, 0), "bf16": (torch.bfloat16, 1)}
DEVICE = "cuda"               # where poisoned() allocates by default
QSCALE = 0.125 * 1.4426950408889634      # S3OD_QSCALE (csrc/common.hpp), an f32 constant in the kernel
QSCALE = float(torch.tensor(QSCALE, dtype=torch.float32))


def wide(t, device="cpu"):
    """the exact values a kernel saw, as float64 on the CPU -- or on `device`: the references below compute where their
    inputs live, so a large case runs its float64 contractions on the GPU"""
    return None if t is None else t.detach().to(device, torch.float64)


# ------------------------------------------------------------------------------------------------ poisoned buffers
def poisoned(shape, ld=None, dtype=torch.float32, device=None, slack=64):
    """A NaN-filled tensor of `shape` whose rows (all dimensions but the last, flattened) are `ld` elements apart
    (ld > shape[-1]: guard columns; only 2-D shapes), with `slack` NaN rows before and after.  Returns the logical
    view; guards_intact(view) checks every other element of the allocation afterwards."""
    cols = shape[-1]
    rows = int(math.prod(shape[:-1]))
    ld = cols if ld is None else ld
    assert ld >= cols and (ld == cols or len(shape) == 2)
    full = torch.full((rows + 2 * slack, ld), NAN, dtype=dtype, device=device or DEVICE)
    v = full[slack:slack + rows, :cols]
    return v if ld != cols else v.view(shape)


def poisoned_from(values, ld=None, dtype=None, device=None, slack=64):
    """an input made the same way: a kernel that reads a pad column or a row past M and multiplies it by zero
    turns NaN"""
    v = poisoned(tuple(values.shape), ld, dtype or values.dtype, device, slack)
    v.copy_(values)
    return v


def _whole(v):
    flat = torch.empty(0, dtype=v.dtype, device=v.device).set_(v.untyped_storage())
    live = torch.zeros(flat.numel(), dtype=torch.bool, device=v.device)
    live.as_strided(v.shape, v.stride(), v.storage_offset()).fill_(True)
    return flat, live


def guards_intact(v):
    """every element of v's allocation outside the logical view is still NaN"""
    flat, live = _whole(v)
    return bool(torch.isnan(flat[~live]).all())


def ld_of(v):
    return v.stride(-2)


# ------------------------------------------------------------------------------------------------ epilogue
def _erf(x):
    return torch.erf(x * 0.70710678118654752)


def gelu(x):
    return 0.5 * x * (1.0 + _erf(x))


def gelu_grad(x):
    return 0.5 * (1.0 + _erf(x)) + x * (0.39894228040143268 * torch.exp(-0.5 * x * x))


def epilogue(acc, bias=None, scale=None, shift=None, act=ACT_NONE, res1=None, res2=None):
    """EpiStd in acc's dtype (float64: the reference; float32: the emulation).  Returns (pre, v, out); for
    ACT_GELU_SG pre is gelu'(v)."""
    cast = lambda t: None if t is None else t.to(acc.dtype)
    bias, scale, shift, res1, res2 = map(cast, (bias, scale, shift, res1, res2))
    pre = acc if bias is None else acc + bias
    v = pre
    if scale is not None:
        v = v * scale
    if shift is not None:
        v = v + shift
    if act == ACT_GELU_BWD:
        o = v * gelu_grad(res1)
    elif act == ACT_RELU_BWD:
        o = torch.where(res1 > 0, v, torch.zeros_like(v))
    elif act == ACT_MUL:
        o = v * res1
    else:
        o = gelu(v) if act in (ACT_GELU, ACT_GELU_SG) else v.clamp_min(0) if act == ACT_RELU else v
        if act == ACT_GELU_SG:
            pre = gelu_grad(v)
        if res1 is not None:
            o = o + res1
    if res2 is not None:
        o = o + res2
    return pre, v, o


class Ref:
    """float64 reference of one call: out / pre with their caps t_out / t_pre, the ReLU skip mask, and the caps
    of the sums taken from the unrounded values (t_sum for colsum, t_pre32 for the BN statistics)."""


def finish(acc, S, kc, dtype, out_f32=False, bias=None, scale=None, shift=None, act=ACT_NONE, res1=None, res2=None,
           extra=0):
    """acc, S: float64 [M, N] contraction and its absolute-value twin; kc: terms per element; extra: further f32
    additions per element (split-K atomics / slab reduce).  dtype: compute dtype ("f32" / "bf16") -- the type `pre`
    is stored in and, unless out_f32, the type of `out`."""
    r = Ref()
    z = torch.zeros((), dtype=torch.float64)
    ab = lambda t: z if t is None else t.abs()
    sc = 1.0 if scale is None else scale.abs()
    pre, v, out = epilogue(acc, bias, scale, shift, act, res1, res2)
    eps = (kc + 8 + extra) * U * S
    bf = dtype == "bf16"
    pre_lin = acc + bias if bias is not None else acc
    r.t_pre32 = eps + U * (ab(bias) + pre_lin.abs())
    tv = eps * sc + U * (ab(bias) * sc + ab(shift) + v.abs())
    erf_v = ERF_FAST if bf else 0.5 * ERF_F32 * v.abs()
    r.skip = None
    if act == ACT_RELU:
        r.skip = v.abs() <= tv
        to = tv
    elif act == ACT_GELU or act == ACT_GELU_SG:
        to = GELU_LIP * tv + erf_v
    elif act == ACT_GELU_BWD:
        to = GELU_LIP * tv + (ERF_FAST if bf else ERF_F32 * (1 + res1.abs())) * v.abs()
    elif act == ACT_MUL:
        to = tv * res1.abs()
    else:
        to = tv
    addend1 = res1 if act in (ACT_NONE, ACT_RELU, ACT_GELU, ACT_GELU_SG) else None
    r.t_sum = to + U * (ab(addend1) + ab(res2) + out.abs())          # the f32 value before any store
    r.t_out = r.t_sum if (out_f32 or not bf) else to + BF * out.abs()
    if act == ACT_GELU_SG:
        r.t_pre = GELU_LIP * tv + (ERF_FAST if bf else ERF_F32) * (1 + v.abs()) + (BF if bf else U) * pre.abs()
    else:
        r.t_pre = eps + BF * pre.abs() if bf else r.t_pre32
    r.pre_lin, r.pre, r.v, r.out = pre_lin, pre, v, out
    r.S = S
    return r


def colsum_ref(r, cs0):
    """csum[n] = cs0[n] + sum_m o[m, n] (EpiStd ADDS its f32 column sums by atomics), and its cap"""
    M = r.out.shape[0]
    ref = cs0.double() + r.out.sum(0)
    t = r.t_sum.sum(0) + (M + 8) * U * (r.out.abs().sum(0) + cs0.double().abs())
    return ref, t


def stats_ref(r):
    """[2][N]: sum and sum of squares of pre over the rows, and their caps"""
    p, t = r.pre_lin, r.t_pre32
    return torch.stack([p.sum(0), (p * p).sum(0)]), torch.stack([t.sum(0), (2 * p.abs() * t + t * t).sum(0)])


# ------------------------------------------------------------------------------------------------ contractions
def chain(a, b):
    """f32 emulation: sum_k a[m, k] b[k, n] with the products added one at a time in k order"""
    a, b = a.float(), b.float()
    acc = torch.zeros(a.shape[0], b.shape[1], dtype=torch.float32)
    for k in range(a.shape[1]):
        p = a[:, k, None] * b[None, k, :]
        acc = acc + p
    return acc


def _epi_only(kw):
    return {k: v for k, v in kw.items() if k in ("bias", "scale", "shift", "act", "res1", "res2")}


def ref_linear(a, b, dtype, emu=False, **epi):
    """a [M, K], b [K, N] float64 (forward: b = w^T; data gradient: b = w; weight gradient: a = dy^T, b = x).
    Returns Ref; with emu=True also r.emu_out / r.emu_pre, the f32 chain through an f32 epilogue."""
    r = finish(a @ b, a.abs() @ b.abs(), a.shape[1], dtype, **epi)
    if emu:
        r.emu_pre, _, r.emu_out = epilogue(chain(a, b), **_epi_only(epi))
    return r


def token_rows(B, P, prefix):
    """row_mode 1: GEMM row m = b P + p -> stored row b (P + prefix) + prefix + p"""
    m = torch.arange(B * P)
    return (m // P) * (P + prefix) + prefix + m % P


def _qkv_split(acc, cos, sin, B, Ntok, P, H):
    """[M, 3 D] -> q, k, v [B, H, Ntok, 64] in acc's dtype: RoPE on the last P tokens of q and k, q times QSCALE"""
    D = 64 * H
    c, s = cos.to(acc.dtype).view(1, P, 1, 64), sin.to(acc.dtype).view(1, P, 1, 64)
    out = []
    for i in range(3):
        a = acc[:, i * D:(i + 1) * D].reshape(B, Ntok, H, 64).clone()
        if i < 2:
            rot = torch.cat([-a[..., 32:], a[..., :32]], -1)
            a[:, Ntok - P:] = a[:, Ntok - P:] * c + rot[:, Ntok - P:] * s
        if i == 0:
            a = a * QSCALE
        out.append(a.permute(0, 2, 1, 3).contiguous())
    return out


def ref_qkv_rope(x, w, bias, cos, sin, B, Ntok, P, H, dtype, emu=False):
    """s3od_qkv_rope_fwd: [q | k | v] = x w^T + bias, RoPE on the last P tokens of q and k (partner column d +- 32
    of the same head, rotate_half sign), q times QSCALE, split to [B, H, Ntok, 64].  Returns {name: (ref, t, emu)}.
    Cap: the accumulation cap of a column and of its partner through |cos| / |sin|, two more f32 roundings for the
    rotation, one for QSCALE, then the store."""
    D = 64 * H
    acc, S = x @ w.T + bias, x.abs() @ w.T.abs()
    eps = (D + 8) * U * S + U * (bias.abs() + acc.abs())
    ref = _qkv_split(acc, cos, sin, B, Ntok, P, H)
    err, mag = [], []        # the same split over caps / magnitudes: |cos|, |sin| and the partner without its sign
    sw = lambda t: torch.cat([t[..., 32:], t[..., :32]], -1)
    c, s = cos.abs().view(1, P, 1, 64), sin.abs().view(1, P, 1, 64)
    for i in range(3):
        e = eps[:, i * D:(i + 1) * D].reshape(B, Ntok, H, 64).clone()
        a = acc[:, i * D:(i + 1) * D].reshape(B, Ntok, H, 64).abs()
        if i < 2:
            e[:, Ntok - P:], a[:, Ntok - P:] = (e[:, Ntok - P:] * c + sw(e)[:, Ntok - P:] * s,
                                                a[:, Ntok - P:] * c + sw(a)[:, Ntok - P:] * s)
        q = QSCALE if i == 0 else 1.0
        err.append((e * q).permute(0, 2, 1, 3))
        mag.append((a * q).permute(0, 2, 1, 3))
    emus = [None] * 3
    if emu:
        emus = _qkv_split(chain(x, w.T) + bias.float(), cos, sin, B, Ntok, P, H)
    out = {}
    for i, name in enumerate("qkv"):
        t = err[i] + 3 * U * mag[i] + (BF if dtype == "bf16" else U) * ref[i].abs()
        out[name] = (ref[i], t, emus[i])
    return out


def _nhwc2d(t):
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def conv_cols(x, KH, KW, stride, pad):
    """im2col in the kernel's k order (tap-major, channel-minor): [B OH OW, KH KW Cin]"""
    B, C = x.shape[:2]
    c = F.unfold(x, (KH, KW), padding=pad, stride=stride)                     # [B, C KH KW, L]
    return c.view(B, C, KH * KW, -1).permute(0, 3, 2, 1).reshape(-1, KH * KW * C)


PER_TAP = False               # test hook: take the per-tap matmul forms on the CPU too (test_gemm_ref_cpu.py)


def _taps(x, w, stride, pad, OH, OW):
    """padded NHWC x and, per tap, the [B, OH, OW, Cin] view of the pixels that tap reads"""
    KH, KW = w.shape[2:]
    xp = F.pad(x.permute(0, 2, 3, 1), (0, 0, pad, pad + stride, pad, pad + stride))
    for kh in range(KH):
        for kw in range(KW):
            yield kh, kw, xp[:, kh:kh + stride * (OH - 1) + 1:stride, kw:kw + stride * (OW - 1) + 1:stride]


def conv2d64(x, w, stride=1, pad=0):
    """float64 conv2d; off the CPU (no float64 convolution there) one matmul per tap"""
    if x.device.type == "cpu" and not PER_TAP:
        return F.conv2d(x, w, stride=stride, padding=pad)
    B, _, H, W = x.shape
    Cout, _, KH, KW = w.shape
    OH, OW = (H + 2 * pad - KH) // stride + 1, (W + 2 * pad - KW) // stride + 1
    out = torch.zeros(B, OH, OW, Cout, dtype=x.dtype, device=x.device)
    for kh, kw, v in _taps(x, w, stride, pad, OH, OW):
        out += v @ w[:, :, kh, kw].T
    return out.permute(0, 3, 1, 2)


def conv_transpose2d64(dy, w, stride, pad, hw):
    """float64 data gradient of conv2d(., w [Cout, Cin, KH, KW]) onto an hw = (H, W) input"""
    H, W = hw
    B, Cout, OH, OW = dy.shape
    _, Cin, KH, KW = w.shape
    if dy.device.type == "cpu" and not PER_TAP:
        op = (H - ((OH - 1) * stride - 2 * pad + KH), W - ((OW - 1) * stride - 2 * pad + KW))
        return F.conv_transpose2d(dy, w, stride=stride, padding=pad, output_padding=op)
    buf = torch.zeros(B, max((OH - 1) * stride + KH, pad + H), max((OW - 1) * stride + KW, pad + W), Cin, dtype=dy.dtype,
                      device=dy.device)
    d = dy.permute(0, 2, 3, 1)
    for kh in range(KH):
        for kw in range(KW):
            buf[:, kh:kh + stride * (OH - 1) + 1:stride, kw:kw + stride * (OW - 1) + 1:stride] += d @ w[:, :, kh, kw]
    return buf[:, pad:pad + H, pad:pad + W].permute(0, 3, 1, 2)


def conv2d_weight64(x, wshape, dy, stride, pad):
    if x.device.type == "cpu" and not PER_TAP:
        return torch.nn.grad.conv2d_weight(x, wshape, dy, stride=stride, padding=pad)
    Cout, Cin, KH, KW = wshape
    OH, OW = dy.shape[2:]
    d = dy.permute(0, 2, 3, 1).reshape(-1, Cout).T.contiguous()
    dw = torch.zeros(KH, KW, Cout, Cin, dtype=x.dtype, device=x.device)
    for kh, kw, v in _taps(x, torch.empty(0, 0, KH, KW), stride, pad, OH, OW):
        dw[kh, kw] = d @ v.reshape(-1, Cin)
    return dw.permute(2, 3, 0, 1)


def ref_conv(kind, x, w, dy=None, stride=1, pad=0, relu_in=False, hw=None, dw0=None, dtype="f32", emu=False, **epi):
    """float64 reference of one conv call on NCHW doubles; w is [Cout, Cin, KH, KW] (the conv view).
      "fwd":   conv2d(relu?(x), w)                      -> Ref over [B OH OW, Cout] (NHWC rows)
      "dgrad": conv_transpose2d(dy, w) onto hw = (H, W) -> Ref over [B H W, Cin]
      "wgrad": dw0 + conv2d_weight(relu?(x), dy)        -> Ref over [Cout, Cin KH KW]
    Epilogue tensors (res1, res2) are NHWC rows, like the outputs."""
    Cout, Cin, KH, KW = w.shape
    if relu_in and x is not None:
        x = x.clamp_min(0)
    if kind == "fwd":
        acc = _nhwc2d(conv2d64(x, w, stride, pad))
        S = _nhwc2d(conv2d64(x.abs(), w.abs(), stride, pad))
        r = finish(acc, S, KH * KW * Cin, dtype, **epi)
        if emu:
            r.emu_pre, _, r.emu_out = epilogue(chain(conv_cols(x, KH, KW, stride, pad), w.permute(2, 3, 1, 0).reshape(-1, Cout)),
                                                **_epi_only(epi))
        return r
    if kind == "dgrad":
        H, W = hw
        OH, OW = dy.shape[2:]
        op = (H - ((OH - 1) * stride - 2 * pad + KH), W - ((OW - 1) * stride - 2 * pad + KW))
        ct = lambda a, b: F.conv_transpose2d(a, b, stride=stride, padding=pad, output_padding=op)
        # a parity class has at most ceil(KH / s) ceil(KW / s) taps of Cout channels
        kc = -(-KH // stride) * -(-KW // stride) * Cout
        ct64 = lambda a, b: conv_transpose2d64(a, b, stride, pad, hw)
        r = finish(_nhwc2d(ct64(dy, w)), _nhwc2d(ct64(dy.abs(), w.abs())), kc, dtype, **epi)
        if emu:
            dy32, w32 = dy.float(), w.float()
            acc = torch.zeros(dy.shape[0], Cin, H, W, dtype=torch.float32)
            for kh in range(KH):
                for kw in range(KW):
                    for co in range(Cout):          # one product per output element and step, added in f32
                        wz = torch.zeros(1, Cin, KH, KW, dtype=torch.float32)
                        wz[0, :, kh, kw] = w32[co, :, kh, kw]
                        acc = acc + ct(dy32[:, co:co + 1], wz)
            r.emu_pre, _, r.emu_out = epilogue(_nhwc2d(acc), **_epi_only(epi))
        return r
    assert kind == "wgrad"
    g = lambda a, b: conv2d_weight64(a, w.shape, b, stride, pad)
    npix = dy.shape[0] * dy.shape[2] * dy.shape[3]
    r = finish(g(x, dy).reshape(Cout, -1), g(x.abs(), dy.abs()).reshape(Cout, -1), npix, "f32", res1=dw0.reshape(Cout, -1), **epi)
    if emu:
        e = chain(_nhwc2d(dy).T, conv_cols(x, KH, KW, stride, pad))               # [Cout, (tap, cin)]
        r.emu_out = e.view(Cout, KH * KW, Cin).permute(0, 2, 1).reshape(Cout, -1) + dw0.reshape(Cout, -1).float()
    return r


# ------------------------------------------------------------------------------------------------ assertions
def ratio(got, ref, t, skip=None):
    r = (got.double() - ref).abs() / t.clamp_min(1e-300)
    if skip is not None:
        r = torch.where(skip, torch.zeros_like(r), r)
    return r


def check(got, ref, t, emu=None, skip=None, label=""):
    """1. every element finite; 2. max |got - ref| / t <= 1; 3. (emu given: f32 outputs) that ratio <= MARGIN x the
    emulation's.  Prints the worst ratio and its index; returns (kernel ratio, emulation ratio or None)."""
    g = got.detach().to(ref.device, torch.float64)       # a device-side reference is compared where it lives
    ref = ref.reshape(g.shape)
    t = t.expand_as(ref) if t.dim() else t
    emu = None if emu is None else emu.to(ref.device)
    bad = int((~torch.isfinite(g)).sum())
    assert bad == 0, f"{label}: {bad} of {g.numel()} elements not finite (never written, or poison read)"
    if skip is not None:
        skip = skip.reshape(g.shape)
        share = float(skip.double().mean())
        assert share <= MAX_SKIP, f"{label}: {share:.3%} of the elements within the cap of the ReLU kink"
    r = ratio(g, ref, t, skip)
    worst, at = float(r.max()), tuple(int(i) for i in torch.unravel_index(r.argmax(), r.shape)) if r.numel() else ()
    we = None if emu is None else float(ratio(emu.reshape(g.shape), ref, t, skip).max())
    print(f"[{label}] worst |err| / cap {worst:.3e} at {at}" + ("" if we is None else f"; emulation {we:.3e}; kernel / emulation {worst / max(we, 1e-300):.2f}"))
    assert worst <= 1.0, f"{label}: |err| / cap = {worst:.3e} at {at} (got {float(g[at]):.9g}, ref {float(ref[at]):.9g})"
    if we is not None:
        assert worst <= MARGIN * we, f"{label}: |err| / cap = {worst:.3e} at {at} > {MARGIN} x {we:.3e} (emulation)"
    return worst, we


def check_token_rows(full, ref, t, B, P, prefix, emu=None, label=""):
    """row_mode 1 output [B (P + prefix), N] written into a NaN-filled tensor: the prefix rows of every image are
    still NaN, the patch rows pass check()"""
    rows = token_rows(B, P, prefix)
    keep = torch.ones(B * (P + prefix), dtype=torch.bool)
    keep[rows] = False
    f = full.detach().cpu()
    assert bool(torch.isnan(f[keep]).all()), f"{label}: a prefix row was written"
    return check(f[rows], ref, t, emu, label=label)


# ------------------------------------------------------------------------------------------------ fused mask heads
def ref_heads(x, w1, b1, w2, b2, dtype="bf16"):
    """s3od_mask_heads_fwd on NCHW float64 x: h = relu(conv3x3(x, w1 [32 NM, 64, 3, 3]) + b1), stored in `dtype` (hsave);
    logit_k = b2[k] + sum_j h[32 k + j] w2[k, j] from the UNROUNDED h.  Returns (Ref of h over [B H W, 32 NM],
    logits [B, NM, H, W], their cap).  With t_h the cap of the f32 h (ReLU is 1-Lipschitz, so the cap of v bounds it and
    nothing is skipped): t = sum_j t_h |w2| + (32 + 8) 2^-23 sum_j |h w2| + 2^-23 |b2|."""
    B, _, H, W = x.shape
    NM = w2.shape[0]
    rh = ref_conv("fwd", x, w1, stride=1, pad=1, dtype=dtype, bias=b1, act=ACT_RELU)
    t_h = rh.t_sum - U * rh.out.abs()                      # the cap of v: the ReLU adds no rounding
    h, t_h = rh.out.view(B, H, W, NM, 32), t_h.view(B, H, W, NM, 32)
    logit = (h * w2).sum(-1) + b2
    t = (t_h * w2.abs()).sum(-1) + (32 + 8) * U * (h * w2).abs().sum(-1) + U * b2.abs()
    return rh, logit.permute(0, 3, 1, 2), t.permute(0, 3, 1, 2)


# ------------------------------------------------------------------------------------------------ exact mode
# Operands are small integers held in bf16, so every product and partial sum is an integer: exact in f32 below 2^24 and
# in a bf16 output up to 256, whatever the summation order.  A correct kernel then matches the float64 reference bit for
# bit, and ONE missing or doubled product is a mismatch -- at any K, where the worst-case cap (K + 8) 2^-23 S of the
# random mode has long outgrown a single product (weight gradients over 10^4 .. 10^5 pixels).
F32_EXACT, BF16_EXACT = 2.0 ** 24, 256.0


def ints(shape, seed, p=0.5, device=None, dtype=torch.bfloat16):
    """values in {-1, 0, 1}, non-zero with probability p, random signs"""
    g = torch.Generator(device=device or DEVICE).manual_seed(seed)
    u = torch.rand(shape, generator=g, device=device or DEVICE)
    return (torch.where(u < p / 2, -1.0, 0.0) + torch.where(u > 1 - p / 2, 1.0, 0.0)).to(dtype)


def small_ints(shape, seed, lo=-3, hi=3, device=None, dtype=torch.float32):
    g = torch.Generator(device=device or DEVICE).manual_seed(seed)
    return torch.randint(lo, hi + 1, shape, generator=g, device=device or DEVICE).to(dtype)


def assert_exact_domain(f32_sums=(), bf16_values=()):
    """the bounds under which exact mode is exact, asserted on float64 reference quantities: every f32 partial sum is
    bounded by the sum of the absolute terms (< 2^24), every value stored as bf16 by 256"""
    for s in f32_sums:
        assert float(s.abs().max()) < F32_EXACT, float(s.abs().max())
    for v in bf16_values:
        assert float(v.abs().max()) <= BF16_EXACT, float(v.abs().max())


def check_exact(got, ref, label=""):
    """every element finite and EQUAL to the float64 reference (torch.equal of the values); prints the mismatch count"""
    g = got.detach().to(ref.device, torch.float64)
    ref = ref.reshape(g.shape)
    bad = int((~torch.isfinite(g)).sum())
    assert bad == 0, f"{label}: {bad} of {g.numel()} elements not finite (never written, or poison read)"
    ne = g != ref
    n = int(ne.sum())
    at = tuple(int(i) for i in torch.unravel_index(ne.double().argmax(), ne.shape)) if n else ()
    print(f"[{label}] exact: {n} of {g.numel()} elements differ" + (f", first at {at}: got {float(g[at])}, ref {float(ref[at])}" if n else ""))
    assert n == 0 and torch.equal(g, ref), f"{label}: {n} of {g.numel()} elements differ from the exact reference, first at {at}"


# ------------------------------------------------------------------------------------------------ tile schedules
def rw_schedule(T, C):
    """Restates the persistent register-weight kernels (gemm_ops.hip): nwg = min(max(T, 8), C) workgroups; XCD x =
    blockIdx % 8 owns tiles [T x / 8, T (x + 1) / 8) and its workgroups stride through that range.  Returns the tile
    list of every workgroup."""
    nwg = min(max(T, 8), C)
    out = []
    for blk in range(nwg):
        xcd, wi = blk & 7, blk >> 3
        wpx = (nwg + 7 - xcd) >> 3
        out.append(list(range(T * xcd // 8 + wi, T * (xcd + 1) // 8, wpx)))
    return out


def wgrad_schedule(T, C, nblk):
    """Restates the weight-gradient launchers: wpc = max(1, min(T, C // nblk)) workgroups per channel block, workgroup wi
    owns the contiguous tiles [T wi / wpc, T (wi + 1) / wpc).  Returns (wpc, tile list per workgroup)."""
    wpc = max(1, min(T, max(1, C // nblk)))
    return wpc, [list(range(T * wi // wpc, T * (wi + 1) // wpc)) for wi in range(wpc)]


def crosses_image(sched, tiles_per_image):
    """some workgroup's tiles come from two images (its buffer descriptor is rebased mid-range)"""
    return any(len({t // tiles_per_image for t in tl}) > 1 for tl in sched)
