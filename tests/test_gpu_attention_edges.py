"""GPU: the flash-attention kernels (csrc/attention.hip) PER ROW at ragged lengths -- forward and backward, f32 and
bf16, the fused QKV epilogue (s3od_attn_bwd_qkv), s3od_qkv_unrope, the S3OD_ATTN_FAST=0 branch and the backward after
the forward's overflow fallback.  The full-size tests (test_gpu_attention_fullsize.py) compare whole tensors at
N = 4101 / 16389, where an error confined to the 5 rows of the partial last block moves the rel-L2 by ~1e-3 of itself.

Reference: fp64 torch on the device, from the exact operands the kernel saw (q_eff = qs / (log2 e / 8), qs the rounded
pre-scaled q): S = q_eff k^T / 8, softmax, O = P v, natural-log LSE, dq / dk / dv by autograd.

Metric: per row r of each tensor, |got_r - ref_r|_2 / max(|ref_r|_2, median reference row norm of that tensor); for
LSE the absolute difference in natural units.  The worst row is what is asserted, and its index is reported.

Tolerance: MARGIN (4) x the worst-row error of an EMULATION against the same fp64 reference at the same inputs, never
a number taken from the kernel.  The emulation is plain fp32 torch with the kernel's formulas (base-2 scores from the
pre-scaled q, P = exp2(s - lse2), dS = P (dP - delta), delta from the rounded O, dK = dS^T qs ln 2); for bf16 it also
rounds where the kernel does: P = exp2(s - m) before P.V and before the row sum (attn_fwd_kernel: pb feeds both MFMAs)
with m the max of the FIRST key tile as in the kernel (a larger score in a later tile gives P > 1, rounded there; with
the true row max the dominant P would be exactly 1 and the emulated LSE 4 x better than any such kernel can be), O; in the
backward P before P^T.dO and dS before dS.K and dS^T.Q (pack_acc in attn_bwd_dkdv32_kernel / attn_bwd_dq32_kernel),
and the outputs.  The fused epilogue rounds once, after the inverse RoPE; the two-step path rounds dq / dk / dv and
then d_qkv.

Every input is carved out of the middle of a larger tensor whose slack (>= 128 rows on both sides) is NaN: a kernel
that reads past N of the last head and multiplies by a zero weight, instead of masking, turns NaN.  Every output is
carved out of a tensor filled with a sentinel byte, itself pre-filled with NaN: afterwards the slack must be untouched
and the output all finite (every element written).

N = 1: dq and dk are exactly zero in the reference, so they are bounded by eps x |dO| |v| |k| instead, and dv must
equal dO to output rounding.

Shapes: B = 2, H = 3 (a real head stride and a real batch stride in the [B, N, H*64] layout of o / dO).  The two-step
path s3od_attn_bwd + s3od_qkv_unrope runs at H = 12, the smallest head count s3od_qkv_unrope is built for.

Measured on an MI355X, worst-row error of the kernel / of the emulation (72 cases, 5.3 s in all).  N = 322:
  attn_fwd_kernel<float>                 o   9.8e-07 / 9.6e-07    lse 3.1e-06 / 2.1e-06
  attn_fwd_kernel<bf16, DMA>             o   3.6e-03 / 3.6e-03    lse 1.6e-03 / 1.6e-03
  attn_fwd_kernel<bf16, DMA>, FAST=0     o   3.4e-03 / 3.4e-03    lse 1.8e-03 / 2.5e-03
  attn_bwd_dq_kernel (f32)               dq  6.7e-06 / 1.8e-06    (a planted row: dP - delta cancels, the kernel adds 322 keys in one chain)
  attn_bwd_dkdv_kernel (f32)             dk  1.0e-06 / 1.2e-06    dv  1.1e-06 / 1.1e-06
  attn_bwd_dq32_kernel (bf16)            dq  1.6e-02 / 1.6e-02
  attn_bwd_dkdv32_kernel (bf16)          dk  4.1e-03 / 4.1e-03    dv  3.7e-03 / 3.7e-03
(N, P) = (261, 256), thirds of d_qkv and the bias sums:
  s3od_attn_bwd_qkv f32                  q 2.5e-06 / 1.9e-06  k 1.3e-06 / 1.1e-06  v 1.2e-06 / 9.8e-07  dbq 5.9e-07 / 5.4e-07  dbv 3.2e-07 / 2.9e-07
  s3od_attn_bwd_qkv bf16                 q 1.5e-02 / 1.5e-02  k 4.9e-03 / 4.9e-03  v 3.8e-03 / 3.8e-03  dbq 1.9e-03 / 1.9e-03  dbv 2.4e-04 / 2.4e-04
  s3od_attn_bwd + s3od_qkv_unrope f32    q 2.6e-06 / 3.7e-06  k 1.4e-06 / 1.5e-06  v 1.3e-06 / 1.2e-06  dbq 5.2e-07 / 5.2e-07  dbv 3.0e-07 / 2.9e-07
  s3od_attn_bwd + s3od_qkv_unrope bf16   q 4.5e-02 / 4.5e-02  k 1.0e-02 / 1.0e-02  v 3.7e-03 / 3.7e-03  dbq 2.7e-03 / 2.7e-03  dbv 3.5e-04 / 3.5e-04
Before the f32 backward kernels were changed to accumulate their scores from zero (they accumulated on top of -LSE and
-delta), the f32 dk / dv figures were 2.5 - 5 x the emulation's (N = 2: dk 9.4e-07 / 1.9e-07; N = 64: 2.8e-06 /
7.6e-07) and at N = 1 dv differed from dO by 4.8e-07 |dO|.
"""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

LOG2E = 1.4426950408889634
LN2 = 0.6931471805599453
QSCALE = LOG2E * 0.125          # the QKV epilogue's pre-scale of q
MARGIN = 4                      # allowed worst-row error = MARGIN x the emulation's
B, H = 2, 3
SLACK_ROWS = 128                # one full 128-row workgroup block of slack on each side of every carved tensor
SENTINEL = 0x5A

RAGGED = [1, 2, 3, 31, 32, 33, 63, 64, 65, 66, 67, 127, 128, 129, 130, 131, 191, 193, 255, 257, 261, 322]
DTYPES = ["f32", "bf16"]


def _tdt(dt):
    return torch.bfloat16 if dt == "bf16" else torch.float32


def _code(dt):
    from s3od_amd._lib import BF16, F32
    return BF16 if dt == "bf16" else F32


# ------------------------------------------------------------------------------------------------ carved tensors
class _Out:
    """An output carved out of a larger allocation: slack = sentinel bytes, the output itself NaN."""

    def __init__(self, shape, dtype, row):
        n = math.prod(shape)
        self.slack = SLACK_ROWS * row
        self.buf = torch.empty(n + 2 * self.slack, dtype=dtype, device="cuda")
        self.buf.view(torch.uint8).fill_(SENTINEL)
        self.t = self.buf[self.slack:self.slack + n].view(shape)
        self.t.fill_(float("nan"))

    def check(self, name):
        """slack untouched, every element written"""
        n = self.t.numel()
        lo, hi = self.buf[:self.slack].view(torch.uint8), self.buf[self.slack + n:].view(torch.uint8)
        assert bool((lo == SENTINEL).all()), f"{name}: wrote before the start of the output"
        assert bool((hi == SENTINEL).all()), f"{name}: wrote past the end of the output"
        bad = (~torch.isfinite(self.t.float())).flatten().nonzero()
        assert bad.numel() == 0, f"{name}: {bad.numel()} elements not written or not finite, first flat index {int(bad[0])}"
        return self.t


def _carve_in(x, row):
    """a copy of x in the middle of a larger allocation whose slack is NaN"""
    n, slack = x.numel(), SLACK_ROWS * row
    buf = torch.full((n + 2 * slack,), float("nan"), dtype=x.dtype, device="cuda")
    t = buf[slack:slack + n].view(x.shape)
    t.copy_(x)
    return t


# ------------------------------------------------------------------------------------------------ inputs
def _inputs(N, dt, seed, Hh=H):
    """unit-variance q, k, v, dO; two planted high-score keys per head in the last key tile (the full-size test's
    trick scaled down), so score rows are not flat.  Returned in the kernel's dtype: qs = rounded pre-scaled q."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    BH = B * Hh
    q = torch.randn(BH, N, 64, device="cuda", generator=g)
    k = torch.randn(BH, N, 64, device="cuda", generator=g)
    v = torch.randn(BH, N, 64, device="cuda", generator=g)
    do = torch.randn(B, N, Hh * 64, device="cuda", generator=g)
    if N >= 8:          # (at N <= 3 planted keys would replace the whole row)
        t0 = (N - 1) // 64 * 64
        hot = torch.randint(t0, N, (BH, 2), device="cuda", generator=g)
        k.scatter_(1, hot[..., None].expand(-1, -1, 64), q[:, :4, :].mean(1, keepdim=True).expand(-1, 2, -1) * 3.0)
    return _finish_inputs(q, k, v, do, dt)


def _finish_inputs(q, k, v, do, dt):
    T = _tdt(dt)
    q, k, v, do = q.to(T), k.to(T), v.to(T), do.to(T)
    qs = (q.float() * QSCALE).to(T)
    return qs, k, v, do


def _to_bh(x, Hh):      # [B, N, H*64] -> [B*H, N, 64]
    Bb, N, _ = x.shape
    return x.view(Bb, N, Hh, 64).permute(0, 2, 1, 3).reshape(Bb * Hh, N, 64)


def _to_tok(x, Hh):     # [B*H, N, 64] -> [B*N, H*64]
    BH, N, _ = x.shape
    return x.view(BH // Hh, Hh, N, 64).permute(0, 2, 1, 3).reshape(BH // Hh * N, Hh * 64)


# ------------------------------------------------------------------------------------------------ reference, emulation
def _reference(qs, k, v, do, Hh=H):
    """fp64: o, lse (natural), dq (w.r.t. q_eff), dk, dv -- all [B*H, N, 64] / [B*H, N]"""
    q = (qs.double() / QSCALE).requires_grad_(True)
    k = k.double().requires_grad_(True)
    v = v.double().requires_grad_(True)
    s = torch.matmul(q, k.transpose(1, 2)) * 0.125
    lse = torch.logsumexp(s, dim=-1)
    o = torch.matmul(torch.softmax(s, dim=-1), v)
    o.backward(_to_bh(do.double(), Hh))
    return {"o": o.detach(), "lse": lse.detach(), "dq": q.grad, "dk": k.grad, "dv": v.grad}


def _emulate(qs, k, v, do, dt, Hh=H, round_out=True):
    """fp32 torch with the kernel's formulas; bf16: rounded where the kernel rounds (see the module docstring).
    dq is returned as the gradient w.r.t. q_eff (the kernel's dS.K x 1/8, an exact scaling)."""
    bf = dt == "bf16"
    r = (lambda x: x.bfloat16().float()) if bf else (lambda x: x)
    ro = r if round_out else (lambda x: x)
    qs, k, v, do = qs.float(), k.float(), v.float(), _to_bh(do.float(), Hh)
    s2 = torch.matmul(qs, k.transpose(1, 2))                  # scores in log2 units
    # bf16: the kernel fixes the row max on the first 64-key tile (S3OD_ATTN_FAST) and the lazy-rescale loop only moves
    # it when a score exceeds it by 2^8, so a later, larger score gives P > 1 and P is rounded THERE (with the true
    # row max the dominant P would be exactly 1 and carry no rounding error at all)
    mt = s2.max(-1, keepdim=True).values
    m = s2[..., :64].max(-1, keepdim=True).values if bf else mt
    # ... unless that overflows: the kernel then reruns the block with the lazy rescale, which moves m onto the score
    m = torch.where(torch.isfinite(torch.exp2(s2 - m).sum(-1, keepdim=True)), m, mt)
    p = r(torch.exp2(s2 - m))
    l = p.sum(-1, keepdim=True)
    o = r(torch.matmul(p, v) / l)                             # the forward always rounds its output
    lse2 = m + torch.log2(l)
    delta = (o * do).sum(-1, keepdim=True)
    P = torch.exp2(s2 - lse2)
    dS = P * (torch.matmul(do, v.transpose(1, 2)) - delta)
    dv = ro(torch.matmul(r(P).transpose(1, 2), do))
    dk = ro(torch.matmul(r(dS).transpose(1, 2), qs) * LN2)
    dq = ro(torch.matmul(r(dS), k)) * 0.125
    return {"o": o, "lse": lse2[..., 0] / LOG2E, "dq": dq, "dk": dk, "dv": dv}


def _row_err(got, ref):
    """per-row error (see the module docstring) of a [..., 64]-shaped tensor against the fp64 reference -> [rows]"""
    got, ref = got.double().reshape(-1, ref.shape[-1]), ref.reshape(-1, ref.shape[-1])
    rn = ref.norm(dim=1)
    return (got - ref).norm(dim=1) / torch.maximum(rn, rn.median())


def _worst(err, shape):
    i = int(err.argmax())
    return float(err[i]), tuple(int(x) for x in np.unravel_index(i, tuple(shape)))


def _errors(got, ref):
    """name -> per-row error vector"""
    out = {}
    for name, x in got.items():
        out[name] = (x.double() - ref[name]).abs().flatten() if name == "lse" else _row_err(x, ref[name])
    return out


def _compare(label, got, emu, ref, names=None):
    """worst row of the kernel <= MARGIN x worst row of the emulation, per tensor; every figure printed, every
    miss reported with its row"""
    eg, ee = _errors(got, ref), _errors(emu, ref)
    misses, tol = [], {}
    for name in names or got.keys():
        shape = ref[name].shape if name == "lse" else ref[name].shape[:-1]
        wk, ik = _worst(eg[name], shape)
        we, _ = _worst(ee[name], shape)
        tol[name] = MARGIN * we
        print(f"{label} {name}: kernel {wk:.3e} at row {ik}, emulation {we:.3e}")
        if not wk <= MARGIN * we:
            misses.append(f"{name}: worst row {ik} error {wk:.3e} > {MARGIN} x {we:.3e} (emulation)")
    assert not misses, f"{label}: " + "; ".join(misses)
    return eg, tol


# ------------------------------------------------------------------------------------------------ kernel runs
def _forward(dt, qs, k, v, N, Hh=H):
    """s3od_attn_fwd on carved tensors -> o [B, N, H*64], lse2 [B*H, N] (log2 units), both checked"""
    from s3od_amd._lib import lib, stream
    T = _tdt(dt)
    o = _Out((B, N, Hh * 64), T, Hh * 64)
    lse2 = _Out((B * Hh, N), torch.float32, 1)
    lib()("s3od_attn_fwd", _code(dt), _carve_in(qs, 64), _carve_in(k, 64), _carve_in(v, 64), o.t, lse2.t, B, Hh, N, stream())
    torch.cuda.synchronize()
    return o.check("o"), lse2.check("lse")


def _fwd_bwd(dt, qs, k, v, do, N, Hh=H):
    """forward + s3od_attn_bwd on carved tensors -> the kernel's o, lse (natural), dq (x 1/8), dk, dv as [B*H, N, ..]
    plus the raw tensors the next stage needs"""
    from s3od_amd._lib import lib, stream
    T = _tdt(dt)
    o, lse2 = _forward(dt, qs, k, v, N, Hh)
    ins = [_carve_in(qs, 64), _carve_in(k, 64), _carve_in(v, 64), _carve_in(o, Hh * 64), _carve_in(do, Hh * 64), _carve_in(lse2, 1)]
    delta = _Out((B * Hh, N), torch.float32, 1)
    dq, dk, dv = (_Out((B * Hh, N, 64), T, 64) for _ in range(3))
    lib()("s3od_attn_bwd", _code(dt), *ins, delta.t, dq.t, dk.t, dv.t, B, Hh, N, stream())
    torch.cuda.synchronize()
    delta.check("delta")
    got = {"o": _to_bh(o, Hh).float(), "lse": lse2 / LOG2E, "dq": dq.check("dq").float() * 0.125,
           "dk": dk.check("dk").float(), "dv": dv.check("dv").float()}
    return got, {"ins": ins, "dq": dq.t, "dk": dk.t, "dv": dv.t}


# ================================================================================================ 2 + 3: ragged lengths
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("N", RAGGED)
def test_attention_ragged_fwd_bwd_per_row(N, dt):
    qs, k, v, do = _inputs(N, dt, seed=1000 + N)
    got, _ = _fwd_bwd(dt, qs, k, v, do, N)
    ref = _reference(qs, k, v, do)
    emu = _emulate(qs, k, v, do, dt)
    label = f"[{dt} N={N}]"
    if N > 1:
        _compare(label, got, emu, ref)
        return
    # N = 1: P = 1, dS = 0 -- dq and dk are exactly zero in the reference (the row metric has no scale there)
    _compare(label, got, emu, ref, names=["o", "lse"])
    eps = torch.finfo(_tdt(dt)).eps
    do_bh = _to_bh(do.double(), H)
    n = lambda x: x.double().norm(dim=-1).flatten()
    scale = n(do_bh) * n(v)
    dq_raw, q_eff = got["dq"] * 8.0, qs.double() / QSCALE        # the kernel's dS.K; dk = dS^T q_eff / 8
    bq, bk = eps * scale * n(k), eps * scale * torch.minimum(n(k), n(q_eff) * 0.125)
    edv = (got["dv"].double() - do_bh).norm(dim=-1).flatten()
    print(f"{label} |dq| {float(n(dq_raw).max()):.3e} (bound {float(bq.min()):.3e})  |dk| {float(n(got['dk']).max()):.3e} "
          f"(bound {float(bk.min()):.3e})  |dv - dO| / |dO| {float((edv / n(do_bh)).max()):.3e} (eps {eps:.3e})")
    assert bool((n(dq_raw) <= bq).all()), f"{label} dq not zero: {n(dq_raw).tolist()} vs {bq.tolist()}"
    assert bool((n(got["dk"]) <= bk).all()), f"{label} dk not zero: {n(got['dk']).tolist()} vs {bk.tolist()}"
    assert bool((edv <= eps * n(do_bh)).all()), f"{label} dv != dO: {(edv / n(do_bh)).tolist()}"


# ================================================================================================ 4: fused QKV epilogue
def _rotate_half(t):
    return torch.cat([-t[..., 32:], t[..., :32]], dim=-1)


def _unrope(g, cos, sin, P):
    """transpose of the forward RoPE y = t cos + rotate_half(t) sin on the last P tokens of g [B*H, N, 64], by
    autograd (the map is linear, so its vector-Jacobian product does not depend on the point); prefix tokens pass"""
    if P == 0:
        return g.clone()
    N = g.shape[1]
    t = torch.zeros_like(g[:, N - P:]).requires_grad_(True)
    y = t * cos.to(g.dtype) + _rotate_half(t) * sin.to(g.dtype)
    y.backward(g[:, N - P:])
    return torch.cat([g[:, :N - P], t.grad], dim=1)


def _dqkv(d, cos, sin, P, Hh, rnd=lambda x: x):
    """dq (w.r.t. q_eff: the 1/8 of S = q_eff k^T / 8 is in it), dk, dv [B*H, N, 64] -> thirds of d_qkv, each as
    [B*N, H*64] (token rows, head-major columns)"""
    return {"q": rnd(_to_tok(_unrope(d["dq"], cos, sin, P), Hh)), "k": rnd(_to_tok(_unrope(d["dk"], cos, sin, P), Hh)),
            "v": rnd(_to_tok(d["dv"], Hh))}


def _thirds(dqkv, Hh):
    D = 64 * Hh
    x = dqkv.float()
    return {n: x[:, i * D:(i + 1) * D] for i, n in enumerate("qkv")}


def _seg(x, Hh):        # [B*N, H*64] -> [B*N, H, 64]: the row metric runs per (token, head)
    return x.reshape(x.shape[0], Hh, 64)


def _qkv_case(dt, N, P, Hh, fused):
    from s3od_amd._lib import lib, stream, NREP, HipLibError
    T, D = _tdt(dt), 64 * Hh
    label = f"[{dt} N={N} P={P} H={Hh} {'fused' if fused else 'two-step'}]"
    qs, k, v, do = _inputs(N, dt, seed=2000 + N, Hh=Hh)
    g = torch.Generator(device="cuda").manual_seed(N)
    th = torch.rand(max(P, 1), 32, device="cuda", generator=g) * 6.28     # [P][64] tables (one unused row at P = 0)
    cs = torch.cat([th.cos(), th.cos()], 1).contiguous()
    sn = torch.cat([th.sin(), th.sin()], 1).contiguous()
    cs_c, sn_c = _carve_in(cs, 64), _carve_in(sn, 64)
    dbq0 = torch.randn(D, device="cuda", generator=g)
    dbv0 = torch.randn(D, device="cuda", generator=g)
    dbq, dbv = dbq0.clone(), dbv0.clone()
    ws = torch.zeros(NREP * 2 * D, device="cuda")
    out = _Out((B * N, 3 * D), T, 3 * D)
    if fused:
        o, lse2 = _forward(dt, qs, k, v, N, Hh)
        ins = [_carve_in(qs, 64), _carve_in(k, 64), _carve_in(v, 64), _carve_in(o, D), _carve_in(do, D), _carve_in(lse2, 1)]
        delta = _Out((B * Hh, N), torch.float32, 1)
        lib()("s3od_attn_bwd_qkv", _code(dt), *ins, delta.t, cs_c, sn_c, P, out.t, dbq, dbv, ws, B, Hh, N, stream())
        torch.cuda.synchronize()
        delta.check("delta")
    else:
        _, raw = _fwd_bwd(dt, qs, k, v, do, N, Hh)
        lib()("s3od_qkv_unrope", _code(dt), _carve_in(raw["dq"], 64), _carve_in(raw["dk"], 64), _carve_in(raw["dv"], 64),
              cs_c, sn_c, out.t, dbq, dbv, ws, B, N, P, Hh, stream())
        torch.cuda.synchronize()
    dqkv = out.check("dqkv")
    assert int((ws != 0).sum()) == 0, f"{label} workspace not left all zero"

    ref = _dqkv(_reference(qs, k, v, do, Hh), cs.double(), sn.double(), P, Hh)
    r = (lambda x: x.bfloat16().float()) if dt == "bf16" else (lambda x: x)
    # fused: one rounding, after the inverse RoPE; two-step: dq / dk / dv rounded, then d_qkv
    emu_raw = _dqkv(_emulate(qs, k, v, do, dt, Hh, round_out=not fused), cs, sn, P, Hh)
    emu = {n: r(x) for n, x in emu_raw.items()}
    got = _thirds(dqkv, Hh)
    _compare(label, {n: _seg(x, Hh) for n, x in got.items()}, {n: _seg(x, Hh) for n, x in emu.items()},
             {n: _seg(x, Hh) for n, x in ref.items()})
    # bias gradients: previous contents + column sums of the q and v thirds (the entries accumulate)
    misses = []
    for n, got_b, prev in (("q", dbq, dbq0), ("v", dbv, dbv0)):
        want = prev.double() + ref[n].sum(0)
        emu_b = prev + emu_raw[n].sum(0)                                 # the same sum in fp32 torch
        ek = float((got_b.double() - want).norm() / want.norm())
        ee = float((emu_b.double() - want).norm() / want.norm())
        print(f"{label} db{n}: kernel {ek:.3e}, emulation {ee:.3e}")
        if not ek <= MARGIN * ee:
            misses.append(f"db{n}: {ek:.3e} > {MARGIN} x {ee:.3e}")
    assert not misses, f"{label} " + "; ".join(misses)
    if not fused:
        return
    # no bias gradients, no workspace: the call succeeds and d_qkv is bit-identical
    out2 = _Out((B * N, 3 * D), T, 3 * D)
    lib()("s3od_attn_bwd_qkv", _code(dt), *ins, delta.t, cs_c, sn_c, P, out2.t, None, None, None, B, Hh, N, stream())
    torch.cuda.synchronize()
    assert torch.equal(out2.check("dqkv (no bias)").view(torch.uint8), dqkv.view(torch.uint8)), f"{label} d_qkv differs without bias sums"
    # a bias gradient without the workspace is refused
    with pytest.raises(HipLibError, match=r"rc=22\): .*workspace"):
        lib()("s3od_attn_bwd_qkv", _code(dt), *ins, delta.t, cs_c, sn_c, P, out2.t, dbq, None, None, B, Hh, N, stream())
    torch.cuda.synchronize()


QKV_SHAPES = [(226, 221), (69, 64), (261, 256), (5, 0), (64, 64)]


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("N,P", QKV_SHAPES)
def test_attn_bwd_qkv_vs_reference(N, P, dt):
    """the engine's path: 17x13 patches + 5 prefix tokens, one tile, the golden's shape, prefix only, no prefix"""
    _qkv_case(dt, N, P, H, fused=True)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("N,P,Hh", [pytest.param(n, p, 12, id=f"{n}-{p}") for n, p in QKV_SHAPES]
                         + [pytest.param(69, 64, 16, id="69-64-H16")])
def test_attn_bwd_then_qkv_unrope_vs_reference(N, P, Hh, dt):
    """s3od_attn_bwd + s3od_qkv_unrope against the same reference (s3od_qkv_unrope is built for H = 12 / 16: the
    shapes at 12 heads, and one at 16, the other instance, which nothing else runs; B*N = 138 rows there and in
    69-64 is no multiple of the 4 rows the kernel loads together)"""
    _qkv_case(dt, N, P, Hh, fused=False)


# ================================================================================================ 5: untested branches
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("N", [65, 200, 322])
def test_attention_fwd_lazy_rescale_throughout(N, dt, monkeypatch):
    """S3OD_ATTN_FAST=0: the lazy-rescale loop from the first tile on, against the reference; bf16 also against the
    default (fixed-max) path, within the same tolerance"""
    qs, k, v, do = _inputs(N, dt, seed=3000 + N)
    ref = _reference(qs, k, v, do)
    emu = _emulate(qs, k, v, do, dt)
    monkeypatch.setenv("S3OD_ATTN_FAST", "0")          # read per call: tests/conftest.py sets S3OD_AB=1
    o, lse2 = _forward(dt, qs, k, v, N)
    got = {"o": _to_bh(o, H).float(), "lse": lse2 / LOG2E}
    _, tol = _compare(f"[{dt} N={N} FAST=0]", got, emu, ref, names=["o", "lse"])
    if dt != "bf16":
        return
    monkeypatch.setenv("S3OD_ATTN_FAST", "1")
    o1, l1 = _forward(dt, qs, k, v, N)
    dflt = {"o": _to_bh(o1, H).double(), "lse": (l1 / LOG2E).double()}
    e = _errors(got, dflt)
    for name in ("o", "lse"):
        shape = dflt[name].shape if name == "lse" else dflt[name].shape[:-1]
        w, i = _worst(e[name], shape)
        print(f"[bf16 N={N}] FAST=0 vs default {name}: {w:.3e} at row {i} (allowed {tol[name]:.3e})")
        assert w <= tol[name], f"FAST=0 vs default {name}: row {i} differs by {w:.3e} > {tol[name]:.3e}"


@pytest.mark.parametrize("dt", DTYPES)
def test_attention_bwd_after_overflow_fallback(dt):
    """the row_sum inputs of test_attention_fwd_fixed_max_overflow_falls_back at N = 200 (query 5 meets key 150 with a
    score of 200 natural units, ~290 log2 units above the rest): forward (bf16: through the fallback), then backward"""
    N, Q, K = 200, 5, 150
    g = torch.Generator(device="cuda").manual_seed(21)
    q = torch.randn(B * H, N, 64, device="cuda", generator=g)
    k = torch.randn(B * H, N, 64, device="cuda", generator=g)
    v = torch.randn(B * H, N, 64, device="cuda", generator=g)
    do = torch.randn(B, N, H * 64, device="cuda", generator=g)
    q[:, Q] = 0.0
    k[:, K] = 0.0
    q[:, Q, 0] = 40.0
    k[:, K, 0] = 40.0
    qs, k, v, do = _finish_inputs(q, k, v, do, dt)
    got, _ = _fwd_bwd(dt, qs, k, v, do, N)          # asserts every output finite
    ref = _reference(qs, k, v, do)
    emu = _emulate(qs, k, v, do, dt)
    eg, tol = _compare(f"[{dt} overflow N={N}]", got, emu, ref)
    for name, row in (("dq", Q), ("dk", K), ("dv", K)):
        e = eg[name].view(B * H, N)[:, row]
        print(f"[{dt} overflow] planted row {row} of {name}: {float(e.max()):.3e} (allowed {tol[name]:.3e})")
        assert float(e.max()) <= tol[name], f"{name} planted row {row}: {e.tolist()} > {tol[name]:.3e}"


# ================================================================================================ 6: the two staging forms
@pytest.mark.parametrize("fast", ["1", "0"])
@pytest.mark.parametrize("N", [1, 63, 65, 129, 322])
def test_attention_fwd_bf16_staging_forms_bit_identical(N, fast, monkeypatch):
    """S3OD_ATTN_DMA=0 (K / V staged through registers) against =1 (LDS-DMA), fixed-max and lazy-rescale loops: both
    kernels run the one tile body of attn_fwd_kernel on the same LDS images, so o and lse are bit-identical -- an
    equality, not a tolerance (the full-size test asserts it at N = 4101)"""
    qs, k, v, _ = _inputs(N, "bf16", seed=4000 + N)
    monkeypatch.setenv("S3OD_ATTN_FAST", fast)         # read per call: tests/conftest.py sets S3OD_AB=1
    got = {}
    for dma in ("1", "0"):
        monkeypatch.setenv("S3OD_ATTN_DMA", dma)
        got[dma] = _forward("bf16", qs, k, v, N)       # carved: slack untouched, every element written and finite
    for name, a, b in zip(("o", "lse"), got["0"], got["1"]):
        ndiff = int((a.contiguous().view(torch.uint8) != b.contiguous().view(torch.uint8)).sum())
        print(f"[bf16 N={N} FAST={fast}] DMA=0 vs DMA=1 {name}: {ndiff} differing bytes")
        assert torch.equal(a, b) and ndiff == 0, f"{name}: DMA=0 differs from DMA=1 in {ndiff} bytes"
