"""GPU: s3od_linear_fwd / _dgrad / _wgrad and s3od_qkv_rope_fwd (csrc/linear_ops.hip on the implicit-GEMM engine of
csrc/gemm.hpp) element by element against float64, in both compute dtypes, at the shapes the large bf16 rel-L2 tests
never reach: M < 256, M tails of 1 / 44 / 255 rows (the skinny tail kernel in bf16: K % 32 != 0, K / 32 not a multiple
of its unroll, N % 64 != 0, its N-contiguous-B staging at unroll 16 / 12 / 8), N off the 64 / 128 / 256-column tiles,
K below one K tile, every tile configuration 0 - 4 with fewer K tiles than stages, token-row mode, every leading
dimension padded, and the epilogue forms (scale / shift / res2 / bf16 residuals / GELU_SG / ACT_MUL / column sums).

Every tensor a kernel touches comes from _gemm_ref.poisoned: NaN guard columns (ld = natural + 8 or + 16) and 64 NaN
slack rows around it, inputs included -- a pad column or a row past M that is read and multiplied by zero turns the
output NaN, an unwritten output element stays NaN, and a written guard is found afterwards.  References, caps and the
f32 emulation are tests/_gemm_ref.py's (derived there, none taken from a kernel); each case prints its worst ratio
(pytest -s).  Knobs are toggled with monkeypatch.setenv (the suite sets S3OD_AB=1: read per call)."""
import ctypes

import pytest
import torch

import _gemm_ref as R

pytestmark = pytest.mark.gpu
NAN = R.NAN


def _lib():
    from s3od_amd._lib import lib, stream
    return lib(), stream()


def _rand(g, *shape, dt=torch.float32, scale=1.0):
    """CPU values already rounded to the dtype the kernel reads"""
    return (torch.randn(*shape, generator=g) * scale).to(dt)


def _up(v, pad=0, dtype=None):
    """upload into a poisoned buffer (2-D: rows `pad` elements wider than the logical row)"""
    if v is None:
        return None
    return R.poisoned_from(v, (v.shape[-1] + pad) if pad else None, dtype or v.dtype)


def _ld(t, natural=0):
    return natural if t is None else R.ld_of(t)


_REFS = {}


def _shared(key, make):
    """a reference is computed once per case and shared by the knob variants that reuse it"""
    if key not in _REFS:
        _REFS[key] = make()
    return _REFS[key]


# ------------------------------------------------------------------------------------------------ s3od_linear_fwd
FWD_FORMS = {
    #            bias  scale/shift  act               res1   res2   res_f32 out_f32 pre
    "none":     (False, False, R.ACT_NONE,    False, False, False, False, False),
    "bias":     (True,  False, R.ACT_NONE,    False, False, False, False, False),
    "relu_res": (True,  True,  R.ACT_RELU,    True,  True,  False, False, True),
    "oproj":    (True,  True,  R.ACT_NONE,    True,  False, True,  True,  True),
    "gelu":     (True,  False, R.ACT_GELU,    False, False, False, False, True),
    "gelu_sg":  (True,  False, R.ACT_GELU_SG, False, False, False, False, True),
}
FWD_CASES = [
    ((1, 8, 8), "none"), ((1, 8, 8), "relu_res"),
    ((5, 24, 40), "bias"), ((5, 24, 40), "oproj"),
    ((130, 96, 72), "gelu"), ((130, 96, 72), "gelu_sg"), ((130, 96, 72), "relu_res"),
    ((256, 128, 64), "none"), ((256, 128, 64), "oproj"),
    ((257, 136, 200), "bias"), ((257, 136, 200), "relu_res"), ((257, 136, 200), "gelu"), ((257, 136, 200), "oproj"),
    ((511, 768, 768), "bias"), ((511, 768, 768), "gelu_sg"), ((511, 768, 768), "oproj"),
    ((300, 256, 2112), "none"), ((300, 256, 2112), "relu_res"), ((300, 256, 2112), "gelu"),
]


def _fwd_case(dtype, M, N, K, form):
    """operands (CPU, in the kernel's dtypes) and the Ref of one forward case"""
    def make():
        dt = R.DT[dtype][0]
        has_b, has_s, act, has_r1, has_r2, res_f32, out_f32, _ = FWD_FORMS[form]
        g = torch.Generator().manual_seed(M * 7 + N * 3 + K + len(form))
        c = dict(x=_rand(g, M, K, dt=dt), w=_rand(g, N, K, dt=dt, scale=K ** -0.5),
                 bias=_rand(g, N, scale=0.5) if has_b else None,
                 scale=(torch.rand(N, generator=g) + 0.5) if has_s else None,
                 shift=_rand(g, N, scale=0.3) if has_s else None,
                 res1=_rand(g, M, N, dt=torch.float32 if res_f32 else dt) if has_r1 else None,
                 res2=_rand(g, M, N, dt=torch.float32 if res_f32 else dt) if has_r2 else None)
        f32_out = out_f32 or dtype == "f32"
        c["ref"] = R.ref_linear(R.wide(c["x"]), R.wide(c["w"]).T, dtype, emu=f32_out, out_f32=out_f32, act=act,
                                **{k: R.wide(c[k]) for k in ("bias", "scale", "shift", "res1", "res2")})
        return c
    return _shared(("fwd", dtype, M, N, K, form), make)


def _run_fwd(dtype, M, N, K, form, label):
    L, st = _lib()
    dt, code = R.DT[dtype]
    _, _, act, _, _, res_f32, out_f32, has_pre = FWD_FORMS[form]
    c = _fwd_case(dtype, M, N, K, form)
    r = c["ref"]
    x, w = _up(c["x"], 16), _up(c["w"])
    bias, scale, shift = _up(c["bias"]), _up(c["scale"]), _up(c["shift"])
    res1, res2 = _up(c["res1"], 8), _up(c["res2"], 16)
    out = R.poisoned((M, N), N + 8, torch.float32 if out_f32 else dt)
    pre = R.poisoned((M, N), N + 16, dt) if has_pre else None
    L("s3od_linear_fwd", code, M, N, K, x, R.ld_of(x), w, bias, scale, shift, act, res1, _ld(res1), res2, _ld(res2),
      int(res_f32), out, R.ld_of(out), int(out_f32), pre, _ld(pre), 0, 0, 0, st)
    torch.cuda.synchronize()
    f32_out = out_f32 or dtype == "f32"
    R.check(out, r.out, r.t_out, r.emu_out if f32_out else None, r.skip, label=f"{label} out")
    if has_pre:
        R.check(pre, r.pre, r.t_pre, r.emu_pre if dtype == "f32" else None, label=f"{label} pre")
    assert R.guards_intact(out) and (pre is None or R.guards_intact(pre)), "a guard column or slack row was written"
    return out, pre


def _both(cases, bf16_only):
    """(dtype, shape, form) of every case in both dtypes; the bf16-mode forms in bf16 alone"""
    p = [(d, s, f) for d in ("f32", "bf16") for s, f in cases if d == "bf16" or f not in bf16_only]
    return dict(argvalues=p, ids=[f"{d}-{s[0]}x{s[1]}x{s[2]}-{f}" for d, s, f in p])


@pytest.mark.parametrize("dtype,shape,form", **_both(FWD_CASES, ("gelu_sg",)))
def test_linear_fwd(dtype, shape, form):
    """ACT_GELU_SG is a bf16-mode form (the f32 path keeps the pre-activation): bf16 only"""
    _run_fwd(dtype, *shape, form, f"linear_fwd {dtype} {shape} {form}")


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("B,P,prefix", [(3, 49, 5), (2, 196, 5)])
def test_linear_fwd_token_rows(dtype, B, P, prefix):
    """row_mode 1 (the patch embedding): GEMM row b P + p lands in row b (P + prefix) + prefix + p of an f32
    tensor; the prefix rows of every image stay NaN."""
    L, st = _lib()
    dt, code = R.DT[dtype]
    M, N, K = B * P, 768, 768
    g = torch.Generator().manual_seed(B * P)
    x, w, bias = _rand(g, M, K, dt=dt), _rand(g, N, K, dt=dt, scale=K ** -0.5), _rand(g, N, scale=0.5)
    r = R.ref_linear(R.wide(x), R.wide(w).T, dtype, emu=True, out_f32=True, bias=R.wide(bias))
    xg = _up(x, 8)
    out = R.poisoned((B * (P + prefix), N), N + 8, torch.float32)
    L("s3od_linear_fwd", code, M, N, K, xg, R.ld_of(xg), _up(w), _up(bias), None, None, R.ACT_NONE, None, 0, None, 0, 0,
      out, R.ld_of(out), 1, None, 0, 1, P, prefix, st)
    torch.cuda.synchronize()
    R.check_token_rows(out, r.out, r.t_out, B, P, prefix, r.emu_out, label=f"linear_fwd token rows {dtype} B{B} P{P}")
    assert R.guards_intact(out)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("cfg", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("K", [8, 72, 136, 200])
def test_linear_fwd_tile_configs(monkeypatch, dtype, cfg, K):
    """(300, 264, K) under every forced tile configuration: 1 - 4 K tiles (bf16; 1 - 7 in f32) against 2 or 3
    pipeline stages, an N tail in the 128- and 256-wide tiles, and the 44-row M tail (always the 128x128 / skinny
    launch).  Configs 5 and 6 have their own files."""
    monkeypatch.setenv("S3OD_GEMM_CFG", str(cfg))
    _run_fwd(dtype, 300, 264, K, "bias", f"linear_fwd {dtype} (300, 264, {K}) cfg {cfg}")


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_linear_fwd_tail_skinny_knob(monkeypatch, dtype):
    """S3OD_TAIL_SKINNY=0 (the 128x128 tail launch) and the default (bf16: the skinny kernel) both pass, and the
    bf16 results are bit-identical: the skinny kernel runs the same MFMA chain."""
    outs = []
    for knob in ("0", None):
        if knob is None:
            monkeypatch.delenv("S3OD_TAIL_SKINNY", raising=False)
        else:
            monkeypatch.setenv("S3OD_TAIL_SKINNY", knob)
        outs.append(_run_fwd(dtype, 257, 136, 200, "relu_res", f"linear_fwd {dtype} (257, 136, 200) TAIL_SKINNY={knob}"))
    if dtype == "bf16":
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


# ------------------------------------------------------------------------------------------------ s3od_linear_dgrad
#               act              aux       out_f32  colsum
DG_FORMS = {
    "plain":       (R.ACT_NONE,     None,      False, False),
    "aux":         (R.ACT_NONE,     "sep",     False, False),
    "aux_inplace": (R.ACT_NONE,     "inplace", False, False),
    "f32_inplace": (R.ACT_NONE,     "inplace", True,  False),
    "gelu_bwd":    (R.ACT_GELU_BWD, "sep",     False, False),
    "act_mul":     (R.ACT_MUL,      "sep",     False, False),
    "colsum":      (R.ACT_NONE,     None,      False, True),
}
DG_CASES = [
    ((1, 8, 8), "plain"), ((1, 8, 8), "aux_inplace"),
    ((130, 96, 72), "plain"), ((130, 96, 72), "aux"), ((130, 96, 72), "gelu_bwd"), ((130, 96, 72), "colsum"),
    ((130, 96, 72), "f32_inplace"),
    ((257, 136, 200), "plain"), ((257, 136, 200), "aux_inplace"), ((257, 136, 200), "act_mul"),
    ((257, 136, 200), "colsum"), ((257, 136, 200), "gelu_bwd"),
    ((300, 768, 512), "plain"), ((300, 768, 512), "aux"), ((300, 768, 512), "f32_inplace"),
    ((300, 768, 384), "plain"), ((300, 768, 384), "act_mul"), ((300, 768, 384), "colsum"),
    ((300, 768, 776), "plain"), ((300, 768, 776), "gelu_bwd"), ((300, 768, 776), "aux_inplace"),
]


def _dg_case(dtype, M, N, K, form):
    def make():
        dt = R.DT[dtype][0]
        act, aux_kind, out_f32, has_cs = DG_FORMS[form]
        g = torch.Generator().manual_seed(M * 5 + N * 3 + K + len(form))
        c = dict(dy=_rand(g, M, K, dt=dt), w=_rand(g, K, N, dt=dt, scale=K ** -0.5),
                 aux=_rand(g, M, N, dt=torch.float32 if out_f32 else dt) if aux_kind else None,
                 cs0=_rand(g, N) if has_cs else None)
        c["ref"] = R.ref_linear(R.wide(c["dy"]), R.wide(c["w"]), dtype, emu=out_f32 or dtype == "f32", out_f32=out_f32,
                                act=act, res1=R.wide(c["aux"]))
        return c
    return _shared(("dgrad", dtype, M, N, K, form), make)


def _run_dgrad(dtype, M, N, K, form, label):
    L, st = _lib()
    dt, code = R.DT[dtype]
    act, aux_kind, out_f32, has_cs = DG_FORMS[form]
    c = _dg_case(dtype, M, N, K, form)
    r = c["ref"]
    dy, w = _up(c["dy"], 8), _up(c["w"])
    odt = torch.float32 if out_f32 else dt
    if aux_kind == "inplace":
        dx = _up(c["aux"], 16, odt)
        aux = dx
    else:
        dx = R.poisoned((M, N), N + 16, odt)
        aux = _up(c["aux"], 8)
    cs = _up(c["cs0"])
    L("s3od_linear_dgrad", code, M, N, K, dy, R.ld_of(dy), w, act, aux, _ld(aux, N), dx, R.ld_of(dx), int(out_f32),
      0, 0, 0, cs, st)
    torch.cuda.synchronize()
    R.check(dx, r.out, r.t_out, r.emu_out if (out_f32 or dtype == "f32") else None, label=f"{label} dx")
    assert R.guards_intact(dx), "a guard column or slack row of dx was written"
    if has_cs:
        ref, t = R.colsum_ref(r, c["cs0"])
        R.check(cs, ref, t, label=f"{label} colsum")
        assert R.guards_intact(cs)


@pytest.mark.parametrize("dtype,shape,form", **_both(DG_CASES, ("act_mul",)))
def test_linear_dgrad(dtype, shape, form):
    """ACT_MUL consumes the derivative ACT_GELU_SG saves, a bf16-mode form: bf16 only"""
    _run_dgrad(dtype, *shape, form, f"linear_dgrad {dtype} {shape} {form}")


@pytest.mark.parametrize("blaslt", ["1", "0"])
@pytest.mark.parametrize("shape,form", [c for c in DG_CASES if c[1] in ("plain", "aux", "aux_inplace")],
                         ids=[f"{m}x{n}x{k}-{f}" for (m, n, k), f in DG_CASES if f in ("plain", "aux", "aux_inplace")])
def test_linear_dgrad_blaslt_knob(monkeypatch, blaslt, shape, form):
    """the plain bf16 data gradients with S3OD_DGRAD_BLASLT 1 (whole 256-row panels through the library GEMM, which
    must leave the guard columns of a padded lddx / ldaux alone too) and 0 (everything on the engine)"""
    monkeypatch.setenv("S3OD_DGRAD_BLASLT", blaslt)
    _run_dgrad("bf16", *shape, form, f"linear_dgrad bf16 {shape} {form} BLASLT={blaslt}")


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_linear_dgrad_token_rows(dtype):
    """the projection data gradient as the engine calls it: row_mode 1, f32 out accumulated in place (aux = dx,
    ldaux = N).  Patch rows gain dy w; the prefix rows keep their values bit for bit."""
    L, st = _lib()
    dt, code = R.DT[dtype]
    B, P, prefix, N, K = 2, 196, 5, 768, 256
    M = B * P
    g = torch.Generator().manual_seed(17)
    dy, w = _rand(g, M, K, dt=dt), _rand(g, K, N, dt=dt, scale=K ** -0.5)
    dx0 = _rand(g, B * (P + prefix), N)
    rows = R.token_rows(B, P, prefix)
    r = R.ref_linear(R.wide(dy), R.wide(w), dtype, emu=True, out_f32=True, res1=R.wide(dx0[rows]))
    dyg, dx = _up(dy, 8), _up(dx0)
    L("s3od_linear_dgrad", code, M, N, K, dyg, R.ld_of(dyg), _up(w), R.ACT_NONE, dx, N, dx, N, 1, 1, P, prefix, None, st)
    torch.cuda.synchronize()
    got = dx.cpu()
    keep = torch.ones(B * (P + prefix), dtype=torch.bool)
    keep[rows] = False
    assert torch.equal(got[keep], dx0[keep]), "a prefix row changed"
    R.check(got[rows], r.out, r.t_out, r.emu_out, label=f"linear_dgrad token rows {dtype}")
    assert R.guards_intact(dx)


# ------------------------------------------------------------------------------------------------ s3od_linear_wgrad
WG_SHAPES = [(8, 8, 1), (24, 40, 7), (96, 72, 130), (264, 136, 1000), (1032, 1024, 300)]


def _wg_case(dtype, Nout, Kin, rows, split):
    def make():
        dt = R.DT[dtype][0]
        g = torch.Generator().manual_seed(Nout + Kin * 3 + rows)
        c = dict(dy=_rand(g, rows, Nout, dt=dt), x=_rand(g, rows, Kin, dt=dt), dw0=_rand(g, Nout, Kin))
        # one more f32 addition per split (atomics or the slab reduce); split 0: at most a quarter of the K tiles
        extra = split if split else max(1, -(-rows // 32) // 4)
        c["ref"] = R.ref_linear(R.wide(c["dy"]).T, R.wide(c["x"]), "f32", emu=True, res1=R.wide(c["dw0"]), extra=extra)
        return c
    return _shared(("wgrad", dtype, Nout, Kin, rows, split), make)


def _run_wgrad(dtype, Nout, Kin, rows, split, with_slab, label):
    L, st = _lib()
    dt, code = R.DT[dtype]
    c = _wg_case(dtype, Nout, Kin, rows, split)
    r = c["ref"]
    dy, x, dw = _up(c["dy"], 8), _up(c["x"], 16), _up(c["dw0"])
    slab, nbytes = None, 0
    if with_slab:
        nb = ctypes.c_long(0)
        L("s3od_linear_wgrad_ws", code, Nout, Kin, rows, split, ctypes.addressof(nb))
        nbytes = int(nb.value)
        slab = torch.full((nbytes // 4 + 128,), NAN, device=R.DEVICE)[64:-64] if nbytes else None
    L("s3od_linear_wgrad", code, Nout, Kin, rows, dy, R.ld_of(dy), x, R.ld_of(x), dw, split, slab, nbytes, st)
    torch.cuda.synchronize()
    R.check(dw, r.out, r.t_out, r.emu_out, label=f"{label} dw (slab bytes {nbytes})")
    assert R.guards_intact(dw) and (slab is None or R.guards_intact(slab))
    return nbytes


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("split", [0, 3])
@pytest.mark.parametrize("Nout,Kin,rows", WG_SHAPES[:4])
def test_linear_wgrad(dtype, split, Nout, Kin, rows):
    """dw = dw0 + dy^T x from a non-zero dw0, padded lddy / ldx, the split-K factor chosen by the library and forced
    to 3 (more splits than K tiles at rows 1 and 7)"""
    _run_wgrad(dtype, Nout, Kin, rows, split, False, f"linear_wgrad {dtype} ({Nout}, {Kin}, {rows}) split {split}")


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("with_slab", [True, False])
@pytest.mark.parametrize("split", [0, 3])
def test_linear_wgrad_large_output(dtype, with_slab, split):
    """(1032, 1024, 300): over 1M outputs, so bf16 runs the 4-wave 256x256 kernel -- with the caller's NaN-poisoned
    slab from s3od_linear_wgrad_ws (split-K partials in slabs, summed by the reduce kernel) and without (atomics)."""
    nbytes = _run_wgrad(dtype, *WG_SHAPES[4], split, with_slab, f"linear_wgrad {dtype} {WG_SHAPES[4]} split {split}")
    if dtype == "bf16" and with_slab and split == 3:
        assert nbytes == 4 * 3 * 1032 * 1024, "the forced 3-way split of the 256x256 kernel wants three slabs"


# ------------------------------------------------------------------------------------------------ s3od_qkv_rope_fwd
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("B,Ntok,P,H", [(2, 9, 4, 2), (2, 54, 49, 12), (5, 54, 49, 12), (1, 261, 256, 12)])
def test_qkv_rope_fwd(dtype, B, Ntok, P, H):
    """q | k | v = x w^T + bias with RoPE on the P patch tokens of q and k (random angle tables), q times
    S3OD_QSCALE, split to [B, H, Ntok, 64] tensors carved from NaN.  (5, 54, ...) = 270 rows: a 14-row tail launch
    whose rows start inside image 4, so the launch's row offset must enter the token index."""
    L, st = _lib()
    dt, code = R.DT[dtype]
    D, M = 64 * H, B * Ntok
    g = torch.Generator().manual_seed(B * 100 + Ntok)
    x, w, bias = _rand(g, M, D, dt=dt), _rand(g, 3 * D, D, dt=dt, scale=D ** -0.5), _rand(g, 3 * D, scale=0.5)
    ang = torch.rand(P, 64, generator=g) * 6.2831853
    cos, sin = ang.cos(), ang.sin()
    ref = R.ref_qkv_rope(R.wide(x), R.wide(w), R.wide(bias), R.wide(cos), R.wide(sin), B, Ntok, P, H, dtype, emu=dtype == "f32")
    q, k, v = (R.poisoned((B, H, Ntok, 64), None, dt) for _ in range(3))
    L("s3od_qkv_rope_fwd", code, B, Ntok, P, H, _up(x), _up(w), _up(bias), _up(cos), _up(sin), q, k, v, st)
    torch.cuda.synchronize()
    for name, got in zip("qkv", (q, k, v)):
        R.check(got, *ref[name], label=f"qkv_rope {dtype} B{B} Ntok{Ntok} P{P} H{H} {name}")
        assert R.guards_intact(got)
