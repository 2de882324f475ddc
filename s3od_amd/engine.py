"""Native executor of the S3OD hot path: DINOv3 ViT-B/16 encoder + DPT decoder + mask heads.

Every arithmetic op runs in libs3od_hip.so (gfx950 HIP kernels); PyTorch only provides
device memory (caching allocator), streams and the autograd / nn.Module surface.

Layouts: tokens [B, Ntok, 768] (fp32 residual stream); q/k/v [B*12, Ntok, 64]; decoder
activations NHWC [B, H, W, C]; compute dtype T = bf16 (fast) or f32 (strict parity).
Parameters stay fp32 in the reference's state_dict layout; ``prepare()`` repacks them into
kernel layouts ([Cout][KH][KW][Cin], fused QKV [2304][768]) in T.

Reference structure: src/s3od/model.py:62-467 and tf:models/dinov3_vit/modeling_dinov3_vit.py.
"""
from __future__ import annotations

import ctypes
import os
from collections import namedtuple
from dataclasses import dataclass, field
from functools import partial

import torch

from ._lib import lib, stream, F32, BF16, NREP
from .weights import OUT_CH, VARIANTS

NREG = 4
ACT_NONE, ACT_RELU, ACT_GELU, ACT_GELU_BWD, ACT_RELU_BWD = 0, 1, 2, 3, 4
# bf16 training: the up-projection saves gelu'(v) (one erf for both outputs) and the down dgrad multiplies by it;
# the f32 strict path keeps the pre-activation and the exact erf GELU' (ACT_GELU_BWD)
ACT_GELU_SG, ACT_MUL = 5, 6


def _E(n, dt, dev):
    return torch.empty(n, dtype=dt, device=dev)


class ConvGeom(namedtuple("ConvGeom", "B H W Cin OH OW Cout k s p")):
    """One conv layer's geometry in the view the C ABI uses: input grid [B, H, W, Cin], output grid [B, OH, OW, Cout],
    square kernel k, stride s, padding p.  Built once by the forward; the backward reads it from the Ctx."""
    __slots__ = ()

    @classmethod
    def conv(cls, B, H, W, Cin, Cout, k, s, p):
        return cls(B, H, W, Cin, (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1, Cout, k, s, p)

    @classmethod
    def convT(cls, B, IH, IW, Cin_T, Cout_T, k, s, p):
        """A ConvTranspose2d in the module's own terms, as the conv whose data gradient it is: the module's output
        is the conv's input grid, and its weight [Cin_T][Cout_T] is the conv's [Cout][Cin]."""
        return cls(B, (IH - 1) * s - 2 * p + k, (IW - 1) * s - 2 * p + k, Cout_T, IH, IW, Cin_T, k, s, p)

    @property
    def abi(self):
        """The argument prefix s3od_conv_fwd / s3od_conv_dgrad / s3od_conv_wgrad share."""
        return (self.B, self.H, self.W, self.Cin, self.OH, self.OW, self.Cout, self.k, self.k, self.s, self.p)


def decoder_geometry(B, ph, pw, n_masks):
    """name -> ConvGeom of every conv of the DPT head on a ph x pw patch grid (the 1x1 linears keep M, N, K)."""
    g = {"rs0": ConvGeom.convT(B, ph, pw, 256, 256, 4, 4, 0),         # resize_layers.0 / .1: ConvTranspose2d
         "rs1": ConvGeom.convT(B, ph, pw, 512, 512, 2, 2, 0),
         "rs3": ConvGeom.conv(B, ph, pw, 1024, 1024, 3, 2, 1)}
    grids = [(g["rs0"].H, g["rs0"].W), (g["rs1"].H, g["rs1"].W), (ph, pw), (g["rs3"].OH, g["rs3"].OW)]
    for i, ((h, w), c) in enumerate(zip(grids, OUT_CH)):
        g[f"rn{i + 1}"] = ConvGeom.conv(B, h, w, c, 256, 3, 1, 1)
        g[f"rcu{i + 1}"] = ConvGeom.conv(B, h, w, 256, 256, 3, 1, 1)   # all four RCU convs of refinenet i+1
    H1, W1 = 2 * grids[0][0], 2 * grids[0][1]                         # path_1: refinenet1 resizes 2x
    g["oc1"] = ConvGeom.conv(B, H1, W1, 256, 128, 3, 1, 1)
    g["up2x"] = ConvGeom.convT(B, H1, W1, 128, 64, 4, 2, 1)           # upsample_2x.0: ConvTranspose2d
    g["c64"] = ConvGeom.conv(B, g["up2x"].H, g["up2x"].W, 64, 64, 3, 1, 1)
    g["heads1"] = ConvGeom.conv(B, g["up2x"].H, g["up2x"].W, 64, 32 * n_masks, 3, 1, 1)   # the fused mask heads' 3x3
    return g


class SideRunner:
    """Stream discipline of one backward phase: work that only reads its operands (weight gradients, the gradient
    hook) runs on ``side`` beside the data-gradient chain on ``main``.  side=None: everything runs inline and no
    event is created."""

    def __init__(self, main, side=None):
        self.main, self.side = main, side
        self._free = {}                 # reused buffer -> event after its last side-stream reader

    def run(self, fn, tensors=(), names=()):
        """fn() on the side stream once it has caught up with main.  Operands are protected in one of two ways:
        ``tensors`` (fresh per call) are record_stream'd, so the caching allocator keeps them until fn has run;
        ``names`` of buffers the main stream reuses get an event, for claim() to wait on."""
        if self.side is None:
            return fn()
        e = torch.cuda.Event()
        e.record(self.main)
        self.side.wait_event(e)
        with torch.cuda.stream(self.side):
            fn()
        for t in tensors:
            t.record_stream(self.side)
        for n in names:
            f = torch.cuda.Event()
            f.record(self.side)
            self._free[n] = f

    def claim(self, name):
        """Before the main stream overwrites the reused buffer ``name``: wait for its last side-stream reader."""
        f = self._free.pop(name, None)
        if f is not None:
            self.main.wait_event(f)

    def hook(self, fn):
        """The gradient hook (the DDP bucket all-reduce): the gradients are final once both streams are past them,
        so it is issued from the side stream after it has joined main."""
        self.run(fn)

    def join(self):
        if self.side is not None:
            self.main.wait_stream(self.side)


@dataclass
class Ctx:
    """Tensors saved by a training forward for the native backward."""
    B: int = 0
    H: int = 0
    W: int = 0
    ph: int = 0
    pw: int = 0
    t: dict = field(default_factory=dict)


class DPTEngine:
    def __init__(self, params: dict, buffers: dict, compute_dtype: str = "bf16", variant: str = "dinob", n_masks: int = 3):
        """params / buffers: name -> fp32 CUDA tensor in the reference layout (canonical keys).
        variant: encoder geometry (weights.VARIANTS: dinob = ViT-B/16, dinol = ViT-L/16); n_masks: mask heads."""
        self.p = params
        self.buf = buffers
        c = VARIANTS[variant]
        self.D, self.H, self.MLP, self.taps = c.hidden, c.heads, c.mlp, c.taps
        self.last = max(c.taps)      # layers >= last (and the final norm) never reach the outputs
        self.nm = int(n_masks)
        self.set_dtype(compute_dtype)
        self.w = {}
        self._wkey = None
        self._zpool = {}       # persistent all-zero workspaces (the kernels that read them back leave them zero)
        self._nbt = []         # BatchNorm num_batches_tracked counters to bump once per forward
        self._slabs = {}       # hipStream_t -> split-K slab workspace (contents dead between calls)
        self._slab_need = {}   # shape key -> slab bytes the library asks for

    def zero_ws(self, key, n, dtype, dev):
        """Persistent workspace of >= n elements that is all zero between calls: every C-ABI entry given one
        (replicated column sums, BN statistics, split-K wgrad partials) clears what it reads back, so no
        memset is launched per call.  One buffer per key; all users run on one stream, in order."""
        t = self._zpool.get(key)
        if t is None or t.numel() < n or t.dtype != dtype or t.device != dev:
            t = torch.zeros(n, dtype=dtype, device=dev)
            self._zpool[key] = t
        return t

    def set_dtype(self, compute_dtype):
        assert compute_dtype in ("bf16", "f32")
        self.cdt = compute_dtype
        self.dt = BF16 if compute_dtype == "bf16" else F32
        self.tdt = torch.bfloat16 if compute_dtype == "bf16" else torch.float32
        self._wkey = None
        self._packs = None

    # ------------------------------------------------------------------ weights
    def _version_key(self):
        return (self.cdt, sum(int(v._version) for v in self.p.values()), id(self))

    def prepare(self, force=False):
        """Repack / cast all fp32 parameters into kernel layouts (cached until params change).

        The packed buffers are allocated once; every refresh (after each optimizer step) is two
        launches of ``s3od_repack_multi`` -- one for the compute-dtype weights, one for the fp32
        fused bias vectors -- instead of ~100 per-tensor repacks and torch copies."""
        key = self._version_key()
        if not force and key == self._wkey:
            return
        ptrs = tuple(v.data_ptr() for v in self.p.values())
        if getattr(self, "_packs", None) is None or self._packs["ptrs"] != ptrs or self._packs["dt"] != self.dt:
            self._build_packs(ptrs)
        L, st = lib(), stream()
        L.phase = "prepare"
        for dt, tab in self._packs["tabs"]:
            L("s3od_repack_multi", dt, tab["tab"], tab["ct"], tab["co"], tab["n"], self._REPACK_CHUNK, st)
        L.phase = None
        self._wkey = key

    _REPACK_CHUNK = 16384

    def _build_packs(self, ptrs):
        """Allocate the kernel-layout buffers and the device tables that fill them from the masters."""
        P, T = self.p, self.tdt
        dev = next(iter(P.values())).device
        D, MLP, nm = self.D, self.MLP, self.nm
        ents = {self.dt: [], F32: []}          # dtype -> [(src, dst, dst_offset, O, I, KHW)]
        w = {}

        def pack(name, O, I, KH=1, KW=1, dst=None, off=0):
            if dst is None:
                dst = torch.empty((O, KH, KW, I), dtype=T, device=dev)
            ents[self.dt].append((P[name], dst, off, O, I, KH * KW, 0, 0))
            return dst

        def pack_dgrad(name, O, I, dst, off, ld, KHW=9, mode=1):
            """[I][3][3][ld] transposed + tap-reversed copy (column off..off+O): the weight of the
            stride-1 3x3 conv's data gradient run as a forward conv (s3od_conv_dgrad's wT); mode 2: transposed
            without the tap reversal."""
            ents[self.dt].append((P[name], dst, off, O, I, KHW, mode, ld))

        def copy32(name, dst, off, n):
            ents[F32].append((P[name], dst, off, n, 1, 1, 0, 0))

        e = "encoder.embeddings."
        w["pe"] = pack(e + "patch_embeddings.weight", D, 3 * 16 * 16)
        for i in range(self.last):
            p = f"encoder.model.layer.{i}."
            qkv = torch.empty((3 * D, D), dtype=T, device=dev)
            for j, nme in enumerate(("q_proj", "k_proj", "v_proj")):
                pack(p + f"attention.{nme}.weight", D, D, dst=qkv, off=j * D * D)
            w[f"qkv{i}"] = qkv
            bq = torch.zeros(3 * D, dtype=torch.float32, device=dev)      # k_proj has no bias (key_bias=False)
            copy32(p + "attention.q_proj.bias", bq, 0, D)
            copy32(p + "attention.v_proj.bias", bq, 2 * D, D)
            w[f"bqkv{i}"] = bq
            w[f"o{i}"] = pack(p + "attention.o_proj.weight", D, D)
            w[f"up{i}"] = pack(p + "mlp.up_proj.weight", MLP, D)
            w[f"down{i}"] = pack(p + "mlp.down_proj.weight", D, MLP)
        h = "seg_head."
        for i, c in enumerate(OUT_CH):
            w[f"proj{i}"] = pack(h + f"projects.{i}.weight", c, D)
        w["rs0"] = pack(h + "resize_layers.0.weight", 256, 256, 4, 4)   # ConvT: [Cin_T][Cout_T] = conv view
        w["rs1"] = pack(h + "resize_layers.1.weight", 512, 512, 2, 2)
        w["rs3"] = pack(h + "resize_layers.3.weight", 1024, 1024, 3, 3)
        for i, c in enumerate(OUT_CH):
            w[f"rn{i + 1}"] = pack(h + f"scratch.layer{i + 1}_rn.weight", 256, c, 3, 3)
        for r in (1, 2, 3, 4):
            q = h + f"scratch.refinenet{r}."
            w[f"ref{r}.out"] = pack(q + "out_conv.weight", 256, 256)
            for u in (1, 2):
                for cv in (1, 2):
                    w[f"ref{r}.u{u}.c{cv}"] = pack(q + f"resConfUnit{u}.conv{cv}.weight", 256, 256, 3, 3)
        m = h + "mask_head."
        w["oc1"] = pack(m + "output_conv1.weight", 128, 256, 3, 3)
        w["up2x"] = pack(m + "upsample_2x.0.weight", 128, 64, 4, 4)     # ConvT [128][64][4][4]
        w["c64"] = pack(m + "upsample_2x.2.weight", 64, 64, 3, 3)
        heads = torch.empty((32 * nm, 3, 3, 64), dtype=T, device=dev)
        for k in range(nm):
            pack(m + f"mask_heads.{k}.0.weight", 32, 64, 3, 3, dst=heads, off=k * 32 * 9 * 64)
        w["heads1"] = heads
        if self.dt == BF16:       # data-gradient weights of the 3x3 s1 convs, run as forward convs (bf16 only)
            for r in (1, 2, 3, 4):
                q = h + f"scratch.refinenet{r}."
                for u in (1, 2):
                    for cv in (1, 2):
                        key = f"ref{r}.u{u}.c{cv}T"
                        w[key] = torch.empty((256, 3, 3, 256), dtype=T, device=dev)
                        pack_dgrad(q + f"resConfUnit{u}.conv{cv}.weight", 256, 256, w[key], 0, 256)
            for i, c in enumerate(OUT_CH):
                w[f"rn{i + 1}T"] = torch.empty((c, 3, 3, 256), dtype=T, device=dev)
                pack_dgrad(h + f"scratch.layer{i + 1}_rn.weight", 256, c, w[f"rn{i + 1}T"], 0, 256)
            w["oc1T"] = torch.empty((256, 3, 3, 128), dtype=T, device=dev)
            pack_dgrad(m + "output_conv1.weight", 128, 256, w["oc1T"], 0, 128)
            w["up2xT"] = torch.empty((64, 4, 4, 128), dtype=T, device=dev)       # ConvT sub-pixel kernel weight
            pack_dgrad(m + "upsample_2x.0.weight", 128, 64, w["up2xT"], 0, 128, KHW=16, mode=2)
            w["c64T"] = torch.empty((64, 3, 3, 64), dtype=T, device=dev)
            pack_dgrad(m + "upsample_2x.2.weight", 64, 64, w["c64T"], 0, 64)
            w["heads1T"] = torch.empty((64, 3, 3, 32 * nm), dtype=T, device=dev)
            for k in range(nm):
                pack_dgrad(m + f"mask_heads.{k}.0.weight", 32, 64, w["heads1T"], 32 * k, 32 * nm)
        for key, n, per in (("heads1_b", "0.bias", 32), ("heads2", "2.weight", 32), ("heads2_b", "2.bias", 1)):
            w[key] = torch.empty(per * nm, dtype=torch.float32, device=dev)
            for k in range(nm):
                copy32(m + f"mask_heads.{k}.{n}", w[key], k * per, per)
        tabs = []
        for dt, lst in ents.items():
            rows, ct, co = [], [], []
            for t, (src, dst, off, O, I, KHW, mode, ld) in enumerate(lst):
                rows.append([src.data_ptr(), dst.data_ptr(), O, I, KHW, off, mode, ld])
                for o in range(0, O * I * KHW, self._REPACK_CHUNK):
                    ct.append(t); co.append(o)
            tabs.append((dt, dict(tab=torch.tensor(rows, dtype=torch.int64, device=dev),
                                  ct=torch.tensor(ct, dtype=torch.int32, device=dev),
                                  co=torch.tensor(co, dtype=torch.int64, device=dev), n=len(ct))))
        self.w = w
        self._packs = {"ptrs": ptrs, "dt": self.dt, "tabs": tabs}

    # ------------------------------------------------------------------ helpers
    def _lin(self, x, w, M, N, K, out, bias=None, scale=None, shift=None, act=ACT_NONE, res1=None, res_f32=False,
             out_f32=False, pre=None, row_mode=0, P=0, prefix=0):
        lib()("s3od_linear_fwd", self.dt, M, N, K, x, K, w, bias, scale, shift, act,
              res1, N, None, 0, int(res_f32), out, N, int(out_f32), pre, N,
              row_mode, P, prefix, stream())

    def _conv(self, x, w, g, bias=None, scale=None, shift=None, act=ACT_NONE, relu_in=False, res1=None, res2=None,
              stats=None, colsum=None):
        """y [B,OH,OW,Cout] of conv g (also: the data gradient of a ConvTranspose2d given as ConvGeom.convT)."""
        out = torch.empty((g.B, g.OH, g.OW, g.Cout), dtype=self.tdt, device=x.device)
        lib()("s3od_conv_fwd", self.dt, *g.abi, x, int(relu_in), w,
              bias, scale, shift, act, res1, res2, out, None, stats, colsum, stream())
        return out

    def _dgrad_conv(self, dy, w, g, bias=None, act=ACT_NONE, res1=None, res2=None, colsum=None, wT=None):
        """dx [B,H,W,Cin] of conv g from dy on its output grid (res1: the ReLU mask's source for ACT_RELU_BWD; res2:
        a residual gradient added in; colsum: += column sums of dx; wT: the transposed tap-reversed weight of a 3x3
        s1 conv -> the halo-tile kernel)."""
        out = torch.empty((g.B, g.H, g.W, g.Cin), dtype=self.tdt, device=dy.device)
        lib()("s3od_conv_dgrad", self.dt, *g.abi, dy, w, bias, None, None, act, res1,
              res2, out, None, None, colsum, wT, stream())
        return out

    # ConvTranspose2d forward == the data gradient of its conv view g (ConvGeom.convT) with the conv-view weight (no
    # flip); wT: the transposed copy [Cout_T][k][k][Cin_T] for the 4x4 s2 sub-pixel kernel (bf16)
    _convT = _dgrad_conv

    def _bilinear(self, x, B, IH, IW, OH, OW, C):
        y = torch.empty((B, OH, OW, C), dtype=self.tdt, device=x.device)
        lib()("s3od_bilinear_fwd", self.dt, x, y, B, IH, IW, OH, OW, C, stream())
        return y

    # ------------------------------------------------------------------ encoder
    def encoder_forward(self, x, train=False, rope_rescale=None, ctx=None):
        lib().phase = "encoder"
        L, P, W8, dt, T = lib(), self.p, self.w, self.dt, self.tdt
        D, H, MLP = self.D, self.H, self.MLP
        st = stream()
        B, _, Hh, Ww = x.shape
        ph, pw = Hh // 16, Ww // 16
        NP = ph * pw
        Nt = NP + 1 + NREG
        M = B * Nt
        dev = x.device
        cs = _E((NP, 64), torch.float32, dev)
        sn = _E((NP, 64), torch.float32, dev)
        L("s3od_rope_table", cs, sn, ph, pw, float(rope_rescale) if (train and rope_rescale) else -1.0, st)
        cols = _E((B * NP, 768), T, dev)          # 3 x 16 x 16 patch pixels
        L("s3od_patch_im2col", dt, x, cols, B, Hh, Ww, st)
        xs = _E((B, Nt, D), torch.float32, dev)
        e = "encoder.embeddings."
        self._lin(cols, W8["pe"], B * NP, D, 768, xs, bias=P[e + "patch_embeddings.bias"], out_f32=True,
                  row_mode=1, P=NP, prefix=1 + NREG)
        L("s3od_token_prefix", xs, P[e + "cls_token"], P[e + "register_tokens"], B, Nt, D, st)
        if ctx is not None:
            ctx.t.update(cols=cols, cos=cs, sin=sn)
        taps = []
        for i in range(self.last):
            p = f"encoder.model.layer.{i}."
            if ctx is not None or i == 0:     # one set for all layers in eval, a fresh set per layer for the backward
                h1, o, a = _E((M, D), T, dev), _E((M, D), T, dev), _E((M, MLP), T, dev)
                q, k, v = (_E((B * H, Nt, 64), T, dev) for _ in range(3))
            if ctx is not None:
                mean1 = _E((M,), torch.float32, dev); rstd1 = torch.empty_like(mean1)
                mean2 = torch.empty_like(mean1); rstd2 = torch.empty_like(mean1)
                lse = _E((B * H, Nt), torch.float32, dev)
                u1 = _E((M, D), T, dev); u2 = _E((M, D), T, dev)
                hpre = _E((M, MLP), T, dev); h2 = _E((M, D), T, dev)
            else:
                mean1 = rstd1 = mean2 = rstd2 = _E((M,), torch.float32, dev)
                lse = None; u1 = u2 = hpre = None
                h2 = h1
            L("s3od_layernorm_fwd", dt, xs, P[p + "norm1.weight"], P[p + "norm1.bias"], h1, mean1, rstd1, M, D, 1e-5, st)
            L("s3od_qkv_rope_fwd", dt, B, Nt, NP, H, h1, W8[f"qkv{i}"], W8[f"bqkv{i}"], cs, sn, q, k, v, st)
            L("s3od_attn_fwd", dt, q, k, v, o, lse, B, H, Nt, st)
            xm = _E((B, Nt, D), torch.float32, dev)
            self._lin(o, W8[f"o{i}"], M, D, D, xm, bias=P[p + "attention.o_proj.bias"],
                      scale=P[p + "layer_scale1.lambda1"], res1=xs, res_f32=True, out_f32=True, pre=u1)
            L("s3od_layernorm_fwd", dt, xm, P[p + "norm2.weight"], P[p + "norm2.bias"], h2, mean2, rstd2, M, D, 1e-5, st)
            self._lin(h2, W8[f"up{i}"], M, MLP, D, a, bias=P[p + "mlp.up_proj.bias"],
                      act=ACT_GELU_SG if (hpre is not None and dt == BF16) else ACT_GELU, pre=hpre)
            xn = _E((B, Nt, D), torch.float32, dev)
            self._lin(a, W8[f"down{i}"], M, D, MLP, xn, bias=P[p + "mlp.down_proj.bias"],
                      scale=P[p + "layer_scale2.lambda1"], res1=xm, res_f32=True, out_f32=True, pre=u2)
            if ctx is not None:
                ctx.t[f"L{i}"] = dict(x=xs, h1=h1, mean1=mean1, rstd1=rstd1, q=q, k=k, v=v, o=o, lse=lse, u1=u1,
                                      xm=xm, h2=h2, mean2=mean2, rstd2=rstd2, hpre=hpre, a=a, u2=u2)
            xs = xn
            if i + 1 in self.taps:
                tp = _E((B, NP, D), T, dev)
                L("s3od_cast_tap", dt, xs, tp, B, Nt, NP, D, st)
                taps.append(tp)
        return taps, (B, ph, pw, Nt)

    # ------------------------------------------------------------------ decoder
    def _rcu(self, x, r, u, g, train, ctx, x0=None):
        """ResidualConvUnit (src/s3od/model.py:334-345) [+ x0 for the fusion add]; g: the geometry of both convs."""
        P, W8 = self.p, self.w
        q = f"seg_head.scratch.refinenet{r}.resConfUnit{u}."
        tag = f"ref{r}.u{u}"
        if not train:
            st = stream()
            s1, t1 = self._bnfold(q + "bn1", st)
            s2, t2 = self._bnfold(q + "bn2", st)
            a1 = self._conv(x, W8[tag + ".c1"], g, bias=P[q + "conv1.bias"], scale=s1, shift=t1, act=ACT_RELU, relu_in=True)
            return self._conv(a1, W8[tag + ".c2"], g, bias=P[q + "conv2.bias"], scale=s2, shift=t2, res1=x, res2=x0)
        L, st = lib(), stream()
        npix = g.B * g.H * g.W
        z1 = self._conv_bn_train(x, W8[tag + ".c1"], g, P[q + "conv1.bias"], relu_in=True)
        bn1 = self._bn_train(z1["stats"], npix, q + "bn1")
        a1 = torch.empty_like(z1["z"])
        L("s3od_affine_act", self.dt, z1["z"], bn1["scale"], bn1["shift"], 1, None, None, a1, a1.numel(), 256, st)
        z2 = self._conv_bn_train(a1, W8[tag + ".c2"], g, P[q + "conv2.bias"])
        bn2 = self._bn_train(z2["stats"], npix, q + "bn2")
        out = torch.empty_like(z2["z"])
        L("s3od_affine_act", self.dt, z2["z"], bn2["scale"], bn2["shift"], 0, x, x0, out, out.numel(), 256, st)
        if ctx is not None:   # train-mode BN under no_grad: batch statistics, nothing saved
            ctx.t[tag] = dict(x=x, z1=z1["z"], a1=a1, z2=z2["z"], bn1=bn1, bn2=bn2)
        return out

    def _conv_bn_train(self, x, wt, g, bias, relu_in=False):
        stats = self.zero_ws("bn_stats", NREP * 2 * 256, torch.float64, x.device)   # S3OD_NREP replicas, cleared by s3od_bn_finalize
        z = self._conv(x, wt, g, bias=bias, relu_in=relu_in, stats=stats)
        return dict(z=z, stats=stats)

    def _bn_train(self, stats, npix, name):
        P, dev = self.p, stats.device
        d = {k: torch.empty(256, dtype=torch.float32, device=dev) for k in ("mean", "rstd", "scale", "shift")}
        lib()("s3od_bn_finalize", stats, npix, P[name + ".weight"], P[name + ".bias"], self.buf[name + ".running_mean"],
              self.buf[name + ".running_var"], 0.1, 1e-5, d["mean"], d["rstd"], d["scale"], d["shift"], 256, stream())
        nbt = self.buf.get(name + ".num_batches_tracked")
        if nbt is not None:
            self._nbt.append(nbt)      # bumped together at the end of the forward (one launch)
        return d

    def _bnfold(self, name, st):
        P = self.p
        s = torch.empty(256, dtype=torch.float32, device=P[name + ".weight"].device)
        t = torch.empty_like(s)
        lib()("s3od_bn_fold", P[name + ".weight"], P[name + ".bias"], self.buf[name + ".running_mean"],
              self.buf[name + ".running_var"], 1e-5, s, t, 256, st)
        return s, t

    def _fusion(self, r, x0, x1, g, oh, ow, train, ctx):
        """FeatureFusionBlock (src/s3od/model.py:383-405) on the grid of g (its RCU convs' geometry). out_conv (1x1,
        bias) runs before the bilinear resize: both are linear and bilinear weights sum to one, so the order commutes.
        Returns (resized to oh x ow, the tensor before the resize)."""
        P, W8 = self.p, self.w
        B, h, w = g.B, g.H, g.W
        s = x0 if x1 is None else self._rcu(x1, r, 1, g, train, ctx, x0=x0)
        s = self._rcu(s, r, 2, g, train, ctx)
        q = f"seg_head.scratch.refinenet{r}."
        c = torch.empty_like(s)
        self._lin(s, W8[f"ref{r}.out"], B * h * w, 256, 256, c, bias=P[q + "out_conv.bias"])
        if ctx is not None:
            ctx.t[f"ref{r}"] = dict(s=s, h=h, w=w, oh=oh, ow=ow)
        return self._bilinear(c, B, h, w, oh, ow, 256), c

    def decoder_forward(self, taps, B, ph, pw, train=False, ctx=None):
        lib().phase = "decoder"
        L, P, W8, dt = lib(), self.p, self.w, self.dt
        st = stream()
        h = "seg_head."
        dev = taps[0].device
        NP = ph * pw
        proj = []
        for i, c in enumerate(OUT_CH):
            y = torch.empty((B, ph, pw, c), dtype=self.tdt, device=dev)
            self._lin(taps[i], W8[f"proj{i}"], B * NP, c, self.D, y, bias=P[h + f"projects.{i}.bias"])
            proj.append(y)
        geo = decoder_geometry(B, ph, pw, self.nm)     # every conv's geometry, stated once: the backward reads it from ctx
        f0 = self._convT(proj[0], W8["rs0"], geo["rs0"], bias=P[h + "resize_layers.0.bias"])
        f1 = self._convT(proj[1], W8["rs1"], geo["rs1"], bias=P[h + "resize_layers.1.bias"])
        f2 = proj[2]
        f3 = self._conv(proj[3], W8["rs3"], geo["rs3"], bias=P[h + "resize_layers.3.bias"])
        feats = [f0, f1, f2, f3]
        rn = [self._conv(f, W8[f"rn{i + 1}"], geo[f"rn{i + 1}"]) for i, f in enumerate(feats)]
        if ctx is not None:
            ctx.t["geo"] = geo
            ctx.t["dec"] = dict(taps=taps, proj=proj, feats=feats, rn=rn)
        rcu = [geo[f"rcu{r}"] for r in (1, 2, 3, 4)]
        p4, _ = self._fusion(4, rn[3], None, rcu[3], rcu[2].H, rcu[2].W, train, ctx)
        p3, _ = self._fusion(3, p4, rn[2], rcu[2], rcu[1].H, rcu[1].W, train, ctx)
        p2, _ = self._fusion(2, p3, rn[1], rcu[1], rcu[0].H, rcu[0].W, train, ctx)
        p1, c1 = self._fusion(1, p2, rn[0], rcu[0], geo["oc1"].H, geo["oc1"].W, train, ctx)
        # classifier head: AdaptiveAvgPool2d(1) -> Linear -> ReLU -> Linear.  The mean of p1 is taken over the
        # tensor BEFORE refinenet1's 2x bilinear resize (align_corners=False): every source pixel's weights over
        # the 4x outputs sum to 4 (edge rows / columns included: clamped taps add up to the same 2 per axis), so
        # mean(up2(c)) = mean(c) exactly in real arithmetic, read from a 4x smaller tensor (C5: 2.2 -> 0.55 GB)
        pooled = torch.empty((B, 256), dtype=torch.float32, device=dev)
        hw = rcu[0].H * rcu[0].W
        part = torch.empty((B, -(-hw // 1024), 256), dtype=torch.float32, device=dev)   # per-1024-pixel partial sums
        L("s3od_avgpool", dt, c1, pooled, part, B, hw, 256, st)
        hid = torch.empty((B, 64), dtype=torch.float32, device=dev)
        nm = self.nm
        iou = torch.empty((B, nm), dtype=torch.float32, device=dev)
        L("s3od_iou_head_fwd", pooled, P[h + "classifier_head.2.weight"], P[h + "classifier_head.2.bias"],
          P[h + "classifier_head.4.weight"], P[h + "classifier_head.4.bias"], hid, iou, B, nm, st)
        # mask head (src/s3od/model.py:455-467)
        m = h + "mask_head."
        oc1 = self._conv(p1, W8["oc1"], geo["oc1"], bias=P[m + "output_conv1.bias"])
        up = self._convT(oc1, W8["up2x"], geo["up2x"], bias=P[m + "upsample_2x.0.bias"], act=ACT_RELU, wT=W8.get("up2xT"))
        HH, WW = geo["c64"].H, geo["c64"].W
        c64 = self._conv(up, W8["c64"], geo["c64"], bias=P[m + "upsample_2x.2.bias"], act=ACT_RELU)
        # F.interpolate(size=(16ph,16pw), antialias=True) is an exact identity here (HH == 16*ph)
        assert HH == 16 * ph and WW == 16 * pw
        logits = torch.empty((B, nm, HH, WW), dtype=torch.float32, device=dev)
        hsave = torch.empty((B * HH * WW, 32 * nm), dtype=self.tdt, device=dev) if ctx is not None else None
        L("s3od_mask_heads_fwd", dt, B, HH, WW, nm, c64, W8["heads1"], W8["heads1_b"], W8["heads2"], W8["heads2_b"],
          logits, hsave, st)
        if ctx is not None:
            ctx.t["head"] = dict(p1=p1, pooled=pooled, hid=hid, oc1=oc1, up=up, c64=c64, hsave=hsave)
        lib().phase = None
        return {"pred_masks": logits, "pred_iou": iou, "features": p1.permute(0, 3, 1, 2)}

    # ------------------------------------------------------------------ full forward
    def _invalidate(self):
        """After a failed call: the persistent zero workspaces may hold partial sums of kernels whose
        clearing reader never ran, and BN counter bumps may be queued for a forward that did not finish.
        Drop both, so the next call allocates fresh zeros and bumps only its own counters."""
        self._zpool = {}
        self._nbt = []

    def forward(self, x, train=False, rope_rescale=None, ctx: Ctx | None = None):
        """x: [B,3,H,W] fp32 CUDA (normalised image).  Returns the reference output dict."""
        self._nbt = []
        try:
            return self._forward(x, train, rope_rescale, ctx)
        except BaseException:
            self._invalidate()
            raise

    def _forward(self, x, train, rope_rescale, ctx):
        if x.dtype != torch.float32:
            x = x.float()
        Hh, Ww = x.shape[2], x.shape[3]
        if Hh % 16 or Ww % 16:   # the stride-16 patch conv never reads the trailing rows / columns
            x = x[:, :, :16 * (Hh // 16), :16 * (Ww // 16)]
        x = x.contiguous()
        self.prepare()
        taps, (B, ph, pw, Nt) = self.encoder_forward(x, train, rope_rescale, ctx)
        if ctx is not None:
            ctx.B, ctx.H, ctx.W, ctx.ph, ctx.pw = B, x.shape[2], x.shape[3], ph, pw
        out = self.decoder_forward(taps, B, ph, pw, train, ctx)
        if self._nbt:
            torch._foreach_add_(self._nbt, 1)
            self._nbt = []
        return out

    # ================================================================== backward
    def _colsum(self, a, M, N, out):
        """Bias gradient out += column sums of a [M, N]: two fixed-order passes through a caller-owned partial-sum
        buffer (the library's own size query; allocated on the calling stream, so the caching allocator orders its
        reuse behind this stream)."""
        key = ("colsum", M, N)
        nb = self._slab_need.get(key)
        if nb is None:
            n = ctypes.c_long(0)
            lib()("s3od_colsum_ws", M, N, ctypes.addressof(n))
            nb = self._slab_need[key] = int(n.value)
        ws = torch.empty(max(nb // 4, 1), dtype=torch.float32, device=out.device)
        lib()("s3od_colsum", self.dt, a, N, M, N, out, ws, nb, stream())

    def _slab(self, entry, key, *args):
        """Caller-owned split-K slab workspace for a weight-gradient entry (the C ABI never allocates): sized by the
        library's own query (s3od_linear_wgrad_ws / s3od_conv_wgrad_ws; cached per shape), one buffer per stream --
        calls on one stream run in order, and the main and side streams both issue weight gradients.  Allocated
        under the stream that uses it, so the caching allocator orders any later reuse behind that stream."""
        nb = self._slab_need.get(key)
        if nb is None:
            n = ctypes.c_long(0)
            lib()(entry, *args, ctypes.addressof(n))
            nb = self._slab_need[key] = int(n.value)
        if nb == 0:
            return None, 0
        st = torch.cuda.current_stream()
        t = self._slabs.get(st.cuda_stream)
        if t is None or t.numel() * 4 < nb:
            t = self._slabs[st.cuda_stream] = torch.empty(nb // 4, dtype=torch.float32, device=st.device)
        return t, t.numel() * 4

    def _wgrad_lin(self, dy, x, Nout, Kin, rows, dw):
        slab, nb = self._slab("s3od_linear_wgrad_ws", ("lin", self.dt, Nout, Kin, rows), self.dt, Nout, Kin, rows, 0)
        lib()("s3od_linear_wgrad", self.dt, Nout, Kin, rows, dy, Nout, x, Kin, dw, 0, slab, nb, stream())

    def _dgrad_lin(self, dy, w, M, N, K, out, act=ACT_NONE, aux=None, out_f32=False, row_mode=0, P=0, prefix=0, ldaux=None,
                   colsum=None):
        lib()("s3od_linear_dgrad", self.dt, M, N, K, dy, K, w, act, aux, ldaux or N, out, N, int(out_f32),
              row_mode, P, prefix, colsum, stream())

    def _wgrad_conv(self, dy, x, g, dw, relu_x=False):
        """dw += the weight gradient of conv g from dy on its output grid and x on its input grid."""
        # taps > 1: fp32 workspace in the GEMM's [Cout][tap][Cin] layout (contiguous split-K atomics), zero between calls
        ws = self.zero_ws("wgrad", g.Cout * g.k * g.k * g.Cin, torch.float32, dy.device) if g.k > 1 else None
        slab, nb = self._slab("s3od_conv_wgrad_ws", ("conv", self.dt, g), self.dt, *g.abi, 0)
        lib()("s3od_conv_wgrad", self.dt, *g.abi, dy, x, int(relu_x), dw, ws, 0, slab, nb, stream())

    def _runner(self, dev, *knobs):
        """The SideRunner of one backward phase (the knobs are read per call; any of them at 0: one stream)."""
        main = torch.cuda.current_stream(dev)
        on = all(os.environ.get(k, "1") != "0" for k in knobs)
        return SideRunner(main, self._side_stream(dev) if on else None)

    @staticmethod
    def _side_wgrad(run, wgrad, dy, x, *args, **kw):
        """A decoder weight gradient beside the data-gradient chain: it only reads dy and x, both fresh per call, so
        they are record_stream'd and the caching allocator keeps them until it has run."""
        run.run(partial(wgrad, dy, x, *args, **kw), tensors=(dy, x))

    def _rcu_bwd(self, d_out, r, u, ctx, G, run):
        """Backward of a train-mode ResidualConvUnit; returns d(input) (including the skip path)."""
        L, P, W8 = lib(), self.p, self.w
        st = stream()
        q = f"seg_head.scratch.refinenet{r}.resConfUnit{u}."
        tag = f"ref{r}.u{u}"
        c, g = ctx.t[tag], ctx.t["geo"][f"rcu{r}"]
        npix = g.B * g.H * g.W
        sums = self.zero_ws("bn_sums", NREP * 3 * 256, torch.float64, d_out.device)   # S3OD_NREP replicas, zero between calls
        dz2 = torch.empty_like(d_out)
        L("s3od_bn_bwd", self.dt, d_out, c["z2"], None, c["bn2"]["mean"], c["bn2"]["rstd"], P[q + "bn2.weight"], sums, dz2,
          G[q + "bn2.weight"], G[q + "bn2.bias"], G[q + "conv2.bias"], npix, 256, st)
        self._side_wgrad(run, self._wgrad_conv, dz2, c["a1"], g, G[q + "conv2.weight"])
        da1 = self._dgrad_conv(dz2, W8[tag + ".c2"], g, wT=W8.get(tag + ".c2T"))
        dz1 = torch.empty_like(d_out)
        # ReLU mask recomputed from z1 and bn1's scale/shift (bit-identical to a1 > 0): a1 is not read
        L("s3od_bn_relu_bwd", self.dt, da1, c["z1"], c["bn1"]["scale"], c["bn1"]["shift"], c["bn1"]["mean"],
          c["bn1"]["rstd"], P[q + "bn1.weight"], sums, dz1,
          G[q + "bn1.weight"], G[q + "bn1.bias"], G[q + "conv1.bias"], npix, 256, st)
        self._side_wgrad(run, self._wgrad_conv, dz1, c["x"], g, G[q + "conv1.weight"], relu_x=True)
        # RELU_BWD mask from the un-ReLU'd input, plus the skip path's gradient
        return self._dgrad_conv(dz1, W8[tag + ".c1"], g, act=ACT_RELU_BWD, res1=c["x"], res2=d_out, wT=W8.get(tag + ".c1T"))

    def _fusion_bwd(self, r, d_p, ctx, G, run, bcast=None, two_inputs=True):
        """Backward of FeatureFusionBlock r. Returns (d_x0, d_x1) (d_x1 None for refinenet4)."""
        L, W8 = lib(), self.w
        c = ctx.t[f"ref{r}"]
        B, h, w, oh, ow = ctx.B, c["h"], c["w"], c["oh"], c["ow"]
        dc = torch.empty((B, h, w, 256), dtype=self.tdt, device=d_p.device)
        L("s3od_bilinear_bwd", self.dt, d_p, bcast, dc, B, h, w, oh, ow, 256, stream())
        q = f"seg_head.scratch.refinenet{r}."
        npix = B * h * w
        self._colsum(dc, npix, 256, G[q + "out_conv.bias"])
        self._side_wgrad(run, self._wgrad_lin, dc, c["s"], 256, 256, npix, G[q + "out_conv.weight"])
        ds2 = torch.empty_like(dc)
        self._dgrad_lin(dc, W8[f"ref{r}.out"], npix, 256, 256, ds2)
        ds = self._rcu_bwd(ds2, r, 2, ctx, G, run)
        return ds, (self._rcu_bwd(ds, r, 1, ctx, G, run) if two_inputs else None)

    def decoder_backward(self, ctx, d_logits, d_iou, G, d_feat=None):
        lib().phase = "decoder"
        L, P, W8, dt = lib(), self.p, self.w, self.dt
        st = stream()
        dev = d_logits.device
        # weight gradients on the side stream (as in the encoder backward), concurrent with the data-gradient chain:
        # the decoder's many small-map convs (64^2, 32^2 at bs 16: a fraction of a round of tiles) and the wgrads'
        # tails then share the CUs.  S3OD_DEC_SIDE=0 (or S3OD_BWD_SIDE=0): inline on the main stream.
        run = self._runner(dev, "S3OD_BWD_SIDE", "S3OD_DEC_SIDE")
        wg = partial(self._side_wgrad, run, self._wgrad_conv)
        B, geo, hd, dec = ctx.B, ctx.t["geo"], ctx.t["head"], ctx.t["dec"]
        h = "seg_head."
        m = h + "mask_head."
        p1, c64, up, oc1 = hd["p1"], hd["c64"], hd["up"], hd["oc1"]
        # ---- the mask heads (fused, N = 32 * n_masks)
        nm = self.nm
        g = geo["heads1"]
        dh = torch.empty((B * g.H * g.W, 32 * nm), dtype=self.tdt, device=dev)
        L("s3od_mask_heads_bwd", dt, d_logits.contiguous(), hd["hsave"], W8["heads2"], dh, G["heads2_w"], G["heads2_b"],
          G["heads1_b"], B, g.H * g.W, nm, st)
        wg(dh, c64, g, G["heads1_w"])
        # (bias gradients are column sums fused into the epilogue that produces each gradient)
        d64 = self._dgrad_conv(dh, W8["heads1"], g, act=ACT_RELU_BWD, res1=c64, colsum=G[m + "upsample_2x.2.bias"],
                               wT=W8.get("heads1T"))
        # ---- upsample_2x.2 conv 64->64 + ReLU
        wg(d64, up, geo["c64"], G[m + "upsample_2x.2.weight"])
        dup = self._dgrad_conv(d64, W8["c64"], geo["c64"], act=ACT_RELU_BWD, res1=up, colsum=G[m + "upsample_2x.0.bias"],
                               wT=W8.get("c64T"))
        # ---- upsample_2x.0 ConvTranspose 128->64 k4 s2 p1 + ReLU (conv view: Y = oc1 grid, X = up grid)
        wg(oc1, dup, geo["up2x"], G[m + "upsample_2x.0.weight"])
        doc1 = self._conv(dup, W8["up2x"], geo["up2x"], colsum=G[m + "output_conv1.bias"])
        # ---- output_conv1 3x3 256->128
        wg(doc1, p1, geo["oc1"], G[m + "output_conv1.weight"])
        dp1 = self._dgrad_conv(doc1, W8["oc1"], geo["oc1"], wT=W8.get("oc1T"))
        if d_feat is not None:     # gradient of the returned features (= path_1, NCHW view)
            dp1.add_(d_feat.permute(0, 2, 3, 1).to(dp1.dtype))
        # ---- classifier head -> broadcast gradient onto path_1 (folded into the bilinear backward)
        dpix = torch.empty((B, 256), dtype=torch.float32, device=dev)
        L("s3od_iou_head_bwd", hd["pooled"], hd["hid"], P[h + "classifier_head.2.weight"], P[h + "classifier_head.4.weight"],
          d_iou.contiguous(), G[h + "classifier_head.2.weight"], G[h + "classifier_head.2.bias"],
          G[h + "classifier_head.4.weight"], G[h + "classifier_head.4.bias"], dpix, B, geo["oc1"].H * geo["oc1"].W, nm, st)
        # ---- refinenets
        dp2, drn1 = self._fusion_bwd(1, dp1, ctx, G, run, bcast=dpix)
        dp3, drn2 = self._fusion_bwd(2, dp2, ctx, G, run)
        dp4, drn3 = self._fusion_bwd(3, dp3, ctx, G, run)
        drn4, _ = self._fusion_bwd(4, dp4, ctx, G, run, two_inputs=False)
        drn = [drn1, drn2, drn3, drn4]
        dfeat = []
        # the feature gradient's column sums: resize_layers.{0,1,3}.bias; feature 2 is projects.2's output
        fbias = [h + "resize_layers.0.bias", h + "resize_layers.1.bias", h + "projects.2.bias", h + "resize_layers.3.bias"]
        for i, f in enumerate(dec["feats"]):
            g = geo[f"rn{i + 1}"]
            wg(drn[i], f, g, G[h + f"scratch.layer{i + 1}_rn.weight"])
            dfeat.append(self._dgrad_conv(drn[i], W8[f"rn{i + 1}"], g, colsum=G[fbias[i]], wT=W8.get(f"rn{i + 1}T")))
        proj = dec["proj"]
        # resize_layers.0 / .1: ConvTranspose (conv view: Y = proj grid, X = feature grid), so its data gradient is a conv
        dproj = [None, None, dfeat[2], None]
        for i in (0, 1):
            wg(proj[i], dfeat[i], geo[f"rs{i}"], G[h + f"resize_layers.{i}.weight"])
            dproj[i] = self._conv(dfeat[i], W8[f"rs{i}"], geo[f"rs{i}"], colsum=G[h + f"projects.{i}.bias"])
        wg(dfeat[3], proj[3], geo["rs3"], G[h + "resize_layers.3.weight"])
        dproj[3] = self._dgrad_conv(dfeat[3], W8["rs3"], geo["rs3"], colsum=G[h + "projects.3.bias"])
        # projects (1x1, bias) -> tap gradients
        dtaps = []
        for i, c in enumerate(OUT_CH):
            self._side_wgrad(run, self._wgrad_lin, dproj[i], dec["taps"][i], c, self.D, B * ctx.ph * ctx.pw,
                             G[h + f"projects.{i}.weight"])
            dtaps.append((dproj[i], c))
        lib().phase = None
        if self.grad_hook is not None:     # the decoder's gradients are final once both streams are past it
            run.hook(partial(self.grad_hook, "seg_head"))
        return dtaps

    def encoder_backward(self, ctx, dtaps, G):
        lib().phase = "encoder"
        L, P, W8, dt, T = lib(), self.p, self.w, self.dt, self.tdt
        D, H, MLP = self.D, self.H, self.MLP
        st = stream()
        B, ph, pw = ctx.B, ctx.ph, ctx.pw
        NP = ph * pw
        Nt = NP + 1 + NREG
        M = B * Nt
        dev = dtaps[0][0].device
        # the first tap gradient writes the patch rows; only the prefix rows (cls + registers) need zeros
        dx = torch.empty((B, Nt, D), dtype=torch.float32, device=dev)
        dx[:, :1 + NREG].zero_()
        first_tap = True
        tap_of = {t: j for j, t in enumerate(self.taps)}
        # weight gradients run on a side stream, concurrently with the data-gradient chain on the main stream: each
        # wgrad only READS its two operands, so it may trail the chain; its gradient operand is a chain buffer reused
        # by every layer, named to the runner: the chain claims it (waits for the reader's event) before it overwrites
        # it one layer later (in practice long done).  Two single-pipeline kernels then share the CUs: one's
        # store-bound epilogue / tail overlaps the other's MFMA main loop.  S3OD_BWD_SIDE=0: one stream (A/B)
        run = self._runner(dev, "S3OD_BWD_SIDE")

        def wg(name, dy, x, Nout, Kin, dw):
            run.run(partial(self._wgrad_lin, dy, x, Nout, Kin, M, dw), names=(name,))
        du, du2, dh = (_E((M, D), T, dev) for _ in range(3))     # the chain's buffers, reused by every layer
        dhp = _E((M, MLP), T, dev)
        dxm, dxi = (_E((B, Nt, D), torch.float32, dev) for _ in range(2))
        dqkv = _E((M, 3 * D), T, dev)
        delta = _E((B * H, Nt), torch.float32, dev)
        qv_ws = self.zero_ws("qv", NREP * 2 * D, torch.float32, dev)     # S3OD_NREP replicas of the q/v bias partials
        red_ws = self.zero_ws("red", NREP * 2 * D, torch.float32, dev)   # same, for LayerNorm / LayerScale parameter grads
        red2_ws = self.zero_ws("red2", NREP * 2 * D, torch.float32, dev)  # the LayerScale half of the fused LN + LS backward
        ls_done = False       # the layer's layer_scale2 backward already ran inside the layer above's norm1 backward
        for i in reversed(range(self.last)):
            if i + 1 in tap_of:
                dp, c = dtaps[tap_of[i + 1]]
                # dx[prefix-skipped rows] += dproj @ W_proj   (in-place accumulate, fp32)
                self._dgrad_lin(dp, W8[f"proj{tap_of[i + 1]}"], B * NP, D, c, dx, aux=None if first_tap else dx,
                                out_f32=True, row_mode=1, P=NP, prefix=1 + NREG, ldaux=D)
                first_tap = False
            p = f"encoder.model.layer.{i}."
            s = ctx.t[f"L{i}"]
            # ---- MLP half
            if not ls_done:
                run.claim("du")
                L("s3od_layerscale_bwd", dt, dx, s["u2"], P[p + "layer_scale2.lambda1"], du, G[p + "layer_scale2.lambda1"],
                  G[p + "mlp.down_proj.bias"], red_ws, M, D, st)
            wg("du", du, s["a"], D, MLP, G[p + "mlp.down_proj.weight"])
            run.claim("dhp")
            self._dgrad_lin(du, W8[f"down{i}"], M, MLP, D, dhp, act=ACT_MUL if dt == BF16 else ACT_GELU_BWD, aux=s["hpre"],
                            colsum=G[p + "mlp.up_proj.bias"])
            wg("dhp", dhp, s["h2"], MLP, D, G[p + "mlp.up_proj.weight"])
            self._dgrad_lin(dhp, W8[f"up{i}"], M, D, MLP, dh)
            # norm2 backward fused with the attention half's layer_scale1 backward (which reads its dxm)
            run.claim("du2")
            L("s3od_layernorm_ls_bwd", dt, dh, s["xm"], s["mean2"], s["rstd2"], P[p + "norm2.weight"], dx, dxm,
              G[p + "norm2.weight"], G[p + "norm2.bias"], red_ws, s["u1"], P[p + "layer_scale1.lambda1"], du2,
              G[p + "layer_scale1.lambda1"], G[p + "attention.o_proj.bias"], red2_ws, M, D, st)
            # ---- attention half
            wg("du2", du2, s["o"], D, D, G[p + "attention.o_proj.weight"])
            do = dh
            self._dgrad_lin(du2, W8[f"o{i}"], M, D, D, do)
            # attention backward with the inverse RoPE / q scale / q,v bias sums fused into its stores
            run.claim("dqkv")
            L("s3od_attn_bwd_qkv", dt, s["q"], s["k"], s["v"], s["o"], do, s["lse"], delta, ctx.t["cos"], ctx.t["sin"], NP,
              dqkv, G[p + "attention.q_proj.bias"], G[p + "attention.v_proj.bias"], qv_ws, B, H, Nt, st)
            wg("dqkv", dqkv, s["h1"], 3 * D, D, G[f"qkv_w{i}"])
            dh1 = dh
            self._dgrad_lin(dqkv, W8[f"qkv{i}"], M, D, 3 * D, dh1)
            # norm1 backward, fused with layer i-1's layer_scale2 backward unless a tap gradient joins dx in between
            ls_done = i >= 1 and i not in tap_of
            if ls_done:
                q = f"encoder.model.layer.{i - 1}."
                run.claim("du")
                L("s3od_layernorm_ls_bwd", dt, dh1, s["x"], s["mean1"], s["rstd1"], P[p + "norm1.weight"], dxm, dxi,
                  G[p + "norm1.weight"], G[p + "norm1.bias"], red_ws, ctx.t[f"L{i - 1}"]["u2"], P[q + "layer_scale2.lambda1"],
                  du, G[q + "layer_scale2.lambda1"], G[q + "mlp.down_proj.bias"], red2_ws, M, D, st)
            else:
                L("s3od_layernorm_bwd", dt, dh1, s["x"], s["mean1"], s["rstd1"], P[p + "norm1.weight"], dxm, dxi,
                  G[p + "norm1.weight"], G[p + "norm1.bias"], red_ws, M, D, st)
            dx, dxi = dxi, dx
            if self.grad_hook is not None:     # the layer's gradients are final once both streams are past it
                run.hook(partial(self.grad_hook, f"layer{i}"))
        # ---- embeddings
        e = "encoder.embeddings."
        L("s3od_token_prefix_bwd", dx, G[e + "cls_token"], G[e + "register_tokens"], B, Nt, D, st)
        dpatch = _E((B, NP, D), T, dev)
        L("s3od_cast_tap", dt, dx, dpatch, B, Nt, NP, D, st)
        self._colsum(dpatch, B * NP, D, G[e + "patch_embeddings.bias"])
        self._wgrad_lin(dpatch, ctx.t["cols"], D, 768, B * NP, G[e + "patch_embeddings.weight"])
        run.join()                                     # every weight gradient is final on the main stream
        lib().phase = None
        if self.grad_hook is not None:
            self.grad_hook("embeddings")

    grad_hook = None

    def _side_stream(self, dev):
        st = getattr(self, "_side", None)
        if st is None or st.device != dev:
            st = self._side = torch.cuda.Stream(device=dev)
        return st

    def backward(self, ctx: Ctx, d_logits, d_iou, G, d_feat=None):
        """Accumulate parameter gradients into G (name -> fp32 tensor, reference layout; plus the
        fused views 'qkv_w{i}', 'heads1_w', 'heads1_b', 'heads2_w', 'heads2_b').  d_feat: optional
        gradient of the returned ``features`` (NCHW), added to path_1's."""
        try:
            dtaps = self.decoder_backward(ctx, d_logits, d_iou, G, d_feat=d_feat)
            self.encoder_backward(ctx, dtaps, G)
        except BaseException:
            # side-stream weight gradients may still read ctx activations / workspaces and add into G: the main
            # stream waits for them before anything is freed (ctx, zero workspaces) or re-used by a retry
            side = getattr(self, "_side", None)
            if side is not None:
                torch.cuda.current_stream(side.device).wait_stream(side)
            self._invalidate()
            raise
