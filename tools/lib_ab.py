"""Library A/B on the GPU box (dev tool): two or more builds of libs3od_hip.so loaded side by side in ONE process
(separate ctypes handles), their entry points called alternately on the same inputs, HIP-event medians per build and
the relative difference of every output against the first build.

    python tools/lib_ab.py attn old_lib/libs3od_hip.so s3od_amd/libs3od_hip.so

A path may carry knobs, "path@S3OD_GEMM_CFG=6,S3OD_X=1": they are set in the environment around every call into that
build (S3OD_AB=1, set here, makes the library read them per call), so one build can be A/B'd against itself.

Workloads: attn (s3od_attn_fwd + s3od_attn_bwd_qkv at the training shape bs 16 N 4101 and the C5 shape bs 4 N 16389);
lin (the ViT linears of the bs-16 1024^2 step with their real epilogues, the 256-channel 3x3 conv; tools/lin_sweep.py shapes);
glue (every entry point of decoder_ops.hip / vit_ops.hip / loss.hip that reduces, folds, resizes or repacks, at edge
shapes and at the training step's shapes: give the first build twice, `glue parent parent new`, and each output of the
third is judged by whether the first two agree bit for bit -- then it must too -- or only to summation order, as the sums
through fp32 atomics do -- then rel-L2 1e-5, or the first two's own scatter where that is larger; the training
shapes are also timed);
augment (the entries of data_ops.hip, `augment parent parent new` like glue: see augment());
metrics (s3od_eval_metrics and s3od_flip_scores, `metrics parent parent new`: see metrics()).
"""
import ctypes
import os
import sys
from pathlib import Path

os.environ.setdefault("S3OD_AB", "1")
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from s3od_amd import _lib  # noqa: E402
from s3od_amd._lib import BF16, NREP, stream  # noqa: E402
from tools.attn_ab import inputs  # noqa: E402


class Lib(_lib._Lib):
    def __init__(self, spec):
        path, _, knobs = spec.partition("@")
        self.env = dict(kv.split("=", 1) for kv in knobs.split(",") if kv)
        self.lib = ctypes.CDLL(str(Path(path).resolve()))
        self.decls = _lib.parse_header()
        self.fns, self.timers, self.phase, self.cost = {}, {}, None, None
        for name, (ret, types) in self.decls.items():
            fn = getattr(self.lib, name)
            fn.argtypes = [_lib._CT[t] for t in types]
            fn.restype = ctypes.c_char_p if ret.startswith("const char") else ctypes.c_int
            self.fns[name] = (fn, types)

    def __call__(self, *a):
        old = {k: os.environ.get(k) for k in self.env}
        os.environ.update(self.env)
        try:
            return super().__call__(*a)
        finally:
            for k, v in old.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v


def timed(fn, n=3):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def attn(libs, B, N, rounds, H=12):
    q, k, v, do, cs, sn, P = inputs(B, N, H)
    st = stream()
    res = []
    for L in libs:
        o = torch.empty(B, N, H * 64, device="cuda", dtype=torch.bfloat16)
        lse = torch.empty(B * H, N, device="cuda")
        delta = torch.empty(B * H, N, device="cuda")
        dqkv = torch.empty(B * N, 3 * H * 64, device="cuda", dtype=torch.bfloat16)
        dbq, dbv = torch.zeros(H * 64, device="cuda"), torch.zeros(H * 64, device="cuda")
        ws = torch.zeros(NREP * 2 * H * 64, device="cuda")
        fwd = (lambda L=L, o=o, lse=lse: L("s3od_attn_fwd", BF16, q, k, v, o, lse, B, H, N, st))
        bwd = (lambda L=L, o=o, lse=lse, delta=delta, dqkv=dqkv, dbq=dbq, dbv=dbv, ws=ws:
               L("s3od_attn_bwd_qkv", BF16, q, k, v, o, do, lse, delta, cs, sn, P, dqkv, dbq, dbv, ws, B, H, N, st))
        fwd(); bwd(); torch.cuda.synchronize()
        outs = [t.clone() for t in (o, lse, dqkv, dbq, dbv)]
        res.append({"fwd": fwd, "bwd": bwd, "outs": outs, "t": {"fwd": [], "bwd": []}})
    for _ in range(rounds):
        for r in res:
            for nm in ("fwd", "bwd"):
                r["t"][nm].append(timed(r[nm]))
    fl = 4.0 * B * H * N * N * 64
    for i, r in enumerate(res):
        tf, tb = sorted(r["t"]["fwd"]), sorted(r["t"]["bwd"])
        print(f"B{B} N{N} lib{i}: fwd med {tf[len(tf) // 2] * 1e3:8.1f} us min {tf[0] * 1e3:8.1f} ({fl / tf[0] / 1e9:6.1f} TF/s) | "
              f"bwd med {tb[len(tb) // 2] * 1e3:8.1f} us min {tb[0] * 1e3:8.1f} ({2 * fl / tb[0] / 1e9:6.1f} TF/s alg)", flush=True)
        if i:
            errs = [f"{nm} {float((a.float() - b.float()).norm() / b.float().norm()):.2e}"
                    for nm, a, b in zip(("o", "lse", "dqkv", "dbq", "dbv"), r["outs"], res[0]["outs"])]
            print(f"   vs lib0: " + "  ".join(errs), "| finite", bool(torch.isfinite(r["outs"][2].float()).all()), flush=True)


def lin(libs, rounds):
    """Each case: a factory taking a library and returning (call, output tensor) on shared inputs."""
    M, D, F = 65616, 768, 3072
    g = torch.Generator(device="cuda").manual_seed(0)
    r = lambda *s, dt=torch.bfloat16: torch.randn(*s, device="cuda", generator=g).to(dt)
    st = stream()
    x768, x3072 = r(M, D), r(M, F)
    wq, bq = r(3 * D, D), r(3 * D, dt=torch.float32)
    wo, bo, so = r(D, D), r(D, dt=torch.float32), r(D, dt=torch.float32)
    wu, bu = r(F, D), r(F, dt=torch.float32)
    wd, bd, sd = r(D, F), r(D, dt=torch.float32), r(D, dt=torch.float32)
    res = r(M, D, dt=torch.float32)
    B, Nt, P = 16, 4101, 4096
    cs, sn = r(P, 64, dt=torch.float32), r(P, 64, dt=torch.float32)
    dy768, dy3072 = r(M, D), r(M, F)
    xc, wc, bc = r(16, 256, 256, 256), r(256, 3, 3, 256), r(256, dt=torch.float32)

    def c_qkv(L):
        q, k, v = (torch.empty(B * 12, Nt, 64, device="cuda", dtype=torch.bfloat16) for _ in range(3))
        return (lambda: L("s3od_qkv_rope_fwd", BF16, B, Nt, P, 12, x768, wq, bq, cs, sn, q, k, v, st)), q

    def c_fwd(w, b, N, K, x, act=0, resf=False, scale=None, pre=True):
        def mk(L):
            out = torch.empty(M, N, device="cuda", dtype=torch.float32 if resf else torch.bfloat16)
            pr = torch.empty(M, N, device="cuda", dtype=torch.bfloat16) if pre else None
            return (lambda: L("s3od_linear_fwd", BF16, M, N, K, x, K, w, b, scale, None, act, res if resf else None, N, None, 0,
                              int(resf), out, N, int(resf), pr, N, 0, 0, 0, st)), out
        return mk

    def c_dgrad(w, N, K, dy, act=0, aux=None):
        def mk(L):
            out = torch.empty(M, N, device="cuda", dtype=torch.bfloat16)
            return (lambda: L("s3od_linear_dgrad", BF16, M, N, K, dy, K, w, act, aux, N, out, N, 0, 0, 0, 0, None, st)), out
        return mk

    def c_wgrad(Nout, Kin, dy, x):
        """with the caller-owned split-K slab the engine passes (s3od_linear_wgrad_ws): slab partials + reduce"""
        def mk(L):
            dw = torch.zeros(Nout, Kin, device="cuda")
            nb = ctypes.c_long(0)
            L("s3od_linear_wgrad_ws", BF16, Nout, Kin, M, 0, ctypes.addressof(nb))
            slab = torch.empty(max(nb.value, 4) // 4, device="cuda")
            return (lambda: (dw.zero_(), L("s3od_linear_wgrad", BF16, Nout, Kin, M, dy, Nout, x, Kin, dw, 0, slab, nb.value,
                                           st))), dw
        return mk

    def c_conv(L):
        out = torch.empty(16, 256, 256, 256, device="cuda", dtype=torch.bfloat16)
        return (lambda: L("s3od_conv_fwd", BF16, 16, 256, 256, 256, 256, 256, 256, 3, 3, 1, 1, xc, 0, wc, bc, None, None, 0,
                          None, None, out, None, None, None, st)), out

    cases = [("qkv_rope fwd N2304 K768", 2.0 * M * 3 * D * D, c_qkv),
             ("o_proj fwd N768 K768 res f32", 2.0 * M * D * D, c_fwd(wo, bo, D, D, x768, resf=True, scale=so)),
             ("up fwd N3072 K768 GELU+gelu'", 2.0 * M * F * D, c_fwd(wu, bu, F, D, x768, act=5)),
             ("down fwd N768 K3072 res f32", 2.0 * M * D * F, c_fwd(wd, bd, D, F, x3072, resf=True, scale=sd)),
             ("up dgrad N768 K3072", 2.0 * M * D * F, c_dgrad(wu, D, F, dy3072)),
             ("qkv dgrad N768 K2304", 2.0 * M * D * 3 * D, c_dgrad(wq, D, 3 * D, r(M, 3 * D))),
             ("down dgrad N3072 K768 x gelu'", 2.0 * M * D * F, c_dgrad(wd, F, D, dy768, act=6, aux=r(M, F))),
             ("o_proj dgrad N768 K768", 2.0 * M * D * D, c_dgrad(wo, D, D, dy768)),
             ("DPT proj fwd N1024 K768 bias", 2.0 * M * 1024 * D, c_fwd(r(1024, D), r(1024, dt=torch.float32), 1024, D, x768, pre=False)),
             ("DPT proj fwd N512 K768 bias", 2.0 * M * 512 * D, c_fwd(r(512, D), r(512, dt=torch.float32), 512, D, x768, pre=False)),
             ("DPT proj fwd N256 K768 bias", 2.0 * M * 256 * D, c_fwd(r(256, D), r(256, dt=torch.float32), 256, D, x768, pre=False)),
             ("wgrad 3072x768", 2.0 * M * F * D, c_wgrad(F, D, dy3072, x768)),
             ("wgrad 768x3072", 2.0 * M * D * F, c_wgrad(D, F, dy768, x3072)),
             ("conv fwd 256->256 3x3 @256^2 bs16", 2.0 * 16 * 256 * 256 * 256 * 256 * 9, c_conv)]
    for name, fl, mk in cases:
        runs = [mk(L) for L in libs]
        ts = [[] for _ in libs]
        for _ in range(rounds):
            for i, (f, _) in enumerate(runs):
                ts[i].append(timed(f))
        line = f"{name:36s}"
        for i, t in enumerate(ts):
            t = sorted(t)
            line += f" | lib{i} {t[len(t) // 2] * 1e3:8.1f} us ({fl / t[len(t) // 2] / 1e9:6.1f} TF/s)"
        o0 = runs[0][1].float()
        errs = [float((rr[1].float() - o0).norm() / o0.norm()) for rr in runs[1:]]
        print(line, "| rel vs lib0", " ".join(f"{e:.1e}" for e in errs), flush=True)


def glue(libs, rounds):
    """Each case: name, timed?, factory taking a library -> (call, {output name: tensor}) on shared seeded inputs."""
    F32 = 0
    g = torch.Generator(device="cuda").manual_seed(0)
    rn = lambda *s, dt=torch.float32: torch.randn(*s, device="cuda", generator=g).to(dt)
    z = lambda *s, dt=torch.float32: torch.zeros(*s, device="cuda", dtype=dt)
    e = lambda *s, dt=torch.float32: torch.empty(*s, device="cuda", dtype=dt)
    st = stream()
    tdt = lambda code: torch.bfloat16 if code == BF16 else torch.float32
    cases = []

    def bn(code, C, npix, relu, dcb, timed=False):
        dy, zz, y = rn(npix, C, dt=tdt(code)), rn(npix, C, dt=tdt(code)), rn(npix, C, dt=tdt(code))
        mean, rstd, w = rn(C) * 0.1, torch.rand(C, device="cuda", generator=g) + 0.5, rn(C)
        sc, sh = (w * rstd).contiguous(), rn(C) * 0.3

        def mk(L):
            o = {"dz": e(npix, C, dt=tdt(code)), "dw": z(C), "db": z(C), "sums": z(NREP * 3 * C, dt=torch.float64)}
            if dcb:
                o["dcb"] = z(C)
            if relu:
                f = lambda: L("s3od_bn_relu_bwd", code, dy, zz, sc, sh, mean, rstd, w, o["sums"], o["dz"], o["dw"], o["db"],
                              o.get("dcb"), npix, C, st)
            else:
                f = lambda: L("s3od_bn_bwd", code, dy, zz, y, mean, rstd, w, o["sums"], o["dz"], o["dw"], o["db"], o.get("dcb"),
                              npix, C, st)
            return f, o
        cases.append((f"bn_{'relu_' if relu else ''}bwd dt{code} C{C} npix{npix} dcb{int(dcb)}", timed, mk))

    def bn_fin(C, count):
        stats0 = rn(NREP * 2 * C).double().abs() * count
        w, b = rn(C), rn(C)

        def mk(L):
            o = {"stats": stats0.clone(), "rm": z(C), "rv": z(C) + 1, "mean": e(C), "rstd": e(C), "scale": e(C), "shift": e(C)}
            def f():
                o["stats"].copy_(stats0)
                L("s3od_bn_finalize", o["stats"], count, w, b, o["rm"], o["rv"], 0.1, 1e-5, o["mean"], o["rstd"], o["scale"],
                  o["shift"], C, st)
            return f, o
        cases.append((f"bn_finalize C{C}", C == 256, mk))

    def ln(code, M, D, dres, timed=False):
        x, w, b = rn(M, D), rn(D), rn(D)
        mean, rstd = x.mean(1), torch.rsqrt(x.var(1, unbiased=False) + 1e-5)
        dy, u, lam = rn(M, D, dt=tdt(code)), rn(M, D, dt=tdt(code)), torch.rand(D, device="cuda", generator=g) + 0.1
        dr = rn(M, D) if dres else None

        def fwd(L):
            o = {"y": e(M, D, dt=tdt(code)), "mean": e(M), "rstd": e(M)}
            return (lambda: L("s3od_layernorm_fwd", code, x, w, b, o["y"], o["mean"], o["rstd"], M, D, 1e-5, st)), o

        def fused(L):
            o = {"dx": e(M, D), "du": e(M, D, dt=tdt(code)), "dw": z(D), "db": z(D), "dlam": z(D), "dbias": z(D),
                 "ws": z(NREP * 2 * D), "ws2": z(NREP * 2 * D)}
            return (lambda: L("s3od_layernorm_ls_bwd", code, dy, x, mean, rstd, w, dr, o["dx"], o["dw"], o["db"], o["ws"], u, lam,
                              o["du"], o["dlam"], o["dbias"], o["ws2"], M, D, st)), o

        def pair(L):
            o = {"dx": e(M, D), "du": e(M, D, dt=tdt(code)), "dw": z(D), "db": z(D), "dlam": z(D), "dbias": z(D),
                 "ws": z(NREP * 2 * D), "ws2": z(NREP * 2 * D)}
            def f():
                L("s3od_layernorm_bwd", code, dy, x, mean, rstd, w, dr, o["dx"], o["dw"], o["db"], o["ws"], M, D, st)
                L("s3od_layerscale_bwd", code, o["dx"], u, lam, o["du"], o["dlam"], o["dbias"], o["ws2"], M, D, st)
            return f, o
        tag = f"dt{code} M{M} D{D} dres{int(dres)}"
        cases.extend([(f"layernorm_fwd {tag}", timed, fwd), (f"layernorm_ls_bwd {tag}", timed, fused),
                      (f"layernorm_bwd + layerscale_bwd {tag}", timed, pair)])

    def colsum(M, N, two_pass, timed=False):
        a, base = rn(M, N, dt=torch.bfloat16), rn(N)
        nb = ctypes.c_long(0)
        libs[0]("s3od_colsum_ws", M, N, ctypes.addressof(nb))

        def mk(L):
            o = {"out": base.clone()}
            ws = e(nb.value // 4) if two_pass else None
            return (lambda: L("s3od_colsum", BF16, a, N, M, N, o["out"], ws, nb.value if two_pass else 0, st)), o
        cases.append((f"colsum {'two' if two_pass else 'one'}-pass M{M} N{N}", timed, mk))

    def unrope(code, B, N, P, H, timed=False):
        dq, dk, dv = (rn(B * H, N, 64, dt=tdt(code)) for _ in range(3))
        cs, sn = rn(max(P, 1), 64), rn(max(P, 1), 64)

        def mk(L):
            o = {"dqkv": e(B * N, 3 * H * 64, dt=tdt(code)), "dbq": z(H * 64), "dbv": z(H * 64), "ws": z(NREP * 2 * H * 64)}
            return (lambda: L("s3od_qkv_unrope", code, dq, dk, dv, cs, sn, o["dqkv"], o["dbq"], o["dbv"], o["ws"], B, N, P, H, st)), o
        cases.append((f"qkv_unrope dt{code} B{B} N{N} P{P} H{H}", timed, mk))

    def bilinear(code, B, IH, IW, OH, OW, C, timed=False):
        x, dy, bc = rn(B, IH, IW, C, dt=tdt(code)), rn(B, OH, OW, C, dt=tdt(code)), rn(B, C)

        def fwd(L):
            o = {"y": e(B, OH, OW, C, dt=tdt(code))}
            return (lambda: L("s3od_bilinear_fwd", code, x, o["y"], B, IH, IW, OH, OW, C, st)), o

        def bwd(L):
            o = {"dx": e(B, IH, IW, C, dt=tdt(code))}
            return (lambda: L("s3od_bilinear_bwd", code, dy, bc, o["dx"], B, IH, IW, OH, OW, C, st)), o
        tag = f"dt{code} B{B} {IH}x{IW}->{OH}x{OW} C{C}"
        cases.extend([(f"bilinear_fwd {tag}", timed, fwd), (f"bilinear_bwd {tag}", timed, bwd)])

    def avgpool(code, B, HW, C, timed=False):
        x = rn(B, HW, C, dt=tdt(code))

        def mk(L):
            o = {"out": e(B, C)}
            ws = e(B * cdiv(HW, 1024) * C)
            return (lambda: L("s3od_avgpool", code, x, o["out"], ws, B, HW, C, st)), o
        cases.append((f"avgpool dt{code} B{B} HW{HW} C{C}", timed, mk))

    def heads(code, B, HW, NM, timed=False):
        dl, h, w2 = rn(B, NM, HW), rn(B * HW, 32 * NM, dt=tdt(code)), rn(NM, 32)

        def mk(L):
            o = {"dh": e(B * HW, 32 * NM, dt=tdt(code)), "dw2": z(NM, 32), "db2": z(NM), "db1": z(32 * NM)}
            def f():
                for k in ("dw2", "db2", "db1"):
                    o[k].zero_()
                L("s3od_mask_heads_bwd", code, dl, h, w2, o["dh"], o["dw2"], o["db2"], o["db1"], B, HW, NM, st)
            return f, o
        cases.append((f"mask_heads_bwd dt{code} B{B} HW{HW} NM{NM}", timed, mk))

    def ssim(B, M, H, W, timed=False):
        lg, tg, pi = rn(B, M, H, W), (rn(B, H, W) > 0).float(), rn(B, M)

        def mk(L):
            o = {"out": z(16 + B * M + B), "dlogits": e(B, M, H, W), "d_iou": e(B, M)}
            sums, coef, iws, diu = z(B * M * 8, dt=torch.float64), e(B * M * 4), e(B * M * 2), e(B * M)
            def f():
                L("s3od_mask_loss_fwd", lg, tg, pi, B, M, H * W, W, 1.0, 1.0, 0.0, 1.0, 1.0, 0.05, 0.25, 2.0, sums, coef, iws, diu,
                  o["out"], st)
                L("s3od_mask_loss_bwd", lg, tg, coef, iws, diu, None, o["dlogits"], o["d_iou"], B, M, H * W, W, 1, 0.25, 2.0, st)
            return f, o
        cases.append((f"mask_loss fwd+bwd with SSIM B{B} M{M} {H}x{W}", timed, mk))

    def repack(timed=False):
        """the layouts of tests/test_gpu_repack.py plus the linears of one ViT layer"""
        ents = [(rn(3072, 768), 0, 3072, 768, 1, 0, 0), (rn(768, 3072), 0, 768, 3072, 1, 0, 0), (rn(2304, 768), 0, 2304, 768, 1, 0, 0),
                (rn(256, 128, 3, 3), 0, 256, 128, 9, 0, 0), (rn(64, 96, 3, 3), 32, 64, 96, 9, 1, 128),
                (rn(128, 64, 4, 4), 0, 128, 64, 16, 2, 128), (rn(1 + 768 * 40)[1:], 1, 40, 768, 1, 0, 0)]
        chunk = 16384

        def mk(L):
            o, rows, ct, co = {}, [], [], []
            for t, (src, off, O, I, KHW, mode, ld) in enumerate(ents):
                n = (I * KHW * ld if mode else O * I * KHW) + off
                o[f"w{t}"] = z(n, dt=torch.bfloat16)
                rows.append([src.data_ptr(), o[f"w{t}"].data_ptr(), O, I, KHW, off, mode, ld])
                for c0 in range(0, O * I * KHW, chunk):
                    ct.append(t); co.append(c0)
            tab = torch.tensor(rows, dtype=torch.int64, device="cuda")
            ctt, cot = torch.tensor(ct, dtype=torch.int32, device="cuda"), torch.tensor(co, dtype=torch.int64, device="cuda")
            o["_keep"] = tab                     # (the tables must outlive the launches)
            return (lambda: L("s3od_repack_multi", BF16, tab, ctt, cot, len(ct), chunk, st)), o
        cases.append(("repack_multi", timed, mk))

    cdiv = lambda a, b: (a + b - 1) // b
    # ---- the edge shapes of tests/test_gpu_bn_relu.py, test_gpu_vit_ops.py, test_gpu_colsum.py
    for code in (F32, BF16):
        for C in (8, 64, 256, 2048):
            rows = 256 // (C // 8)
            for npix in dict.fromkeys((1, rows - 1, 4 * rows + 1, 3017)):
                if npix > 0:
                    bn(code, C, npix, relu=npix % 2 == 1, dcb=C != 64)
        for M in (1, 3, 5, 33, 65, 8202):
            for D in (768, 1024):
                ln(code, M, D, dres=M != 33)
        unrope(code, 2, 69, 64, 12); unrope(code, 2, 69, 64, 16); unrope(code, 2, 5, 0, 12)
        bilinear(code, 2, 12, 9, 25, 20, 16); bilinear(code, 2, 7, 5, 14, 10, 8)
        avgpool(code, 2, 1500, 256); avgpool(code, 8, 37, 64)
        heads(code, 2, 1000, 3); heads(code, 1, 33, 1)
    for C in (8, 256, 2048):
        bn_fin(C, 3017)
    for M, N in ((37, 64), (1000, 256), (1000, 8), (600000, 8), (4099, 4096)):
        colsum(M, N, True); colsum(M, N, False)
    ssim(2, 3, 45, 70); ssim(1, 1, 32, 32)
    # ---- the training step's shapes (bs 16, 1024^2; tools/hbm_bench.py, colsum_bench.py, ln_bench.py), timed
    bn(BF16, 256, 16 * 256 * 256, relu=True, dcb=True, timed=True)
    bn(BF16, 256, 16 * 256 * 256, relu=False, dcb=True, timed=True)
    ln(BF16, 16 * 4101, 768, dres=True, timed=True)
    colsum(16 * 256 * 256, 256, True, timed=True); colsum(16 * 256 * 256, 256, False, timed=True)
    unrope(BF16, 16, 4101, 4096, 12, timed=True)
    bilinear(BF16, 16, 128, 128, 256, 256, 256, timed=True)
    bilinear(BF16, 16, 512, 512, 1024, 1024, 32, timed=True)
    avgpool(BF16, 16, 256 * 256, 256, timed=True)
    heads(BF16, 16, 1024 * 1024, 3, timed=True)
    ssim(16, 3, 1024, 1024, timed=True)
    repack(timed=True)

    # sums that go through fp32 atomics (these outputs outside the BatchNorm entries, whose fp64 replicas are exact
    # sums of the block partials; one-pass colsum; the loss sums and what is computed from them): their order is not fixed, so
    # one agreeing pair of runs does not make them repeat (few blocks often agree); they are held to the tolerance
    # whatever the first two builds show
    ATOMIC = {"dw", "db", "dlam", "dbias", "dbq", "dbv", "dw2", "db2", "db1"}
    bad = 0
    cmp = lambda a, b: "equal" if torch.equal(a, b) else f"{float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-300)):.2e}"
    for name, is_timed, mk in cases:
        runs = [mk(L) for L in libs]
        for f, _ in runs:
            f()
        torch.cuda.synchronize()
        line = f"{name}:"
        for k in runs[0][1]:
            if k.startswith("_"):
                continue
            ref = runs[0][1][k]
            res = [cmp(r[1][k], ref) for r in runs[1:]]
            line += f" {k} " + " / ".join(res)
            if len(res) == 2:                       # parent, parent, new
                pp, pn = res
                fixed = pp == "equal" and not (k in ATOMIC and not name.startswith("bn_") or "one-pass" in name or name.startswith("mask_loss"))
                ok = pn == "equal" if fixed else (pn == "equal" or float(pn) <= max(1e-5, 0.0 if pp == "equal" else float(pp)))
                if not ok or (pp != "equal" and float(pp) > 1e-5):
                    line += " <-- " + ("MISS" if not ok else "parent scatter > 1e-5")
                bad += not ok
        print(line, flush=True)
        if is_timed:
            ts = [[] for _ in libs]
            for _ in range(rounds):
                for i, (f, _) in enumerate(runs):
                    ts[i].append(timed(f, 5))
            print("    timed: " + " | ".join(f"lib{i} med {sorted(t)[len(t) // 2] * 1e3:8.1f} us min {min(t) * 1e3:8.1f} max {max(t) * 1e3:8.1f}"
                                             for i, t in enumerate(ts)), flush=True)
        del runs
    print(f"glue: {len(cases)} cases, {bad} outputs MISS the rule (equal where the first two builds agree bit for bit, "
          f"rel-L2 <= max(1e-5, their scatter) elsewhere)")
    attn(libs, 2, 261, 1)
    return bad


def augment(libs, rounds):
    """The training-augmentation entries of data_ops.hip on shared seeded inputs: s3od_augment_sample (one pass with jitter and
    noise; raw with grid + elastic + perspective + radial distortion), s3od_elastic_field, and s3od_augment_synthetic once per
    member and once with everything on, for order 0 and order 1.  Compared at S = 96 and 264, timed at the training canvas
    S = 1024.  Give the first build twice (`augment parent parent new`): an output of the third must equal the first's bit for
    bit where the first two agree bit for bit, and be within their rel-L2 scatter where they differ (ISONoise's float64
    sums go through atomics); its median time must not lie above the spread (min .. max over the rounds) of the first two."""
    import math
    import numpy as np
    from s3od_amd.data import (AugParams, SynthParams, _conv_full, _disk_kernel, _gauss_kernel, _sharpen_kernel,
                               elastic_params, grid_distortion_maps)
    st = stream()
    cmp = lambda a, b: "equal" if torch.equal(a, b) else f"{float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-300)):.2e}"
    bad = slow = 0

    def members(S):
        """-> [(name, {SynthParams field: value}, filter kernel or None)] for both orders"""
        r = np.random.RandomState(5)
        blur = _conv_full(_gauss_kernel(5), _sharpen_kernel(0.4, 0.8))                       # 7x7
        big = _conv_full(_disk_kernel(6, 0.2), _sharpen_kernel(0.3, 1.0))                    # 15x15
        shadow = [[float(v) for xy in zip(r.randint(0, S, 5), r.randint(S // 10, S, 5)) for v in xy] for _ in range(3)]
        slant = -6
        drops = np.stack([r.randint(-slant, S, S * S // 600), r.randint(0, S - 20, S * S // 600)], 1).astype(np.int32)
        one = {"jitter": dict(bright=0.8, contrast=1.3, sat=1.2, hue=0.07, gray_mean=0.4), "hsv": dict(hsv_h=30.0, hsv_s=0.1, hsv_v=-0.08),
               "clahe": dict(clahe_clip=3.0), "iso": dict(iso_intensity=0.25, iso_color_shift=0.02), "gauss": dict(gauss_std=0.4),
               "mult": dict(mult=[0.92, 1.05, 1.08]), "jpeg": dict(jpeg_quality=45), "down": dict(down=0.55),
               "shadow": dict(n_shadow=3, shadow=shadow, shadow_dim=0.5), "rbc": dict(rbc_alpha=1.2, rbc_beta=-0.1),
               "filter7": dict(ksize=7), "filter15": dict(ksize=15), "zoom": dict(zoom_n=3, zoom=[1.0, 1.01, 1.02]),
               "sepia": dict(color_op=1), "gray": dict(color_op=2), "shuffle": dict(color_op=3, perm=[2, 0, 1]),
               "posterize": dict(post_bits=5), "snow": dict(snow_point=0.2, snow_coeff=2.5),
               "rain": dict(rain_n=len(drops), rain_slant=slant, rain_len=20, rain_blur=7, rain_color=200 / 255, rain_bright=0.7)}
        everything = {k: v for n, m in one.items() if n not in ("filter15", "gray", "shuffle") for k, v in m.items()}
        reg = {"sharpen": dict(ksize=3), "jitter": one["jitter"], "iso": one["iso"], "gauss": one["gauss"], "mult": one["mult"]}
        reg["everything"] = {k: v for m in reg.values() for k, v in m.items()}
        kern = lambda m: {3: _sharpen_kernel(0.4, 0.8), 7: blur, 15: big}.get(m.get("ksize"))
        out = [(f"order 0 {n}", dict(m, seed=1234 + i), kern(m)) for i, (n, m) in enumerate({**one, "everything": everything}.items())]
        out += [(f"order 1 {n}", dict(m, order=1, seed=4321 + i), kern(m)) for i, (n, m) in enumerate(reg.items())]
        return out, drops

    def params(S, fields, drops_dev, ws):
        q = SynthParams.identity()
        for k, v in fields.items():
            if k == "shadow":
                for t, poly in enumerate(v):
                    for i, c in enumerate(poly):
                        q.shadow[t][i] = c
            elif isinstance(v, list):
                for i, c in enumerate(v):
                    getattr(q, k)[i] = c
            else:
                setattr(q, k, v)
        q.rain_drops, q.ws = drops_dev.data_ptr() if q.rain_n else None, ws.data_ptr()
        return q

    for S, is_timed in ((96, False), (264, False), (1024, True)):
        g = torch.Generator(device="cuda").manual_seed(S)
        h0, w0 = 3 * S // 4, S
        img = torch.randint(0, 256, (h0, w0, 3), device="cuda", generator=g, dtype=torch.uint8)
        msk = (torch.rand(h0, w0, device="cuda", generator=g) > 0.5).to(torch.uint8) * 255
        raw0 = torch.nn.functional.interpolate(torch.rand(1, 3, S // 4, S // 4, device="cuda", generator=g), size=(S, S), mode="bilinear")[0].contiguous()
        th, c = math.radians(9.0), S / 2
        T = lambda tx, ty: np.array([[1, 0, tx], [0, 1, ty], [0, 0, 1]], np.float64)
        R = np.array([[math.cos(th), math.sin(th), 0], [-math.sin(th), math.cos(th), 0], [0, 0, 1]])
        fwd = np.diag([96 / 83, 96 / 91, 1.0]) @ T(-5.0 * S / 96, -2.0 * S / 96) @ T(c, c) @ R @ T(-c, -c)

        def geometry(persp):
            p = AugParams.identity(h0, w0, S)
            Tot = np.linalg.inv(fwd) @ np.array([[1, 0, 0], [0, 1, 0], [persp[0], persp[1], 1.0]])
            Tot /= Tot[2, 2]
            for i, v in enumerate(list(Tot[0]) + list(Tot[1])):
                p.A[i] = float(v)
            p.persp[0], p.persp[1] = float(Tot[2, 0]), float(Tot[2, 1])
            return p
        one_pass = geometry((0.0, 0.0))
        one_pass.bright, one_pass.contrast, one_pass.sat, one_pass.hue, one_pass.gray_mean = 0.8, 1.3, 1.2, 0.07, 0.3
        one_pass.mult[0], one_pass.mult[1], one_pass.mult[2], one_pass.gauss_std, one_pass.seed = 0.92, 1.05, 1.08, 0.3, 99
        rs = np.random.RandomState(11)
        grid = torch.from_numpy(np.concatenate(grid_distortion_maps(S, 1 + rs.uniform(-0.3, 0.3, 7), 1 + rs.uniform(-0.3, 0.3, 7), 6))
                                .astype(np.float32)).cuda()
        ep = elastic_params(777, alpha=3.0)
        field, tmp0 = torch.empty(2, S, S, device="cuda"), torch.empty(2, S, S, device="cuda")
        libs[0]("s3od_elastic_field", ctypes.addressof(ep), S, tmp0, field, st)                  # shared input of the raw pass
        distorted = geometry((0.3 / S, -0.2 / S))
        distorted.kdist, distorted.raw, distorted.grid, distorted.elastic = 0.05, 1, grid.data_ptr(), field.data_ptr()
        chain, drops = members(S)
        drops_dev = torch.from_numpy(drops).cuda()
        nws = ctypes.c_long(0)
        libs[0]("s3od_augment_ws_floats", S, ctypes.addressof(nws))
        cases = []

        # every build of a case runs on the SAME buffers (outputs are cloned after its run): with buffers of their own, two
        # handles of one library measured up to 1.5 % apart on the 20 .. 100 us entries
        def sample(p):
            o = {"img": torch.empty(3, S, S, device="cuda"), "mask": torch.empty(S, S, device="cuda")}
            return lambda L: ((lambda: L("s3od_augment_sample", img, msk, ctypes.addressof(p), S, o["img"], o["mask"], st)), o)

        def elastic():
            o, tmp = {"field": torch.empty(2, S, S, device="cuda")}, torch.empty(2, S, S, device="cuda")
            return lambda L: ((lambda: L("s3od_elastic_field", ctypes.addressof(ep), S, tmp, o["field"], st)), o)

        def synthetic(fields, ker):
            kw = torch.tensor(ker.reshape(-1), dtype=torch.float32, device="cuda") if ker is not None else None
            o, raw, ws = {"out": torch.empty(3, S, S, device="cuda")}, torch.empty_like(raw0), torch.zeros(nws.value, device="cuda")
            q = params(S, fields, drops_dev, ws)

            def mk(L):
                def f():
                    raw.copy_(raw0)                                                               # (the entry uses raw as scratch)
                    q.ws = ws.data_ptr()                                                          # (and keeps ws alive: q holds an address only)
                    L("s3od_augment_synthetic", raw, ctypes.addressof(q), kw, S, o["out"], st)
                return f, o
            return mk
        cases += [("augment_sample one pass", sample(one_pass)), ("augment_sample raw, distorted", sample(distorted)), ("elastic_field", elastic())]
        cases += [(f"augment_synthetic {n}", synthetic(m, k)) for n, m, k in chain]
        for name, mk in cases:
            runs, outs = [mk(L) for L in libs], []
            for f, o in runs:
                for t in o.values():
                    t.fill_(float("nan"))
                f()
                torch.cuda.synchronize()
                outs.append({k: t.clone() for k, t in o.items()})
            line = f"S{S} {name}:"
            for k in outs[0]:
                res = [cmp(o[k], outs[0][k]) for o in outs[1:]]
                line += f" {k} " + " / ".join(res)
                if len(res) == 2:                   # parent, parent, new
                    pp, pn = res
                    ok = pn == "equal" if pp == "equal" else (pn == "equal" or float(pn) <= float(pp))
                    line += "" if ok else " <-- MISS"
                    bad += not ok
            if is_timed:
                ts = [[] for _ in libs]
                for r in range(rounds):                                     # the later slots of a round measure ~1 % slower on
                    for i in [(r + j) % len(libs) for j in range(len(libs))]:     # 20 us entries: every build takes every slot
                        ts[i].append(timed(runs[i][0], 20) * 1e3)
                med = [sorted(t)[len(t) // 2] for t in ts]
                line += " | us " + " | ".join(f"lib{i} med {m:8.1f} ({min(t):8.1f} .. {max(t):8.1f})" for i, (m, t) in enumerate(zip(med, ts)))
                if len(libs) == 3:
                    lo, hi = min(ts[0] + ts[1]), max(ts[0] + ts[1])
                    verdict = "within" if lo <= med[2] <= hi else ("below" if med[2] < lo else "ABOVE")
                    line += f" | parents' spread {lo:.1f} .. {hi:.1f}: new median {verdict}"
                    slow += verdict == "ABOVE"
            print(line, flush=True)
            del runs
    print(f"augment: {bad} outputs MISS the rule (equal where the first two builds agree bit for bit, within their rel-L2 scatter "
          f"elsewhere); {slow} timed entries with the last build's median above the spread of the first two")
    return bad + slow


def metrics(libs, rounds):
    """The entries of metrics.hip, `metrics parent parent new`: s3od_eval_metrics (full with binarize 0 and 1 on a binary gt,
    sm_only with binarize 0 and 1 on a soft gt: out[6] and the gt plane it leaves) and s3od_flip_scores (out[9], soft gt) at
    3x85 and 16x16 (one block), 3x86 (two live threads in a second block), 65x63, 1024x1000 (a second trip of the
    grid-stride loop) and 1536x2048, 10 calls per build and entry on the same buffers.  Per output number: the sums of
    integers (MaxF with a binary gt, the six IoU counts) equal the first build's bit for bit; where all 20 numbers of the
    first two builds are one value the third's are that value; elsewhere (float64 atomics of many blocks) the third's
    largest distance from the first two's mean is at most 4x their spread (max - min: 10 calls undersample the orders of up
    to 2048 blocks' atomics) and inside the bound tests/test_gpu_metrics.py and test_gpu_flip_scores.py hold against the
    reference.  Timed at 1024x1000, 1536x2048 and 1024^2: full eval, three sm_only steps, one flip score; the third build's
    median must not lie above the first two's max + (max - min)."""
    import numpy as np
    from s3od_amd.metrics import _K7, _THR
    CALLS = 10
    TOL = [1e-9, 2e-7, 2e-6, 2e-6, 1e-9, 1e-9]               # tests/test_gpu_metrics.py, relative to max(1, |value|)
    KEYS = ("mae", "max_f", "avg_f", "s", "em", "wfm")
    FKEYS = ("s_ag", "s_bg", "s_ab", "i_ag", "u_ag", "i_bg", "u_bg", "i_ab", "u_ab")
    st = stream()
    bad = slow = 0

    def planes(H, W):
        g = torch.Generator(device="cuda").manual_seed(1000 * H + W)
        u = lambda: torch.rand(H, W, device="cuda", generator=g)
        gb = (u() < 0.4).float()
        a, b = (0.7 * gb + 0.3 * u()).clamp(0, 1), (0.6 * gb + 0.4 * u()).clamp(0, 1)
        return a, b, torch.flip(b, [1]).contiguous(), gb, 0.8 * gb + 0.1

    def workspace(H, W):
        nb = ctypes.c_long(0)
        libs[0]("s3od_eval_metrics_ws", H, W, ctypes.addressof(nb))
        return torch.empty(nb.value, dtype=torch.uint8, device="cuda")

    def judge(tag, keys, exact, tol, vals):
        """vals[build][call] = float64 outputs -> report lines; exact: indices that are sums of integers"""
        nonlocal bad
        bits = lambda x: np.asarray(x, np.float64).view(np.int64)
        for k, key in enumerate(keys):
            par = np.array([v[k] for b in vals[:2] for v in b])
            new = np.array([v[k] for v in vals[2]]) if len(vals) == 3 else par
            fixed = len(set(bits(par).tolist())) == 1
            if fixed or k in exact:
                ok = bool(np.all(bits(new) == bits(par)[0])) and (fixed or k not in exact)
                line = f"  {tag} {key}: parents {'one value' if fixed else 'DIFFER'} {float(par[0])!r}, new {'equal' if ok else f'DIFFERS by up to {float(np.abs(new - par[0]).max()):.3g}'}"
            else:
                spread, dev = float(par.max() - par.min()), float(np.abs(new - par.mean()).max())
                ok = dev <= 4 * spread and dev <= tol[k] * max(1.0, abs(par.mean()))
                line = f"  {tag} {key}: parents' spread {spread:.3g} about {float(par.mean())!r}, new deviates {dev:.3g} (bound {tol[k] * max(1.0, abs(par.mean())):.1g})"
            print(line + ("" if ok else " <-- MISS"), flush=True)
            bad += not ok

    def bench(tag, fns):
        nonlocal slow
        ts = [[] for _ in libs]
        for r in range(max(rounds, 5)):
            for i in [(r + j) % len(libs) for j in range(len(libs))]:
                ts[i].append(timed(fns[i], 20) * 1e3)
        med = [sorted(t)[len(t) // 2] for t in ts]
        line = f"  timed {tag}: us " + " | ".join(f"lib{i} med {m:8.1f} ({min(t):8.1f} .. {max(t):8.1f})" for i, (m, t) in enumerate(zip(med, ts)))
        if len(libs) == 3:
            lo, hi = min(ts[0] + ts[1]), max(ts[0] + ts[1])
            verdict = "below" if med[2] < lo else "within" if med[2] <= hi else "within the widened range" if med[2] <= hi + (hi - lo) else "ABOVE"
            line += f" | parents' range {lo:.1f} .. {hi:.1f}: new median {verdict}"
            slow += verdict == "ABOVE"
        print(line, flush=True)

    for H, W in ((3, 85), (16, 16), (3, 86), (65, 63), (1024, 1000), (1536, 2048), (1024, 1024)):
        a, b, bm, gbin, gsoft = planes(H, W)
        ws, out6, out9 = workspace(H, W), torch.empty(6, dtype=torch.float64, device="cuda"), torch.empty(9, dtype=torch.float64, device="cuda")
        fws = torch.empty(128, dtype=torch.float64, device="cuda")
        gt = torch.empty_like(gbin)
        ev = lambda L, p, g, sm, bz: L("s3od_eval_metrics", p, g, H, W, _THR.ctypes.data, _K7.ctypes.data, ws, ws.numel(), sm, bz, out6, st)
        fl = lambda L: L("s3od_flip_scores", a, bm, gsoft, H, W, 0.5, fws, fws.numel() * 8, out9, st)
        print(f"{H}x{W} ({-(-H * W // 256)} blocks of 256 pixels, at most 2048 run):", flush=True)
        if (H, W) != (1024, 1024):                                        # (1024^2 is timed only)
            for sm, g0, bz in ((0, gbin, 1), (0, gbin, 0), (1, gsoft, 1), (1, gsoft, 0)):
                vals, left = [[] for _ in libs], []
                for _ in range(CALLS):
                    for i, L in enumerate(libs):
                        gt.copy_(g0)
                        ev(L, a, gt, sm, bz)
                        vals[i].append(out6.cpu().numpy())
                        left.append(gt.clone())
                tag = f"eval {'sm_only' if sm else 'full'} binarize {bz}"
                judge(tag, KEYS, {1} if not sm else set(), TOL, vals)
                same = all(torch.equal(t, left[0]) for t in left)
                print(f"  {tag} gt plane left behind: {'equal in every call' if same else 'DIFFERS <-- MISS'}", flush=True)
                bad += not same
            vals = [[] for _ in libs]
            for _ in range(CALLS):
                for i, L in enumerate(libs):
                    fl(L)
                    vals[i].append(out9.cpu().numpy())
            judge("flip", FKEYS, set(range(3, 9)), [2e-6] * 9, vals)
        if H * W >= 1024 * 1000:
            gt.copy_(gbin)
            b3 = b.clone()                                               # step 3's mask: binarised in place by the first call
            bench("full eval, binary gt", [lambda L=L: ev(L, a, gt, 0, 1) for L in libs])
            bench("three sm_only steps", [lambda L=L: (ev(L, a, gt, 1, 1), ev(L, b, gt, 1, 1), ev(L, a, b3, 1, 1)) for L in libs])
            bench("one flip score", [lambda L=L: fl(L) for L in libs])
    print(f"metrics: {bad} outputs MISS the rule, {slow} timed entries with the last build's median above the first two's "
          f"range widened by its width")
    return bad + slow


if __name__ == "__main__":
    what, paths = sys.argv[1], sys.argv[2:]
    libs = [Lib(p) for p in paths]
    rounds = int(os.environ.get("AB_ROUNDS", 5))
    if what == "attn":
        attn(libs, 16, 4101, rounds)
        if not os.environ.get("AB_SMALL"):
            attn(libs, 4, 16389, rounds)
    elif what == "lin":
        lin(libs, rounds)
    elif what == "glue":
        sys.exit(1 if glue(libs, rounds) else 0)
    elif what == "augment":
        sys.exit(1 if augment(libs, rounds) else 0)
    elif what == "metrics":
        sys.exit(1 if metrics(libs, rounds) else 0)
