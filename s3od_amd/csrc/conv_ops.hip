// C-ABI conv entry points: forward, data and weight gradients and the fused mask heads, routed to the
// implicit-GEMM engine (gemm.hpp) or to the hand-pipelined kernels of gemm_ops.hip / wgrad_dma.hip.
#include "gemm_dispatch.hpp"
#include "conv_kernels.hpp"

// ------------------------------------------------------------------ fused mask heads
// per pixel: h = relu(conv3x3_64->32NM(feat) + b1) ; logit_k = h[32k:32k+32] . w2[k] + b2[k]
// (src/s3od/model.py:440-452,461-467; the NM Sequential heads run as one N=32NM GEMM)
template <typename T> struct EpiHeads {
  float* logits; T* hsave; const float* b1; const float* w2; const float* b2;
  int M, HW, NM;
  RowMap rm;                                                  // staged row -> pixel (mode 0 dense)
  DEV void prepare(int) {}
  DEV void operator()(const float* ct, int LDT, int m0, int n0, int tid, int BM, int BN, int NT) const {
    const int C = 32 * NM, SPR = 4 * NM;                      // channels / 8-channel segments per row
    // h = relu(acc + b1) is formed on the fly from the staged fp32 tile (no in-place pass)
    if (hsave) {
      const int segs = BM * SPR;
      for (int s = tid; s < segs; s += NT) {
        int r = s / SPR, c = (s - r * SPR) * 8, m = m0 + r;
        if (m >= M) continue;
        const long px = rm.map(m);
        if (px < 0) continue;
        const float4* src = (const float4*)(ct + r * LDT + c);
        float4 x0 = src[0], x1 = src[1];
        float v[8] = {x0.x, x0.y, x0.z, x0.w, x1.x, x1.y, x1.z, x1.w};
#pragma unroll
        for (int e = 0; e < 8; e++) v[e] = fmaxf(v[e] + b1[c + e], 0.f);
        store8<T>(hsave + px * C + c, v);
      }
    }
    // logit_k = b2[k] + sum_j relu(acc[32k + j] + b1[32k + j]) * w2[32k + j]; k is wave-uniform
    for (int s = tid; s < NM * BM; s += NT) {
      int k = s / BM, r = s - k * BM;
      int m = m0 + r;
      if (m >= M) continue;
      const long px = rm.map(m);
      if (px < 0) continue;
      const float4* row = (const float4*)(ct + r * LDT + 32 * k);
      const float* bb = b1 + 32 * k;
      const float* ww = w2 + 32 * k;
      float acc = b2[k];
#pragma unroll
      for (int q = 0; q < 8; q++) {
        float4 x = row[q];
        acc += fmaxf(x.x + bb[4 * q + 0], 0.f) * ww[4 * q + 0];
        acc += fmaxf(x.y + bb[4 * q + 1], 0.f) * ww[4 * q + 1];
        acc += fmaxf(x.z + bb[4 * q + 2], 0.f) * ww[4 * q + 2];
        acc += fmaxf(x.w + bb[4 * q + 3], 0.f) * ww[4 * q + 3];
      }
      const long b = px / HW, pix = px - b * HW;
      logits[(b * NM + k) * HW + pix] = acc;
    }
  }
};

// the 3x3 s1 p1 convs whose output channels fill 256-wide tiles and whose pixel tiles fill whole rounds of the
// chip run on the ping-pong kernel when there are >= 8 rounds of tiles or K >= 9 * 512 (measured, tools/conv_cfg_bench.py,
// bs 16: 256^2 RCU 1.38 vs 1.51-1.66 ms with BN sums, plain 1.21 vs 1.34-1.38 ms; 128^2 512 -> 256 0.56 vs 0.69-0.81 ms;
// the 128^2 256 -> 256 RCU 0.39 vs 0.37-0.38 ms with BN sums stays on 128x128 tiles), and from 2 rounds without BN
// statistics (eval: 4 rounds = the C5 256^2 bs-4 RCUs, C5 74.72 -> 74.47 ms, C2 24.99 -> 24.91 ms per batch; 2 rounds =
// the C2 128^2 bs-8 RCUs, C2 25.37 -> 25.25 ms; 1 round mixed; profiles/r04b_conv_pp_rounds_ab.txt).
// S3OD_CONV_PP=0 (under S3OD_AB=1: per call): the 128x128 implicit GEMM (A/B runs).
static bool conv_pp_ok(const ConvGeo& g, int M, int N, bool stats) {
  const int nch = g.SC / 64;
  const long tiles = (long)(M / 256) * (N / 256);
  const bool rounds = tiles >= 2048 || g.SC >= 512 || (tiles >= 512 && !stats);   // 512 tiles = 2 rounds: the eval threshold
  // 128-channel inputs (the output_conv1 data gradient, K = 9 x 128): the ping-pong kernel's per-tap A tiles are half
  // width there and the generic path measured faster in the whole step (150.1 -> 147.5 ms median, same box)
  if (g.SC < 256) return false;
  return gemm_cfg() < 0 && g.KH == 3 && g.KW == 3 && g.s == 1 && g.p == 1 && g.RH == g.SH && g.RW == g.SW &&
         g.SC % 64 == 0 && (nch & (nch - 1)) == 0 && N % 256 == 0 && pp_pays(M, N) && rounds && !S3OD_OFF("S3OD_CONV_PP");
}

// implicit-GEMM conv forward (im2col gathered per K tile by ConvFwdA); also the stride-1 3x3 data gradient run as a
// forward conv of dy with the transposed, tap-reversed weight (s3od_conv_dgrad with wT)
static int conv_fwd_igemm(int dtype, ConvGeo g, int M, int N, int K, int Cin, int Cout, const void* x, int relu_in,
                          const void* wp, const float* bias, const float* scale, const float* shift, int act,
                          const void* res1, const void* res2, void* out, void* pre, double* stats, float* colsum,
                          hipStream_t st) {
  DISPATCH_T(dtype, {
    const int KTILES = cdiv(K, KT<T>::BK);
    if constexpr (sizeof(T) == 2) {
      if (conv_pp_ok(g, M, N, stats != nullptr)) {
        // 3x3 s1 p1 with 256-multiple output channels: the 256x256 ping-pong kernel (one workgroup per CU covers
        // all 256 output channels of 256 pixels, so each im2col A tile is gathered once) with the Conv3A loader
        auto pp = [&](auto rl) -> int {
          Conv3A<128, decltype(rl)::value> la{};
          la.x = (const bf16*)x; la.B = g.B; la.H = g.SH; la.W = g.SW; la.SC = g.SC; la.M = M;
          la.lgc = __builtin_ctz((unsigned)(g.SC / 64));
          DenseKC<bf16, 128> lb{{}, (const bf16*)wp, (long)K, N, K};
          EpiStd<bf16, bf16> e{(bf16*)out, (long)Cout, 0, bias, scale, shift, (const bf16*)res1, (long)Cout, (const bf16*)res2,
                               (long)Cout, (bf16*)pre, (long)Cout, stats, act, M, N, dense_rm(), colsum};
          return launch_igemm<bf16, 256, 256, decltype(la), decltype(lb), decltype(e)>(la, lb, e, M, N, KTILES, 1, 1, st);
        };
        return relu_in ? pp(std::true_type{}) : pp(std::false_type{});
      }
    }
    // 128-output-channel 3x3 convs over >= 2M pixels (output_conv1 at 512^2): 256x128 tiles, 3 stages (one workgroup
    // per CU) -- 2630 vs 2765 us at bs 16 (tools/lin_sweep.py, S3OD_GEMM_CFG 0 vs 1)
    const int def = Cout <= 64 ? 3 : (g.KH == 3 && Cout < 256 && M >= (1 << 21)) ? 0 : 1;
    auto go = [&](auto bn, auto rl) -> int {
      return with_cfg<T>(def, false, [&](auto C0) -> int {
        typedef ConvCfg<decltype(C0), decltype(bn)::value> CC;
        constexpr int BM = CC::BM, NST = CC::NST;
        constexpr int BN = decltype(bn)::value < CC::BN ? decltype(bn)::value : CC::BN;
        constexpr int LN = CC::PP ? CC::LN : BN;
        CC C{};
        ConvFwdA<T, CC::LM, decltype(rl)::value, CC::W> la{}; la.x = (const T*)x; la.g = g; la.M = M;
        DenseKC<T, LN, CC::W> lb{{}, (const T*)wp, (long)K, N, K};
        EpiStd<T, T> e{(T*)out, (long)Cout, 0, bias, scale, shift, (const T*)res1, (long)Cout, (const T*)res2, (long)Cout,
                       (T*)pre, (long)Cout, stats, act, M, N, dense_rm(), colsum};
        return launch_igemm<T, BM, BN, decltype(la), decltype(lb), decltype(e), NST, decltype(C)::WM>(la, lb, e, M, N, KTILES, 1, 1, st);
      });
    };
    if (relu_in) {
      if (Cout <= 64) return go(std::integral_constant<int, 64>{}, std::true_type{});
      if (Cout < 256) return go(std::integral_constant<int, 128>{}, std::true_type{});
      return go(std::integral_constant<int, 256>{}, std::true_type{});
    }
    if (Cout <= 64) return go(std::integral_constant<int, 64>{}, std::false_type{});
    if (Cout < 256) return go(std::integral_constant<int, 128>{}, std::false_type{});
    return go(std::integral_constant<int, 256>{}, std::false_type{});
  });
  return 0;
}

// ---------------------------------------------------------------------------------- weight-gradient route
// Which kernel a conv weight gradient runs on, decided once for s3od_conv_wgrad_ws (the slab query) and
// s3od_conv_wgrad (the call), from the shape arguments and whether the caller gave the GEMM-layout workspace ws:
//   Dma4s2   the 4x4 s2 p1 conv view of ConvTranspose2d(128, 64, 4, 2, 1) (upsample_2x.0) by LDS-DMA (gemm_ops.hip)
//   Dma3x3   the LDS-DMA 3x3 kernel (wgrad_dma.hip): every 3x3 s1 p1 bf16 conv whose tiles are whole (H % 8, W % 32),
//            input channels a multiple of 64 and output channels a multiple of 64 (or the 96 of the mask heads, Cin 64;
//            they run as two output blocks, the second reading 32 channels past each pixel's 96 -- finite data of the
//            next pixel, zeros past the image -- whose products are never flushed).  Measured at bs 16 against the
//            ping-pong Wgrad3B kernel (tools/wgrad_bench.py big, same box): 256^2 256->256 1523-1571 vs 822-834 us,
//            128^2 256->256 401 vs 215, 128^2 512->256 755 vs 394, 64^2 1024->256 425 vs 220, 64^2 256->256 128 vs 84.
//            S3OD_WGRAD_DMA=0 restores the earlier routing (both DMA kernels off).
//   Halo     the register-staged halo-tile kernel (gemm_ops.hip) where the tiles are not whole: 3x3 s1 p1, Cin a multiple
//            of 64, Cout a multiple of 64 (or 96).  Measured at bs 16 (tools/lin_sweep.py SWEEP=conv64): 2.4x / 1.75x on
//            the 1024^2 64 -> 64 / 96 convs, 1.2x on 512^2 256 -> 128, equal at 256^2 / 128^2 and 8 % slower at 64^2
//            -> used for Cin 64 or >= 512^2 maps
//   PpSlab / PpAtomic   the 256-channel RCU / layerK_rn weight gradients on the ping-pong kernel (Wgrad3B): one 256 x 256
//            tile = 256 output channels x one tap's 256 input channels, K = pixels split over ~one round of workgroups,
//            the partials in `split` caller-owned slabs (slab_floats; S3OD_WGRAD_SLAB=0: never) or added into ws by
//            fp32 atomics.  Measured vs the 128x128 implicit GEMM (tools/conv_cfg_bench.py WG=1, bs 16): 256^2 1.47 vs
//            1.63-1.66 ms (ReLU'd input 1.52 vs 1.77-1.97), 128^2 0.39 vs 0.42, 128^2 512 -> 256 0.76 vs 0.85, 64^2
//            1024 -> 256 0.38 vs 0.44; the 64^2 256 -> 256 one (0.14 vs 0.13 ms) stays on 128x128.  S3OD_WGRAD_PP=0: off.
//   Igemm    the generic implicit GEMM (any dtype), split-K by wgrad_split inside the call
enum class WgradPath { Dma4s2, Dma3x3, Halo, PpSlab, PpAtomic, Igemm };
struct WgradRoute {
  WgradPath path;
  int split;           // split-K factor of the ping-pong paths
  long slab_floats;    // PpSlab: split x Cout x 9 Cin
};
static WgradRoute conv_wgrad_route(int dtype, int B, int H, int W, int Cin, int OH, int OW, int Cout, int KH, int KW,
                                   int stride, int pad, int relu_x, int split, bool has_ws) {
  const WgradRoute generic{WgradPath::Igemm, 0, 0};
  if (dtype != S3OD_BF16 || !has_ws) return generic;
  const bool dma_on = !S3OD_OFF("S3OD_WGRAD_DMA");
  if (KH == 4 && KW == 4 && stride == 2 && pad == 1 && H == 2 * OH && W == 2 * OW && Cin % 64 == 0 && Cout % 64 == 0 &&
      !relu_x && (long)H * W * Cin * 2 < (1L << 31) && (long)OH * OW * Cout * 2 < (1L << 31) && dma_on)
    return {WgradPath::Dma4s2, 0, 0};
  if (!(KH == 3 && KW == 3 && stride == 1 && pad == 1 && OH == H && OW == W)) return generic;
  const bool blocks = Cin % 64 == 0 && (Cout % 64 == 0 || (Cout == 96 && Cin == 64));
  if (blocks && H % HT_TH == 0 && W % HT_TW == 0 && (long)H * W * (Cin > Cout ? Cin : Cout) * 2 < (1L << 31) && dma_on)
    return {WgradPath::Dma3x3, 0, 0};
  if (Cin % 64 == 0 && (Cout % 64 == 0 || Cout == 96) && (Cin == 64 || (long)H * W >= 512L * 512))
    return {WgradPath::Halo, 0, 0};
  if (W % 64 == 0 && Cin % 256 == 0 && Cout % 256 == 0 && ((long)H * W >= 128L * 128 || Cin >= 512) && gemm_cfg() < 0 &&
      !S3OD_OFF("S3OD_WGRAD_PP")) {
    const int KTILES = B * OH * OW / 64, tiles = (Cout / 256) * (9 * Cin / 256);
    const int sp = split > 0 ? split : std::max(1, std::min(256 / tiles, KTILES / 8));
    if (slab_ok() && sp > 1) return {WgradPath::PpSlab, sp, (long)sp * Cout * 9 * Cin};
    return {WgradPath::PpAtomic, sp, 0};
  }
  return generic;
}

// The gathers walk a K tile over at most three taps, so a conv needs 2 Cin >= BK (bf16: 32 channels, f32: 16): the forward
// loader refuses anything narrower (buf_ok), and the gradients of such a conv -- whose own gathers read dy or x and
// would run -- are refused with it, before anything is launched.
static bool conv_cin_ok(int dtype, int Cin) { return 2 * Cin >= (dtype == S3OD_BF16 ? KT<bf16>::BK : KT<float>::BK); }

extern "C" {

// ---------------------------------------------------------------------------------- convs
// NHWC activations, weights repacked [Cout][KH][KW][Cin].
// pre = conv(relu?(x)) + bias[n]; out[b,oy,ox,n] = act(pre*scale[n] + shift[n]) (+res1 +res2);
// stats: BN batch sums of pre, fp64 [S3OD_NREP = 32][sum | sum of squares][Cout] replicas, all zero on entry
// (s3od_bn_finalize folds and clears them).
int s3od_conv_fwd(int dtype, int B, int H, int W, int Cin, int OH, int OW, int Cout, int KH, int KW,
                  int stride, int pad, const void* x, int relu_in, const void* wp,
                  const float* bias, const float* scale, const float* shift, int act, const void* res1, const void* res2,
                  void* out, void* pre, double* stats, float* colsum, void* stream) {
  S3OD_REQUIRE(Cin % 8 == 0 && Cout % 8 == 0, "conv_fwd: channels %% 8 (Cin=%d Cout=%d)", Cin, Cout);
  ConvGeo g{}; g.B = B; g.SH = H; g.SW = W; g.SC = Cin; g.RH = OH; g.RW = OW; g.KH = KH; g.KW = KW; g.s = stride; g.p = pad;
  const int M = B * OH * OW, N = Cout, K = KH * KW * Cin;
  hipStream_t st = (hipStream_t)stream;
  if (KH == 4 && KW == 4 && stride == 2 && pad == 1 && H == 2 * OH && W == 2 * OW && Cin == 64 && Cout == 128 && !relu_in &&
      !bias && !scale && !shift && !res1 && !res2 && !pre && !stats && act == ACT_NONE && convt_rw_ok(dtype, B, OH, OW))
    // the data gradient of upsample_2x.0 (ConvTranspose2d(128, 64, 4, 2, 1)): register-weight strided conv
    return conv4s2_rw_launch((const bf16*)x, (const bf16*)wp, colsum, (bf16*)out, B, OH, OW, st);
  if (KH == 3 && KW == 3 && stride == 1 && pad == 1 && OH == H && OW == W && Cin == 64 && Cout == 64 && !relu_in && !stats &&
      !scale && !shift && !res1 && !res2 && !pre && !colsum && (act == ACT_NONE || act == ACT_RELU) && rw_ok(dtype, B, H, W))
    return conv3x3_rw_launch(act == ACT_RELU, (const bf16*)x, (const bf16*)wp, bias, (bf16*)out, B, H, W, st);
  return conv_fwd_igemm(dtype, g, M, N, K, Cin, Cout, x, relu_in, wp, bias, scale, shift, act, res1, res2, out, pre, stats,
                        colsum, st);
}

// conv dgrad == ConvTranspose2d forward.  dy: [B,OH,OW,Cout] (conv output grid); w: [Cout][KH][KW][Cin];
// dx: [B,H,W,Cin] (conv input grid).  One launch per output parity class.  wT (nullable, bf16): [Cin][KH][KW][Cout],
// taps reversed for 3x3 s1 (the data gradient as a forward conv of dy), as-is for the 4x4 s2 sub-pixel kernel.
int s3od_conv_dgrad(int dtype, int B, int H, int W, int Cin, int OH, int OW, int Cout, int KH, int KW,
                    int stride, int pad, const void* dy, const void* wp,
                    const float* bias, const float* scale, const float* shift, int act, const void* res1,
                    const void* res2, void* dx, void* pre, double* stats, float* colsum, const void* wT, void* stream) {
  S3OD_REQUIRE(Cin % 8 == 0 && Cout % 8 == 0, "conv_dgrad: channels %% 8");
  S3OD_REQUIRE(conv_cin_ok(dtype, Cin), "conv_dgrad: Cin %d is below half a K tile: no forward conv of this shape runs", Cin);
  if (wT && KH == 4 && KW == 4 && stride == 2 && pad == 1 && H == 2 * OH && W == 2 * OW && Cout == 128 && Cin == 64 && !scale &&
      !shift && !res1 && !res2 && !pre && !stats && !colsum && (act == ACT_NONE || act == ACT_RELU) && convt_rw_ok(dtype, B, OH, OW))
    // ConvTranspose2d(128, 64, 4, 2, 1) forward (upsample_2x.0): the register-weight sub-pixel kernel; wT =
    // [Cin = 64][4][4][Cout = 128], the conv-view weight transposed WITHOUT tap reversal (s3od_repack_multi mode 2)
    return convT4s2_rw_launch((const bf16*)dy, (const bf16*)wT, bias, act == ACT_RELU, (bf16*)dx, B, OH, OW, (hipStream_t)stream);
  if (wT && KH == 3 && KW == 3 && stride == 1 && pad == 1 && OH == H && OW == W && Cin == 64 && (Cout == 64 || Cout == 96) &&
      !bias && !scale && !shift && !res2 && !pre && !stats && act == ACT_RELU_BWD && res1 && rw_ok(dtype, B, H, W))
    // stride-1 3x3 data gradient = forward conv of dy with the transposed, tap-reversed weight wT ([Cin][3][3][Cout])
    return conv3x3_rw_dgrad_launch(Cout, (const bf16*)dy, (const bf16*)wT, (const bf16*)res1, colsum, (bf16*)dx, B, H, W,
                                   (hipStream_t)stream);
  if (wT && KH == 3 && KW == 3 && stride == 1 && pad == 1 && OH == H && OW == W && (Cin != 64 || Cout > 96) && !pre &&
      !stats) {
    // stride-1 3x3 data gradient = forward conv of dy (Cout channels) with wT [Cin][3][3][Cout]: the forward
    // gather (ConvFwdA) instead of the transposed-conv gather (measured faster on the 256-channel RCU convs)
    ConvGeo gf{}; gf.B = B; gf.SH = H; gf.SW = W; gf.SC = Cout; gf.RH = H; gf.RW = W; gf.KH = 3; gf.KW = 3; gf.s = 1; gf.p = 1;
    return conv_fwd_igemm(dtype, gf, B * H * W, Cin, 9 * Cout, Cout, Cin, dy, 0, wT, bias, scale, shift, act, res1, res2, dx,
                          nullptr, nullptr, colsum, (hipStream_t)stream);
  }
  ConvGeo g0{}; g0.B = B; g0.SH = OH; g0.SW = OW; g0.SC = Cout; g0.KH = KH; g0.KW = KW; g0.s = stride; g0.p = pad;
  hipStream_t st = (hipStream_t)stream;
  DISPATCH_T(dtype, {
    for (int py = 0; py < stride; py++)
      for (int px = 0; px < stride; px++) {
        ConvGeo g = make_class(g0, H, W, py, px);
        const int M = B * g.RH * g.RW, N = Cin, K = g.nth * g.ntw * Cout;
        if (M == 0) continue;
        RowMap rm{}; rm.mode = 2; rm.RH = g.RH; rm.RW = g.RW; rm.OH = H; rm.OW = W; rm.s = stride; rm.py = py; rm.px = px;
        auto go = [&](auto bn) -> int {
          return with_cfg<T>(Cin <= 64 ? 3 : 1, false, [&](auto C0) -> int {
            typedef ConvCfg<decltype(C0), decltype(bn)::value> CC;
            constexpr int BM = CC::BM, NST = CC::NST;
            constexpr int BN = decltype(bn)::value < CC::BN ? decltype(bn)::value : CC::BN;
            constexpr int LN = CC::PP ? CC::LN : BN;
            CC C{};
            ConvDgradA<T, CC::LM, CC::W> la{}; la.x = (const T*)dy; la.g = g; la.M = M;
            ConvDgradB<T, LN, CC::W> lb{}; lb.w = (const T*)wp; lb.g = g; lb.NC = Cin;
            EpiStd<T, T> e{(T*)dx, (long)Cin, 0, bias, scale, shift, (const T*)res1, (long)Cin, (const T*)res2, (long)Cin,
                           (T*)pre, (long)Cin, stats, act, M, N, rm, colsum};
            return launch_igemm<T, BM, BN, decltype(la), decltype(lb), decltype(e), NST, decltype(C)::WM>(la, lb, e, M, N, cdiv(K, KT<T>::BK), 1, 1, st);
          });
        };
        int rc = Cin <= 64 ? go(std::integral_constant<int, 64>{})
                           : (Cin < 256 ? go(std::integral_constant<int, 128>{}) : go(std::integral_constant<int, 256>{}));
        if (rc) return rc;
      }
  });
  return 0;
}

// bytes of the slab workspace s3od_conv_wgrad uses for these arguments when it is given ws (0 = none needed)
int s3od_conv_wgrad_ws(int dtype, int B, int H, int W, int Cin, int OH, int OW, int Cout, int KH, int KW, int stride,
                       int pad, int split, long* bytes) {
  S3OD_REQUIRE(bytes != nullptr, "conv_wgrad_ws: null output");
  // relu_x only decides between two routes that use no slab
  *bytes = 4 * conv_wgrad_route(dtype, B, H, W, Cin, OH, OW, Cout, KH, KW, stride, pad, 0, split, true).slab_floats;
  return 0;
}

// conv wgrad: dw[Cout][Cin][KH][KW] (PyTorch layout, fp32) += sum_pix dy[pix][co] * x[src(pix,tap)][ci]
// dy: [B,OH,OW,Cout]; x: [B,H,W,Cin].  Also serves ConvTranspose2d weights (conv view).
// ws (nullable): Cout*KH*KW*Cin floats, all zero on entry and left all zero (split-K partials in the GEMM layout)
// slab (nullable): caller-owned scratch of slab_bytes (>= s3od_conv_wgrad_ws) for the ping-pong kernel's split-K slabs;
// without it that path adds its partials into ws by fp32 atomics.  The library never allocates.
int s3od_conv_wgrad(int dtype, int B, int H, int W, int Cin, int OH, int OW, int Cout, int KH, int KW,
                    int stride, int pad, const void* dy, const void* x, int relu_x, float* dw, float* ws, int split,
                    float* slab, long slab_bytes, void* stream) {
  S3OD_REQUIRE(Cin % 8 == 0 && Cout % 8 == 0, "conv_wgrad: channels %% 8");
  S3OD_REQUIRE(conv_cin_ok(dtype, Cin), "conv_wgrad: Cin %d is below half a K tile: no forward conv of this shape runs", Cin);
  ConvGeo g{}; g.B = B; g.SH = H; g.SW = W; g.SC = Cin; g.RH = OH; g.RW = OW; g.KH = KH; g.KW = KW; g.s = stride; g.p = pad;
  const int NPIX = B * OH * OW, M = Cout, N = KH * KW * Cin;
  hipStream_t st = (hipStream_t)stream;
  // after a launch that left the partial sums in ws ([Cout][tap][Cin], the GEMM's own layout: a wave's adds hit
  // contiguous addresses): one pass adds them into dW's PyTorch layout and clears ws
  auto permute_ws = [&](int rc) -> int {
    if (rc) return rc;
    hipLaunchKernelGGL(wgrad_permute_add_kernel, dim3(cdiv((long)M * N, 256)), dim3(256), 0, st, ws, dw, M, Cin, KH * KW);
    return s3od_check_launch("conv_wgrad permute");
  };
  WgradRoute r = conv_wgrad_route(dtype, B, H, W, Cin, OH, OW, Cout, KH, KW, stride, pad, relu_x, split, ws != nullptr);
  if (r.path == WgradPath::PpSlab && !(slab && slab_bytes >= 4 * r.slab_floats)) r.path = WgradPath::PpAtomic;
  switch (r.path) {
    case WgradPath::Dma4s2:
      return permute_ws(wgrad4s2_dma_launch((const bf16*)dy, (const bf16*)x, ws, B, OH, OW, Cin, Cout, st));
    case WgradPath::Dma3x3:
      return permute_ws(wgrad3x3_dma_launch(relu_x, (const bf16*)dy, (const bf16*)x, ws, B, H, W, Cin, Cout, st));
    case WgradPath::Halo:
      return permute_ws(wgrad3x3_halo_launch(relu_x, (const bf16*)dy, (const bf16*)x, ws, B, H, W, Cin, Cout, st));
    case WgradPath::PpSlab:
    case WgradPath::PpAtomic: {
      const int KTILES = NPIX / 64;
      DenseMC<bf16, 128> la{{}, (const bf16*)dy, (long)Cout, NPIX, Cout};
      auto pp = [&](auto rl, auto e) -> int {
        Wgrad3B<128, decltype(rl)::value> lb{}; lb.x = (const bf16*)x; lb.B = B; lb.H = H; lb.W = W; lb.Cin = Cin;
        return launch_igemm<bf16, 256, 256, decltype(la), decltype(lb), decltype(e)>(la, lb, e, M, N, KTILES, r.split, 1, st);
      };
      if (r.path == WgradPath::PpSlab) {   // summed straight into dW's PyTorch layout (the atomic workspace stays untouched)
        EpiWgradPart e{slab, M, N};
        int rc = relu_x ? pp(std::true_type{}, e) : pp(std::false_type{}, e);
        if (rc) return rc;
        hipLaunchKernelGGL(wgrad_reduce_kernel, dim3(cdiv((long)M * N / 4, 256)), dim3(256), 0, st, slab, r.split, M, N, dw, Cin, KH * KW);
        return s3od_check_launch("conv_wgrad reduce");
      }
      EpiWgrad e{ws, M, N, N, 1};
      return permute_ws(relu_x ? pp(std::true_type{}, e) : pp(std::false_type{}, e));
    }
    case WgradPath::Igemm:
      break;
  }
  DISPATCH_T(dtype, {
    const int KTILES = cdiv(NPIX, KT<T>::BK);
    auto go = [&](auto bm, auto rl) -> int {
      constexpr int BM = decltype(bm)::value, BN = 128, NST = 2;
      int sp = split > 0 ? split : wgrad_split<T, BM, BN, NST>(cdiv(M, BM) * cdiv(N, BN), KTILES);
      DenseMC<T, BM> la{{}, (const T*)dy, (long)Cout, NPIX, Cout};
      WgradB<T, BN, decltype(rl)::value> lb{}; lb.x = (const T*)x; lb.g = g;
      // taps > 1: the split-K atomics go to the workspace, else straight into dW
      const bool viaws = ws != nullptr && KH * KW > 1;
      EpiWgrad e = viaws ? EpiWgrad{ws, M, N, N, 1} : EpiWgrad{dw, M, N, Cin, KH * KW};
      int rc = launch_igemm<T, BM, BN, decltype(la), decltype(lb), decltype(e), NST>(la, lb, e, M, N, KTILES, sp, 1, st);
      return viaws ? permute_ws(rc) : rc;
    };
    if (relu_x) {
      if (Cout <= 64) return go(std::integral_constant<int, 64>{}, std::true_type{});
      return go(std::integral_constant<int, 128>{}, std::true_type{});
    }
    if (Cout <= 64) return go(std::integral_constant<int, 64>{}, std::false_type{});
    return go(std::integral_constant<int, 128>{}, std::false_type{});
  });
  return 0;
}

// NM (3 for dinob, 1 for dinol) 3x3 64->32 + ReLU + 1x1 32->1 mask heads as one GEMM (N=32NM) with
// a fused epilogue.  feat: [B,H,W,64] T ; w1p: [32NM][3][3][64] T ; b1: [32NM]; w2: [NM][32]; b2: [NM]
// logits: [B,NM,H,W] fp32 (NCHW, the reference output layout); hsave: optional [B*H*W, 32NM] T
int s3od_mask_heads_fwd(int dtype, int B, int H, int W, int NM, const void* feat, const void* w1p, const float* b1,
                        const float* w2, const float* b2, float* logits, void* hsave, void* stream) {
  S3OD_REQUIRE(NM == 1 || NM == 3, "mask_heads_fwd: %d heads not built (1 or 3)", NM);
  ConvGeo g{}; g.B = B; g.SH = H; g.SW = W; g.SC = 64; g.RH = H; g.RW = W; g.KH = 3; g.KW = 3; g.s = 1; g.p = 1;
  const int M = B * H * W, N = 32 * NM, K = 9 * 64;
  hipStream_t st = (hipStream_t)stream;
  if (N == 96 && rw_ok(dtype, B, H, W) && (long)3 * H * W * 4 < (1L << 31))
    return mask_heads_rw_launch((const bf16*)feat, (const bf16*)w1p, b1, w2, b2, logits, (bf16*)hsave, B, H, W, st);
  DISPATCH_T(dtype, {
    constexpr int BM = 128;
    ConvFwdA<T, BM> la{}; la.x = (const T*)feat; la.g = g; la.M = M;
    EpiHeads<T> e{logits, (T*)hsave, b1, w2, b2, M, H * W, NM};
    // 2 K stages -> 2 workgroups per CU, so one's epilogue overlaps the other's K loop
    if (NM == 3) {
      DenseKC<T, 128> lb{{}, (const T*)w1p, (long)K, N, K};
      return launch_igemm<T, BM, 128, decltype(la), decltype(lb), decltype(e), 2>(la, lb, e, M, 128, cdiv(K, KT<T>::BK), 1, 1, st);
    }
    DenseKC<T, 64> lb{{}, (const T*)w1p, (long)K, N, K};
    return launch_igemm<T, BM, 64, decltype(la), decltype(lb), decltype(e), 2>(la, lb, e, M, 64, cdiv(K, KT<T>::BK), 1, 1, st);
  });
  return 0;
}

}  // extern "C"
