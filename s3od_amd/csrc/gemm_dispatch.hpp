// What the GEMM entry files (linear_ops.hip, conv_ops.hip) share on the host side: the tile
// configurations, the split-K model and the kernels that fold split-K partials into dW.
#pragma once
#include "gemm.hpp"
#include <stdlib.h>
#include <type_traits>
#include <utility>

static RowMap dense_rm() { RowMap r{}; r.mode = 0; return r; }

// Tile configuration (dev knob for the micro-benchmarks): S3OD_GEMM_CFG=<n> forces one config for
// every GEMM entry point; default (-1) = per-op choice below.
//   0: 256x128, 3 stages (1 WG/CU)   1: 128x128, 2 stages (2 WG/CU)   2: 128x128, 3 stages
//   3: 256x128, 2 stages (BN is clamped to 64 for 64-channel convs: 256x64 x 2 stages = 80 KB)
//   4: 256x256, 2 stages (1 WG/CU, per-wave 64x128; C staged in two 128-row halves)
static int gemm_cfg() { return S3OD_KNOB("S3OD_GEMM_CFG", -1); }
// W = waves that issue the operand loads (the loaders are built for that many waves)
// PP_: the 256x256 ping-pong kernel (bf16 only), whose loaders stage half tiles (LM / LN rows)
template <int BM_, int BN_, int NST_, int W_ = GEMM_WAVES, int WM_ = 0, bool PP_ = false> struct TileCfg {
  static constexpr int BM = BM_, BN = BN_, NST = NST_, W = W_, WM = WM_;
  static constexpr bool PP = PP_;
  static constexpr bool SLAB = PP_ || WM_ < 0;   // split-K partials into caller slabs (the 256x256 kernels)
  static constexpr int LM = PP_ ? BM_ / 2 : BM_, LN = PP_ ? BN_ / 2 : BN_;
};
// a conv whose output-channel tile is narrower than 256 cannot run the ping-pong kernel
template <class C, int BNW> using ConvCfg = std::conditional_t<(C::PP && BNW < 256), TileCfg<128, 128, 2>, C>;
// the 256x256 ping-pong kernel (one workgroup per CU) only pays when its tiles fill whole rounds of
// the 256 CUs: at bs 8 (M = 32808) o_proj / down-projection / QKV have 384 / 384 / 1152 tiles = 1.5 /
// 1.5 / 4.5 rounds, where the 128x128 config (2 per CU) runs whole rounds (o_proj 138 us at 281 TF/s)
static bool pp_pays(int M, int N) {
  const long tiles = (long)(M / 256) * cdiv(N, 256), rounds = (tiles + 255) / 256;
  return tiles >= 256 && (double)tiles / (double)(rounds * 256) >= 0.95;
}
// call f(TileCfg) for the selected config; `def` = per-op default config index.  An M-tail launch (linear_ops.hip:
// for_row_panels) runs the 128x128 config whatever S3OD_GEMM_CFG says.
// Q: the op may run config 6, the 4-wave 256x256 kernel (gemm_q.hip: instantiated for the linears only)
template <typename T, bool Q = false, class F> static int with_cfg(int def, bool tail, F f) {
  int c = tail ? 1 : gemm_cfg(); if (c < 0) c = def;
  switch (c) {
    case 6:
      if constexpr (Q && sizeof(T) == 2) return f(TileCfg<256, 256, 2, 4, -1>{});
      else return f(TileCfg<128, 128, 2>{});
    case 1: return f(TileCfg<128, 128, 2>{});
    case 2: return f(TileCfg<128, 128, 3>{});
    case 3: return f(TileCfg<256, 128, 2>{});
    case 4: return f(TileCfg<256, 256, 2>{});
    case 5:
      if constexpr (sizeof(T) == 2) return f(TileCfg<256, 256, 2, GEMM_WAVES, 0, true>{});
      else return f(TileCfg<128, 128, 2>{});
    default: return f(TileCfg<256, 128, 3>{});
  }
}

// split-K factor of a wgrad GEMM from a time model: ceil(tiles*sp / slots) rounds of ceil(KT/sp)
// K tiles each, plus the split-K fp32 atomics at the chip-wide atomic rate (~1.3 TB/s, guide
// "Global float atomics").  slots = resident workgroups (256 CUs x WGs per CU by LDS).
template <typename T, int BM, int BN, int NST> static int wgrad_split(int tiles, int KT) {
  typedef GemmShape<T, BM, BN, NST> S;
  const int per_cu = (160 * 1024) / S::LDS > 0 ? (160 * 1024) / S::LDS : 1;
  const long slots = 256L * per_cu;
  const double ck = 2.0 * BM * BN * S::BK / (3.9e6 / per_cu);      // us per K tile per WG
  const double atom = (double)BM * BN * 4 / 1.3e6;                 // us of chip atomics per WG
  int best = 1; double bt = 1e30;
  for (int sp = 1; sp <= (KT >= 8 ? KT / 4 : 1); sp++) {
    long wgs = (long)tiles * sp;
    double t = (double)((wgs + slots - 1) / slots) * ((KT + sp - 1) / sp) * ck + wgs * atom;
    if (t < bt * 0.999) { bt = t; best = sp; }
  }
  return best;
}

// dW (+)= the sum of the split-K slabs ws[sp][M][N] (EpiWgradPart), scattered to the PyTorch layout
// dW[(m*Cx + cin)*taps + tap] for n = tap*Cx + cin (Linear: taps = 1, Cx = N).  One thread per 4 consecutive n.
inline __global__ void wgrad_reduce_kernel(const float* __restrict__ ws, int sp, int M, int N, float* __restrict__ dw, int Cx, int taps) {
  const long i4 = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 4;
  const long MN = (long)M * N;
  if (i4 >= MN) return;
  // the slabs' loads go out 8 at a time before any add (a load-add chain waits out one memory latency per slab:
  // 81 us for 7 slabs of 3072 x 768 in the step, 4x the bytes' HBM time); summation order z = 0, 1, .. unchanged
  float4 s = *(const float4*)(ws + i4);
  for (int z0 = 1; z0 < sp; z0 += 8) {
    float4 v[8];
#pragma unroll
    for (int u = 0; u < 8; u++)
      if (z0 + u < sp) v[u] = *(const float4*)(ws + (long)(z0 + u) * MN + i4);
#pragma unroll
    for (int u = 0; u < 8; u++)
      if (z0 + u < sp) { s.x += v[u].x; s.y += v[u].y; s.z += v[u].z; s.w += v[u].w; }
  }
  const int m = (int)(i4 / N), n = (int)(i4 - (long)m * N);
  if (taps == 1) {
    float4* d = (float4*)(dw + i4);
    const float4 o = *d;
    *d = make_float4(o.x + s.x, o.y + s.y, o.z + s.z, o.w + s.w);
    return;
  }
  const float sv[4] = {s.x, s.y, s.z, s.w};
#pragma unroll
  for (int e = 0; e < 4; e++) {
    const int tap = (n + e) / Cx, cin = (n + e) - tap * Cx;
    dw[((long)m * Cx + cin) * taps + tap] += sv[e];
  }
}

// S3OD_WGRAD_SLAB=0 (under S3OD_AB=1: per call): the fp32-atomic split-K epilogue instead of the slabs (A/B)
static bool slab_ok() { return !S3OD_OFF("S3OD_WGRAD_SLAB"); }

// dw[(co*Cin + ci)*taps + tap] += ws[(co*taps + tap)*Cin + ci]   (one thread per dw element)
// ws enters all zero (split-K atomics land in it) and leaves all zero: each element is cleared as it is read,
// so a persistent workspace needs no memset per call
inline __global__ void wgrad_permute_add_kernel(float* __restrict__ ws, float* __restrict__ dw, int Cout, int Cin, int taps) {
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)Cout * Cin * taps) return;
  int tap = i % taps; long r = i / taps;
  int ci = r % Cin; int co = r / Cin;
  const long src = ((long)co * taps + tap) * Cin + ci;
  dw[i] += ws[src];
  ws[src] = 0.f;
}
