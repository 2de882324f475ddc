// C-ABI linear entry points built on the implicit-GEMM engine (gemm.hpp): forward, data and weight gradients, the
// fused QKV projection, and the skinny kernel of their M-tail launches.
#include "gemm_dispatch.hpp"
// blaslt.hip: row-major D = A . B (+ C) through hipBLASLt; 0 = done, nonzero = not run (no algorithm / error)
int blaslt_gemm_rm(const void* A, long lda, const void* B, long ldb, const void* C, long ldc, void* D, long ldd, int M,
                   int N, int K, hipStream_t st);

// ------------------------------------------------------------------ QKV + RoPE epilogue
// n in [0,2304): q | k | v ; RoPE on patch tokens for q,k (tf:…/modeling_dinov3_vit.py:238-268);
// q pre-multiplied by the softmax scale 1/8 (exact in any binary float format).
template <typename T> struct EpiQKV {
  T* q; T* k; T* v; const float* bias; const float* cs; const float* sn;
  int M, Ntok, P, H;
  int moff = 0;                       // global token row of local row 0 (M-tail launch)
  DEV void prepare(int) {}
  DEV void operator()(const float* ct, int LDT, int m0, int n0, int tid, int BM, int BN, int NT) const {
    // this thread's fixed 8-column group: bias of its columns and of their RoPE partners (d +- 32)
    float b8[8], bp8[8];
    {
      const int nn = n0 + (tid % (BN / 8)) * 8, dd = nn & 63, dc = dd < 32 ? 32 : -32;
#pragma unroll
      for (int e = 0; e < 8; e++) { b8[e] = bias ? bias[nn + e] : 0.f; bp8[e] = bias ? bias[nn + dc + e] : 0.f; }
    }
    const bool fixed_cols = NT % (BN / 8) == 0;
    for_segments(ct, LDT, BM, BN, m0, n0, M, 3 * H * 64, tid, NT, [&](int m, int n, const float* a, int r, int c) {
      int which = n / (H * 64), nn = n - which * H * 64, h = nn >> 6, d0 = nn & 63;
      int b = (m + moff) / Ntok, t = (m + moff) - b * Ntok;
      float val[8];
#pragma unroll
      for (int e = 0; e < 8; e++) val[e] = a[e] + (fixed_cols ? b8[e] : (bias ? bias[n + e] : 0.f));
      if (which < 2 && t >= Ntok - P) {
        int dc = d0 < 32 ? 32 : -32;
        const float4* pa = (const float4*)(ct + r * LDT + c + dc);
        float4 p0 = pa[0], p1 = pa[1];
        float pv[8] = {p0.x, p0.y, p0.z, p0.w, p1.x, p1.y, p1.z, p1.w};
        int tp = t - (Ntok - P);
        const float4* cr = (const float4*)(cs + (long)tp * 64 + d0);
        const float4* sr = (const float4*)(sn + (long)tp * 64 + d0);
        float4 c0 = cr[0], c1 = cr[1], s0 = sr[0], s1 = sr[1];
        float cv[8] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w};
        float sv[8] = {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w};
#pragma unroll
        for (int e = 0; e < 8; e++) {
          float q = pv[e] + (fixed_cols ? bp8[e] : (bias ? bias[n + dc + e] : 0.f));
          float rot = d0 < 32 ? -q : q;
          val[e] = val[e] * cv[e] + rot * sv[e];
        }
      }
      if (which == 0) {
#pragma unroll
        for (int e = 0; e < 8; e++) val[e] *= S3OD_QSCALE;
      }
      T* dst = which == 0 ? q : (which == 1 ? k : v);
      store8<T>(dst + (((long)b * H + h) * Ntok + t) * 64 + d0, val);
    });
  }
};

// M tail: rows past the last full 256-row panel (M = 16 * 4101 = 65616 leaves 80) would cost a whole extra round of
// full-K tiles (e.g. o_proj 3078 tiles on 512 slots = 7 rounds, 6 without the tail); they run as a second, small
// launch instead.  f(first row, rows, tail) runs on the whole panels, then on the tail rows with tail = true.
template <class F> static int for_row_panels(int M, int row_mode, F f) {
  if (!(row_mode == 0 && M > 256 && (M & 255) != 0)) return f(0, M, false);
  const int M1 = M & ~255;
  if (int rc = f(0, M1, false)) return rc;
  return f(M1, M - M1, true);
}

// M-tail launches (for_row_panels: the <= 255 rows past the last full 256-row panel).  On 128x128 tiles a tail has only
// N/128 workgroups (6 for N 768), each a full-K main loop on an otherwise idle chip (13-45 us at K 768-3072).  bf16:
// a skinny full-K kernel instead -- one wave per 16 x 16 output block (240 waves for 80 x 768), operands straight from
// global memory (80 rows of A and the B panel stay in L2), and the SAME v_mfma_f32_16x16x32_bf16 chain over K, in the
// same order and fragment layout as the ping-pong / 128x128 kernels (lane (g, l) holds row l, k = 32 kk + 8 g .. +7,
// zero past K), so every tail row is bit-identical to what a full panel computes: outputs do not depend on where a
// row falls, i.e. on the batch size.  (A split-K tail was as fast but broke that: bf16 bs-8 vs bs-1 rel-L2 1e-2.)
// Block = 4 waves = 16 rows x 64 columns; the fp32 tile is staged in LDS and the op's own epilogue functor runs on it.
template <bool BKC, int U, class EPI>
__global__ void __launch_bounds__(256) tail_gemm_kernel(const bf16* __restrict__ A, long lda, const bf16* __restrict__ Bp,
                                                        long ldb, int M, int N, int K, EPI epi) {
  constexpr int LDT = 64 + 4;
  __shared__ __attribute__((aligned(16))) float ct[2048];     // 16 x 68 C tile; the column-sum reduction reads 256 x 8
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, l = lane & 15;
  const int m0 = blockIdx.y * 16, nb0 = blockIdx.x * 64, am = m0 + l, bn = nb0 + wave * 16 + l;
  const bool aok = am < M, bok = bn < N;
  // rows past M / columns past N read row 0 / column 0 instead (clamped addresses, no branches in the loop): an
  // output element only sees its own A row and B column, and those rows / columns are never stored
  const bf16* ar = A + (long)(aok ? am : 0) * lda;
  const long bo = bok ? bn : 0;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  // N-contiguous B (dgrad: w [K][N]): a fragment wants 8 k of one column, so the wave stages each k-step's 32 x 16
  // block through LDS -- lane j fetches 16 B of row k = j / 2 (columns 8 (j & 1) ..), the fragment is read back as 8
  // bf16 of column l (row stride 24 elements = 48 B: 16-B aligned stores; no bank conflicts on the reads)
  constexpr int RS = 24;
  static_assert(sizeof(float) * 2048 + (BKC ? 2 : 2 * 4 * U * 32 * RS) <= 160 * 1024, "tail_gemm: LDS budget (gfx950: 160 KiB)");
  __shared__ bf16 bst[BKC ? 1 : 4 * U * 32 * RS];
  bf16* wst = bst + (BKC ? 0 : wave * U * 32 * RS);
  const int bj = lane >> 1, bc = 8 * (lane & 1);
  const long bcol = (nb0 + wave * 16 + bc < N) ? nb0 + wave * 16 + bc : 0;   // whole 16-B chunks: N % 8 == 0
  auto load = [&](int k, bf16x8& fa, bf16x8& fb) {            // K % 8 == 0: a lane's 8 k are all in range or all out
    fa = *(const bf16x8*)(ar + k);
    if constexpr (BKC) fb = *(const bf16x8*)(Bp + bo * ldb + k);
  };
  // a lone wave's chain is load-latency bound: the loads of U k-steps are issued together, then their U MFMAs run
  // in k order ((B, A) operand order, as Mma<bf16> in the kernels)
  const int KF = K / 32;
  int kk = 0;
  for (; kk + U <= KF; kk += U) {
    bf16x8 fa[U], fb[U];
    uint4 braw[BKC ? 1 : U];
#pragma unroll
    for (int u = 0; u < U; u++) {
      load((kk + u) * 32 + 8 * g, fa[u], fb[u]);
      if constexpr (!BKC) braw[u] = *(const uint4*)(Bp + (long)((kk + u) * 32 + bj) * ldb + bcol);
    }
    if constexpr (!BKC) {
      // the wave's LDS block is written and read back by different lanes of the same wave: order the previous
      // batch's reads before these stores and these stores before the reads (wave-scope fence + wave barrier: the
      // C++ model does not order cross-lane LDS traffic within a wave by itself)
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int u = 0; u < U; u++) *(uint4*)(wst + (u * 32 + bj) * RS + bc) = braw[u];
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int u = 0; u < U; u++)
#pragma unroll
        for (int e = 0; e < 8; e++) fb[u][e] = wst[(u * 32 + 8 * g + e) * RS + l];
    }
    __builtin_amdgcn_sched_barrier(0);                        // all U loads in flight before the first MFMA waits
#pragma unroll
    for (int u = 0; u < U; u++) acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fb[u], fa[u], acc, 0, 0, 0);
  }
  for (; kk < KF; kk++) {
    bf16x8 fa, fb;
    load(kk * 32 + 8 * g, fa, fb);
    if constexpr (!BKC) {
#pragma unroll
      for (int e = 0; e < 8; e++) fb[e] = Bp[(long)(kk * 32 + 8 * g + e) * ldb + bo];
    }
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fb, fa, acc, 0, 0, 0);
  }
  if (K % 32) {                                               // K tail: lanes past K contribute zeros
    bf16x8 fa, fb;
    const int k = KF * 32 + 8 * g;
    if (k < K) {
      load(k, fa, fb);
      if constexpr (!BKC) {
#pragma unroll
        for (int e = 0; e < 8; e++) fb[e] = Bp[(long)(k + e) * ldb + bo];
      }
    } else {
#pragma unroll
      for (int e = 0; e < 8; e++) { fa[e] = (bf16)0.f; fb[e] = (bf16)0.f; }
    }
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fb, fa, acc, 0, 0, 0);
  }
  *(f32x4*)(ct + l * LDT + wave * 16 + 4 * g) = acc;          // lane (g, l) owns C[m0 + l][n + 4g .. 4g+3]
  __syncthreads();
  epi.prepare(0);
  epi(ct, LDT, m0, nb0, tid, 16, 64, 256);
}
template <class LA, class LB, class EPI>
static int launch_tail_gemm(const LA& la, const LB& lb, EPI e, int M, int N, hipStream_t st) {
  // U = k-steps whose loads are in flight together: the largest that divides K / 32 (a remainder runs one step at a
  // time, each paying the full latency).  K-contiguous B: up to 24 (U = 32: 283 VGPRs, spills); N-contiguous B (LDS
  // staging, 4 U KB per wave): up to 16.
  const int KF = la.K / 32;
  auto go = [&](auto u) {
    hipLaunchKernelGGL((tail_gemm_kernel<LB::KCL, decltype(u)::value, EPI>), dim3(cdiv(N, 64), cdiv(M, 16)), dim3(256), 0, st,
                       (const bf16*)la.p, la.ld, (const bf16*)lb.p, lb.ld, M, N, la.K, e);
    return s3od_check_launch("igemm tail");
  };
  if constexpr (LB::KCL) {
    if (KF % 24 == 0) return go(std::integral_constant<int, 24>{});
    if (KF % 16 == 0) return go(std::integral_constant<int, 16>{});
  } else {
    if (KF % 16 == 0) return go(std::integral_constant<int, 16>{});
    if (KF % 12 == 0) return go(std::integral_constant<int, 12>{});
  }
  return go(std::integral_constant<int, 8>{});
}
// the launch of one with_cfg config: the skinny tail kernel for a bf16 M-tail launch (A K-contiguous, no
// ReLU-on-load); f32 tails stay on the 128x128 kernel (same summation order too).  S3OD_TAIL_SKINNY=0 (under S3OD_AB=1: per call):
// the 128x128 tail launch in bf16 as well.
template <typename T, class C, class LA, class LB, class EPI>
static int launch_op(LA la, LB lb, EPI e, int M, int N, int KTILES, bool tail, hipStream_t st) {
  if constexpr (!C::PP && sizeof(T) == 2 && LA::KCL)
    if (tail && !LA::RELU && !LB::RELU && !S3OD_OFF("S3OD_TAIL_SKINNY"))
      return launch_tail_gemm(la, lb, e, M, N, st);
  return launch_igemm<T, C::BM, C::BN, LA, LB, EPI, C::NST, C::WM>(la, lb, e, M, N, KTILES, 1, 1, st);
}

// one launch of s3od_linear_fwd: all of its rows, or one part of for_row_panels
static int linear_fwd_rows(int dtype, int M, int N, int K, const void* x, long ldx, const void* w,
                           const float* bias, const float* scale, const float* shift, int act,
                           const void* res1, long ldr1, const void* res2, long ldr2, int res_f32,
                           void* out, long ldo, int out_f32, void* pre, long ldp,
                           int row_mode, int P, int prefix, bool tail, void* stream) {
  RowMap rm = dense_rm(); rm.mode = row_mode; rm.P = P; rm.prefix = prefix;
  hipStream_t st = (hipStream_t)stream;
  DISPATCH_T(dtype, {
    const int KTILES = cdiv(K, KT<T>::BK);
    auto go = [&](auto tile, auto tout, auto tres) -> int {
      typedef decltype(tout) TO; typedef decltype(tres) TR;
      // measured (tools/lin_sweep.py, bs 16 1024^2): the 256x256 ping-pong kernel for the large ViT
      // linears (o_proj 241 -> 215 us, up 576 -> 563, down 487 -> 418); else 256x128 x 3 stages for
      // K >= 2048, 128x128 otherwise.  Since the quarter-staged ping-pong epilogue (round 6) the plain bias-only
      // DPT projections M=65536 K=768 run on it too (tools/lib_ab.py: N 1024 160 -> 156 us, 512 90 -> 87, 256 54 -> 52)
      const int def = (pp_pays(M, N) && N % 256 == 0) ? 5 : (K >= 2048 ? 0 : 1);
      return with_cfg<T, true>(def, tail, [&](auto C) -> int {
        DenseKC<T, decltype(C)::LM, decltype(C)::W> la{{}, (const T*)x, ldx, M, K};
        DenseKC<T, decltype(C)::LN, decltype(C)::W> lb{{}, (const T*)w, (long)K, N, K};
        EpiStd<TO, TR, T> e{(TO*)out, ldo, 0, bias, scale, shift, (const TR*)res1, ldr1, (const TR*)res2, ldr2,
                            (T*)pre, ldp, nullptr, act, M, N, rm};
        return launch_op<T, decltype(C)>(la, lb, e, M, N, KTILES, tail, st);
      });
    };
    if (out_f32 && res_f32) return go(0, float{}, float{});
    if (out_f32) return go(0, float{}, T{});
    if (res_f32) return go(0, T{}, float{});
    return go(0, T{}, T{});
  });
  return 0;
}

// one launch of s3od_linear_dgrad: all of its rows, or one part of for_row_panels
static int linear_dgrad_rows(int dtype, int M, int N, int K, const void* dy, long lddy, const void* w,
                             int act, const void* aux, long ldaux, void* dx, long lddx, int out_f32,
                             int row_mode, int P, int prefix, float* colsum, bool tail, void* stream) {
  // plain bf16 data gradients -- no activation derivative, no column sums, dense rows; aux an accumulate -- are plain
  // library GEMMs: hipBLASLt (blaslt.hip), 1.24-1.35x faster on the ViT backward's long-K shapes.  Only the whole
  // 256-row panels: left a tail, hipBLASLt adds a 16x16-tile kernel over the full K for it, which beside the side
  // stream's weight gradients took 300-370 us in the step (profiles/r06z_summary.md) -- the M-tail stays on the skinny
  // tail kernel above.  S3OD_DGRAD_BLASLT=0 (or no algorithm for the shape) keeps everything here.
  if (!tail && dtype == S3OD_BF16 && act == ACT_NONE && !out_f32 && row_mode == 0 && !colsum &&
      S3OD_KNOB("S3OD_DGRAD_BLASLT", 1) &&
      blaslt_gemm_rm(dy, lddy, w, N, aux, ldaux, dx, lddx, M, N, K, (hipStream_t)stream) == 0)
    return s3od_check_launch("linear_dgrad (hipBLASLt)");
  RowMap rm = dense_rm(); rm.mode = row_mode; rm.P = P; rm.prefix = prefix;
  hipStream_t st = (hipStream_t)stream;
  DISPATCH_T(dtype, {
    const int KTILES = cdiv(K, KT<T>::BK);
    // ping-pong 256x256 for the long-K dgrads (up 441 -> 374 us, qkv 334 -> 292) and the K = 768 ones with an
    // activation-derivative epilogue (down-projection x gelu': 519 -> 500 us, round 6); 128x128 for plain K = 768
    // (o_proj 118 vs 118 us)
    const int def = (pp_pays(M, N) && N % 256 == 0 && (K >= 2048 || act != ACT_NONE)) ? 5 : 1;
    return with_cfg<T, true>(def, tail, [&](auto C) -> int {
      DenseKC<T, decltype(C)::LM, decltype(C)::W> la{{}, (const T*)dy, lddy, M, K};
      DenseMC<T, decltype(C)::LN, decltype(C)::W> lb{{}, (const T*)w, (long)N, K, N};
      if (out_f32) {
        // f32 output: aux is an f32 tensor to add (e.g. the residual-stream gradient, in place)
        EpiStd<float, float> e{(float*)dx, lddx, 0, nullptr, nullptr, nullptr, (const float*)aux, ldaux, nullptr, 0, nullptr, 0, nullptr, act, M, N, rm, colsum};
        return launch_op<T, decltype(C)>(la, lb, e, M, N, KTILES, tail, st);
      }
      EpiStd<T, T> e{(T*)dx, lddx, 0, nullptr, nullptr, nullptr, (const T*)aux, ldaux, nullptr, 0, nullptr, 0, nullptr, act, M, N, rm, colsum};
      return launch_op<T, decltype(C)>(la, lb, e, M, N, KTILES, tail, st);
    });
  });
  return 0;
}

// The route of a linear weight gradient, shared by the slab query and the call: f(TileCfg, split-K factor, slab
// floats).  Tile config: a 256x256 kernel with split-K slabs for the large outputs -- the 4-wave kernel (gemm_q.hip),
// whose ring of k-step stages beats the ping-pong kernel in every round of a same-process A/B over 65616 rows
// (3072x768 348-411 -> 287-316 us, 768x3072 345-390 -> 273-278, 2304x768 269-289 -> 206-221;
// profiles/gemm_q_ring_lin_ab.txt), same split factor and slabs, bit-identical partial sums -- and 256x128 x 3 stages
// with fp32 atomics otherwise.  (The small outputs over
// >= 64K rows are faster alone on the ping-pong kernel too -- tools/wgrad_sweep.py: 768x768 127 -> 110 us, 1024x768
// 154 -> 144, 256x256 x 1M rows 283 -> 268; profiles/r05t_wgrad_sweep.txt -- but null in the step, where these run on
// the side stream beside the data gradients: tools/ab_step.py medians 151.4 vs 151.0 ms.)
// Slab floats (0: the fp32-atomic epilogue, no slab): the 256x256 kernels' split-K partials go to sp caller-owned
// fp32 slabs [sp][Nout][Kin], summed by wgrad_reduce_kernel.
template <typename T, class F> static int linear_wgrad_route(int Nout, int Kin, int rows, int split, F f) {
  const int def = (long)Nout * Kin > 1024L * 1024 ? 6 : 0;
  return with_cfg<T, true>(def, false, [&](auto C) -> int {
    typedef decltype(C) CC;
    const int KTILES = cdiv(rows, KT<T>::BK);
    const int sp = split > 0 ? split : wgrad_split<T, CC::BM, CC::BN, CC::NST>(cdiv(Nout, CC::BM) * cdiv(Kin, CC::BN), KTILES);
    const bool slabs = CC::SLAB && slab_ok() && Kin % 4 == 0 && sp > 1;
    return f(C, sp, slabs ? (long)sp * Nout * Kin : 0L);
  });
}

extern "C" {

#ifdef S3OD_TIMELINE
// dev timeline build only (tools/pp_timeline.py): where the ping-pong kernels of this file record their blocks
int s3od_dbg_timeline(unsigned long long* buf) {
  return hipMemcpyToSymbol(HIP_SYMBOL(s3od_tl), &buf, sizeof(buf)) == hipSuccess ? 0 : 1;
}
#endif

// ---------------------------------------------------------------------------------- linear
// pre = sum_k x[m,k] w[n,k] + bias[n];  out[rm(m), n] = act(pre*scale[n] + shift[n]) (+res1 +res2)
// x: [M,K] (ld ldx) dtype T, w: [N,K] T, res: T or f32 (res_f32), out T or f32 (out_f32).
// row_mode 0: dense; 1: token rows (m = b*P + p -> b*(P+prefix) + prefix + p)
int s3od_linear_fwd(int dtype, int M, int N, int K, const void* x, long ldx, const void* w,
                    const float* bias, const float* scale, const float* shift, int act,
                    const void* res1, long ldr1, const void* res2, long ldr2, int res_f32,
                    void* out, long ldo, int out_f32, void* pre, long ldp,
                    int row_mode, int P, int prefix, void* stream) {
  S3OD_REQUIRE(K % 8 == 0 && N % 8 == 0, "linear_fwd: K and N must be multiples of 8 (K=%d N=%d)", K, N);
  const long es = dtype == S3OD_BF16 ? 2 : 4, eo = out_f32 ? 4 : es, er = res_f32 ? 4 : es;
  return for_row_panels(M, row_mode, [&](int m0, int rows, bool tail) -> int {
    return linear_fwd_rows(dtype, rows, N, K, (const char*)x + m0 * ldx * es, ldx, w, bias, scale, shift, act,
                           res1 ? (const char*)res1 + m0 * ldr1 * er : nullptr, ldr1,
                           res2 ? (const char*)res2 + m0 * ldr2 * er : nullptr, ldr2, res_f32,
                           (char*)out + m0 * ldo * eo, ldo, out_f32, pre ? (char*)pre + m0 * ldp * es : nullptr, ldp,
                           row_mode, P, prefix, tail, stream);
  });
}

// dx[rm(m), n] = sum_k dy[m,k] w[k,n] (+ res)  (w: [K=out][N=in]); act=ACT_GELU_BWD multiplies by
// gelu'(aux); with act=ACT_NONE a non-null aux is ADDED (aux may alias dx: in-place accumulate).
int s3od_linear_dgrad(int dtype, int M, int N, int K, const void* dy, long lddy, const void* w,
                      int act, const void* aux, long ldaux, void* dx, long lddx, int out_f32,
                      int row_mode, int P, int prefix, float* colsum, void* stream) {
  S3OD_REQUIRE(K % 8 == 0 && N % 8 == 0, "linear_dgrad: K,N %% 8");
  const long es = dtype == S3OD_BF16 ? 2 : 4, eo = out_f32 ? 4 : es;
  return for_row_panels(M, row_mode, [&](int m0, int rows, bool tail) -> int {
    return linear_dgrad_rows(dtype, rows, N, K, (const char*)dy + m0 * lddy * es, lddy, w, act,
                             aux ? (const char*)aux + m0 * ldaux * eo : nullptr, ldaux, (char*)dx + m0 * lddx * eo, lddx,
                             out_f32, row_mode, P, prefix, colsum, tail, stream);
  });
}

// bytes of the slab workspace s3od_linear_wgrad uses for these arguments (0 = none needed)
int s3od_linear_wgrad_ws(int dtype, int Nout, int Kin, int rows, int split, long* bytes) {
  S3OD_REQUIRE(bytes != nullptr, "linear_wgrad_ws: null output");
  *bytes = 0;                                             // only the bf16 configs write slabs
  if (dtype != S3OD_BF16) return 0;
  return linear_wgrad_route<bf16>(Nout, Kin, rows, split, [&](auto, int, long slab_floats) -> int {
    *bytes = 4 * slab_floats;
    return 0;
  });
}

// dw[n_out, k_in] += sum_rows dy[row, n_out] x[row, k_in]  (split over rows: fp32 atomics into dw, or -- when the
// caller passes a slab of >= s3od_linear_wgrad_ws bytes -- per-split fp32 slabs summed into dw by a second kernel)
int s3od_linear_wgrad(int dtype, int Nout, int Kin, int rows, const void* dy, long lddy,
                      const void* x, long ldx, float* dw, int split, float* slab, long slab_bytes, void* stream) {
  S3OD_REQUIRE(Nout % 8 == 0 && Kin % 8 == 0, "linear_wgrad: dims %% 8");
  hipStream_t st = (hipStream_t)stream;
  DISPATCH_T(dtype, {
    const int KTILES = cdiv(rows, KT<T>::BK);
    return linear_wgrad_route<T>(Nout, Kin, rows, split, [&](auto C, int sp, long slab_floats) -> int {
      constexpr int BM = decltype(C)::BM, BN = decltype(C)::BN, NST = decltype(C)::NST;
      DenseMC<T, decltype(C)::LM, decltype(C)::W> la{{}, (const T*)dy, lddy, rows, Nout};
      DenseMC<T, decltype(C)::LN, decltype(C)::W> lb{{}, (const T*)x, ldx, rows, Kin};
      if constexpr (decltype(C)::SLAB) {
        if (slab && slab_floats > 0 && slab_bytes >= 4 * slab_floats) {
          EpiWgradPart e{slab, Nout, Kin};
          int rc = launch_igemm<T, BM, BN, decltype(la), decltype(lb), decltype(e), NST, decltype(C)::WM>(la, lb, e, Nout, Kin, KTILES, sp, 1, st);
          if (rc) return rc;
          hipLaunchKernelGGL(wgrad_reduce_kernel, dim3(cdiv((long)Nout * Kin / 4, 256)), dim3(256), 0, st, slab, sp, Nout, Kin, dw, Kin, 1);
          return s3od_check_launch("linear_wgrad reduce");
        }
      }
      EpiWgrad e{dw, Nout, Kin, Kin, 1};
      return launch_igemm<T, BM, BN, decltype(la), decltype(lb), decltype(e), NST, decltype(C)::WM>(la, lb, e, Nout, Kin, KTILES, sp, 1, st);
    });
  });
  return 0;
}

// fused QKV projection + bias + RoPE + head split. x: [B*Ntok, D] T ; w: [3D, D] T ; D = 64 H
int s3od_qkv_rope_fwd(int dtype, int B, int Ntok, int P, int H, const void* x, const void* w, const float* bias,
                      const float* cos_t, const float* sin_t, void* q, void* k, void* v, void* stream) {
  const int D = 64 * H, N = 3 * D;
  hipStream_t st = (hipStream_t)stream;
  DISPATCH_T(dtype, {
    return for_row_panels(B * Ntok, 0, [&](int m_first, int M, bool tail) -> int {
      return with_cfg<T>(pp_pays(M, N) ? 5 : 1, tail, [&](auto C) -> int {
        DenseKC<T, decltype(C)::LM, decltype(C)::W> la{{}, (const T*)x + (long)m_first * D, (long)D, M, D};
        DenseKC<T, decltype(C)::LN, decltype(C)::W> lb{{}, (const T*)w, (long)D, N, D};
        EpiQKV<T> e{(T*)q, (T*)k, (T*)v, bias, cos_t, sin_t, M, Ntok, P, H};
        e.moff = m_first;
        return launch_op<T, decltype(C)>(la, lb, e, M, N, cdiv(D, KT<T>::BK), tail, st);
      });
    });
  });
  return 0;
}

}  // extern "C"
