// 256x256 GEMM on FOUR waves, one per SIMD, each owning a 128x128 sub-tile (8 x 8 blocks of 16x16: 256 fp32
// accumulators per lane, in AGPRs -- this translation unit is built WITHOUT the VGPR MFMA form, see the Makefile).
//
// Why: the 8-wave ping-pong kernel (gemm.hpp igemm_pp_kernel, two 128x64 waves per SIMD) reads 0.38 LDS instructions
// and issues 1.1 SALU + 0.5 VALU per MFMA and spends 37 % of its wave-cycles in s_waitcnt / barrier waits: 8192^3 bf16
// on random data 1040 TF/s at 58 % MFMA-busy, where hipBLASLt's 256x256x64 kernel -- four waves, one per SIMD --
// reaches 1450-1470 TF/s at 87 % MFMA-busy with 0.25 LDS instructions per MFMA (profiles/r06d_gemm_pmc.txt).
// A 128x128 wave tile halves the fragment reads per MFMA (each A / B fragment feeds 8 MFMAs instead of 4).
//
// K loop: a ring of four LDS stages, one 32-deep k-step (64 MFMAs per wave) each: A 256 x 64 B | B 256 x 64 B = 32 KB
// (images and loaders: KStep / QFrag below).  K-step s computes from fragment buffer s & 1 and, INSIDE its MFMA
// stream, reads the fragments of k-step s + 1 (stage (s + 1) & 3) into the other buffer and issues the LDS-DMA of
// k-step s + 4 into its own stage s & 3:
//   lgkmcnt(0)                  this k-step's fragments (read a whole block ago) are in
//   MFMA 0-3
//   vmcnt(16) + s_barrier       own pieces of k-step s + 1 landed; s + 2 and s + 3 (8 pieces per wave each) stay in
//                               flight, so a stage has three k-steps = 192 MFMAs to arrive and the wait is never 0
//                               (k-steps past the end of the K range are staged too, as zeros from the range
//                               check and never computed, so the count holds in the prologue and the tail as well)
//   MFMA 4-..                   two fragment reads per MFMA gap (one where both operands are ds_read_b64_tr pairs),
//                               then one DMA piece every fourth gap
//   RAW: a stage is read only behind the barrier that follows every wave's counted wait for its pieces of that stage.
//   WAR: stage s & 3 is restaged behind the barrier of k-step s; its only reads (the fragments of k-step s, issued
//        in block s - 1) are behind every wave's lgkmcnt(0) at the head of block s, ahead of that barrier.
// The loop body is one pair of stages; fragment addresses are per-lane constants plus immediates, moved to the other
// pair once per iteration.  One barrier per k-step.
// Epilogue: the fp32 C tile is staged through the (free) ring LDS in two 128-row halves and handed to the same
// block-level epilogue functors as the other kernels (NT = 256 threads).
#include "gemm.hpp"

// ------------------------------------------------------------------ k-step images: loaders and fragment readers
// ONE 32-deep k-step of an operand per LDS image: 256 rows x 64 B = 16 LDS-DMA pieces of 1 KiB, piece = wave * 4 + i.
//   KC image [256 rows][64 B]: four rows share a 256-B bank row, so the 16-B chunk c of row r sits at physical chunk
//     c ^ kc64_x(r), kc64_x = (0, 3, 2, 1)[(r >> 2) & 3].  A fragment read (lane (g, l): row row0 + l, chunk g) is then
//     conflict-free: ds_read_b128 serves lanes {g = 0: l 0-3, 12-15; g = 1: l 4-11} (and the three like groups)
//     together, i.e. per l & 3 the four (g, l >> 2) pairs (0,0) (0,3) (1,1) (1,2), whose physical chunks g ^ kc64_x are
//     0, 1, 2, 3.  Piece p, lane j: row p * 16 + (j >> 2), physical chunk j & 3 -- the same XOR on the DMA source
//     offset and on the read (guide §5.4 rule 21).
//   MC image [32 k][512 B]: the k rows kk * 32 .. + 31 of the 64-deep MC tile image, swizzle unchanged (g(k) depends on
//     k & 3 and (k >> 3) & 1 only, both k-step-local).  Piece p, lane j: k row p * 2 + (j >> 5), byte (j & 31) * 16.
DEV int kc64_x(int r) { const int h = (r >> 2) & 3; return h ^ ((h & 1) << 1); }
// The pieces are issued by inline asm, descriptor built by hand (base, stride 0, bytes, raw-buffer flags -- the words
// make_rsrc's builtin produces): the waitcnt pass does not see them, so it adds no vmcnt(0) of its own in front of LDS
// reads it cannot tell from the DMA's target (it does in front of every ds_read_b64_tr_b16, which would drain the
// ring); the kernel's counted waits order them.  The asm sets M0 (the wave's LDS base) itself: nothing else in these
// kernels uses M0.
typedef __attribute__((address_space(3))) const char lds_cchar;
DEV unsigned lds_addr(const char* p) { return (unsigned)(unsigned long)(lds_cchar*)p; }
DEV const char* lds_ptr(unsigned a) { return (const char*)(lds_cchar*)(unsigned long)a; }
typedef int i32x4_t __attribute__((ext_vector_type(4)));
DEV i32x4_t q_rsrc(const void* p, unsigned long bytes) {
  const unsigned long a = (unsigned long)p;
  return i32x4_t{(int)(unsigned)a, (int)((a >> 32) & 0xffff), (int)(unsigned)(bytes < BUF_MAX ? bytes : BUF_MAX), 0x00020000};
}
DEV void blds16s(i32x4_t r, unsigned voff, unsigned soff, unsigned lds_wave_base) {
  asm volatile("s_mov_b32 m0, %3\n\ts_nop 0\n\tbuffer_load_dwordx4 %0, %1, %2 offen lds"
               :: "v"(voff), "s"(r), "s"(soff), "s"(lds_wave_base) : "memory");
}
// klim = the end of the block's K range (K, or the end of its split-K share): k-steps at or past it are staged as
// zeros without touching memory, by a descriptor of zero bytes (scalar).
template <class L, bool KCL = L::KCL> struct KStep;
template <class L> struct KStep<L, true> {          // over DenseKC<bf16, 256, 4>
  const bf16* pb; unsigned long nb; unsigned vo[4], vt[4]; int wb, klim, kpart;
  DEV void setup(const L& l, int t0, int tid, int klim_) {
    const int lane = tid & 63, wave = wave_id(), rem = l.nrows - t0;
    wb = wave * 4096;
    klim = klim_;
    kpart = (klim & 31) ? klim >> 5 : -1;           // the k-step that klim cuts (K % 32 != 0), if any
    pb = l.p + (long)t0 * l.ld;
    nb = rem > 0 ? ((unsigned long)(min(rem, 256) - 1) * l.ld + l.K) * 2 : 0;
    const int kel = ((lane & 3) ^ kc64_x(lane >> 2)) * 8;
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const int r = (wave * 4 + i) * 16 + (lane >> 2);
      vo[i] = r < rem ? (unsigned)(((long)r * l.ld + kel) * 2) : BUF_OOB;
      vt[i] = (klim & ~31) + kel < klim ? vo[i] : BUF_OOB;     // offsets for k-step kpart: chunks past K read zeros
    }
  }
  // piece i of k-step ks into the image at img; the k-step's byte offset rides in the scalar offset
  DEV void piece(const L&, int ks, char* img, int i) const {
    const auto rs = q_rsrc(pb, ks * 32 < klim ? nb : 0);
    blds16s(rs, ks == kpart ? vt[i] : vo[i], (unsigned)ks * 64u, lds_addr(img) + wb + i * 1024);
  }
};
template <class L> struct KStep<L, false> {         // over DenseMC<bf16, 256, 4>
  unsigned vo[4]; int wb; unsigned long tot;
  DEV void setup(const L& l, int t0, int tid, int klim) {
    const int lane = tid & 63, wave = wave_id();
    wb = wave * 4096;
    // bytes up to the end of k row klim - 1: the range check zero-fills every later row, no per-lane K-tail test
    tot = klim > 0 ? ((unsigned long)(klim - 1) * l.ld + l.ncols) * 2 : 0;
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const int k = wave * 8 + (lane >> 5) + 2 * i;
      const int cl = t0 + mc_logical_byte<512>(k, (lane & 31) * 16) / 2;
      vo[i] = cl < l.ncols ? (unsigned)(((long)k * l.ld + cl) * 2) : BUF_OOB;
    }
  }
  // the descriptor is rebased to the k-step's first row, as DenseMC rebases it per K tile
  DEV void piece(const L& l, int ks, char* img, int i) const {
    const unsigned long e0 = (unsigned long)ks * 32 * l.ld * 2;
    const auto rs = q_rsrc((const char*)l.p + e0, e0 < tot ? tot - e0 : 0);
    blds16s(rs, vo[i], 0u, lds_addr(img) + wb + i * 1024);
  }
};
// Fragment reads of a k-step image inside the ring of four 32 KB stages.  The per-lane address is computed once; the
// row block (i * 16 rows) and the stage's place inside its PAIR of stages (st01 * 32 KB) are immediates.  A DS offset
// field holds 16 bits, so the pair (stages 0-1 / 2-3) is in the address register: flip() moves it to the other pair
// (one VALU per address register and pair of k-steps).
template <bool KCL> struct QFrag;
template <> struct QFrag<true> {
  unsigned a;
  DEV void init(const char* img, int lane, int half) {
    const int l = lane & 15;
    a = lds_addr(img) + half * 8192 + l * 64 + (((lane >> 4) ^ kc64_x(l)) << 4);
  }
  DEV void flip(int d) { a += d; }
  DEV bf16x8 read(int st01, int i) const { return *(const bf16x8*)(lds_ptr(a) + st01 * 32768 + i * 1024); }
};
template <> struct QFrag<false> {
  unsigned a[8];
  DEV void init(const char* img, int lane, int half) {
    const int g = lane >> 4, l = lane & 15, q = l >> 2, p = l & 3, gk = q | ((g & 1) << 2);
#pragma unroll
    for (int i = 0; i < 8; i++) a[i] = lds_addr(img) + (8 * g + q) * 512 + half * 256 + ((i ^ gk) << 5) + 8 * p;
  }
  DEV void flip(int d) {
#pragma unroll
    for (int i = 0; i < 8; i++) a[i] += d;
  }
  DEV bf16x8 read(int st01, int i) const {
    const char* s = lds_ptr(a[i]) + st01 * 32768;
    return read_tr_pair(s, s + 2048);
  }
};

namespace {
constexpr int Q_THREADS = 256, Q_BM = 256, Q_BN = 256, Q_IMG = 256 * 64, Q_STAGE = 2 * Q_IMG, Q_RING = 4, Q_LDT = Q_BN + 4;
constexpr int Q_LDS = (Q_RING * Q_STAGE > 128 * Q_LDT * 4) ? Q_RING * Q_STAGE : 128 * Q_LDT * 4;
static_assert(Q_LDS <= 160 * 1024, "q kernel LDS budget");
template <int V> using IC = std::integral_constant<int, V>;
// f(IC<0>) .. f(IC<N - 1>): a compile-time loop (a `#pragma unroll` loop around the barrier of a k-step stays rolled,
// which would index the accumulators at run time)
template <class F, int... I> DEV void q_seq(F& f, std::integer_sequence<int, I...>) { (f(IC<I>{}), ...); }
template <int N, class F> DEV void q_for(F f) { q_seq(f, std::make_integer_sequence<int, N>{}); }
}

// lgkmcnt(0) as the builtin (vmcnt 63, expcnt 7 = no wait): unlike the inline-asm wait_lgkm0(), the waitcnt pass sees
// it and clears its scoreboard, so it does not add its own lgkmcnt(0) behind the next fragment reads
DEV void q_wait_lgkm0() { __builtin_amdgcn_s_waitcnt(0xC07F); }

template <class LA, class LB, class EPI>
__global__ void __launch_bounds__(Q_THREADS, 1) igemm_q_kernel(LA la, LB lb, EPI epi, int KTILES, int split, int group) {
  static_assert(LA::ROWS == 256 && LB::ROWS == 256 && LA::NIW == 8 && LB::NIW == 8, "q kernel: 256-row loaders on 4 waves");
  static_assert(!LA::RELU && !LB::RELU, "q kernel: no ReLU-on-load (a VALU write of a fragment inside the MFMA stream)");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = wave_id();
  const int wm = wave >> 1, wn = wave & 1;
  int m0, n0;
  {
    int mt, nt_;
    tile_of_block(group, mt, nt_);
    m0 = mt * Q_BM; n0 = nt_ * Q_BN;
  }
  // split-K ranges stay in 64-deep K tiles (the ping-pong kernel's ranges: same partial sums per split); a tile is
  // two k-steps, the second all zeros where K % 64 <= 32
  const int per = (KTILES + split - 1) / split;
  const int kt0 = blockIdx.z * per, kt1 = min(KTILES, kt0 + per);
  const int ks0 = 2 * kt0, n = 2 * (kt1 - kt0);
  epi.prepare(blockIdx.z);
  // K-steps at or past klim (the end of this block's K range) are zero-filled by the range check, so EVERY k-step
  // issues its eight pieces and the counted wait is the same number in the prologue, in steady state and in the tail
  const int klim = min(la.K, (ks0 + n) * 32);
  KStep<LA> sa; KStep<LB> sb;
  sa.setup(la, m0, tid, klim);
  sb.setup(lb, n0, tid, klim);
  QFrag<LA::KCL> qa; QFrag<LB::KCL> qb;
  qa.init(smem, lane, wm);
  qb.init(smem + Q_IMG, lane, wn);
  f32x4 acc[8][8];
#pragma unroll
  for (int i = 0; i < 8; i++)
#pragma unroll
    for (int j = 0; j < 8; j++) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  bf16x8 fa[2][8], fb[2][8];
  // fragment f of a k-step: B blocks 0-7, then A blocks 0-7; st01 = the stage's place in the current pair of stages
  auto read_frag = [&](int buf, int st01, int f) {
    if (f < 8) fb[buf][f] = qb.read(st01, f);
    else fa[buf][f - 8] = qa.read(st01, f - 8);
  };
  // DMA piece d of k-step ks into a stage: A pieces 0-3, then B pieces 0-3
  auto dma_piece = [&](int ks, char* stage, int d) {
    if (d < 4) sa.piece(la, ks, stage, d);
    else sb.piece(lb, ks, stage + Q_IMG, d - 4);
  };
  // One k-step: ks = its index in K, stage = its own stage (restaged with k-step ks + 4), P = its place in its pair
  // of stages (0: the next k-step's fragments are in this pair's second stage; 1: in the other pair's first stage,
  // to which the fragment addresses are moved first: `flip` = +- 64 KB).
  // The MFMAs are inline asm with tied "+a" accumulators: with the builtin, the register allocator rotates the 64
  // accumulator tuples through VGPRs at the loop back-edge (180 v_accvgpr moves per K tile).  Inline asm is outside
  // the hazard recogniser, so the block covers its own hazards: s_nop 1 ahead of it (VALU write -> XDL SrcA/B read),
  // every fragment kept live to its end (no register of a fragment an in-flight MFMA still reads is reallocated
  // inside the block), the first read into the other buffer behind MFMA 3 and the barrier (the previous block's
  // MFMAs, which read that buffer, have all issued and read their sources by then), and s_nop 7 x 3 ahead of the
  // accumulator reads of the epilogue.
  constexpr int FPG = (LA::KCL || LB::KCL) ? 2 : 1;       // fragment reads per MFMA gap
  constexpr int D0 = 4 + 16 / FPG + 4, DS = 4;            // first DMA gap, gaps between pieces
  static_assert(D0 + 7 * DS < 64, "DMA pieces inside the block");
  auto kstep = [&](auto PC, int ks, char* stage, int flip) __attribute__((always_inline)) {
    constexpr int P = decltype(PC)::value;
    if constexpr (P == 1) { qa.flip(flip); qb.flip(flip); }
    q_wait_lgkm0();
    asm volatile("s_nop 1");
    q_for<64>([&](auto MC) __attribute__((always_inline)) {
      constexpr int m = decltype(MC)::value, i = m >> 3, j = m & 7;
      asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+a"(acc[i][j]) : "v"(fb[P][j]), "v"(fa[P][i]));
      if constexpr (m == 3) { wait_vmcnt<16>(); raw_barrier(); }
      if constexpr (m >= 4 && m < 4 + 16 / FPG) {
#pragma unroll
        for (int u = 0; u < FPG; u++) read_frag(P ^ 1, P ^ 1, (m - 4) * FPG + u);
      }
      if constexpr (m >= D0 && (m - D0) % DS == 0 && (m - D0) / DS < 8) dma_piece(ks + 4, stage, (m - D0) / DS);
      __builtin_amdgcn_sched_barrier(0);
    });
    asm volatile("" :: "v"(fa[P][0]), "v"(fa[P][1]), "v"(fa[P][2]), "v"(fa[P][3]),
                 "v"(fa[P][4]), "v"(fa[P][5]), "v"(fa[P][6]), "v"(fa[P][7]), "v"(fb[P][0]), "v"(fb[P][1]),
                 "v"(fb[P][2]), "v"(fb[P][3]), "v"(fb[P][4]), "v"(fb[P][5]), "v"(fb[P][6]), "v"(fb[P][7]));
  };
  if (n > 0) {
    // prologue: four stages (24 pieces stay in flight behind stage 0), then stage 0's fragments
#pragma unroll
    for (int q = 0; q < Q_RING; q++)
#pragma unroll
      for (int d = 0; d < 8; d++) dma_piece(ks0 + q, smem + q * Q_STAGE, d);
    wait_vmcnt<24>();
    raw_barrier();
#pragma unroll
    for (int f = 0; f < 16; f++) read_frag(0, 0, f);
    // one pair of stages (= one 64-deep K tile) per iteration; the pair alternates
    int pair = 0, flip = 2 * Q_STAGE;
    for (int s = 0; s < n; s += 2) {
      kstep(IC<0>{}, ks0 + s, smem + pair, flip);
      kstep(IC<1>{}, ks0 + s + 1, smem + pair + Q_STAGE, flip);
      pair ^= 2 * Q_STAGE; flip = -flip;
    }
  }
  asm volatile("s_nop 7\n\ts_nop 7\n\ts_nop 7" ::: "memory");   // XDL write -> accumulator read (epilogue)
  vm_drain();
  // stage the C tile (fp32) through LDS in two 128-row halves: waves wm = h write half h
  float* ct = (float*)smem;
#pragma unroll
  for (int h = 0; h < 2; h++) {
    lds_barrier();
    if (wm == h) {
#pragma unroll
      for (int i = 0; i < 8; i++)
#pragma unroll
        for (int j = 0; j < 8; j++) {
          const int r = i * 16 + (lane & 15), c = wn * 128 + j * 16 + (lane >> 4) * 4;
          *(f32x4*)(ct + r * Q_LDT + c) = acc[i][j];
        }
    }
    lds_barrier();
    epi(ct, Q_LDT, m0 + h * 128, n0, tid, 128, Q_BN, Q_THREADS);
  }
}

template <class LA, class LB, class EPI>
int launch_igemm_q(LA la, LB lb, EPI epi, int M, int N, int KTILES, int split, int zdim_extra, hipStream_t st) {
  if (!la.buf_ok() || !lb.buf_ok()) {
    s3od_set_error("igemm_q: operand window too large for a buffer descriptor");
    return 22;
  }
  auto kfn = igemm_q_kernel<LA, LB, EPI>;
  static const bool attr = ((void)hipFuncSetAttribute((const void*)kfn, hipFuncAttributeMaxDynamicSharedMemorySize, Q_LDS), true);
  (void)attr;
  dim3 grid(cdiv(N, Q_BN), cdiv(M, Q_BM), split * zdim_extra);
  const int group = S3OD_KNOB("S3OD_GEMM_GROUP", 0);
  hipLaunchKernelGGL(kfn, grid, dim3(Q_THREADS), Q_LDS, st, la, lb, epi, KTILES, split, group);
  return s3od_check_launch("igemm_q");
}

// the (loader, epilogue) combinations the linears use (linear_ops.hip: s3od_linear_fwd / _dgrad / _wgrad)
typedef DenseKC<bf16, 256, 4> QKC;
typedef DenseMC<bf16, 256, 4> QMC;
template int launch_igemm_q<QKC, QKC, EpiStd<bf16, bf16, bf16>>(QKC, QKC, EpiStd<bf16, bf16, bf16>, int, int, int, int, int, hipStream_t);
template int launch_igemm_q<QKC, QKC, EpiStd<float, float, bf16>>(QKC, QKC, EpiStd<float, float, bf16>, int, int, int, int, int, hipStream_t);
template int launch_igemm_q<QKC, QKC, EpiStd<float, bf16, bf16>>(QKC, QKC, EpiStd<float, bf16, bf16>, int, int, int, int, int, hipStream_t);
template int launch_igemm_q<QKC, QKC, EpiStd<bf16, float, bf16>>(QKC, QKC, EpiStd<bf16, float, bf16>, int, int, int, int, int, hipStream_t);
template int launch_igemm_q<QKC, QMC, EpiStd<bf16, bf16, bf16>>(QKC, QMC, EpiStd<bf16, bf16, bf16>, int, int, int, int, int, hipStream_t);
template int launch_igemm_q<QKC, QMC, EpiStd<float, float, float>>(QKC, QMC, EpiStd<float, float, float>, int, int, int, int, int, hipStream_t);
template int launch_igemm_q<QMC, QMC, EpiWgradPart>(QMC, QMC, EpiWgradPart, int, int, int, int, int, hipStream_t);
template int launch_igemm_q<QMC, QMC, EpiWgrad>(QMC, QMC, EpiWgrad, int, int, int, int, int, hipStream_t);
