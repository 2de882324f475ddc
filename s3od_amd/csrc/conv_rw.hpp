// What the hand-pipelined conv kernels of gemm_ops.hip and wgrad_dma.hip share: the tile schedules, the LDS-DMA halo
// ring with its counted wait, the double-buffered MFMA step loop, the store / column-sum / weight-gradient epilogues
// and the host launch helper.
#pragma once
#include "gemm.hpp"
#include "conv_kernels.hpp"

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) char lds_char;
// Transposed 16 x 32 fragment (rows = K) at a per-lane LDS address: the low 16 rows there, the high 16 rows HI bytes on
template <int HI> DEV bf16x8 trf_at(const lds_char* a) { return read_tr_pair((const char*)a, (const char*)a + HI); }

// ---------------------------------------------------------------- tile schedules
struct TileAt { int txi, tyi, bb; };
DEV TileAt tile_at(int tile, int tiles_x, int tiles_y) {           // row-major: x fastest
  const int t2 = tile / tiles_x;
  return {tile % tiles_x, t2 % tiles_y, t2 / tiles_y};
}
// y fastest (the LDS-DMA weight gradients): a workgroup's consecutive tiles walk DOWN a column of tiles, so each halo
// shares its top 2 rows with the previous tile's (read moments ago: L2) -- 8 of 10 halo rows per tile from HBM
// instead of 10 (3x3), 4 of 6 (4x4 s2)
DEV TileAt tile_at_ymaj(int tile, int tiles_x, int tiles_y) {
  const TileAt t = tile_at(tile, tiles_y, tiles_x);
  return {t.tyi, t.txi, t.bb};
}
// Register-weight kernels, one persistent workgroup per CU: XCD x = blockIdx % 8 owns the contiguous range
// [x n / 8, (x+1) n / 8) (neighbouring tiles share halo rows in that XCD's L2); its workgroups stride through it
struct PersistentTiles {
  int beg, end, first, stride;
  DEV PersistentTiles(int ntiles) {
    const int xcd = blockIdx.x & 7;
    stride = ((int)gridDim.x + 7 - xcd) >> 3;
    beg = (int)((long)ntiles * xcd / 8), end = (int)((long)ntiles * (xcd + 1) / 8);
    first = beg + ((int)blockIdx.x >> 3);
  }
};
// Weight-gradient kernels: a workgroup owns the channel block (co0 .. co0+CO) x (ci0 .. ci0+64) of a CoT x CinT conv;
// the wpc workgroups of one block split the tiles into contiguous ranges (neighbouring tiles share halo rows)
struct ChannelBlock {
  int co0, ci0, t_beg, t_end;
  DEV ChannelBlock(int CO, int ntiles, int nci, int wpc) {
    const int combo = blockIdx.x / wpc, wi = blockIdx.x - combo * wpc;
    co0 = (combo / nci) * CO, ci0 = (combo % nci) * 64;
    t_beg = (int)((long)ntiles * wi / wpc), t_end = (int)((long)ntiles * (wi + 1) / wpc);
  }
};

// ---------------------------------------------------------------- halo ring
// A 3-deep ring of input halos, G::PX pixels in rows of G::HC, G::ROWB LDS bytes each (G::CHUNKS real 16-B chunks of a
// global pixel of G::GPIX bytes, the rest padding), filled by LDS-DMA in G::PIECES pieces of 1 KiB, G::PPW per wave.
// Piece p = PPW wave + i covers LDS bytes [1024 p, 1024 p + 1024) of a ring slot, laid out [px][16-B slot]; a lane
// writes bytes 16 lane .. +15 of the piece = logical chunk G::slot^-1 (an involution) of pixel px.
// The counted waits (ring_wait) need every wave to issue exactly PPW vector-memory instructions per call, so
//   * a dummy piece (padding, the tail past the halo, a pixel outside the image) uses the out-of-range offset and
//     reads zeros through the buffer range check, never a branch;
//   * live == false (no tile left: zeros into a free slot) issues the same PPW pieces.
template <class G> struct HaloRing {
  int dm[G::PPW];                                      // (halo row << 16) | (halo column << 4) | chunk, -1 = dummy
  char* base;                                          // this wave's pieces of slot 0
  DEV HaloRing(char* smem, int wave, int lane) : base(smem + wave * G::PPW * 1024) {
#pragma unroll
    for (int i = 0; i < G::PPW; i++) {
      const unsigned b = (wave * G::PPW + i) * 1024 + lane * 16, px = b / G::ROWB, c = (b % G::ROWB) >> 4;
      dm[i] = (px < G::PX && c < G::CHUNKS) ? (int)(((px / G::HC) << 16) | ((px % G::HC) << 4) | G::slot(c, px)) : -1;
    }
  }
  // the halo whose pixel (0, 0) is (y0, x0) of the Hi x Wi image behind r
  DEV void issue(__amdgpu_buffer_rsrc_t r, int y0, int x0, int Hi, int Wi, bool live, int slot) const {
    char* dst = base + slot * G::BUF;
#pragma unroll
    for (int i = 0; i < G::PPW; i++) {
      const int v = dm[i], gy = y0 + (v >> 16), gx = x0 + ((v >> 4) & 0xfff);
      const bool ok = live && v >= 0 && (unsigned)gy < (unsigned)Hi && (unsigned)gx < (unsigned)Wi;
      blds16(r, ok ? (unsigned)((gy * Wi + gx) * G::GPIX + (v & 15) * 16) : 0x80000000u, dst + i * 1024);
    }
  }
};
// Retires tile k's halo (the wave's own pieces) and meets the other waves: every wave's pieces landed, every wave is
// done with slot k - 1, which the caller refills next.  Per tile a wave issues, in this order, NM mask loads, the
// PPW pieces of the halo two tiles on and NS stores, after the halos of tiles 0 and 1 up front; so the vector-memory
// instructions younger than tile k's pieces, which may stay in flight, are a per-phase constant:
//   k = 0: halo 1, masks 0;   k = 1: masks 0, halo 2, stores 0, masks 1;
//   k >= 2: stores k-2, masks k-1, halo k+1, stores k-1, masks k (tile k's pieces went out in the middle of tile k-2)
template <int PPW, int NS, int NM> DEV void ring_wait(int k) {
  if (k == 0) wait_vmcnt<PPW + NM>();
  else if (k == 1) wait_vmcnt<NM + PPW + NS + NM>();
  else wait_vmcnt<NS + NM + PPW + NS + NM>();
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}

// ---------------------------------------------------------------- MFMA step loop
// NST steps of rd(step, fragments[N]) / mm(step, fragments[N]), double-buffered: the next step's fragments are read
// before this step's MFMAs; between(pair) runs after the MFMAs of each pair's first step
template <int NST, int N, class RD, class MM, class BT> DEV void rw_steps(RD rd, MM mm, BT between) {
  bf16x8 fa0[N], fa1[N];
  rd(0, fa0);
#pragma unroll
  for (int st = 0; st < NST; st += 2) {
    if (st + 1 < NST) rd(st + 1, fa1);
    __builtin_amdgcn_sched_barrier(0);
    mm(st, fa0);
    between(st / 2);
    __builtin_amdgcn_sched_barrier(0);
    if (st + 2 < NST) rd(st + 2, fa0);
    __builtin_amdgcn_sched_barrier(0);
    if (st + 1 < NST) mm(st + 1, fa1);
    __builtin_amdgcn_sched_barrier(0);
  }
}
template <int NST, int N, class RD, class MM> DEV void rw_steps(RD rd, MM mm) {
  rw_steps<NST, N>(rd, mm, [](int) {});
}

// ---------------------------------------------------------------- epilogues
// One 16-px block: a lane holds out[px][co = ch0 + 16 nb + 4 lg .. +3] in a0 (nb 0) and a1 (nb 1).  v_permlane16_swap
// trades rows 1 / 3 of the first operand with rows 0 / 2 of the second (row = 16 lanes = one lg): the even lg keeps
// its nb 0 and receives the odd partner's nb 0, the odd lg keeps nb 1 and receives the even's, so the lane owns the
// 8 channels cb = ch0 + 16 (lg & 1) + 8 (lg >> 1) .. +7: edit(o) (mask, sum), pack to bf16, one 16-B store at p
template <bool RELU, class F>
DEV void trade_store8(const f32x4& a0, const f32x4& a1, __amdgpu_buffer_rsrc_t r, unsigned p, F edit) {
  float o[8];
#pragma unroll
  for (int e = 0; e < 4; e++) {
    float v0 = a0[e], v1 = a1[e];
    if (RELU) { v0 = fmaxf(v0, 0.f); v1 = fmaxf(v1, 0.f); }
    const auto sw = __builtin_amdgcn_permlane16_swap(__float_as_uint(v0), __float_as_uint(v1), false, false);
    o[e] = __uint_as_float(sw[0]);                 // channels cb + 0..3
    o[4 + e] = __uint_as_float(sw[1]);             // channels cb + 4..7
  }
  edit(o);
  bf16x8 ob;
#pragma unroll
  for (int e = 0; e < 8; e++) ob[e] = (bf16)o[e];
  __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, ob), r, p, 0, 0);
}
template <bool RELU> DEV void trade_store8(const f32x4& a0, const f32x4& a1, __amdgpu_buffer_rsrc_t r, unsigned p) {
  trade_store8<RELU>(a0, a1, r, p, [](float (&)[8]) {});
}
// Column sums of the NCH output channels: cs = a lane's partials of channels cb .. cb+7; 16 lanes (lr) -> 1, LDS
// atomics into the zeroed aux, one global add per channel and workgroup
template <int NCH> DEV void flush_colsum(const float (&cs)[8], float* aux, float* colsum, int cb) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int e = 0; e < 8; e++) {
    float c = cs[e];
    c += __shfl_xor(c, 1); c += __shfl_xor(c, 2); c += __shfl_xor(c, 4); c += __shfl_xor(c, 8);
    if ((tid & 15) == 0) atomicAdd(aux + cb + e, c);
  }
  __syncthreads();
  if (tid < NCH) atomicAdd(colsum + tid, aux[tid]);
}
// Weight-gradient partial sums -> the [co][tap][ci] fp32 workspace (wgrad_permute_add_kernel follows): the lane holds
// D[co = co0 + 16 cb + 4 g + r][ci = ci0 + 16 cib + li] of tap `tap`, where 4 tap + cib = pair0 + step j for accumulator row j
// (GUARD: CoT = 96 in 64-channel blocks, the second block's top half is padding)
template <int TAPS, bool GUARD, int NP, int NCO>
DEV void flush_wgrad(const f32x4 (&acc)[NP][NCO], float* ws, int co0, int ci0, int CinT, int CoT, int lane, int pair0, int step) {
  const int g = lane >> 4, li = lane & 15;
#pragma unroll
  for (int j = 0; j < NP; j++) {
    const int pr = pair0 + step * j, tap = pr >> 2, cib = pr & 3;
#pragma unroll
    for (int cb = 0; cb < NCO; cb++)
#pragma unroll
      for (int r = 0; r < 4; r++)
        if (!GUARD || co0 + cb * 16 + 4 * g + r < CoT)
          atomicAdd(ws + (long)(co0 + cb * 16 + 4 * g + r) * (TAPS * CinT) + tap * CinT + ci0 + cib * 16 + li, acc[j][cb][r]);
  }
}

// ---------------------------------------------------------------- host
// The two grid policies: one persistent workgroup per CU over the XCD ranges (>= 8, so every XCD owns its range), or
// wpc workgroups for each of nblk channel blocks (one per CU over all blocks: each block gets ~CUs / nblk of them)
static inline int grid_xcd(long tiles) { return (int)std::min<long>(std::max<long>(tiles, 8), (long)s3od_cu_count()); }
static inline int grid_wpc(long tiles, int nblk) {
  return (int)std::max<long>(1, std::min<long>(tiles, std::max(1, s3od_cu_count() / nblk)));
}
// Launches KFN on nwg workgroups of NT threads with LDS bytes of dynamic shared memory (the attribute is set once per
// process and instantiation: thread-safe static init); the kernels take the tile count as an int
template <auto KFN, int LDS, int NT, class... A>
static int launch_tiled(const char* what, const char* too_many, long tiles, int nwg, hipStream_t st, A... args) {
  static const bool attr = ((void)hipFuncSetAttribute((const void*)KFN, hipFuncAttributeMaxDynamicSharedMemorySize, LDS), true);
  (void)attr;
  if (tiles >= (1L << 31)) { s3od_set_error(too_many); return 22; }
  hipLaunchKernelGGL(KFN, dim3(nwg), dim3(NT), LDS, st, args...);
  return s3od_check_launch(what);
}
