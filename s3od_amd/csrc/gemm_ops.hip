// Hand-pipelined conv kernels with counted vmcnt waits (their shared parts are in conv_rw.hpp):
//   conv3x3_c64_rw_kernel      register-weight 3x3 s1 convs: forward (+ ReLU), ReLU'-masked data gradient, mask heads
//   convT4s2_rw_kernel         register-weight ConvTranspose2d(128, 64, 4, s2, p1), sub-pixel forward
//   conv4s2_rw_kernel          its data gradient, the strided Conv2d(64, 128, 4, s2, p1)
//   conv3x3_wgrad_halo_kernel  register-staged halo-tile 3x3 weight gradient
//   conv4s2_wgrad_dma_kernel   LDS-DMA weight gradient of the 4x4 s2 conv view
// with their launchers and shape predicates (declared in conv_kernels.hpp; the entries that route to them are in
// conv_ops.hip).
#include "conv_rw.hpp"

// ---------------------------------------------------------------- register-weight 3x3 conv, 64 -> 64
// The full-resolution 64-channel convs (upsample_2x.2 forward and its stride-1 data gradient) move
// 4.3 / 6.4 GB per call at bs 16 (1024^2): HBM-bound at ~5.5 TB/s if loads, MFMAs and stores overlap.
//   * one workgroup of 4 waves per CU (one wave per SIMD); wave w = output rows 4 (w>>1) .. +3 of the
//     tile x output channels 32 (w&1) .. +31 and holds those channels' 9 taps x 64 weights as MFMA A
//     fragments in registers (144 VGPRs), so the only LDS traffic is the input halo (B fragments);
//   * tile = 8 x 32 output pixels; its (8+2) x (32+2) x 64 halo arrives by LDS-DMA (44 x 1 KiB pieces,
//     11 per wave, zeros outside the image via the buffer range check) into a 3-deep ring, issued two
//     tiles ahead, so the only per-tile synchronisation is one s_barrier behind a counted vmcnt;
//   * the epilogue runs from the accumulators: bias / ReLU (forward) or the ReLU' mask of res1 (data
//     gradient, its rows loaded at the start of the tile), the lane pair (lg, lg^1) trades 4-channel
//     groups so every lane stores one 16-B run of 8 channels per 16-pixel block; column sums of the
//     output (bias gradient) go through LDS atomics, one global flush per workgroup.
// Input channels CI = 64 (tile 8 x 32) or 96 (the mask heads' data gradient: tile 8 x 16, 192-B halo rows).
template <int CI> struct RwShape {
  static constexpr int TH = 8, TW = CI == 64 ? 32 : 16, HC = TW + 2, PX = (TH + 2) * HC;   // halo pixels
  static constexpr int ROWB = CI * 2, CHUNKS = CI / 8, GPIX = ROWB;                       // LDS row = global pixel
  static constexpr int KK = CI / 32, NPC = TW / 16, PB = 4 * NPC;                         // 16-px blocks per wave
  static constexpr int PIECES = ((PX * ROWB + 4095) / 4096) * 4, PPW = PIECES / 4;        // 1 KiB DMA pieces
  static constexpr int BUF = PIECES * 1024, LDS = 3 * BUF + 2048;       // + bias / column sums / head partials
  static_assert(LDS <= 160 * 1024, "register-weight conv LDS budget");
  // 16-B slot of logical chunk c in halo row px (an involution; conflict-free ds_read_b128 for every tap offset,
  // checked against the gfx950 lane groups): CI 64: c ^ (px & 7); CI 96: XOR of the low 2 bits, groups of 4 kept
  DEV static int slot(int c, int px) {
    if constexpr (CI == 64) return c ^ (px & 7);
    else return (c & ~3) | ((c & 3) ^ ((px ^ (px >> 1)) & 3));
  }
};

// MODE 0: out = acc + bias;  MODE 2: out = ReLU(acc + bias);  MODE 1: out = res1 > 0 ? acc : 0, colsum += out;
// MODE 3: the 3 mask heads (src/s3od/model.py:440-452,461-467): 96 output channels (48 per wave, NB = 3),
//   h = ReLU(acc + b1) -> hsave (bf16 [px][96]) and logit_k = b2[k] + h[32k .. 32k+31] . w2[k] -> logits [B][3][H][W];
//   head 1 straddles the two waves of a row group: the odd wave's part goes through LDS (one extra barrier)
// Every wave issues a FIXED sequence of vector-memory instructions per tile (PB mask loads, PPW DMA pieces, PB stores:
// dummy pieces / out-of-image lanes use an out-of-range buffer offset instead of a branch), so the counted vmcnt
// that retires a tile's halo is a per-phase constant (ring_wait).
// The tile's PB blocks run in groups (all 9 * KK steps of one group's accumulators, then the next group's).
// GB = 0 (mode 1, see conv3x3_rw_dgrad_launch, and mode 3): one group of PB blocks, its epilogue at once.
// GB > 0 (MODE 0 / 2): groups of GB blocks, and each group's epilogue (ReLU, lane-pair trade, pack, store) is issued between the
// NEXT group's MFMAs -- the last group's carried into the next tile's first group (a dummy group with out-of-range
// stores before the first tile) -- so with one wave per SIMD the matrix pipe no longer idles through the epilogue.
// Same MFMA chain per accumulator (outputs bit-identical to GB = 0); per tile still PB stores after the halo issue,
// so the counted waits are unchanged.
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
template <int MODE, int CI, int GB>
__global__ void __launch_bounds__(256, 1) conv3x3_c64_rw_kernel(const bf16* __restrict__ x, const bf16* __restrict__ w,
                                                                 const float* __restrict__ bias,
                                                                 const bf16* __restrict__ res1, float* __restrict__ colsum,
                                                                 bf16* __restrict__ out, int H, int W, int tiles_x,
                                                                 int tiles_y, int ntiles, const float* __restrict__ w2,
                                                                 const float* __restrict__ b2, float* __restrict__ logits) {
  typedef RwShape<CI> S;
  constexpr int PB = S::PB, PPW = S::PPW, NPC = S::NPC, HC = S::HC, ROWB = S::ROWB;
  constexpr int NB = MODE == 3 ? 3 : 2, CO = 32 * NB;     // 16-channel blocks per wave / output channels
  static_assert(MODE != 3 || (CI == 64 && NPC == 2), "mask heads: 64 input channels, 8 x 32 tiles");
  static_assert(GB == 0 || ((MODE == 0 || MODE == 2) && PB % GB == 0), "grouped epilogue: whole groups, forward only");
  extern __shared__ __attribute__((aligned(1024))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = wave_id();
  const int lr = lane & 15, lg = lane >> 4, odd = lg & 1;
  const int row0 = 4 * (wave >> 1), ch0 = 16 * NB * (wave & 1);   // this wave's output rows / channels
  const PersistentTiles pt(ntiles);
  const long img_i = (long)H * W * CI, img_o = (long)H * W * CO;    // elements per image

  // weights -> registers: lane (lr, lg) holds w[co = ch0 + 16 nb + lr][tap][ci = 32 kk + 8 lg .. +7]
  bf16x8 wr[9][S::KK][NB];
#pragma unroll
  for (int tap = 0; tap < 9; tap++)
#pragma unroll
    for (int kk = 0; kk < S::KK; kk++)
#pragma unroll
      for (int nb = 0; nb < NB; nb++)
        wr[tap][kk][nb] = *(const bf16x8*)(w + ((long)(ch0 + nb * 16 + lr) * 9 + tap) * CI + kk * 32 + lg * 8);

  const HaloRing<S> ring(smem, wave, lane);
  auto issue = [&](int tile, int slot) {            // tile >= pt.end: dummy pieces (zeros into a free slot)
    const bool live = tile < pt.end;
    const TileAt t = tile_at(live ? tile : pt.beg, tiles_x, tiles_y);
    ring.issue(make_rsrc(x + t.bb * img_i, (unsigned long)img_i * 2), t.tyi * S::TH - 1, t.txi * S::TW - 1, H, W, live, slot);
  };
  // halo fragment addresses: px = L + off (L = row0 * HC + lr per lane, off compile-time per (block, tap)); the
  // slot term depends on the lane and on off & 7 only, so yb[off & 7][kk] + ROWB * off = per-lane base + immediate
  int yb[8][S::KK];
  {
    const int L = row0 * HC + lr;
#pragma unroll
    for (int j = 0; j < 8; j++)
#pragma unroll
      for (int kk = 0; kk < S::KK; kk++) yb[j][kk] = L * ROWB + 16 * S::slot(kk * 4 + lg, L + j);
  }
  // after the lane-pair trade in the epilogue a lane owns channels cb .. cb+7 of its pixel
  const int cb = ch0 + (odd ? 16 : 0) + 8 * (lg >> 1);
  // 64 floats after the ring: the bias (MODE 0/2, the accumulators' initial value) or the column sums (MODE 1)
  // MODE 3: aux[0..95] = b1, aux[96..191] = w2, aux[192..194] = b2, aux[256..511] = head-1 partials [8 rows][32 px]
  float* aux = (float*)(smem + 3 * S::BUF);
  if (tid < CO) aux[tid] = (MODE != 1 && bias) ? bias[tid] : 0.f;
  if constexpr (MODE == 3) {
    if (tid < 96) aux[96 + tid] = w2[tid];
    if (tid < 3) aux[192 + tid] = b2[tid];
  }
  __syncthreads();
  float cs[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};

  // GB > 0: the carried group (accumulators, store offsets, batch index); a dummy before the first tile
  constexpr int GBC = GB > 0 ? GB : 1;
  f32x4 cacc[GBC][NB];
  unsigned cpo[GBC];
#pragma unroll
  for (int q = 0; q < GBC; q++) {
    cpo[q] = 0x80000000u;
#pragma unroll
    for (int nb = 0; nb < NB; nb++) cacc[q][nb] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  int cbb = 0;                                        // batch index of the carried group's tile
  // epilogue of one 16-px block (trade_store8; mode 1: the ReLU' mask, out-of-image lanes read 0, and the column sums)
  // (the output descriptor is built here from the batch index: in a round-5 build a descriptor carried across tiles
  // in SGPRs lost its range word in the grouped mode-1 instance, whose in-tile group stores were dropped)
  auto epi_blk = [&](const f32x4 (&a)[NB], unsigned p, int bbx, u32x4 mraw = u32x4{0u, 0u, 0u, 0u}) {
    const auto r = make_rsrc(out + bbx * img_o, out ? (unsigned long)img_o * 2 : 0ul);
    trade_store8<MODE == 2>(a[0], a[1], r, p, [&](float (&o)[8]) {
      if constexpr (MODE == 1) {
        const bf16x8 m = __builtin_bit_cast(bf16x8, mraw);
#pragma unroll
        for (int e = 0; e < 8; e++) o[e] = (float)m[e] > 0.f ? o[e] : 0.f;
#pragma unroll
        for (int e = 0; e < 8; e++) cs[e] += o[e];
      }
    });
  };

  int k = 0;
  issue(pt.first, 0);
  issue(pt.first + pt.stride, 1);
  for (int tile = pt.first; tile < pt.end; tile += pt.stride, k++) {
    const TileAt t = tile_at(tile, tiles_x, tiles_y);
    unsigned po[PB];                                  // byte offset of this lane's 8-channel run per 16-px block (or OOB)
#pragma unroll
    for (int pb = 0; pb < PB; pb++) {
      const int gy = t.tyi * S::TH + row0 + pb / NPC, gx = t.txi * S::TW + (pb % NPC) * 16 + lr;
      po[pb] = (gy < H && gx < W) ? (unsigned)((gy * W + gx) * (CO * 2) + cb * 2) : 0x80000000u;
    }
    // data-gradient mask runs of this tile, issued before the next halo's DMA (their wait leaves it in flight)
    u32x4 rm_[PB];
    if constexpr (MODE == 1) {
      const auto rr = make_rsrc(res1 + t.bb * img_o, (unsigned long)img_o * 2);
#pragma unroll
      for (int pb = 0; pb < PB; pb++) rm_[pb] = __builtin_amdgcn_raw_buffer_load_b128(rr, po[pb], 0, 0);
    }
    // stores per tile: PB, or (MODE 3) 2 PB hsave runs + 8 logit rows = 3 PB; mask loads: PB (MODE 1)
    ring_wait<PPW, MODE == 3 ? 3 * PB : PB, MODE == 1 ? PB : 0>(k);
    issue(tile + 2 * pt.stride, (k + 2) % 3);
    const char* hb = smem + (k % 3) * S::BUF;
    constexpr int G = GB > 0 ? GB : PB;               // blocks per group
#pragma unroll
    for (int gi = 0; gi < PB / G; gi++) {
      f32x4 acc[G][NB];                               // acc[q][nb]: D[co = ch0 + 16 nb + 4 lg + e][px = block gi G + q, lr]
#pragma unroll
      for (int nb = 0; nb < NB; nb++) {
        const f32x4 b0 = MODE != 1 ? *(const f32x4*)(aux + ch0 + nb * 16 + 4 * lg) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int q = 0; q < G; q++) acc[q][nb] = b0;
      }
      // 9 * KK (tap, k-chunk) steps of G x NB MFMAs on the group's G halo fragments; the carried group's epilogue in
      // the first GB step pairs
      auto rd = [&](int st, bf16x8 (&fa)[G]) {
        const int tap = st / S::KK, kk = st % S::KK, dy = tap / 3, dx = tap - 3 * (tap / 3);
#pragma unroll
        for (int q = 0; q < G; q++) {
          const int pb = gi * G + q, off = (pb / NPC + dy) * HC + (pb % NPC) * 16 + dx;
          fa[q] = *(const bf16x8*)(hb + yb[off & 7][kk] + off * ROWB);
        }
      };
      auto mm = [&](int st, const bf16x8 (&fa)[G]) {
#pragma unroll
        for (int q = 0; q < G; q++)
#pragma unroll
          for (int nb = 0; nb < NB; nb++)
            acc[q][nb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wr[st / S::KK][st % S::KK][nb], fa[q], acc[q][nb], 0, 0, 0);
      };
      rw_steps<9 * S::KK, G>(rd, mm, [&](int pair) {
        if constexpr (GB > 0) { if (pair < GB) epi_blk(cacc[pair], cpo[pair], cbb); }
      });
      if constexpr (GB > 0) {
#pragma unroll
        for (int q = 0; q < GB; q++) {
#pragma unroll
          for (int nb = 0; nb < NB; nb++) cacc[q][nb] = acc[q][nb];
          cpo[q] = po[gi * GB + q];
        }
        cbb = t.bb;
      } else if constexpr (MODE == 3) {
        const auto ro = make_rsrc(out + t.bb * img_o, out ? (unsigned long)img_o * 2 : 0ul);   // hsave is optional
        // h = ReLU(acc) (b1 was the initial value); hsave: channels cb .. cb+7 (nb 0 / 1, trade_store8) and
        // ch0 + 32 + 4 lg .. +3 (nb 2); head partials: per 16-channel block, summed over the 4 lg lanes
        float hp[PB][3];
#pragma unroll
        for (int pb = 0; pb < PB; pb++) {
          float v[3][4];
#pragma unroll
          for (int nb = 0; nb < 3; nb++)
#pragma unroll
            for (int e = 0; e < 4; e++) v[nb][e] = fmaxf(acc[pb][nb][e], 0.f);
          trade_store8<true>(acc[pb][0], acc[pb][1], ro, po[pb]);
          const unsigned p2 = po[pb] == 0x80000000u ? po[pb] : po[pb] - cb * 2 + (ch0 + 32 + 4 * lg) * 2;
          const bf16x4 o2 = {(bf16)v[2][0], (bf16)v[2][1], (bf16)v[2][2], (bf16)v[2][3]};
          __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, o2), ro, p2, 0, 0);
#pragma unroll
          for (int nb = 0; nb < 3; nb++) {
            float d = 0.f;
#pragma unroll
            for (int e = 0; e < 4; e++) d += v[nb][e] * aux[96 + ch0 + 16 * nb + 4 * lg + e];
            d += __shfl_xor(d, 16);
            d += __shfl_xor(d, 32);
            hp[pb][nb] = d;
          }
        }
        // wave half 0 (channels 0-47): head 0 = blocks 0 + 1, head 1 = block 2 + the odd wave's block 0;
        // half 1 (48-95): head 2 = blocks 1 + 2
        float* part = aux + 256 + (row0 + 0) * 32;
        if (wave & 1) {
#pragma unroll
          for (int pb = 0; pb < PB; pb++)
            if (lg == 0) part[(pb / NPC) * 32 + (pb % NPC) * 16 + lr] = hp[pb][0];
        }
        lds_barrier();
        const auto rl = make_rsrc(logits + (long)t.bb * 3 * H * W, (unsigned long)3 * H * W * 4);
#pragma unroll
        for (int r = 0; r < 4; r++) {
          // lanes lg 0 / 1 store the row's two 16-pixel blocks (64 + 64 contiguous bytes); lg 2 / 3 are out of range
          const int gy = t.tyi * S::TH + row0 + r, gx = t.txi * S::TW + (lg & 1) * 16 + lr;
          const bool ok = lg < 2 && gy < H && gx < W;
          const unsigned base = (unsigned)(gy * W + gx) * 4;
          if (!(wave & 1)) {
            const float l0 = aux[192] + hp[2 * r][0] + hp[2 * r][1], l0b = aux[192] + hp[2 * r + 1][0] + hp[2 * r + 1][1];
            const float l1 = aux[193] + hp[2 * r][2] + part[r * 32 + lr], l1b = aux[193] + hp[2 * r + 1][2] + part[r * 32 + 16 + lr];
            __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint((lg & 1) ? l0b : l0), rl, ok ? base : 0x80000000u, 0, 0);
            __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint((lg & 1) ? l1b : l1), rl, ok ? base + (unsigned)H * W * 4 : 0x80000000u, 0, 0);
          } else {
            const float l2 = aux[194] + hp[2 * r][1] + hp[2 * r][2], l2b = aux[194] + hp[2 * r + 1][1] + hp[2 * r + 1][2];
            __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint((lg & 1) ? l2b : l2), rl, ok ? base + 2u * H * W * 4 : 0x80000000u, 0, 0);
            __builtin_amdgcn_raw_buffer_store_b32(0u, rl, 0x80000000u, 0, 0);   // keeps the per-tile store count uniform
          }
        }
      } else {
#pragma unroll
        for (int pb = 0; pb < PB; pb++) epi_blk(acc[pb], po[pb], t.bb, rm_[pb]);
      }
    }
  }
  if constexpr (GB > 0) {                             // the last tile's carried group
#pragma unroll
    for (int q = 0; q < GB; q++) epi_blk(cacc[q], cpo[q], cbb);
  }
  if (MODE == 1 && colsum) flush_colsum<64>(cs, aux, colsum, cb);
  wait_vmcnt<0>();        // no LDS-DMA (dummy pieces included) may still be landing when the workgroup retires
}

// S3OD_CONV_RW=0 disables the path (an A/B inside one process under S3OD_AB=1)
bool rw_ok(int dtype, int B, int H, int W) {
  return dtype == S3OD_BF16 && !S3OD_OFF("S3OD_CONV_RW") && (long)H * W * 192 < (1L << 31) && B > 0;
}
template <int MODE, int CI, int GB>
static int launch_rw_g(const bf16* x, const bf16* w, const float* bias, const bf16* res1, float* colsum, bf16* out,
                       int B, int H, int W, hipStream_t st, const float* w2, const float* b2, float* logits) {
  typedef RwShape<CI> S;
  const int tx = cdiv(W, S::TW), ty = cdiv(H, S::TH);
  const long tiles = (long)B * tx * ty;
  return launch_tiled<conv3x3_c64_rw_kernel<MODE, CI, GB>, S::LDS, 256>(
      "conv3x3_c64_rw", "conv rw: too many tiles", tiles, grid_xcd(tiles), st, x, w, bias, res1, colsum, out, H, W, tx, ty,
      (int)tiles, w2, b2, logits);
}
// modes 0 / 2 (forward): the grouped epilogue (S3OD_RW_GB = blocks per group: 2 default, or 0 = the epilogue after all
// MFMAs).  Measured (tools/conv64_bench.py, bs 16 x 1024^2 64 -> 64 + ReLU, same box): GB 0 1290-1309 us, GB 2 1225-1242,
// GB 4 1251-1280 (profiles/r05t_rw_grouped_epilogue.txt; GB 4 removed in round 6).
int conv3x3_rw_launch(bool relu, const bf16* x, const bf16* w, const float* bias, bf16* out, int B, int H, int W,
                      hipStream_t st) {
  const bool grouped = S3OD_KNOB("S3OD_RW_GB", 2) == 2;
  auto go = grouped ? (relu ? launch_rw_g<2, 64, 2> : launch_rw_g<0, 64, 2>) : (relu ? launch_rw_g<2, 64, 0> : launch_rw_g<0, 64, 0>);
  return go(x, w, bias, nullptr, nullptr, out, B, H, W, st, nullptr, nullptr, nullptr);
}
// Mode 1 (the ReLU'-masked data gradient) runs ungrouped: its grouped instances were the only register-weight convs
// that spill (GB 2: 62 SGPRs into VGPR lanes + 6 VGPRs into AGPRs; GB 4: 40 + 16), and GB 4 produced wrong outputs
// (in-tile group stores dropped / masks misapplied) although its vector-memory order matches the hand-counted waits
// (ISA audit); GB 2 saved only 60-110 us per step.  tests/test_kernel_resources_cpu.py keeps every
// counted-vmcnt production kernel free of scratch and VGPR spills.
int conv3x3_rw_dgrad_launch(int Cout, const bf16* dy, const bf16* wT, const bf16* res1, float* colsum, bf16* dx, int B,
                            int H, int W, hipStream_t st) {
  auto go = Cout == 64 ? launch_rw_g<1, 64, 0> : launch_rw_g<1, 96, 0>;
  return go(dy, wT, nullptr, res1, colsum, dx, B, H, W, st, nullptr, nullptr, nullptr);
}
// Mode 3 (the mask heads) runs ungrouped too: grouped by output row it was bit-identical but slower, 2160-2174 ->
// 2421-2424 us at bs 16 x 1024^2 (the weights' AGPR reads double the loop's VALU; profiles/r05t_rw_grouped_epilogue.txt)
int mask_heads_rw_launch(const bf16* feat, const bf16* w1p, const float* b1, const float* w2, const float* b2,
                         float* logits, bf16* hsave, int B, int H, int W, hipStream_t st) {
  return launch_rw_g<3, 64, 0>(feat, w1p, b1, nullptr, nullptr, hsave, B, H, W, st, w2, b2, logits);
}

// ---------------------------------------------------------------- register-weight ConvTranspose2d(128, 64, 4, s2, p1)
// upsample_2x.0 of the output head (src/s3od/model.py:146-153: 512^2 x 128 -> 1024^2 x 64, bias, ReLU) moves 3.2 GB
// per call at bs 16; the generic path (conv data gradient, one implicit GEMM per output parity class) ran it at
// 2.56 ms.  Sub-pixel decomposition: output pixel (2j + py, 2i + px) = bias + sum over the 2 x 2 taps
// ky = 1 - py + 2a, kx = 1 - px + 2c of x[j + py - a][i + px - c] . W[:, :, ky, kx], i.e. four 2x2 convs of x.
//   * tile = 8 x 16 input pixels (-> 16 x 32 output pixels); its (8+2) x (16+2) x 128 halo arrives by LDS-DMA into a
//     3-deep ring, rows padded to 288 B (two dummy 16-B slots, conflict-free ds_read_b128 for every tap offset);
//   * wave w: output row parity py = w >> 1, output channels 32 (w & 1) .. +31, both column parities in turn; its
//     2 classes x 4 taps x 128 x 32 weights sit in registers as MFMA A fragments (256 VGPRs, gathered once);
//   * epilogue as in the 3x3 kernel: bias is the accumulators' initial value, ReLU, lane-pair channel trade,
//     one 16-B store per lane per 16-pixel block (stride-2 output columns; the other parity's wave fills the gaps).
struct CtShape {
  static constexpr int TH = 8, TW = 16, HC = TW + 2, PX = (TH + 2) * HC;
  static constexpr int ROWB = 288, CHUNKS = 16, GPIX = 256;                           // 18 slots of 16 B per pixel
  static constexpr int PIECES = ((PX * ROWB + 4095) / 4096) * 4, PPW = PIECES / 4, BUF = PIECES * 1024, LDS = 3 * BUF + 1024;
  static_assert(LDS <= 160 * 1024, "convT LDS budget");
  DEV static int slot(int c, int) { return c; }
};
template <bool RELU>
__global__ void __launch_bounds__(256, 1) convT4s2_rw_kernel(const bf16* __restrict__ x, const bf16* __restrict__ wt,
                                                              const float* __restrict__ bias, bf16* __restrict__ out,
                                                              int H, int W, int tiles_x, int tiles_y, int ntiles) {
  typedef CtShape S;
  constexpr int HC = S::HC, ROWB = S::ROWB;
  extern __shared__ __attribute__((aligned(1024))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = wave_id();
  const int lr = lane & 15, lg = lane >> 4, odd = lg & 1;
  const int py = wave >> 1, ch0 = 32 * (wave & 1);
  const PersistentTiles pt(ntiles);
  const long img_i = (long)H * W * 128, img_o = (long)4 * H * W * 64;

  // weights: wt = [co = 64][ky][kx][ci = 128] (ConvTranspose2d weight [128][64][4][4] transposed, s3od_repack_multi
  // mode 2); wr[pxc][s][nb], s = (2a + c) * 4 + kk: lane (lr, lg) holds W[co = ch0 + 16 nb + lr][ky][kx][ci = 32 kk + 8 lg ..]
  bf16x8 wr[2][16][2];
#pragma unroll
  for (int pxc = 0; pxc < 2; pxc++)
#pragma unroll
    for (int s = 0; s < 16; s++)
#pragma unroll
      for (int nb = 0; nb < 2; nb++) {
        const int a = s >> 3, c = (s >> 2) & 1, kk = s & 3, ky = 1 - py + 2 * a, kx = 1 - pxc + 2 * c;
        wr[pxc][s][nb] = *(const bf16x8*)(wt + ((ch0 + nb * 16 + lr) * 16 + ky * 4 + kx) * 128 + kk * 32 + lg * 8);
      }
  const HaloRing<S> ring(smem, wave, lane);
  auto issue = [&](int tile, int slot) {
    const bool live = tile < pt.end;
    const TileAt t = tile_at(live ? tile : pt.beg, tiles_x, tiles_y);
    ring.issue(make_rsrc(x + t.bb * img_i, (unsigned long)img_i * 2), t.tyi * S::TH - 1, t.txi * S::TW - 1, H, W, live, slot);
  };
  // halo pixel of (row r, tap a, column parity pxc, tap c) for lane lr: (r + 1 + py - a) * HC + lr + 1 + pxc - c
  const int lbase = (lr + HC * py) * ROWB + lg * 16;
  const int cb = ch0 + (odd ? 16 : 0) + 8 * (lg >> 1);
  float* aux = (float*)(smem + 3 * S::BUF);
  if (tid < 64) aux[tid] = bias ? bias[tid] : 0.f;
  __syncthreads();

  int k = 0;
  issue(pt.first, 0);
  issue(pt.first + pt.stride, 1);
  for (int tile = pt.first; tile < pt.end; tile += pt.stride, k++) {
    const TileAt t = tile_at(tile, tiles_x, tiles_y);
    const auto ro = make_rsrc(out + t.bb * img_o, (unsigned long)img_o * 2);
    ring_wait<S::PPW, 16, 0>(k);                                    // 16 stores per tile per wave (2 classes x 8 rows)
    issue(tile + 2 * pt.stride, (k + 2) % 3);
    const char* hb = smem + (k % 3) * S::BUF + lbase;
#pragma unroll
    for (int pxc = 0; pxc < 2; pxc++) {
      f32x4 acc[8][2];
#pragma unroll
      for (int nb = 0; nb < 2; nb++) {
        const f32x4 b0 = *(const f32x4*)(aux + ch0 + nb * 16 + 4 * lg);
#pragma unroll
        for (int r = 0; r < 8; r++) acc[r][nb] = b0;
      }
      auto rd = [&](int s, bf16x8 (&fa)[8]) {
        const int a = s >> 3, c = (s >> 2) & 1, kk = s & 3;
#pragma unroll
        for (int r = 0; r < 8; r++) fa[r] = *(const bf16x8*)(hb + ((r + 1 - a) * HC + 1 + pxc - c) * ROWB + kk * 64);
      };
      auto mm = [&](int s, const bf16x8 (&fa)[8]) {
#pragma unroll
        for (int r = 0; r < 8; r++)
#pragma unroll
          for (int nb = 0; nb < 2; nb++)
            acc[r][nb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wr[pxc][s][nb], fa[r], acc[r][nb], 0, 0, 0);
      };
      rw_steps<16, 8>(rd, mm);
      const int gx = t.txi * S::TW + lr;
#pragma unroll
      for (int r = 0; r < 8; r++) {
        const int gy = t.tyi * S::TH + r;
        const unsigned po = (gy < H && gx < W) ? (unsigned)(((2 * gy + py) * 2 * W + 2 * gx + pxc) * 128 + cb * 2) : 0x80000000u;
        trade_store8<RELU>(acc[r][0], acc[r][1], ro, po);
      }
    }
  }
  wait_vmcnt<0>();
}

// ---------------------------------------------------------------- register-weight Conv2d(64, 128, 4, s2, p1)
// The data gradient of upsample_2x.0 (the ConvTranspose2d's input gradient is this strided conv of dy with the
// same conv-view weight [128][4][4][64]; 1024^2 x 64 -> 512^2 x 128 at bs 16, plus the column sums that are
// output_conv1's bias gradient).  Same design as the kernels above:
//   * tile = 4 x 16 output pixels; its (2*4+2) x (2*16+2) x 64 input halo lands by LDS-DMA in a 3-deep ring, pixel
//     rows padded to 144 B (9 slots, one dummy): the stride-2 tap reads are conflict-free without a swizzle;
//   * wave w = output channels 32 w .. +31 with their 16 taps x 64 weights in registers (256 VGPRs) as MFMA A
//     fragments, read straight from the conv-view pack; all waves share the tile's 4 x 16 pixels;
//   * epilogue: lane-pair channel trade, one 16-B store per lane per 16-pixel row, column sums in fp32 (LDS atomics,
//     one global add per channel and workgroup).
struct Cs2Shape {
  static constexpr int TH = 4, TW = 16, HR = 2 * TH + 2, HC = 2 * TW + 2, PX = HR * HC;
  static constexpr int ROWB = 144, CHUNKS = 8, GPIX = 128;                            // 9 slots of 16 B per pixel
  static constexpr int PIECES = ((PX * ROWB + 4095) / 4096) * 4, PPW = PIECES / 4, BUF = PIECES * 1024, LDS = 3 * BUF + 1024;
  static_assert(LDS <= 160 * 1024, "conv s2 LDS budget");
  DEV static int slot(int c, int) { return c; }
};
__global__ void __launch_bounds__(256, 1) conv4s2_rw_kernel(const bf16* __restrict__ x, const bf16* __restrict__ w,
                                                             float* __restrict__ colsum, bf16* __restrict__ out, int H,
                                                             int W, int tiles_x, int tiles_y, int ntiles) {
  typedef Cs2Shape S;
  constexpr int TH = S::TH, HC = S::HC, ROWB = S::ROWB;
  extern __shared__ __attribute__((aligned(1024))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = wave_id();
  const int lr = lane & 15, lg = lane >> 4, odd = lg & 1;
  const int ch0 = 32 * wave;
  const PersistentTiles pt(ntiles);
  const int Hi = 2 * H, Wi = 2 * W;
  const long img_i = (long)Hi * Wi * 64, img_o = (long)H * W * 128;
  // wr[tap][kk][nb]: lane (lr, lg) holds w[co = ch0 + 16 nb + lr][tap][ci = 32 kk + 8 lg .. +7]
  bf16x8 wr[16][2][2];
#pragma unroll
  for (int tap = 0; tap < 16; tap++)
#pragma unroll
    for (int kk = 0; kk < 2; kk++)
#pragma unroll
      for (int nb = 0; nb < 2; nb++)
        wr[tap][kk][nb] = *(const bf16x8*)(w + ((ch0 + nb * 16 + lr) * 16 + tap) * 64 + kk * 32 + lg * 8);
  const HaloRing<S> ring(smem, wave, lane);
  auto issue = [&](int tile, int slot) {
    const bool live = tile < pt.end;
    const TileAt t = tile_at(live ? tile : pt.beg, tiles_x, tiles_y);
    ring.issue(make_rsrc(x + t.bb * img_i, (unsigned long)img_i * 2), 2 * t.tyi * TH - 1, 2 * t.txi * S::TW - 1, Hi, Wi, live, slot);
  };
  // halo pixel of output (row r, column lr) and tap (ky, kx): (2 r + ky) * HC + 2 lr + kx
  const int lbase = 2 * lr * ROWB + lg * 16;
  const int cb = ch0 + (odd ? 16 : 0) + 8 * (lg >> 1);
  float* aux = (float*)(smem + 3 * S::BUF);
  if (tid < 128) aux[tid] = 0.f;
  __syncthreads();
  float cs[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};

  int k = 0;
  issue(pt.first, 0);
  issue(pt.first + pt.stride, 1);
  for (int tile = pt.first; tile < pt.end; tile += pt.stride, k++) {
    const TileAt t = tile_at(tile, tiles_x, tiles_y);
    const auto ro = make_rsrc(out + t.bb * img_o, (unsigned long)img_o * 2);
    ring_wait<S::PPW, TH, 0>(k);                                    // TH stores per tile per wave
    issue(tile + 2 * pt.stride, (k + 2) % 3);
    const char* hb = smem + (k % 3) * S::BUF + lbase;
    f32x4 acc[TH][2];
#pragma unroll
    for (int r = 0; r < TH; r++) { acc[r][0] = f32x4{0.f, 0.f, 0.f, 0.f}; acc[r][1] = f32x4{0.f, 0.f, 0.f, 0.f}; }
    auto rd = [&](int s, bf16x8 (&fa)[TH]) {
      const int tap = s >> 1, kk = s & 1, ky = tap >> 2, kx = tap & 3;
#pragma unroll
      for (int r = 0; r < TH; r++) fa[r] = *(const bf16x8*)(hb + ((2 * r + ky) * HC + kx) * ROWB + kk * 64);
    };
    auto mm = [&](int s, const bf16x8 (&fa)[TH]) {
#pragma unroll
      for (int r = 0; r < TH; r++)
#pragma unroll
        for (int nb = 0; nb < 2; nb++)
          acc[r][nb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wr[s >> 1][s & 1][nb], fa[r], acc[r][nb], 0, 0, 0);
    };
    rw_steps<32, TH>(rd, mm);
    const int gx = t.txi * S::TW + lr;
#pragma unroll
    for (int r = 0; r < TH; r++) {
      const int gy = t.tyi * TH + r;
      const bool ok = gy < H && gx < W;
      const unsigned po = ok ? (unsigned)(((gy * W + gx) * 128 + cb) * 2) : 0x80000000u;
      trade_store8<false>(acc[r][0], acc[r][1], ro, po, [&](float (&o)[8]) {
        if (ok) {
#pragma unroll
          for (int e = 0; e < 8; e++) cs[e] += o[e];
        }
      });
    }
  }
  if (colsum) flush_colsum<128>(cs, aux, colsum, cb);
  wait_vmcnt<0>();
}
int conv4s2_rw_launch(const bf16* x, const bf16* w, float* colsum, bf16* out, int B, int H, int W, hipStream_t st) {
  typedef Cs2Shape S;
  const int tx = cdiv(W, S::TW), ty = cdiv(H, S::TH);
  const long tiles = (long)B * tx * ty;
  return launch_tiled<conv4s2_rw_kernel, S::LDS, 256>("conv4s2_rw", "conv s2 rw: too many tiles", tiles, grid_xcd(tiles), st,
                                                      x, w, colsum, out, H, W, tx, ty, (int)tiles);
}

// S3OD_CONVT_RW=0 disables the path (under S3OD_AB=1: per call)
bool convt_rw_ok(int dtype, int B, int H, int W) {
  return dtype == S3OD_BF16 && !S3OD_OFF("S3OD_CONVT_RW") && B > 0 && (long)4 * H * W * 128 < (1L << 31);
}
template <bool RELU>
static int launch_convT(const bf16* x, const bf16* wt, const float* bias, bf16* out, int B, int H, int W, hipStream_t st) {
  typedef CtShape S;
  const int tx = cdiv(W, S::TW), ty = cdiv(H, S::TH);
  const long tiles = (long)B * tx * ty;
  return launch_tiled<convT4s2_rw_kernel<RELU>, S::LDS, 256>("convT4s2_rw", "convT rw: too many tiles", tiles, grid_xcd(tiles),
                                                             st, x, wt, bias, out, H, W, tx, ty, (int)tiles);
}
int convT4s2_rw_launch(const bf16* x, const bf16* wt, const float* bias, bool relu, bf16* out, int B, int H, int W,
                       hipStream_t st) {
  return relu ? launch_convT<true>(x, wt, bias, out, B, H, W, st) : launch_convT<false>(x, wt, bias, out, B, H, W, st);
}

// ---------------------------------------------------------------- halo-tile 3x3 weight gradient
// dW[co][tap][ci] = sum_px dy[px][co] * x[px + tap][ci] for a 3x3 / stride 1 / pad 1 conv with Cin = 64
// and Cout = 64 / 96 (the full-resolution decoder convs).  The implicit-GEMM wgrad tiles N = 9*64 into
// 128-column blocks, so every 64-pixel K tile is fetched once per N block: ~7x the unique bytes go
// through L2 (measured: 57 % of wave time parked on vmcnt).  Here a persistent workgroup owns ALL
// 9 x 64 x Cout outputs in registers and sweeps 8 x 32-pixel tiles: dy (256 px x Cout) and the x halo
// (10 x 34 px x 64) are staged once per tile (register-prefetched one tile ahead) and every MFMA
// operand is read with ds_read_b64_tr_b16 (K = pixels, permuted identically on both operands).
// Waves: 4 (one per SIMD, up to 512 registers: the whole 9 x 64 x Cout fp32 block lives in registers),
// 9 of the 36 (tap, ci-block) pairs each, all co blocks per wave so each B fragment feeds NCO MFMAs.  The partial sums are flushed once per
// workgroup with fp32 atomics into the [co][tap][ci] workspace (wgrad_permute_add_kernel follows).
template <int CO> struct WgShape {
  static constexpr int DYB = 256 * CO * 2;                 // dy tile image [px][CO]
  static constexpr int HXB = HT_PX * 128;                  // x halo image [px][64]
  static constexpr int LDS = DYB + HXB;
  static constexpr int DCH = 256 * CO / 8, HCH = HT_PX * 8;           // 16-B chunks to stage
  static constexpr int NT = 256;                                       // 4 waves, one per SIMD
  static constexpr int PT = (DCH + HCH + NT - 1) / NT;                 // 16-B chunks per thread
  static_assert(LDS <= 160 * 1024, "halo wgrad LDS budget");
};
template <int CO> DEV int dy_at(int row, int byte) {       // conflict-free for the transposed reads
  if constexpr (CO == 64) return row * 128 + ((((byte >> 4) ^ (row & 7)) << 4) | (byte & 15));
  else return row * 192 + ((((byte >> 4) ^ ((row >> 1) & 3)) << 4) | (byte & 15));
}
DEV int hx_at(int row, int byte) { return row * 128 + ((((byte >> 4) ^ (row & 7)) << 4) | (byte & 15)); }
// 16 columns x 32 rows fragment, transposed (rows = K, permuted: 4g + q and 16 + 4g + q), of an image with PITCH bytes
// per row: the swizzles of dy_at / hx_at repeat every 8 rows, so row + 16 lies 16 PITCH bytes on in the same slot
template <int PITCH, class AT> DEV bf16x8 trf(const char* img, int r0, int col0, int lane, AT at) {
  const int g = lane >> 4, li = lane & 15, q = li >> 2, p = li & 3;
  const int byte = (col0 + 4 * p) * 2;
  return trf_at<16 * PITCH>((const lds_char*)(img + at(r0 + 4 * g + q, byte)));
}

template <int CO, bool RELU>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1)))
conv3x3_wgrad_halo_kernel(const bf16* __restrict__ dy, const bf16* __restrict__ x, float* __restrict__ ws, int H, int W,
                          int tiles_x, int tiles_y, int ntiles, int CinT, int CoT, int nci, int wpc) {
  typedef WgShape<CO> S;
  constexpr int NCO = CO / 16, CPD = CO / 8;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* dyi = smem;
  char* hxi = smem + S::DYB;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const ChannelBlock cbk(CO, ntiles, nci, wpc);
  const int co0 = cbk.co0, ci0 = cbk.ci0, t_end = cbk.t_end;
  constexpr int NP = 9;                                  // (tap, ci-block) pairs of this wave: 9*wave ..
  const int pair0 = NP * wave;
  f32x4 acc[NP][NCO];
#pragma unroll
  for (int i = 0; i < NP; i++)
#pragma unroll
    for (int j = 0; j < NCO; j++) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  uint4 pf[S::PT];
  auto prefetch = [&](int tile) {
    const TileAt t = tile_at(tile, tiles_x, tiles_y);
    const int ty0 = t.tyi * HT_TH, tx0 = t.txi * HT_TW, b = t.bb;
#pragma unroll
    for (int i = 0; i < S::PT; i++) {
      const int c = tid + S::NT * i;
      pf[i] = make_uint4(0, 0, 0, 0);
      if (c < S::DCH) {                                   // dy tile: px = ty*32 + tx
        const int px = c / CPD, ch = c - px * CPD, gy = ty0 + px / HT_TW, gx = tx0 + px % HT_TW;
        if (gy < H && gx < W) pf[i] = *(const uint4*)(dy + (((long)b * H + gy) * W + gx) * CoT + co0 + ch * 8);
      } else if (c < S::DCH + S::HCH) {                   // x halo
        const int c2 = c - S::DCH, px = c2 >> 3, ch = c2 & 7, hy = px / HT_HC, hx = px - hy * HT_HC;
        const int gy = ty0 - 1 + hy, gx = tx0 - 1 + hx;
        if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
          pf[i] = *(const uint4*)(x + (((long)b * H + gy) * W + gx) * CinT + ci0 + ch * 8);
          if (RELU) pf[i] = relu16<bf16>(pf[i]);
        }
      }
    }
  };
  int tile = cbk.t_beg;
  if (tile < t_end) prefetch(tile);
  for (; tile < t_end; tile++) {
#pragma unroll
    for (int i = 0; i < S::PT; i++) {
      const int c = tid + S::NT * i;
      if (c < S::DCH) { const int px = c / CPD, ch = c - px * CPD; *(uint4*)(dyi + dy_at<CO>(px, ch * 16)) = pf[i]; }
      else if (c < S::DCH + S::HCH) { const int c2 = c - S::DCH; *(uint4*)(hxi + hx_at(c2 >> 3, (c2 & 7) * 16)) = pf[i]; }
    }
    __syncthreads();
    if (tile + 1 < t_end) prefetch(tile + 1);
    for (int ty = 0; ty < HT_TH; ty++) {                  // K step = one output row of 32 pixels
      bf16x8 fa[NCO];
#pragma unroll
      for (int cb = 0; cb < NCO; cb++) fa[cb] = trf<CO * 2>(dyi, ty * HT_TW, cb * 16, lane, dy_at<CO>);
#pragma unroll
      for (int j = 0; j < NP; j++) {
        const int pr = pair0 + j, tap = pr >> 2, cib = pr & 3, tdy = tap / 3, tdx = tap - tdy * 3;
        const bf16x8 fb = trf<128>(hxi, (ty + tdy) * HT_HC + tdx, cib * 16, lane, hx_at);
#pragma unroll
        for (int cb = 0; cb < NCO; cb++) acc[j][cb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[cb], fb, acc[j][cb], 0, 0, 0);
      }
    }
    __syncthreads();
  }
  flush_wgrad<9, false>(acc, ws, co0, ci0, CinT, CoT, lane, pair0, 1);
}

template <int CO, bool RELU>
static int launch_wgrad_halo(const bf16* dy, const bf16* x, float* ws, int B, int H, int W, int CinT, int CoT, hipStream_t st) {
  typedef WgShape<CO> S;
  const int tx = cdiv(W, HT_TW), ty = cdiv(H, HT_TH);
  const long tiles = (long)B * tx * ty;
  const int nci = CinT / 64, nblk = (CoT / CO) * nci, wpc = grid_wpc(tiles, nblk);
  return launch_tiled<conv3x3_wgrad_halo_kernel<CO, RELU>, S::LDS, S::NT>(
      "conv3x3_wgrad_halo", "wgrad halo: too many tiles", tiles, nblk * wpc, st, dy, x, ws, H, W, tx, ty, (int)tiles, CinT, CoT,
      nci, wpc);
}
// CoT a multiple of 64 (64-channel output blocks) or 96 (the mask heads: one 96-channel block)
int wgrad3x3_halo_launch(bool relu_x, const bf16* dy, const bf16* x, float* ws, int B, int H, int W, int CinT, int CoT,
                         hipStream_t st) {
  auto go = CoT % 64 == 0 ? (relu_x ? launch_wgrad_halo<64, true> : launch_wgrad_halo<64, false>)
                          : (relu_x ? launch_wgrad_halo<96, true> : launch_wgrad_halo<96, false>);
  return go(dy, x, ws, B, H, W, CinT, CoT, st);
}

// Weight gradient of the 4x4 / stride-2 / pad-1 conv view of upsample_2x.0 (ConvTranspose2d(128, 64, 4, 2, 1)):
// dW[co][ky][kx][ci] = sum_p dy[p][co] * x[2p - 1 + (ky, kx)][ci], dy on the OH x OW grid (128 channels), x on the
// 2OH x 2OW grid (64).  The same LDS-DMA / register-accumulator scheme as the 3x3 kernel above with 16 taps:
//   * tile = 2 x 32 dy pixels; its x halo (2*2+2) x (2*32+2) is stored column-DE-INTERLEAVED (even / odd halo
//     columns in two 33-pixel sub-rows), so a tap's 32 stride-2 pixels are 32 consecutive image rows and the
//     transposed reads keep the swizzle of the 3x3 kernel;
//   * workgroup = a 64-output-channel block; wave w = taps 4w .. 4w+3 x 4 ci blocks (256 accumulator VGPRs).
namespace wg4 {
constexpr int TH = 2, TW = 32, HR = 2 * TH + 2, HS = TW + 1, HPX = HR * 2 * HS;   // halo rows, sub-row length
constexpr int AB = TH * TW * 128, HB = HPX * 128, PIECES = ((AB + HB + 4095) / 4096) * 4, PPW = PIECES / 4;
constexpr int BUF = PIECES * 1024, LDS = 2 * BUF;
static_assert(AB % 1024 == 0 && LDS <= 160 * 1024, "wgrad 4s2 layout");
}  // namespace wg4
__global__ void __launch_bounds__(256, 1)
conv4s2_wgrad_dma_kernel(const bf16* __restrict__ dy, const bf16* __restrict__ x, float* __restrict__ ws, int OH, int OW,
                         int tiles_x, int tiles_y, int ntiles, int CinT, int CoT, int nci, int wpc) {
  using namespace wg4;
  constexpr int NCO = 4, NP = 16;
  extern __shared__ __attribute__((aligned(1024))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = wave_id();
  const ChannelBlock cbk(64, ntiles, nci, wpc);
  const int co0 = cbk.co0, ci0 = cbk.ci0, t_end = cbk.t_end;
  const int pair0 = NP * wave, IH = 2 * OH, IW = 2 * OW;
  f32x4 acc[NP][NCO];
#pragma unroll
  for (int i = 0; i < NP; i++)
#pragma unroll
    for (int j = 0; j < NCO; j++) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  // dm = (row << 16) | (column << 4) | logical chunk: dy pieces -> tile row / column; halo -> halo row / halo column
  int dm[PPW];
#pragma unroll
  for (int i = 0; i < PPW; i++) {
    const int p = wave * PPW + i, b = p * 1024 + lane * 16;
    if (p < AB / 1024) {
      const int row = b >> 7, c = ((b >> 4) & 7) ^ (row & 7);
      dm[i] = ((row / TW) << 16) | ((row % TW) << 4) | c;
    } else {
      const int hb = b - AB, row = hb >> 7, c = ((hb >> 4) & 7) ^ (row & 7);
      const int hr = row / (2 * HS), rem = row - hr * 2 * HS, sub = rem / HS, idx = rem - sub * HS;
      dm[i] = row < HPX ? (hr << 16) | ((2 * idx + sub) << 4) | c : -1;
    }
  }
  auto issue = [&](int tile, int slot) {
    const TileAt t = tile_at_ymaj(tile, tiles_x, tiles_y);
    const int oy0 = t.tyi * TH, ox0 = t.txi * TW, b = t.bb;
    const long img_d = (long)OH * OW * CoT, img_x = (long)IH * IW * CinT;
    const auto rd = make_rsrc(dy + b * img_d, (unsigned long)img_d * 2);
    const auto rx = make_rsrc(x + b * img_x, (unsigned long)img_x * 2);
    char* dst = smem + slot * BUF + wave * PPW * 1024;
#pragma unroll
    for (int i = 0; i < PPW; i++) {
      const int p = wave * PPW + i, v = dm[i];
      if (p < AB / 1024) {                               // wave-uniform
        const int gy = oy0 + (v >> 16), gx = ox0 + ((v >> 4) & 0xfff);
        const bool ok = gy < OH && gx < OW;
        blds16(rd, ok ? (unsigned)(((gy * OW + gx) * CoT + co0) * 2 + (v & 15) * 16) : 0x80000000u, dst + i * 1024);
      } else {
        const int gy = 2 * oy0 - 1 + (v >> 16), gx = 2 * ox0 - 1 + ((v >> 4) & 0xfff);
        const bool ok = v >= 0 && (unsigned)gy < (unsigned)IH && (unsigned)gx < (unsigned)IW;
        blds16(rx, ok ? (unsigned)(((gy * IW + gx) * CinT + ci0) * 2 + (v & 15) * 16) : 0x80000000u, dst + i * 1024);
      }
    }
  };
  int tile = cbk.t_beg, k = 0;
  if (tile < t_end) issue(tile, 0);
  for (; tile < t_end; tile++, k++) {
    wait_vmcnt<0>();
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    if (tile + 1 < t_end) issue(tile + 1, (k + 1) & 1);
    const char* dyi = smem + (k & 1) * BUF;
    const char* hxi = dyi + AB;
    for (int ty = 0; ty < TH; ty++) {                     // K step = one dy row of 32 pixels
      bf16x8 fa[NCO];
#pragma unroll
      for (int cb = 0; cb < NCO; cb++) fa[cb] = trf<128>(dyi, ty * TW, cb * 16, lane, dy_at<64>);
#pragma unroll
      for (int j = 0; j < NP; j++) {
        const int pr = pair0 + j, tap = pr >> 2, cib = pr & 3, ky = tap >> 2, kx = tap & 3;
        // halo column 2 k + kx of halo row 2 ty + ky = sub-row (kx & 1), entry k + (kx >> 1)
        const bf16x8 fb = trf<128>(hxi, ((2 * ty + ky) * 2 + (kx & 1)) * HS + (kx >> 1), cib * 16, lane, hx_at);
#pragma unroll
        for (int cb = 0; cb < NCO; cb++) acc[j][cb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[cb], fb, acc[j][cb], 0, 0, 0);
      }
    }
  }
  flush_wgrad<16, false>(acc, ws, co0, ci0, CinT, CoT, lane, pair0, 1);
}
int wgrad4s2_dma_launch(const bf16* dy, const bf16* x, float* ws, int B, int OH, int OW, int CinT, int CoT, hipStream_t st) {
  const int tx = cdiv(OW, wg4::TW), ty = cdiv(OH, wg4::TH);
  const long tiles = (long)B * tx * ty;
  const int nci = CinT / 64, nblk = (CoT / 64) * nci, wpc = grid_wpc(tiles, nblk);
  return launch_tiled<conv4s2_wgrad_dma_kernel, wg4::LDS, 256>("conv4s2_wgrad_dma", "wgrad 4s2: too many tiles", tiles, nblk * wpc,
                                                               st, dy, x, ws, OH, OW, tx, ty, (int)tiles, CinT, CoT, nci, wpc);
}
