// remove_background pre/post-processing on device (src/s3od/predictor.py:79-139, src/s3od/utils.py).
//   preprocess: uint8 HWC image -> letterbox resize (cv2.resize INTER_LINEAR fixed-point, SIMD-path
//               rounding) into a zero-padded S x S canvas -> (x/255 - mean)/std (float64 math,
//               rounded to fp32 like numpy) -> fp32 NCHW [1,3,S,S]
//   postprocess: sigmoid -> unpad -> antialiased bilinear resize to the original size
//               (F.interpolate(..., antialias=True), separable triangle filter, horizontal first)
#include "common.hpp"

namespace {
constexpr int COEF_BITS = 11, COEF_SCALE = 1 << COEF_BITS;

// cv2 resizeGeneric_ coefficient for one destination index (INTER_LINEAR, fixed point)
DEV void cv_coef(int d, int ssize, int dsize, int& s0, int& s1, int& a0, int& a1) {
  double scale = (double)ssize / (double)dsize;
  float f = (float)((d + 0.5) * scale - 0.5);
  int s = (int)floorf(f);
  f -= (float)s;
  if (s < 0) { f = 0.f; s = 0; }
  if (s >= ssize - 1) { f = 0.f; s = ssize - 1; }
  s0 = s; s1 = min(s + 1, ssize - 1);
  int c0 = (int)rintf((1.f - f) * COEF_SCALE);      // saturate_cast<short>(float) rounds to nearest
  int c1 = (int)rintf(f * COEF_SCALE);
  a0 = c0; a1 = c1;
}
}  // namespace

// resized-image pixel (x, y) of one uint8 HWC image: cv2 INTER_LINEAR fixed point, or the pixel itself when no resize
DEV void pre_pixel(const unsigned char* __restrict__ img, int H0, int W0, int new_h, int new_w, int x, int y, int v[3]) {
  if (new_h == H0 && new_w == W0) {
    for (int c = 0; c < 3; c++) v[c] = img[((long)y * W0 + x) * 3 + c];
  } else {
    int sx0, sx1, ax0, ax1, sy0, sy1, by0, by1;
    cv_coef(x, W0, new_w, sx0, sx1, ax0, ax1);
    cv_coef(y, H0, new_h, sy0, sy1, by0, by1);
    for (int c = 0; c < 3; c++) {
      int r0 = img[((long)sy0 * W0 + sx0) * 3 + c] * ax0 + img[((long)sy0 * W0 + sx1) * 3 + c] * ax1;
      int r1 = img[((long)sy1 * W0 + sx0) * 3 + c] * ax0 + img[((long)sy1 * W0 + sx1) * 3 + c] * ax1;
      // VResizeLinearVec_32s8u: sat_u8((mulhi16(r0>>4, b0) + mulhi16(r1>>4, b1) + 2) >> 2)
      int t0 = ((short)(r0 >> 4) * (short)by0) >> 16;
      int t1 = ((short)(r1 >> 4) * (short)by1) >> 16;
      int o = (t0 + t1 + 2) >> 2;
      v[c] = o < 0 ? 0 : (o > 255 ? 255 : o);
    }
  }
}

// 8-bit value -> normalised: float32 / python float -> float32 (numpy 2), then imagenet_norm's float64 steps
DEV float pre_norm(int v, int c) { return imagenet_norm((float)v / 255.0f, c); }

// one thread per destination pixel of the resized (new_h x new_w) image; writes normalised fp32
// into the S x S canvas at (pad_h + y, pad_w + x).  The canvas must be pre-filled with the
// normalised value of a zero pixel (kernel below).
__global__ void preprocess_kernel(const unsigned char* __restrict__ img, int H0, int W0, int new_h, int new_w,
                                  int pad_h, int pad_w, int S, float* __restrict__ out) {
  int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
  if (x >= new_w || y >= new_h) return;
  int v[3];
  pre_pixel(img, H0, W0, new_h, new_w, x, y, v);
  for (int c = 0; c < 3; c++) out[((long)c * S + (pad_h + y)) * S + (pad_w + x)] = pre_norm(v[c], c);
}

__global__ void canvas_fill_kernel(float* out, int S) {
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= 3L * S * S) return;
  int c = i / ((long)S * S);
  out[i] = imagenet_norm(0.f, c);
}

// ---------------------------------------------------------------- horizontal mirror (cv2.flip(image, 1))
// dst[y][x][c] = src[y][W - 1 - x][c] on packed uint8 HWC: one byte per thread and grid-stride step, so the stores are
// coalesced and the loads run backwards pixel by pixel within the same row segment
__global__ void __launch_bounds__(256) mirror_u8_kernel(const unsigned char* __restrict__ src, long N, int W, int C,
                                                        unsigned char* __restrict__ dst) {
  const long WC = (long)W * C;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < N; i += gridDim.x * 256L) {
    const long row = i / WC;
    const int r = (int)(i - row * WC), x = r / C, c = r - x * C;
    dst[i] = src[row * WC + (long)(W - 1 - x) * C + c];
  }
}

// ---------------------------------------------------------------- batched entries: descriptor tables
// One descriptor per image; the tables are packed arrays in device memory (the host keeps a copy for the argument
// checks).  include/s3od_hip.h carries these definitions; s3od_amd/infer_many.py mirrors them with ctypes.
struct S3odPreDesc {   // 32 bytes
  long img_off;        // @0  byte offset of the uint8 [H0][W0][3] image in the packed image buffer
  int H0;              // @8  source height
  int W0;              // @12 source width
  int new_h;           // @16 resized height
  int new_w;           // @20 resized width
  int pad_h;           // @24 canvas row of the resized image's first row
  int pad_w;           // @28 canvas column of the resized image's first column
};
struct S3odPostDesc {  // 56 bytes
  long img_off;        // @0  byte offset of the uint8 [H0][W0][3] source image (read for the RGBA output only)
  long mask_off;       // @8  offset in floats of this image's [planes][H0][W0] masks in the packed mask buffer
  long rgba_off;       // @16 byte offset of this image's uint8 [H0][W0][4] RGBA in the packed RGBA buffer
  long tmp_off;        // @24 offset in floats of this image's [planes][h][W0] scratch (two-pass branch only)
  int pad_h;           // @32 first logit row of the crop
  int pad_w;           // @36 first logit column of the crop
  int h;               // @40 crop height
  int w;               // @44 crop width
  int H0;              // @48 output height
  int W0;              // @52 output width
};
struct S3odOutDesc {   // 40 bytes
  long bg_off;         // @0  byte offset of the uint8 [H0][W0][3] background image in the packed image buffer (mode 2 only)
  long out_off;        // @8  byte offset of this output in the packed output buffer (dense rows; a multiple of 4 for mode 0)
  long stats_off;      // @16 byte offset of the image's 288-byte counter block in the stats buffer, < 0: none (first row only)
  long scratch_off;    // @24 offset in floats of the image's [NM][H0][W0] planes in the stats scratch (first row only)
  int mode;            // @32 0 RGBA, 1 RGB over colour, 2 RGB over image, 3 mask as uint8, 4 nothing
  int color;           // @36 background colour r | g << 8 | b << 16 (mode 1)
};
static_assert(sizeof(S3odPreDesc) == 32 && sizeof(S3odPostDesc) == 56 && sizeof(S3odOutDesc) == 40,
              "descriptor layout is part of the C ABI");

// ---------------------------------------------------------------- compositing (src/s3od/visualizer.py:17-21)
enum { OUT_RGBA = 0, OUT_RGB_OVER_COLOR = 1, OUT_RGB_OVER_IMAGE = 2, OUT_MASK_U8 = 3, OUT_NONE = 4 };

static inline __host__ __device__ int out_bpp(int mode) {
  return mode == OUT_RGBA ? 4 : (mode == OUT_MASK_U8 ? 1 : (mode == OUT_NONE ? 0 : 3));
}

// One output pixel from the mask value m, the source pixel s and the background pixel (bg, or the packed colour when
// bg is null).  The blend is numpy's float32 evaluation of (mask * image + (1 - mask) * background).astype(uint8):
// two separately rounded products, a rounded 1 - m, one rounded add, truncation.  Contraction is off for the blend:
// hipcc would otherwise fuse a * b + c * d into an FMA, which changes bytes (so does the lerp bg + m (s - bg)).
// vec4: dst is 4-byte aligned (RGBA only).
DEV void compose_px(int mode, float m, const unsigned char* __restrict__ s, int color, const unsigned char* __restrict__ bg,
                    unsigned char* __restrict__ dst, bool vec4) {
  if (mode == OUT_RGBA) {
    const unsigned char a = (unsigned char)(m * 255.f);
    if (vec4) {
      *(uchar4*)dst = make_uchar4(s[0], s[1], s[2], a);
    } else {
      dst[0] = s[0]; dst[1] = s[1]; dst[2] = s[2]; dst[3] = a;
    }
  } else if (mode == OUT_MASK_U8) {
    dst[0] = (unsigned char)(m * 255.f);
  } else if (mode == OUT_RGB_OVER_COLOR || mode == OUT_RGB_OVER_IMAGE) {
#pragma clang fp contract(off)
    const float om = 1.f - m;
#pragma unroll
    for (int c = 0; c < 3; c++) {
      const int b = bg != nullptr ? bg[c] : (color >> (8 * c)) & 255;
      const float fg = m * (float)s[c], rest = om * (float)b;
      dst[c] = (unsigned char)(fg + rest);
    }
  }
}

// the outputs of pixel (x, y) of image b in the batched kernels: the rows of its descriptor table, or (od null, the
// entry without a table) the RGBA image at d.rgba_off
DEV void compose_rows(const S3odOutDesc* __restrict__ od, int n_out, int b, const S3odPostDesc& d, float m, long pix,
                      const unsigned char* __restrict__ imgs, unsigned char* __restrict__ out) {
  const unsigned char* s = imgs + d.img_off + pix * 3;
  if (od == nullptr) {
    compose_px(OUT_RGBA, m, s, 0, nullptr, out + d.rgba_off + pix * 4, true);
    return;
  }
  for (int k = 0; k < n_out; k++) {
    const S3odOutDesc* o = od + (long)b * n_out + k;
    const int mode = o->mode;
    const unsigned char* bg = mode == OUT_RGB_OVER_IMAGE ? imgs + o->bg_off + pix * 3 : nullptr;
    compose_px(mode, m, s, o->color, bg, out + o->out_off + pix * out_bpp(mode), true);
  }
}

// standalone compositor: one thread per pixel, rows `pitch` bytes apart
__global__ __launch_bounds__(256) void compose_kernel(const float* __restrict__ mask, const unsigned char* __restrict__ src,
                                                      int H0, int W0, int mode, int color,
                                                      const unsigned char* __restrict__ bg, unsigned char* __restrict__ out,
                                                      long pitch, int vec4) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
  if (x >= W0 || y >= H0) return;
  const long pix = (long)y * W0 + x;
  compose_px(mode, mask[pix], src != nullptr ? src + pix * 3 : nullptr, color, bg != nullptr ? bg + pix * 3 : nullptr,
             out + (long)y * pitch + (long)x * out_bpp(mode), vec4 != 0);
}

// ---------------------------------------------------------------- mask statistics
// counter block of one image: 72 uint32 words.  Pair (i, j), i < j < 8, has the fixed slot k = i (15 - i) / 2 + j - i - 1;
// plane c has the slot 56 + c for its own count #(m_c > 0.5), the diagonal of both pair matrices.
constexpr int ST_MAXNM = 8, ST_PAIRS = 28;
constexpr int ST_INTER = 0, ST_UNION = ST_PAIRS, ST_PLANE = 2 * ST_PAIRS, ST_AREA = 64, ST_X0 = 65, ST_Y0 = 66, ST_X1 = 67, ST_Y1 = 68;
constexpr int ST_WORDS = 72, ST_MAXBLK = 1024;

DEV void stats_init(unsigned* __restrict__ st) {
  const int t = threadIdx.x;
  if (t < ST_WORDS) st[t] = (t == ST_X0 || t == ST_Y0) ? 0x7fffffffu : 0u;
}

// Block `blk` of `nblk` (256 threads) counts its share of the N = H0 W0 pixels of planes [NM][N]: one wave-wide ballot
// per plane (lanes past N do not vote); lane c keeps plane c's ballot, lane k < 28 fetches the two ballots of its pair
// and adds the popcounts of their AND / OR (lane 28 + c: plane c with itself, its own count); wave partials in LDS, one
// integer atomic per counter per block.  Integer
// atomics: the result does not depend on scheduling.  MAXNM (4 or 8) >= NM planes are loaded per pixel, the surplus ones
// from plane NM - 1 again (in bounds) without a vote.
template <int MAXNM>
DEV void stats_block(const float* __restrict__ planes, int NM, long N, int W0, int best, float thr, unsigned* __restrict__ st,
                     int nblk, int blk) {
  __shared__ unsigned part[4][ST_WORDS];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  int pa = 0, pc = lane;                             // the pair (pa, pc) of slot k = lane < 28
#pragma unroll
  for (int a = 0; a < ST_MAXNM - 1; a++)
    if (pa == a && pc >= ST_MAXNM - 1 - a) { pc -= ST_MAXNM - 1 - a; pa++; }
  pc = pa + 1 + pc;
  if (lane >= ST_PAIRS) pa = pc = lane - ST_PAIRS;   // lanes 28..35: plane with itself; beyond: lanes that hold no ballot
  unsigned inter = 0, uni = 0, area = 0;
  int x0 = 0x7fffffff, y0 = 0x7fffffff, x1 = 0, y1 = 0;
  for (long base = (long)blk * 256; base < N; base += (long)nblk * 256) {
    const long i = base + tid;
    const bool in = i < N;
    const long ii = in ? i : N - 1;
    float v[MAXNM];
#pragma unroll
    for (int c = 0; c < MAXNM; c++) v[c] = planes[(long)min(c, NM - 1) * N + ii];
    unsigned lo = 0, hi = 0;                         // lane c < 8: the ballot of plane c (0 for c >= NM)
    bool hit = false;
#pragma unroll
    for (int c = 0; c < MAXNM; c++) {
      const unsigned long long bal = __ballot(in && c < NM && v[c] > 0.5f);
      if (lane == c) { lo = (unsigned)bal; hi = (unsigned)(bal >> 32); }
      if (c == best) hit = in && v[c] > thr;
    }
    const unsigned alo = __shfl((int)lo, pa), ahi = __shfl((int)hi, pa), clo = __shfl((int)lo, pc), chi = __shfl((int)hi, pc);
    inter += __popc(alo & clo) + __popc(ahi & chi);
    uni += __popc(alo | clo) + __popc(ahi | chi);
    area += __popcll(__ballot(hit));
    if (hit) {
      const unsigned u = (unsigned)i;                // N <= 65535^2 < 2^32
      const int y = (int)(u / (unsigned)W0), x = (int)(u - (unsigned)y * (unsigned)W0);
      x0 = min(x0, x); y0 = min(y0, y); x1 = max(x1, x + 1); y1 = max(y1, y + 1);
    }
  }
  x0 = wave_min_i(x0); y0 = wave_min_i(y0); x1 = wave_max_i(x1); y1 = wave_max_i(y1);
  if (lane < ST_PAIRS) {
    part[wave][ST_INTER + lane] = inter;
    part[wave][ST_UNION + lane] = uni;
  } else if (lane < ST_PAIRS + ST_MAXNM) {
    part[wave][ST_PLANE + lane - ST_PAIRS] = inter;
  }
  if (lane == 0) {
    part[wave][ST_AREA] = area;
    part[wave][ST_X0] = (unsigned)x0; part[wave][ST_Y0] = (unsigned)y0;
    part[wave][ST_X1] = (unsigned)x1; part[wave][ST_Y1] = (unsigned)y1;
  }
  __syncthreads();
  if (tid <= ST_AREA) {
    const unsigned v = part[0][tid] + part[1][tid] + part[2][tid] + part[3][tid];
    if (v) atomicAdd(st + tid, v);
  } else if (tid == ST_X0 || tid == ST_Y0) {
    atomicMin(st + tid, min(min(part[0][tid], part[1][tid]), min(part[2][tid], part[3][tid])));
  } else if (tid == ST_X1 || tid == ST_Y1) {
    atomicMax(st + tid, max(max(part[0][tid], part[1][tid]), max(part[2][tid], part[3][tid])));
  }
}

__global__ void stats_init_kernel(unsigned* __restrict__ st) { stats_init(st); }

__global__ __launch_bounds__(256) void mask_stats_kernel(const float* __restrict__ planes, int NM, long N, int W0, int best,
                                                         float thr, unsigned* __restrict__ st) {
  if (NM <= 4) stats_block<4>(planes, NM, N, W0, best, thr, st, gridDim.x, blockIdx.x);
  else stats_block<8>(planes, NM, N, W0, best, thr, st, gridDim.x, blockIdx.x);
}

// one launch for B images: each thread writes 4 consecutive canvas pixels of one row for the 3 channels, either the
// resampled image or the normalised zero pixel of the padding (no separate canvas fill).  block (64, 4).
__global__ __launch_bounds__(256) void preprocess_batch_kernel(const unsigned char* __restrict__ imgs,
                                                               const S3odPreDesc* __restrict__ descs, int S, int vec,
                                                               float* __restrict__ out) {
  const int b = blockIdx.z;
  const int x0 = (blockIdx.x * 64 + threadIdx.x) * 4, y = blockIdx.y * 4 + threadIdx.y;
  if (x0 >= S || y >= S) return;
  const S3odPreDesc d = descs[b];
  const unsigned char* img = imgs + d.img_off;
  const int ry = y - d.pad_h;
  const bool row_in = ry >= 0 && ry < d.new_h;
  float o[3][4];
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const int rx = x0 + i - d.pad_w;
    if (row_in && rx >= 0 && rx < d.new_w && x0 + i < S) {
      int v[3];
      pre_pixel(img, d.H0, d.W0, d.new_h, d.new_w, rx, ry, v);
#pragma unroll
      for (int c = 0; c < 3; c++) o[c][i] = pre_norm(v[c], c);
    } else {
#pragma unroll
      for (int c = 0; c < 3; c++) o[c][i] = pre_norm(0, c);
    }
  }
#pragma unroll
  for (int c = 0; c < 3; c++) {
    float* dst = out + (((long)b * 3 + c) * S + y) * S + x0;
    if (vec) {
      *(float4*)dst = make_float4(o[c][0], o[c][1], o[c][2], o[c][3]);
    } else {
#pragma unroll
      for (int i = 0; i < 4; i++)
        if (x0 + i < S) dst[i] = o[c][i];
    }
  }
}

// ---------------------------------------------------------------- antialiased bilinear
// PyTorch _upsample_bilinear2d_aa taps for output index i (align_corners=False, triangle filter with
// support max(scale, 1)).  The taps are not buffered: the span [xmin, xmin + xsize) is derived here and
// each weight is recomputed where it is used, so any downscale factor works (the reference resizes back
// to any original size, predictor.py:118-124).
struct AASpan {
  int xmin, xsize;
  float center, invscale, tot;
};

DEV float aa_tap(const AASpan& s, int j) {
  float x = (j + s.xmin - s.center + 0.5f) * s.invscale;
  return fabsf(x) < 1.f ? 1.f - fabsf(x) : 0.f;
}

DEV AASpan aa_span(int i, int in, int out) {
  AASpan s;
  float scale = (float)in / (float)out;
  float support = scale >= 1.f ? scale : 1.f;
  s.center = scale * (i + 0.5f);
  s.invscale = scale >= 1.f ? 1.f / scale : 1.f;
  s.xmin = max((int)(s.center - support + 0.5f), 0);
  s.xsize = min((int)(s.center + support + 0.5f), in) - s.xmin;
  float tot = 0.f;
  for (int j = 0; j < s.xsize; j++) tot += aa_tap(s, j);
  s.tot = tot;                // weights are w_j / tot (0 when tot == 0), as PyTorch normalises them
  return s;
}

DEV float aa_weight(const AASpan& s, int j) { return s.tot != 0.f ? aa_tap(s, j) / s.tot : 0.f; }

// pass 1: sigmoid + crop + horizontal resample: [NM][LH][LW] logits -> tmp [NM][h][W0]
__global__ void post_h_kernel(const float* __restrict__ logits, int LH, int LW, int pad_h, int pad_w, int h, int w, int W0,
                              float* __restrict__ tmp) {
  int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y, c = blockIdx.z;
  if (x >= W0) return;
  AASpan sp = aa_span(x, w, W0);
  const float* row = logits + ((long)c * LH + (pad_h + y)) * LW + pad_w + sp.xmin;
  float acc = 0.f;
  for (int j = 0; j < sp.xsize; j++) acc += aa_weight(sp, j) * (1.f / (1.f + expf(-row[j])));
  tmp[((long)c * h + y) * W0 + x] = acc;
}

// pass 2: vertical resample -> out [NM][H0][W0]
__global__ void post_v_kernel(const float* __restrict__ tmp, int h, int H0, int W0, float* __restrict__ out) {
  int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y, c = blockIdx.z;
  if (x >= W0) return;
  AASpan sp = aa_span(y, h, H0);
  const float* col = tmp + ((long)c * h + sp.xmin) * W0 + x;
  float acc = 0.f;
  for (int j = 0; j < sp.xsize; j++) acc += aa_weight(sp, j) * col[(long)j * W0];
  out[((long)c * H0 + y) * W0 + x] = acc;
}

// ---------------------------------------------------------------- batched post-processing
// the tile kernel handles scale factors <= 2 on both axes (support <= 2 source pixels, at most 5 taps)
static inline __host__ __device__ bool post_fused(int h, int w, int H0, int W0) {
  return (float)h / (float)H0 <= 2.f && (float)w / (float)W0 <= 2.f;
}

constexpr int PT_W = 64, PT_H = 16, PT_TAPS = 6;           // output tile, taps kept per output row / column
constexpr int PT_SW = 2 * PT_W + 8, PT_SH = 2 * PT_H + 8;  // source window: scale * (tile - 1) + 2 * support + 1 fits

// plane p of image b -> mask index: every mask, or only the best one
DEV int post_plane(int p, int planes, int NM, int best) { return planes == NM ? p : best; }

// the float value of pixel pix of mask c: into the packed masks (every plane, or the best one alone as plane 0) and,
// with mask statistics over planes that are not otherwise kept, into the image's [NM][H0][W0] scratch
DEV void post_store(float* __restrict__ masks, float* __restrict__ scratch, const S3odOutDesc* __restrict__ od, int n_out, int b,
                    const S3odPostDesc& d, int all_masks, int c, int bi, float acc, long pix) {
  const long hw = (long)d.H0 * d.W0;
  if (masks != nullptr) {
    if (all_masks) masks[d.mask_off + c * hw + pix] = acc;
    else if (c == bi) masks[d.mask_off + pix] = acc;
  }
  if (scratch != nullptr) scratch[od[(long)b * n_out].scratch_off + c * hw + pix] = acc;
}

// One 64 x 16 output tile of one mask plane per block (256 threads): the sigmoid of the source window is staged in
// LDS, resampled horizontally into LDS and vertically from LDS; span and normalised weights are computed once per
// tile column / row.  The block of the best plane also writes the RGBA tile (source RGB + truncated alpha).
__global__ __launch_bounds__(256) void post_tile_kernel(const float* __restrict__ logits, int NM, int LH, int LW,
                                                        const int* __restrict__ best, const unsigned char* __restrict__ imgs,
                                                        const S3odPostDesc* __restrict__ descs, int planes, int all_masks,
                                                        float* __restrict__ masks, unsigned char* __restrict__ rgba,
                                                        const S3odOutDesc* __restrict__ od, int n_out,
                                                        float* __restrict__ scratch) {
  __shared__ float src[PT_SH][PT_SW];
  __shared__ float hbuf[PT_SH][PT_W];
  __shared__ float hw[PT_TAPS][PT_W], vw[PT_TAPS][PT_H];
  __shared__ int hmn[PT_W], hsz[PT_W], vmn[PT_H], vsz[PT_H];
  const int b = blockIdx.z / planes, p = blockIdx.z % planes;
  const S3odPostDesc d = descs[b];
  if (!post_fused(d.h, d.w, d.H0, d.W0)) return;
  const int ox0 = blockIdx.x * PT_W, oy0 = blockIdx.y * PT_H;
  if (ox0 >= d.W0 || oy0 >= d.H0) return;
  const int bi = best[b];
  const int c = post_plane(p, planes, NM, bi);
  const int tid = threadIdx.x, tx = tid & 63, ty = tid >> 6;

  if (tid < PT_W) {
    AASpan sp = aa_span(min(ox0 + tid, d.W0 - 1), d.w, d.W0);
    hmn[tid] = sp.xmin;
    hsz[tid] = max(min(sp.xsize, PT_TAPS), 0);
    for (int j = 0; j < PT_TAPS; j++) hw[j][tid] = j < sp.xsize ? aa_weight(sp, j) : 0.f;
  } else if (tid < PT_W + PT_H) {
    const int r = tid - PT_W;
    AASpan sp = aa_span(min(oy0 + r, d.H0 - 1), d.h, d.H0);
    vmn[r] = sp.xmin;
    vsz[r] = max(min(sp.xsize, PT_TAPS), 0);
    for (int j = 0; j < PT_TAPS; j++) vw[j][r] = j < sp.xsize ? aa_weight(sp, j) : 0.f;
  }
  __syncthreads();
  // spans are monotone in the output index: the window runs from the first span's start to the last span's end
  const int sx_lo = hmn[0], sy_lo = vmn[0];
  const int sw = min(hmn[PT_W - 1] + hsz[PT_W - 1] - sx_lo, PT_SW);
  const int sh = min(vmn[PT_H - 1] + vsz[PT_H - 1] - sy_lo, PT_SH);

  const float* lp = logits + (((long)b * NM + c) * LH + d.pad_h + sy_lo) * LW + d.pad_w + sx_lo;
  for (int r = ty; r < sh; r += 4)
    for (int q = tx; q < sw; q += 64) src[r][q] = 1.f / (1.f + expf(-lp[(long)r * LW + q]));
  __syncthreads();

  {
    const int base = hmn[tx] - sx_lo, n = min(hsz[tx], PT_SW - base);
    float wj[PT_TAPS];
#pragma unroll
    for (int j = 0; j < PT_TAPS; j++) wj[j] = hw[j][tx];
    for (int r = ty; r < sh; r += 4) {
      float acc = 0.f;
#pragma unroll
      for (int j = 0; j < PT_TAPS; j++)
        if (j < n) acc += wj[j] * src[r][base + j];
      hbuf[r][tx] = acc;
    }
  }
  __syncthreads();

  const int ox = ox0 + tx;
  if (ox >= d.W0) return;
  const bool alpha = rgba != nullptr && c == bi;
#pragma unroll
  for (int k = 0; k < PT_H / 4; k++) {
    const int r = ty + 4 * k, oy = oy0 + r;
    if (oy >= d.H0) break;
    const int base = vmn[r] - sy_lo, n = min(vsz[r], PT_SH - base);
    float acc = 0.f;
#pragma unroll
    for (int j = 0; j < PT_TAPS; j++)
      if (j < n) acc += vw[j][r] * hbuf[base + j][tx];
    const long pix = (long)oy * d.W0 + ox;
    post_store(masks, scratch, od, n_out, b, d, all_masks, c, bi, acc, pix);
    if (alpha) compose_rows(od, n_out, b, d, acc, pix, imgs, rgba);
  }
}

// batched form of post_h_kernel / post_v_kernel for the images the tile kernel leaves (a scale factor > 2)
__global__ void post_h_batch_kernel(const float* __restrict__ logits, int NM, int LH, int LW, const int* __restrict__ best,
                                    const S3odPostDesc* __restrict__ descs, int planes, float* __restrict__ tmp) {
  const int b = blockIdx.z / planes, p = blockIdx.z % planes;
  const S3odPostDesc d = descs[b];
  if (post_fused(d.h, d.w, d.H0, d.W0)) return;
  int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
  if (x >= d.W0 || y >= d.h) return;
  const int c = post_plane(p, planes, NM, best[b]);
  AASpan sp = aa_span(x, d.w, d.W0);
  const float* row = logits + (((long)b * NM + c) * LH + (d.pad_h + y)) * LW + d.pad_w + sp.xmin;
  float acc = 0.f;
  for (int j = 0; j < sp.xsize; j++) acc += aa_weight(sp, j) * (1.f / (1.f + expf(-row[j])));
  tmp[d.tmp_off + ((long)p * d.h + y) * d.W0 + x] = acc;
}

__global__ void post_v_batch_kernel(const float* __restrict__ tmp, int NM, const int* __restrict__ best,
                                    const unsigned char* __restrict__ imgs, const S3odPostDesc* __restrict__ descs, int planes,
                                    int all_masks, float* __restrict__ masks, unsigned char* __restrict__ rgba,
                                    const S3odOutDesc* __restrict__ od, int n_out, float* __restrict__ scratch) {
  const int b = blockIdx.z / planes, p = blockIdx.z % planes;
  const S3odPostDesc d = descs[b];
  if (post_fused(d.h, d.w, d.H0, d.W0)) return;
  int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
  if (x >= d.W0 || y >= d.H0) return;
  const int bi = best[b];
  AASpan sp = aa_span(y, d.h, d.H0);
  const float* col = tmp + d.tmp_off + ((long)p * d.h + sp.xmin) * d.W0 + x;
  float acc = 0.f;
  for (int j = 0; j < sp.xsize; j++) acc += aa_weight(sp, j) * col[(long)j * d.W0];
  const long pix = (long)y * d.W0 + x;
  const int c = post_plane(p, planes, NM, bi);
  post_store(masks, scratch, od, n_out, b, d, all_masks, c, bi, acc, pix);
  if (rgba != nullptr && c == bi) compose_rows(od, n_out, b, d, acc, pix, imgs, rgba);
}

// batched mask statistics: grid (blocks, B); the planes of image b are its packed masks or its scratch
__global__ void stats_init_batch_kernel(const S3odOutDesc* __restrict__ od, int n_out, unsigned char* __restrict__ stats) {
  const long off = od[(long)blockIdx.x * n_out].stats_off;
  if (off >= 0) stats_init((unsigned*)(stats + off));
}

__global__ __launch_bounds__(256) void mask_stats_batch_kernel(const float* __restrict__ planes, int from_scratch, int NM,
                                                               const int* __restrict__ best,
                                                               const S3odPostDesc* __restrict__ descs,
                                                               const S3odOutDesc* __restrict__ od, int n_out, float thr,
                                                               unsigned char* __restrict__ stats) {
  const int b = blockIdx.y;
  const S3odOutDesc* o = od + (long)b * n_out;
  if (o->stats_off < 0) return;
  const S3odPostDesc d = descs[b];
  const long N = (long)d.H0 * d.W0;
  if ((long)blockIdx.x * 256 >= N) return;
  const float* pl = planes + (from_scratch ? o->scratch_off : d.mask_off);
  unsigned* st = (unsigned*)(stats + o->stats_off);
  if (NM <= 4) stats_block<4>(pl, NM, N, d.W0, best[b], thr, st, gridDim.x, blockIdx.x);
  else stats_block<8>(pl, NM, N, d.W0, best[b], thr, st, gridDim.x, blockIdx.x);
}

// sigmoid of the IoU logits and the index of the first maximum (numpy.argmax), one thread per image
__global__ void best_index_kernel(const float* __restrict__ iou_logits, int B, int NM, float* __restrict__ ious,
                                  int* __restrict__ best) {
  int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  float bv = 0.f;
  int bi = 0;
  for (int c = 0; c < NM; c++) {
    float s = 1.f / (1.f + expf(-iou_logits[(long)b * NM + c]));
    ious[(long)b * NM + c] = s;
    if (c == 0 || s > bv) { bv = s; bi = c; }
  }
  best[b] = bi;
}

// the batched post-processing behind s3od_postprocess_batch (no output table: RGBA at rgba_off) and
// s3od_postprocess_batch_out
static int post_batch_impl(const float* logits, int B, int NM, int LH, int LW, const int* best, const void* imgs, const void* descs,
                           const void* descs_host, const void* odescs, const void* odescs_host, int n_out, int all_masks,
                           float* masks, void* rgba, float* tmp, float* scratch, void* stats, float threshold, void* stream) {
  S3OD_REQUIRE(B >= 1 && NM >= 1 && NM <= 64 && (long)B * NM <= 65535 && descs_host != nullptr,
               "postprocess_batch: bad batch / mask count");
  S3OD_REQUIRE(best != nullptr, "postprocess_batch: best index / mask buffer missing");
  S3OD_REQUIRE(rgba == nullptr || (imgs != nullptr && (uintptr_t)rgba % 4 == 0), "postprocess_batch: RGBA output needs the source images and 4-byte alignment");
  const S3odPostDesc* hd = (const S3odPostDesc*)descs_host;
  const S3odOutDesc* ho = (const S3odOutDesc*)odescs_host;
  const bool planes_kept = all_masks && masks != nullptr;      // the statistics read the packed masks
  if (stats != nullptr) {
    S3OD_REQUIRE(ho != nullptr && NM <= ST_MAXNM && (uintptr_t)stats % 4 == 0, "postprocess_batch: mask statistics need the output table, at most %d masks and an aligned counter buffer", ST_MAXNM);
    S3OD_REQUIRE(planes_kept || scratch != nullptr, "postprocess_batch: mask statistics need every plane: all masks or the scratch");
  }
  if (ho == nullptr || stats == nullptr || planes_kept) scratch = nullptr;
  int fw = 0, fh = 0, tw = 0, th = 0, tH = 0;                 // tile-kernel and two-pass launch extents
  long max_n = 0;
  for (int b = 0; b < B; b++) {
    const S3odPostDesc& d = hd[b];
    S3OD_REQUIRE(d.h > 0 && d.w > 0, "postprocess_batch: image %d: bad crop", b);
    S3OD_REQUIRE(d.H0 > 0 && d.W0 > 0 && d.H0 <= 65535 && d.h <= 65535, "postprocess_batch: image %d: output size out of range", b);
    S3OD_REQUIRE(d.pad_h >= 0 && d.pad_w >= 0 && d.pad_h + d.h <= LH && d.pad_w + d.w <= LW,
                 "postprocess_batch: image %d: crop outside the logits", b);
    S3OD_REQUIRE(d.mask_off >= 0 && d.rgba_off >= 0 && d.rgba_off % 4 == 0 && d.img_off >= 0 && d.tmp_off >= 0,
                 "postprocess_batch: image %d: bad offset", b);
    for (int k = 0; ho != nullptr && k < n_out; k++) {
      const S3odOutDesc& o = ho[(long)b * n_out + k];
      S3OD_REQUIRE(o.mode >= OUT_RGBA && o.mode <= OUT_NONE, "postprocess_batch: image %d: unknown output mode %d", b, o.mode);
      S3OD_REQUIRE(o.mode == OUT_NONE || (rgba != nullptr && o.out_off >= 0 && (o.mode != OUT_RGBA || o.out_off % 4 == 0)),
                   "postprocess_batch: image %d: output buffer missing / bad output offset", b);
      S3OD_REQUIRE(o.mode != OUT_RGB_OVER_IMAGE || o.bg_off >= 0, "postprocess_batch: image %d: bad background offset", b);
    }
    if (stats != nullptr) {
      const S3odOutDesc& o = ho[(long)b * n_out];
      S3OD_REQUIRE(o.stats_off % 4 == 0 && o.scratch_off >= 0 && d.W0 <= 65535, "postprocess_batch: image %d: bad statistics offset / size", b);
      if (o.stats_off >= 0) max_n = (long)d.H0 * d.W0 > max_n ? (long)d.H0 * d.W0 : max_n;
    }
    if (post_fused(d.h, d.w, d.H0, d.W0)) {
      fw = d.W0 > fw ? d.W0 : fw; fh = d.H0 > fh ? d.H0 : fh;
    } else {
      S3OD_REQUIRE(tmp != nullptr, "postprocess_batch: image %d needs the two-pass scratch", b);
      tw = d.W0 > tw ? d.W0 : tw; th = d.h > th ? d.h : th; tH = d.H0 > tH ? d.H0 : tH;
    }
  }
  hipStream_t st = (hipStream_t)stream;
  const int planes = (all_masks || stats != nullptr) ? NM : 1;
  const S3odPostDesc* dd = (const S3odPostDesc*)descs;
  const S3odOutDesc* od = (const S3odOutDesc*)odescs;
  if (stats != nullptr)
    hipLaunchKernelGGL(stats_init_batch_kernel, dim3(B), dim3(128), 0, st, od, n_out, (unsigned char*)stats);
  if (fw > 0)
    hipLaunchKernelGGL(post_tile_kernel, dim3(cdiv(fw, PT_W), cdiv(fh, PT_H), B * planes), dim3(256), 0, st, logits, NM, LH, LW,
                       best, (const unsigned char*)imgs, dd, planes, all_masks, masks, (unsigned char*)rgba, od, n_out, scratch);
  if (tw > 0) {
    hipLaunchKernelGGL(post_h_batch_kernel, dim3(cdiv(tw, 256), th, B * planes), dim3(256), 0, st, logits, NM, LH, LW, best, dd,
                       planes, tmp);
    hipLaunchKernelGGL(post_v_batch_kernel, dim3(cdiv(tw, 256), tH, B * planes), dim3(256), 0, st, (const float*)tmp, NM, best,
                       (const unsigned char*)imgs, dd, planes, all_masks, masks, (unsigned char*)rgba, od, n_out, scratch);
  }
  if (stats != nullptr && max_n > 0)
    hipLaunchKernelGGL(mask_stats_batch_kernel, dim3(min(cdiv(max_n, 256), ST_MAXBLK), B), dim3(256), 0, st,
                       planes_kept ? (const float*)masks : (const float*)scratch, planes_kept ? 0 : 1, NM, best, dd, od, n_out,
                       threshold, (unsigned char*)stats);
  return s3od_check_launch("postprocess_batch");
}

extern "C" {

// img: device uint8 [H0][W0][3]; out: fp32 [1][3][S][S]
int s3od_preprocess(const void* img, int H0, int W0, int new_h, int new_w, int pad_h, int pad_w, int S, float* out, void* stream) {
  S3OD_REQUIRE(new_h + pad_h <= S && new_w + pad_w <= S, "preprocess: resized image does not fit the canvas");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(canvas_fill_kernel, dim3(cdiv(3L * S * S, 256)), dim3(256), 0, st, out, S);
  hipLaunchKernelGGL(preprocess_kernel, dim3(cdiv(new_w, 256), new_h), dim3(256), 0, st, (const unsigned char*)img, H0, W0,
                     new_h, new_w, pad_h, pad_w, S, out);
  return s3od_check_launch("preprocess");
}

// src, dst: device uint8 [H][W][C], contiguous, C in 1..4, src != dst; dst[y][x][c] = src[y][W-1-x][c] (the horizontal
// mirror of the source image, taken before the letterbox)
int s3od_mirror_u8(const void* src, int H, int W, int C, void* dst, void* stream) {
  S3OD_REQUIRE(src != nullptr && dst != nullptr && src != dst, "mirror_u8: source / destination missing or the same buffer");
  S3OD_REQUIRE(H >= 1 && W >= 1 && C >= 1 && C <= 4, "mirror_u8: %d x %d x %d outside H, W >= 1, C in 1..4", H, W, C);
  S3OD_REQUIRE((long)W * C <= 2147483647L, "mirror_u8: row longer than 2^31 - 1 bytes");
  const long N = (long)H * W * C;
  hipLaunchKernelGGL(mirror_u8_kernel, dim3((unsigned)std::min<long>(4096, (N + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     (const unsigned char*)src, N, W, C, (unsigned char*)dst);
  return s3od_check_launch("mirror_u8");
}

// logits: fp32 [NM][LH][LW] (one image, NM masks; LH x LW = S x S, or S x 16*floor(new_w/16) for the
// reference's unpadded Quirk-2 input); tmp: fp32 [NM][h][W0]; out: fp32 [NM][H0][W0]
int s3od_sigmoid_unpad_resize(const float* logits, int NM, int LH, int LW, int pad_h, int pad_w, int h, int w, int H0, int W0,
                              float* tmp, float* out, void* stream) {
  S3OD_REQUIRE(NM >= 1 && NM <= 64 && h > 0 && w > 0, "postprocess: bad mask count / crop");
  S3OD_REQUIRE(H0 > 0 && W0 > 0 && H0 <= 65535 && h <= 65535, "postprocess: output size out of range");
  S3OD_REQUIRE(pad_h + h <= LH && pad_w + w <= LW, "postprocess: crop outside the logits");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(post_h_kernel, dim3(cdiv(W0, 256), h, NM), dim3(256), 0, st, logits, LH, LW, pad_h, pad_w, h, w, W0, tmp);
  hipLaunchKernelGGL(post_v_kernel, dim3(cdiv(W0, 256), H0, NM), dim3(256), 0, st, tmp, h, H0, W0, out);
  return s3od_check_launch("sigmoid_unpad_resize");
}

// imgs: device uint8, B HWC images packed at descs[b].img_off; descs / descs_host: the same S3odPreDesc[B] table in
// device and in host memory (the host copy is read for the argument checks before the launch); out: fp32 [B][3][S][S]
int s3od_preprocess_batch(const void* imgs, const void* descs, const void* descs_host, int B, int S, float* out, void* stream) {
  S3OD_REQUIRE(B >= 1 && B <= 65535 && S >= 1 && descs_host != nullptr, "preprocess_batch: bad batch / canvas size");
  const S3odPreDesc* hd = (const S3odPreDesc*)descs_host;
  for (int b = 0; b < B; b++) {
    S3OD_REQUIRE(hd[b].img_off >= 0 && hd[b].H0 > 0 && hd[b].W0 > 0 && hd[b].new_h > 0 && hd[b].new_w > 0,
                 "preprocess_batch: image %d: bad size / offset", b);
    S3OD_REQUIRE(hd[b].pad_h >= 0 && hd[b].pad_w >= 0 && hd[b].new_h + hd[b].pad_h <= S && hd[b].new_w + hd[b].pad_w <= S,
                 "preprocess_batch: image %d: resized image does not fit the canvas", b);
  }
  const int vec = (S % 4 == 0) && ((uintptr_t)out % 16 == 0);
  hipLaunchKernelGGL(preprocess_batch_kernel, dim3(cdiv(S, 256), cdiv(S, 4), B), dim3(64, 4), 0, (hipStream_t)stream,
                     (const unsigned char*)imgs, (const S3odPreDesc*)descs, S, vec, out);
  return s3od_check_launch("preprocess_batch");
}

// iou_logits: fp32 [B][NM]; ious: fp32 [B][NM] = sigmoid; best: int32 [B] = index of the first maximum of ious
int s3od_best_index(const float* iou_logits, int B, int NM, float* ious, int* best, void* stream) {
  S3OD_REQUIRE(B >= 1 && NM >= 1 && NM <= 64, "best_index: bad batch / mask count");
  hipLaunchKernelGGL(best_index_kernel, dim3(cdiv(B, 64)), dim3(64), 0, (hipStream_t)stream, iou_logits, B, NM, ious, best);
  return s3od_check_launch("best_index");
}

// logits: fp32 [B][NM][LH][LW]; best: device int32 [B]; imgs: the packed uint8 source images (nullable when rgba is);
// descs / descs_host: the same S3odPostDesc[B] table in device and host memory.  all_masks != 0: masks holds
// [NM][H0][W0] per image at mask_off, otherwise only the best plane [H0][W0].  rgba (nullable): uint8 [H0][W0][4] per
// image at rgba_off = source RGB + alpha (unsigned char)(best mask * 255).
int s3od_postprocess_batch(const float* logits, int B, int NM, int LH, int LW, const int* best, const void* imgs,
                           const void* descs, const void* descs_host, int all_masks, float* masks, void* rgba, float* tmp,
                           void* stream) {
  S3OD_REQUIRE(masks != nullptr, "postprocess_batch: best index / mask buffer missing");
  return post_batch_impl(logits, B, NM, LH, LW, best, imgs, descs, descs_host, nullptr, nullptr, 0, all_masks, masks, rgba, tmp,
                         nullptr, nullptr, 0.5f, stream);
}

// s3od_postprocess_batch with a table of n_out >= 1 S3odOutDesc rows per image ([B][n_out], device and host copy): the
// block that holds the best mask's value and the source pixel writes every row's output (RGBA, the mask composited
// over a colour or over a background image packed beside the sources in imgs, or the mask as uint8) into `out`.
// masks is nullable: no float plane is stored.  stats (nullable): 288-byte counter blocks at stats_off, initialised
// here on the stream and filled as by s3od_mask_stats with the image's best index and `threshold`; all NM planes are
// then resampled (tmp_off must leave room for NM planes), into masks when all_masks != 0 and masks is given, otherwise
// into scratch at scratch_off.
int s3od_postprocess_batch_out(const float* logits, int B, int NM, int LH, int LW, const int* best, const void* imgs,
                               const void* descs, const void* descs_host, const void* odescs, const void* odescs_host, int n_out,
                               int all_masks, float* masks, void* out, float* tmp, float* scratch, void* stats, float threshold,
                               void* stream) {
  S3OD_REQUIRE(odescs != nullptr && odescs_host != nullptr && n_out >= 1 && n_out <= 8,
               "postprocess_batch_out: output descriptor table missing / bad row count");
  return post_batch_impl(logits, B, NM, LH, LW, best, imgs, descs, descs_host, odescs, odescs_host, n_out, all_masks, masks, out,
                         tmp, scratch, stats, threshold, stream);
}

// mask: device fp32 [H0][W0]; src: device uint8 [H0][W0][3] (nullable for mode 3); mode: 0 RGBA (source RGB + alpha
// (unsigned char)(mask * 255)), 1 RGB over `color` (r | g << 8 | b << 16), 2 RGB over the device image bg [H0][W0][3],
// 3 the mask as one uint8 channel; out: uint8, row y at out + y * pitch, pitch >= W0 * bytes per pixel (4, 3, 3, 1);
// bytes between the rows are left untouched.  Modes 1 and 2 are numpy's float32
// (mask * image + (1 - mask) * background).astype(uint8), byte for byte, for results in (-1, 256).
int s3od_compose(const float* mask, const void* src, int H0, int W0, int mode, int color, const void* bg, void* out, long pitch,
                 void* stream) {
  S3OD_REQUIRE(mode >= OUT_RGBA && mode <= OUT_MASK_U8, "compose: unknown mode %d", mode);
  S3OD_REQUIRE(H0 > 0 && W0 > 0 && H0 <= 65535 && W0 <= 65535, "compose: image size out of range");
  S3OD_REQUIRE(mask != nullptr && out != nullptr && (src != nullptr || mode == OUT_MASK_U8), "compose: mask / source / output missing");
  S3OD_REQUIRE((mode == OUT_RGB_OVER_IMAGE) == (bg != nullptr), "compose: a background image goes with mode 2 and with no other");
  S3OD_REQUIRE(pitch >= (long)W0 * out_bpp(mode), "compose: pitch shorter than a row");
  const int vec4 = (uintptr_t)out % 4 == 0 && pitch % 4 == 0;
  hipLaunchKernelGGL(compose_kernel, dim3(cdiv(W0, 256), H0), dim3(256), 0, (hipStream_t)stream, mask, (const unsigned char*)src,
                     H0, W0, mode, color, (const unsigned char*)bg, (unsigned char*)out, pitch, vec4);
  return s3od_check_launch("compose");
}

// masks: device fp32 [NM][H0][W0], NM <= 8; stats: caller-owned device block of 72 uint32, initialised here on the
// stream.  Words: [k] = #(m_i > 0.5 && m_j > 0.5) and [28 + k] = #(m_i > 0.5 || m_j > 0.5) for the pair i < j at
// k = i (15 - i) / 2 + j - i - 1; [56 + c] = #(m_c > 0.5); [64] = #(m_best > threshold); [65..68] = x0, y0, x1, y1 of
// those pixels' bounding box (x1, y1 exclusive; undefined when the area is 0).  Exact integers for any H0, W0 <= 65535.
int s3od_mask_stats(const float* masks, int NM, int H0, int W0, int best, float threshold, void* stats, void* stream) {
  S3OD_REQUIRE(NM >= 1 && NM <= ST_MAXNM, "mask_stats: mask count %d outside 1..%d", NM, ST_MAXNM);
  S3OD_REQUIRE(H0 > 0 && W0 > 0 && H0 <= 65535 && W0 <= 65535, "mask_stats: image size out of range");
  S3OD_REQUIRE(masks != nullptr && stats != nullptr && (uintptr_t)stats % 4 == 0 && best >= 0 && best < NM,
               "mask_stats: masks / counter block missing or best index out of range");
  hipStream_t st = (hipStream_t)stream;
  const long N = (long)H0 * W0;
  hipLaunchKernelGGL(stats_init_kernel, dim3(1), dim3(128), 0, st, (unsigned*)stats);
  hipLaunchKernelGGL(mask_stats_kernel, dim3(min(cdiv(N, 256), ST_MAXBLK)), dim3(256), 0, st, masks, NM, N, W0, best, threshold,
                     (unsigned*)stats);
  return s3od_check_launch("mask_stats");
}

}  // extern "C"
