// Edge-aware alpha refinement and foreground colour estimation over the full-size image.
//   refine:     colour guided filter (He, Sun, Tang 2013) of the soft mask p against the source image I = src / 255:
//               a = (cov(I) + eps Id)^-1 cov(I, p), b = mean(p) - a . mean(I), q = clip(mean(a) . I + mean(b), 0, 1)
//   foreground: blur-fusion estimate (Forte & Pitie 2021), one pass: F^ = mean(I a) / (mean(a) + 1e-5),
//               B^ = mean(I (1 - a)) / (mean(1 - a) + 1e-5), F = clip(F^ + a (I - a F^ - (1 - a) B^), 0, 1)
// Every mean is the box mean over [y-r, y+r] x [x-r, x+r] clipped to the image, divided by the number of pixels inside
// (He's boxfilter / N).  One separable box family serves both: a horizontal pass sums the moments of a row from an LDS
// tile with a one-dimensional halo (each tap is added directly, no running total), a vertical pass slides the window
// down a strip of rows per thread and ends in the solve / the apply.  Sums are float64 in registers and float32 between
// the passes; a vertical running total spans one strip plus its halo.  The image enters as its integer levels 0..255
// and is scaled where the means are formed, so the image-only moments of a window are exact sums and a flat region has
// a covariance of exactly 0.  No atomics and no cross-block accumulation: the same inputs give the same bits.
#include "common.hpp"

namespace {
constexpr int MT_TW = 256;                       // output columns per block (one thread each), both passes
constexpr int MT_MAXR = 256;
constexpr int MT_LW = MT_TW + 2 * MT_MAXR;       // LDS row of the horizontal pass: the tile and both halos
constexpr int MT_MOM = 13, MT_COEF = 4, MT_FG = 7;
constexpr int MT_WS_PLANES = MT_MOM + MT_COEF;   // fp32 [H][W] planes of the workspace

// pixels of [i - r, i + r] inside [0, n)
DEV int win_count(int i, int n, int r) { return min(i + r, n - 1) - max(i - r, 0) + 1; }

// ---- the four values a horizontal pass keeps per pixel
struct SrcImagePlane {       // uint8 [H][W][3] levels and one fp32 plane (the mask / the alpha)
  const unsigned char* __restrict__ img;
  const float* __restrict__ plane;
  DEV void load(long pix, float v[4]) const {
    const unsigned char* s = img + pix * 3;
    v[0] = (float)s[0]; v[1] = (float)s[1]; v[2] = (float)s[2]; v[3] = plane[pix];
  }
};
struct SrcPlanes4 {          // four fp32 planes hw apart (the coefficients a0, a1, a2, b)
  const float* __restrict__ planes;
  long hw;
  DEV void load(long pix, float v[4]) const {
#pragma unroll
    for (int c = 0; c < 4; c++) v[c] = planes[c * hw + pix];
  }
};

// ---- the window sums formed from them (products in float64: exact)
struct MomRefine {           // I (3) | p | I p (3) | I_i I_j (00 01 02 11 12 22)
  static constexpr int P = MT_MOM;
  DEV static void add(const float v[4], double s[P]) {
    const double i0 = v[0], i1 = v[1], i2 = v[2], p = v[3];
    s[0] += i0; s[1] += i1; s[2] += i2; s[3] += p;
    s[4] += i0 * p; s[5] += i1 * p; s[6] += i2 * p;
    s[7] += i0 * i0; s[8] += i0 * i1; s[9] += i0 * i2; s[10] += i1 * i1; s[11] += i1 * i2; s[12] += i2 * i2;
  }
};
struct MomCoef {             // a0 a1 a2 b
  static constexpr int P = MT_COEF;
  DEV static void add(const float v[4], double s[P]) {
#pragma unroll
    for (int c = 0; c < 4; c++) s[c] += (double)v[c];
  }
};
struct MomFg {               // I (3) | I alpha (3) | alpha; I (1 - alpha) and 1 - alpha follow from these and the count
  static constexpr int P = MT_FG;
  DEV static void add(const float v[4], double s[P]) {
    const double a = v[3];
#pragma unroll
    for (int c = 0; c < 3; c++) { s[c] += (double)v[c]; s[3 + c] += (double)v[c] * a; }
    s[6] += a;
  }
};

// Horizontal window sums of one row segment: grid (ceil(W / MT_TW), H), MT_TW threads.  The segment and its halo of r
// pixels on either side (zero outside the image) are staged in LDS as four planes; thread t then adds the 2 r + 1 taps
// of column x0 + t.  r <= min(MT_MAXR, W - 1).  out: fp32 [P][H][W].
template <class Src, class Mom>
__global__ __launch_bounds__(MT_TW) void box_h_kernel(Src in, int H, int W, int r, float* __restrict__ out) {
  __shared__ float tile[4][MT_LW];
  const int y = blockIdx.y, x0 = blockIdx.x * MT_TW, tid = threadIdx.x;
  const int n = min(MT_TW, W - x0) + 2 * r;      // <= MT_LW
  for (int i = tid; i < n; i += MT_TW) {
    const int x = x0 - r + i;
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    if (x >= 0 && x < W) in.load((long)y * W + x, v);
#pragma unroll
    for (int c = 0; c < 4; c++) tile[c][i] = v[c];
  }
  __syncthreads();
  const int x = x0 + tid;
  if (x >= W) return;
  double s[Mom::P];
#pragma unroll
  for (int k = 0; k < Mom::P; k++) s[k] = 0.0;
  for (int i = tid; i <= tid + 2 * r; i++) {     // tid + 2 r < n
    const float v[4] = {tile[0][i], tile[1][i], tile[2][i], tile[3][i]};
    Mom::add(v, s);
  }
  const long hw = (long)H * W, pix = (long)y * W + x;
#pragma unroll
  for (int k = 0; k < Mom::P; k++) out[k * hw + pix] = (float)s[k];
}

// Vertical window sums of the P planes `in` (fp32 [P][H][W]) and what follows from them: grid (ceil(W / MT_TW),
// ceil(H / rows)), MT_TW threads.  A thread owns column x and the strip of `rows` rows from y0: it adds the window of
// row y0 and slides it down, one row added and one subtracted per step, in float64.  r <= H - 1.
template <int P, class Epi>
__global__ __launch_bounds__(MT_TW) void box_v_kernel(const float* __restrict__ in, int H, int W, int r, int rows, Epi epi) {
  const int x = blockIdx.x * MT_TW + threadIdx.x;
  if (x >= W) return;
  const int y0 = blockIdx.y * rows, y1 = min(y0 + rows, H);
  const long hw = (long)H * W;
  const float* col = in + x;
  double s[P];
#pragma unroll
  for (int k = 0; k < P; k++) s[k] = 0.0;
  for (int yy = max(y0 - r, 0); yy <= min(y0 + r, H - 1); yy++) {
#pragma unroll
    for (int k = 0; k < P; k++) s[k] += (double)col[k * hw + (long)yy * W];
  }
  for (int y = y0; y < y1; y++) {
    epi(s, y, x);
    const int ya = y + r + 1, ys = y - r;
    if (y + 1 < y1 && ya < H) {
#pragma unroll
      for (int k = 0; k < P; k++) s[k] += (double)col[k * hw + (long)ya * W];
    }
    if (y + 1 < y1 && ys >= 0) {
#pragma unroll
      for (int k = 0; k < P; k++) s[k] -= (double)col[k * hw + (long)ys * W];
    }
  }
}

// ---- what a vertical pass does with the sums of pixel (x, y)
// guided-filter coefficients: the 3 x 3 system (cov(I) + eps Id) a = cov(I, p) by LDL^T in float64
struct EpiSolve {
  float* __restrict__ coef;    // fp32 [4][H][W]: a0 a1 a2 b
  int H, W, rh, rv;
  double eps;
  DEV void operator()(const double* s, int y, int x) const {
    const double inv = 1.0 / ((double)win_count(x, W, rh) * (double)win_count(y, H, rv));
    const double k1 = inv / 255.0, k2 = inv / 65025.0;
    const double m0 = s[0] * k1, m1 = s[1] * k1, m2 = s[2] * k1, mp = s[3] * inv;
    const double c0 = s[4] * k1 - m0 * mp, c1 = s[5] * k1 - m1 * mp, c2 = s[6] * k1 - m2 * mp;
    const double a00 = s[7] * k2 - m0 * m0 + eps, a01 = s[8] * k2 - m0 * m1, a02 = s[9] * k2 - m0 * m2;
    const double a11 = s[10] * k2 - m1 * m1 + eps, a12 = s[11] * k2 - m1 * m2, a22 = s[12] * k2 - m2 * m2 + eps;
    const double l1 = a01 / a00, l2 = a02 / a00;
    const double d1 = a11 - l1 * a01;
    const double l21 = (a12 - l2 * a01) / d1;
    const double d2 = a22 - l2 * a02 - l21 * l21 * d1;
    const double z1 = c1 - l1 * c0, z2 = c2 - l2 * c0 - l21 * z1;
    const double x2 = z2 / d2, x1 = z1 / d1 - l21 * x2, x0 = c0 / a00 - l1 * x1 - l2 * x2;
    const long hw = (long)H * W, pix = (long)y * W + x;
    coef[pix] = (float)x0; coef[hw + pix] = (float)x1; coef[2 * hw + pix] = (float)x2;
    coef[3 * hw + pix] = (float)(mp - x0 * m0 - x1 * m1 - x2 * m2);
  }
};

// q = clip(mean(a) . I + mean(b), 0, 1)
struct EpiApply {
  const unsigned char* __restrict__ src;
  float* __restrict__ out;
  int H, W, rh, rv;
  DEV void operator()(const double* s, int y, int x) const {
    const double inv = 1.0 / ((double)win_count(x, W, rh) * (double)win_count(y, H, rv));
    const long pix = (long)y * W + x;
    const unsigned char* p = src + pix * 3;
    const double q = (s[0] * (double)p[0] + s[1] * (double)p[1] + s[2] * (double)p[2]) * (inv / 255.0) + s[3] * inv;
    out[pix] = (float)fmin(fmax(q, 0.0), 1.0);
  }
};

// the blur-fusion foreground of one pixel as uint8
struct EpiForeground {
  const unsigned char* __restrict__ src;
  const float* __restrict__ alpha;
  unsigned char* __restrict__ out;
  int H, W, rh, rv;
  DEV void operator()(const double* s, int y, int x) const {
    const double inv = 1.0 / ((double)win_count(x, W, rh) * (double)win_count(y, H, rv));
    const long pix = (long)y * W + x;
    const double a = (double)alpha[pix], ma = s[6] * inv;
    const double fden = ma + 1e-5, bden = (1.0 - ma) + 1e-5;
#pragma unroll
    for (int c = 0; c < 3; c++) {
      const double I = (double)src[pix * 3 + c] / 255.0;
      const double fh = s[3 + c] * (inv / 255.0) / fden, bh = (s[c] - s[3 + c]) * (inv / 255.0) / bden;
      const double f = fmin(fmax(fh + a * (I - a * fh - (1.0 - a) * bh), 0.0), 1.0);
      out[pix * 3 + c] = (unsigned char)(f * 255.0 + 0.5);
    }
  }
};

// rows per thread of a vertical pass: the window's own height, so the strip's first window costs about as much as its
// slides, within [16, 64] so that a 4K image still fills the device
int strip_rows(int r) { return r < 16 ? 16 : (r > 64 ? 64 : r); }

template <class Src, class Mom>
void launch_h(Src in, int H, int W, int r, float* out, hipStream_t st) {
  hipLaunchKernelGGL((box_h_kernel<Src, Mom>), dim3(cdiv(W, MT_TW), H), dim3(MT_TW), 0, st, in, H, W, r, out);
}
template <int P, class Epi>
void launch_v(const float* in, int H, int W, int r, Epi epi, hipStream_t st) {
  const int rows = strip_rows(r);
  hipLaunchKernelGGL((box_v_kernel<P, Epi>), dim3(cdiv(W, MT_TW), cdiv(H, rows)), dim3(MT_TW), 0, st, in, H, W, r, rows, epi);
}

long matte_ws_bytes(int H, int W) { return (long)MT_WS_PLANES * H * W * 4; }
bool matte_size_ok(int H, int W) { return H >= 2 && W >= 2 && H <= 32768 && W <= 32768; }
}  // namespace

extern "C" {

// bytes of the scratch s3od_matte_refine and s3od_matte_foreground need for an H x W image
int s3od_matte_ws(int H, int W, long* bytes) {
  S3OD_REQUIRE(bytes != nullptr, "matte_ws: result pointer missing");
  S3OD_REQUIRE(matte_size_ok(H, W), "matte_ws: %d x %d outside 2..32768", H, W);
  *bytes = matte_ws_bytes(H, W);
  return 0;
}

// mask: device fp32 [H][W] soft mask; src: device uint8 [H][W][3] (any byte alignment); out: fp32 [H][W], may alias
// mask.  Colour guided filter of the mask against src / 255 with box radius r (1..256; the window is clipped to the
// image and may cover all of it) and regulariser eps (1e-6..1), clipped to [0, 1].  Four passes on the stream:
// 13 moment planes summed along rows, summed down columns + the float64 3 x 3 solve, the 4 coefficient planes along
// rows, down columns + apply.
int s3od_matte_refine(const float* mask, const void* src, int H, int W, int r, float eps, void* ws, long ws_bytes, float* out,
                      void* stream) {
  S3OD_REQUIRE(mask != nullptr && src != nullptr && ws != nullptr && out != nullptr, "matte_refine: mask / source / workspace / output missing");
  S3OD_REQUIRE(matte_size_ok(H, W), "matte_refine: %d x %d outside 2..32768", H, W);
  S3OD_REQUIRE(r >= 1 && r <= MT_MAXR, "matte_refine: radius %d outside 1..%d", r, MT_MAXR);
  S3OD_REQUIRE(eps >= 1e-6f && eps <= 1.f, "matte_refine: eps %g outside 1e-6..1", (double)eps);
  S3OD_REQUIRE(ws_bytes >= matte_ws_bytes(H, W) && (uintptr_t)ws % 4 == 0, "matte_refine: workspace of %ld bytes, %ld needed (4-byte aligned)",
               ws_bytes, matte_ws_bytes(H, W));
  hipStream_t st = (hipStream_t)stream;
  const int rh = std::min(r, W - 1), rv = std::min(r, H - 1);
  const long hw = (long)H * W;
  float* mom = (float*)ws;                 // 13 planes; the row sums of the coefficients reuse the first 4
  float* coef = mom + MT_MOM * hw;         // 4 planes
  const unsigned char* img = (const unsigned char*)src;
  launch_h<SrcImagePlane, MomRefine>(SrcImagePlane{img, mask}, H, W, rh, mom, st);
  launch_v<MT_MOM>(mom, H, W, rv, EpiSolve{coef, H, W, rh, rv, (double)eps}, st);
  launch_h<SrcPlanes4, MomCoef>(SrcPlanes4{coef, hw}, H, W, rh, mom, st);
  launch_v<MT_COEF>(mom, H, W, rv, EpiApply{img, out, H, W, rh, rv}, st);
  return s3od_check_launch("matte_refine");
}

// alpha: device fp32 [H][W]; src: device uint8 [H][W][3]; out_rgb: uint8 [H][W][3], not src.  Blur-fusion foreground
// colours with box radius r (1..256): (unsigned char)(F * 255 + 0.5).  Two passes on the stream: 7 planes summed
// along rows, summed down columns + the estimate.
int s3od_matte_foreground(const float* alpha, const void* src, int H, int W, int r, void* ws, long ws_bytes, void* out_rgb,
                          void* stream) {
  S3OD_REQUIRE(alpha != nullptr && src != nullptr && ws != nullptr && out_rgb != nullptr && out_rgb != src,
               "matte_foreground: alpha / source / workspace / output missing, or the output is the source");
  S3OD_REQUIRE(matte_size_ok(H, W), "matte_foreground: %d x %d outside 2..32768", H, W);
  S3OD_REQUIRE(r >= 1 && r <= MT_MAXR, "matte_foreground: radius %d outside 1..%d", r, MT_MAXR);
  S3OD_REQUIRE(ws_bytes >= matte_ws_bytes(H, W) && (uintptr_t)ws % 4 == 0, "matte_foreground: workspace of %ld bytes, %ld needed (4-byte aligned)",
               ws_bytes, matte_ws_bytes(H, W));
  hipStream_t st = (hipStream_t)stream;
  const int rh = std::min(r, W - 1), rv = std::min(r, H - 1);
  const unsigned char* img = (const unsigned char*)src;
  launch_h<SrcImagePlane, MomFg>(SrcImagePlane{img, alpha}, H, W, rh, (float*)ws, st);
  launch_v<MT_FG>((const float*)ws, H, W, rv, EpiForeground{img, alpha, (unsigned char*)out_rgb, H, W, rh, rv}, st);
  return s3od_check_launch("matte_foreground");
}

}  // extern "C"
