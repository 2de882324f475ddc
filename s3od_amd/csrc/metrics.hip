// SOD evaluation metrics on device: synth_sod/src/synth_sod/model_training/metrics.py:213-424
// (EvaluationMetrics.step: MAE, MaxF/AvgF over 255 thresholds, S-measure) with :14-137 (EMeasure,
// changeable E-measure over 256 uint8 thresholds) and :140-210 (WeightedFMeasure, exact Euclidean
// distance transform with nearest-feature indices + 7x7 sigma-5 Gaussian).
//
// One image per call (the reference steps image by image at the image's own size).  HBM-bound
// byte/float work: every pass is a coalesced grid-stride sweep over the H*W plane with block-level
// LDS reductions and one global (vector) atomic per block and accumulator; the only serial work is
// the distance transform's 1D lower envelopes (one thread per column / per row).
//
// Pass order on `stream` (sm_only runs stats, region, final):
//   stats   : MAE, sum gt, binarised-mask moments (S_object), centroid moments, PR histogram
//             (bin = last threshold <= p), uint8 E-measure histograms
//   edt_col : nearest foreground row per column (ties -> lower row)
//   edt_row : Maurer lower envelope per row (strict remove / strict advance: ties -> lower column),
//             which reproduces scipy.ndimage.distance_transform_edt(return_indices=True)'s choice
//   wf_et   : E = |p - g|, Et = E at the nearest foreground pixel
//   wf_sum  : EA = f32(7x7 Gaussian of Et, zero border), Ew sums
//   region  : centroid -> quadrant moments (S_region); optional in-place binarisation of gt.  It is the only pass
//             that writes gt, so it runs after the distance transform and the weighted-F passes: every reader
//             sees gt as the caller gave it (their foreground, gt >= 0.5, is the same before and after)
//   final   : one block: E-measure curve, F curve, S-measure, weighted F -> out[6]
#include "common.hpp"

namespace {

constexpr int NT = 255;          // PR thresholds (metrics.py:251)
constexpr int TB = 256;          // threads per block for the sweeps
constexpr double EPS = 2.220446049250313e-16;   // np.spacing(1)

// accumulator slots (double) at the start of the workspace; a kernel's partial sums are indexed by these names and go
// out as one consecutive run (block_add): A_MAE .. A_PSUM from stats_kernel, A_EWFG, A_EWBG from wf_sum_kernel
enum {
  A_MAE = 0, A_YSUM, A_N1, A_FG1, A_FG2, A_BG1, A_BG2, A_CX, A_CY, A_PSUM,
  A_EWFG, A_EWBG, A_NSCAL
};
// quadrant moments: [4][6] = n, sp, sm, spp, smm, spm
constexpr int Q_OFF = 16;
constexpr int H_CNT = Q_OFF + 24;            // u64 [256] pixels per PR bin
constexpr int H_TP = H_CNT + 256;            // double [256] gt mass per PR bin
constexpr int H_FG = H_TP + 256;             // u64 [256] uint8 histogram of pred on gt
constexpr int H_BG = H_FG + 256;             // u64 [256] uint8 histogram of pred off gt
constexpr int ACC_WORDS = H_BG + 256;        // 8-byte words

struct Tables {
  float thr[NT];     // torch.linspace(0, 1 - 1e-10, 255) float32
  double k7[49];     // matlab_style_gauss2D((7,7), 5)
};

// one grid-stride sweep over N pixels by blocks of TB threads
#define SWEEP(i, N) for (long i = blockIdx.x * (long)TB + threadIdx.x; i < (N); i += (long)gridDim.x * TB)

// block-wide sums of NV doubles; thread i < NV adds sum i to acc[i]
template <int NV>
DEV void block_add(const double (&v)[NV], double* acc) {
  static_assert(NV <= TB, "one thread of the block per accumulator");
  __shared__ double red[TB / 64][NV];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < NV; i++) {
    double s = warp_sum(v[i]);
    if (lane == 0) red[w][i] = s;
  }
  __syncthreads();
  if (threadIdx.x < NV) {
    double s = 0.0;
    for (int j = 0; j < TB / 64; j++) s += red[j][threadIdx.x];
    atomicAdd(acc + threadIdx.x, s);
  }
}

// The per-pixel updates below pick their accumulators by a condition.  That branch is a macro, so that it stays in
// the kernel: as part of a function the compiler turns it into one update at a computed index before it inlines
// it, and the kernel's partial sums, which must be registers, land in private memory.
DEV void mom_add(double* o, double x) { o[0] += x; o[1] += x * x; }
template <int K>
DEV void terms_add(double* v, const double (&t)[K]) {
#pragma unroll
  for (int j = 0; j < K; j++) v[j] += t[j];
}

// S_object moments of one pixel: o[0..3] = sum p, p^2 on the mask, sum q, q^2 off it; q = 1 - p is taken in float32,
// as the reference does
#define OBJ_ADD(o, on, p) \
  do { if (on) mom_add(o, (double)(p)); else mom_add((o) + 2, (double)(1.f - (p))); } while (0)

// adds the terms t[K] of one pixel to the moments of its quadrant q in v[4][K]
#define QUAD_ADD(v, q, t) \
  _Pragma("unroll") for (int k = 0; k < 4; k++) if (k == (q)) terms_add((v) + (int)std::size(t) * k, t)

DEV int pr_bin(const float* thr, float p) {     // largest i with thr[i] <= p, -1 if none
  int lo = 0, hi = NT;                            // invariant: thr[<lo] <= p, thr[>=hi] > p
  while (lo < hi) {
    int mid = (lo + hi) >> 1;
    if (thr[mid] <= p) lo = mid + 1; else hi = mid;
  }
  return lo - 1;
}

__global__ void __launch_bounds__(TB) stats_kernel(const float* __restrict__ pred, const float* __restrict__ gt, long N, int W,
                                                   Tables T, int sm_only, double* __restrict__ acc) {
  __shared__ float thr[NT];
  __shared__ unsigned long long hc[256], hf[256], hb[256];
  __shared__ double ht[256];
  for (int i = threadIdx.x; i < NT; i += TB) thr[i] = T.thr[i];
  hc[threadIdx.x] = hf[threadIdx.x] = hb[threadIdx.x] = 0ull;
  ht[threadIdx.x] = 0.0;
  __syncthreads();
  double v[A_PSUM + 1] = {};                     // A_MAE .. A_PSUM
  SWEEP(i, N) {
    const float p = pred[i], m = gt[i];
    const double pd = p, md = m;
    v[A_MAE] += fabs(pd - md);                   // |pred - mask| in float64 (pred f32, mask f64)
    v[A_YSUM] += md;
    v[A_PSUM] += pd;
    if (m >= 0.5f) {                             // binarised mask (metrics.py:239-240)
      const long y = i / W, x = i - y * W;
      v[A_N1] += 1.0; v[A_CX] += (double)x; v[A_CY] += (double)y;
    }
    OBJ_ADD(v + A_FG1, m >= 0.5f, p);
    if (!sm_only) {
      const int b = pr_bin(thr, p);
      if (b >= 0) {
        atomicAdd(&hc[b], 1ull);
        atomicAdd(&ht[b], md);
      }
      float s = p * 255.f;                       // (pred * 255).astype(np.uint8): truncation
      s = fminf(fmaxf(s, 0.f), 255.f);
      const int u = (int)s;
      if (m >= 0.5f) atomicAdd(&hf[u], 1ull); else atomicAdd(&hb[u], 1ull);
    }
  }
  block_add(v, acc + A_MAE);
  if (!sm_only) {
    __syncthreads();
    const int t = threadIdx.x;
    unsigned long long* acc_u = (unsigned long long*)acc;
    if (hc[t]) atomicAdd(acc_u + H_CNT + t, hc[t]);
    if (ht[t] != 0.0) atomicAdd(acc + H_TP + t, ht[t]);
    if (hf[t]) atomicAdd(acc_u + H_FG + t, hf[t]);
    if (hb[t]) atomicAdd(acc_u + H_BG + t, hb[t]);
  }
}

// centroid (metrics.py:358-378): round-half-even of the exact mean coordinate; empty mask -> round(dim/2)
DEV void centroid(double n1, double cx, double cy, int H, int W, long& X, long& Y) {
  if (n1 == 0.0) {
    X = (long)rint(W / 2.0); Y = (long)rint(H / 2.0);
  } else {
    X = (long)rint(cx / n1); Y = (long)rint(cy / n1);
  }
}

DEV int quadrant(long x, long y, long X, long Y) { return (y < Y ? 0 : 2) + (x < X ? 0 : 1); }   // LT, RT, LB, RB

__global__ void __launch_bounds__(TB) region_kernel(const float* __restrict__ pred, float* __restrict__ gt, int H, int W,
                                                    int binarize, double* __restrict__ acc) {
  long X, Y;
  centroid(acc[A_N1], acc[A_CX], acc[A_CY], H, W, X, Y);
  const long N = (long)H * W;
  const double ysum = acc[A_YSUM];
  const bool special = ysum == 0.0 || ysum == (double)N;   // y == 0 / y == 1: no binarisation
  double v[24] = {};
  SWEEP(i, N) {
    const long y = i / W, x = i - y * W;
    const float m = gt[i];
    const double p = pred[i], mb = m >= 0.5f ? 1.0 : 0.0;
    const double t[6] = {1.0, p, mb, p * p, mb * mb, p * mb};
    QUAD_ADD(v, quadrant(x, y, X, Y), t);
    if (binarize && !special) gt[i] = m >= 0.5f ? 1.f : 0.f;
  }
  block_add(v, acc + Q_OFF);
}

// nearest foreground row in each column (scipy's first-axis pass; ties -> lower row).  One thread
// per column; rows are read 16 at a time so each thread keeps 16 independent loads in flight.
__global__ void edt_col_kernel(const float* __restrict__ gt, int H, int W, int* __restrict__ feat) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x;
  if (x >= W) return;
  constexpr int R = 16;
  int last = -1;
  for (int y0 = 0; y0 < H; y0 += R) {            // nearest foreground at or above
    float g[R];
#pragma unroll
    for (int r = 0; r < R; r++) g[r] = y0 + r < H ? gt[(long)(y0 + r) * W + x] : 0.f;
#pragma unroll
    for (int r = 0; r < R; r++) {
      if (y0 + r < H) {
        if (g[r] >= 0.5f) last = y0 + r;
        feat[(long)(y0 + r) * W + x] = last;
      }
    }
  }
  int next = -1;
  for (int y1 = H - 1; y1 >= 0; y1 -= R) {       // nearest foreground at or below; the upper one wins ties
    float g[R];
    int up[R];
#pragma unroll
    for (int r = 0; r < R; r++) {
      const int y = y1 - r;
      g[r] = y >= 0 ? gt[(long)y * W + x] : 0.f;
      up[r] = y >= 0 ? feat[(long)y * W + x] : -1;
    }
#pragma unroll
    for (int r = 0; r < R; r++) {
      const int y = y1 - r;
      if (y >= 0) {
        if (g[r] >= 0.5f) next = y;
        int best = up[r];
        if (next >= 0 && (best < 0 || (next - y) < (y - best))) best = next;
        feat[(long)y * W + x] = best;
      }
    }
  }
}

// per row: Maurer's lower envelope of the column features (remove when c*dv - b*du - a*dw - a*b*c > 0,
// advance while d(l) > d(l+1)); frow/gx/gd live in LDS when the row fits, else in global scratch
DEV void envelope_row(const int* frow, int y, int W, int* gx, int* gd, int* __restrict__ idx_row, int* __restrict__ d2_row) {
  int n = 0;
  for (int x = 0; x < W; x++) {
    const int fy = frow[x];
    if (fy < 0) continue;
    const int dw = (fy - y) * (fy - y);
    while (n >= 2) {
      const long long u = gx[n - 2], v = gx[n - 1], du = gd[n - 2], dv = gd[n - 1];
      const long long a = v - u, b = x - v, c = x - u;
      if (c * dv - b * du - a * (long long)dw - a * b * c > 0) n--;
      else break;
    }
    gx[n] = x; gd[n] = dw; n++;
  }
  if (n == 0) {                                  // no foreground anywhere in the image
    for (int x = 0; x < W; x++) { idx_row[x] = -1; d2_row[x] = 0; }
    return;
  }
  int l = 0;
  for (int x = 0; x < W; x++) {
    while (l < n - 1) {
      const long long d1 = gd[l] + (long long)(gx[l] - x) * (gx[l] - x);
      const long long d2 = gd[l + 1] + (long long)(gx[l + 1] - x) * (gx[l + 1] - x);
      if (d1 > d2) l++; else break;
    }
    const int fx = gx[l], fy = frow[fx];
    idx_row[x] = fy * W + fx;
    d2_row[x] = gd[l] + (fx - x) * (fx - x);
  }
}

constexpr int EDT_LDS_W = 4096;

__global__ void __launch_bounds__(64) edt_row_kernel(const int* __restrict__ feat, int H, int W, int* __restrict__ idx,
                                                     int* __restrict__ d2, int* __restrict__ sx, int* __restrict__ sd) {
  __shared__ int fr[EDT_LDS_W], gx[EDT_LDS_W], gd[EDT_LDS_W];
  const int y = blockIdx.x;
  const long o = (long)y * W;
  if (W <= EDT_LDS_W) {
    for (int x = threadIdx.x; x < W; x += 64) fr[x] = feat[o + x];     // coalesced row copy
    __syncthreads();
    if (threadIdx.x == 0) envelope_row(fr, y, W, gx, gd, idx + o, d2 + o);
  } else if (threadIdx.x == 0) {
    envelope_row(feat + o, y, W, sx + o, sd + o, idx + o, d2 + o);
  }
}

__global__ void __launch_bounds__(TB) wf_et_kernel(const float* __restrict__ pred, const float* __restrict__ gt, long N,
                                                   const int* __restrict__ idx, float* __restrict__ et) {
  SWEEP(i, N) {
    const bool g = gt[i] >= 0.5f;
    float e;
    if (g) {
      e = fabsf(pred[i] - 1.f);
    } else {
      const int j = idx[i];
      e = j >= 0 ? fabsf(pred[j] - 1.f) : fabsf(pred[i]);   // Et = E at the nearest foreground pixel
    }
    et[i] = e;
  }
}

__global__ void __launch_bounds__(TB) wf_sum_kernel(const float* __restrict__ pred, const float* __restrict__ gt, int H, int W,
                                                    const float* __restrict__ et, const int* __restrict__ d2, Tables T,
                                                    double* __restrict__ acc) {
  __shared__ double k7[49];
  if (threadIdx.x < 49) k7[threadIdx.x] = T.k7[threadIdx.x];
  __syncthreads();
  const long N = (long)H * W;
  const double c5 = log(0.5) / 5.0;
  double v[2] = {0.0, 0.0};                        // A_EWFG, A_EWBG
  SWEEP(i, N) {
    const long y = i / W, x = i - y * W;
    double s = 0.0;                               // scipy.ndimage.convolve(mode="constant", cval=0)
    for (int dy = -3; dy <= 3; dy++) {
      const long yy = y + dy;
      if (yy < 0 || yy >= H) continue;
      for (int dx = -3; dx <= 3; dx++) {
        const long xx = x + dx;
        if (xx < 0 || xx >= W) continue;
        s += k7[(3 - dy) * 7 + (3 - dx)] * (double)et[yy * W + xx];
      }
    }
    const float ea = (float)s;                     // output keeps the input dtype (float32)
    const bool g = gt[i] >= 0.5f;
    const float e = g ? fabsf(pred[i] - 1.f) : fabsf(pred[i]);
    const float mn = (g && ea < e) ? ea : e;
    if (g) v[0] += (double)mn;
    else v[1] += (double)mn * (2.0 - exp(c5 * sqrt((double)d2[i])));
  }
  block_add(v, acc + A_EWFG);
}

DEV float fsc(float prec, float rec) {            // (1 + 0.3) * prec * recall / (0.3 * prec + recall), f32 ops
  const float num = (1.3f * prec) * rec;
  const float den = 0.3f * prec + rec;
  const float f = num / den;
  return f != f ? 0.f : f;
}

// S-measure SSIM of one quadrant (metrics.py:405-424) from its moments
DEV double q_ssim(const double* q) {
  const double n = q[0];
  const double x = q[1] / n, y = q[2] / n;
  const double sx2 = (q[3] - n * x * x) / (n - 1 + 1e-20);
  const double sy2 = (q[4] - n * y * y) / (n - 1 + 1e-20);
  const double sxy = (q[5] - n * x * y) / (n - 1 + 1e-20);
  const double al = 4 * x * y * sxy, be = (x * x + y * y) * (sx2 + sy2);
  if (al != 0.0) return al / (be + 1e-20);       // NaN (empty quadrant) lands here, as in the reference
  if (be == 0.0) return 1.0;
  return 0.0;
}

DEV double o_score(double n, double s1, double s2) {   // _object: 2x / (x^2 + 1 + std + 1e-20), unbiased std
  const double x = s1 / n;
  const double var = (s2 - n * x * x) / (n - 1);
  const double sd = sqrt(var < 0.0 ? 0.0 : var);           // n == 1 -> 0/0 = NaN, as torch.std
  return 2.0 * x / (x * x + 1.0 + sd + 1e-20);
}

// the sums of one (pred, mask) pair that the S-measure takes besides its quadrant moments: raw sums of mask and pred,
// then of the binarised mask its count, the object moments of pred on / off it and its centroid moments
struct PairSums {
  double ysum, psum, n1, fg1, fg2, bg1, bg2, cx, cy;
};

// S-measure (metrics.py:257-272, 329-356) of one pair; q holds the four quadrants' [n, sp, sm, spp, smm, spm]
DEV double s_measure(const PairSums& s, const double* q, int H, int W) {
  const double Nd = (double)H * W;
  const double y = s.ysum / Nd, xm = s.psum / Nd;
  if (y == 0.0) return 1.0 - xm;
  if (y == 1.0) return xm;
  const double n0 = Nd - s.n1, u = s.n1 / Nd;
  const double so = u * o_score(s.n1, s.fg1, s.fg2) + (1 - u) * o_score(n0, s.bg1, s.bg2);
  long X, Y;
  centroid(s.n1, s.cx, s.cy, H, W, X, Y);
  const double w1 = (double)X * Y / Nd, w2 = (double)(W - X) * Y / Nd, w3 = (double)X * (H - Y) / Nd;
  const double w4 = 1 - w1 - w2 - w3;
  const double sr = w1 * q_ssim(q) + w2 * q_ssim(q + 6) + w3 * q_ssim(q + 12) + w4 * q_ssim(q + 18);
  const double S = 0.5 * so + 0.5 * sr;
  return S < 0 ? 0.0 : S;
}

__global__ void __launch_bounds__(256) final_kernel(const double* __restrict__ acc, int H, int W, int sm_only,
                                                    double* __restrict__ out) {
  __shared__ double red[256];
  __shared__ float fs[256];
  const int t = threadIdx.x;
  const long N = (long)H * W;
  const double Nd = (double)N;
  const unsigned long long* acc_u = (const unsigned long long*)acc;
  // ---- S-measure (every thread computes it; thread 0 writes)
  const PairSums ps = {acc[A_YSUM], acc[A_PSUM], acc[A_N1], acc[A_FG1], acc[A_FG2], acc[A_BG1], acc[A_BG2], acc[A_CX], acc[A_CY]};
  const double S = s_measure(ps, acc + Q_OFF, H, W);
  if (sm_only) {
    if (t == 0) { out[0] = 0; out[1] = 0; out[2] = 0; out[3] = S; out[4] = 0; out[5] = 0; }
    return;
  }
  // ---- PR curve: counts of p >= thr[i] are suffix sums over the bins
  __shared__ double cnt_s[256], tp_s[256];
  cnt_s[t] = t < NT ? (double)acc_u[H_CNT + t] : 0.0;
  tp_s[t] = t < NT ? acc[H_TP + t] : 0.0;
  __syncthreads();
  if (t == 0) {                                   // 255-long suffix scan: trivial, serial
    double c = 0, p = 0;
    for (int i = NT - 1; i >= 0; i--) { c += cnt_s[i]; p += tp_s[i]; cnt_s[i] = c; tp_s[i] = p; }
  }
  __syncthreads();
  const double ysum = acc[A_YSUM];
  if (t < NT) {
    const float cnt = (float)cnt_s[t];            // y_temp.sum() in float32 (+1e-20 is absorbed unless 0)
    const double den = cnt == 0.f ? (double)1e-20f : (double)cnt;
    const float prec = (float)(tp_s[t] / den);
    const float rec = (float)(tp_s[t] / (ysum + 1e-20));
    fs[t] = fsc(prec, rec);
  }
  __syncthreads();
  // ---- E-measure over the 256 uint8 thresholds (metrics.py:80-110, 112-132)
  {
    // thresholds k = 0..255 count pred values >= 255 - k (cumsum of the flipped histogram)
    __shared__ double ff[256], fb[256];
    ff[t] = (double)acc_u[H_FG + 255 - t];
    fb[t] = (double)acc_u[H_BG + 255 - t];
    __syncthreads();
    if (t == 0) {
      double a = 0, b = 0;
      for (int i = 0; i < 256; i++) { a += ff[i]; b += fb[i]; ff[i] = a; fb[i] = b; }
    }
    __syncthreads();
    const double gfg = acc[A_N1], gsz = Nd;
    const double fgfg = ff[t], fgbg = fb[t], predfg = fgfg + fgbg, predbg = gsz - predfg;
    double em_sum;
    if (gfg == 0.0) em_sum = predbg;
    else if (gfg == gsz) em_sum = predfg;
    else {
      const double bgfg = gfg - fgfg, bgbg = predbg - bgfg;
      const double mp = predfg / gsz, mg = gfg / gsz;
      const double parts[4] = {fgfg, fgbg, bgfg, bgbg};
      const double cp[4] = {1 - mp, 1 - mp, 0 - mp, 0 - mp}, cg[4] = {1 - mg, 0 - mg, 1 - mg, 0 - mg};
      em_sum = 0.0;
      for (int i = 0; i < 4; i++) {
        const double al = 2 * (cp[i] * cg[i]) / (cp[i] * cp[i] + cg[i] * cg[i] + EPS);
        const double en = (al + 1) * (al + 1) / 4;
        em_sum += en * parts[i];
      }
    }
    red[t] = em_sum / (gsz - 1 + EPS);
  }
  __syncthreads();
  if (t == 0) {
    double em = 0.0;
    for (int i = 0; i < 256; i++) em += red[i];
    float mx = fs[0];
    double fsum = 0.0;
    for (int i = 0; i < NT; i++) { mx = fmaxf(mx, fs[i]); fsum += fs[i]; }
    // weighted F (metrics.py:147-191): 0 when the mask has no foreground
    double wf = 0.0;
    const double ng = acc[A_N1];
    if (ng > 0) {
      const double tpw = ng - acc[A_EWFG], fpw = acc[A_EWBG];
      const double R = 1 - acc[A_EWFG] / ng, P = tpw / (tpw + fpw + EPS);
      wf = (1 + 1.0) * R * P / (R + 1.0 * P + EPS);
    }
    out[0] = acc[A_MAE] / Nd;
    out[1] = (double)mx;
    out[2] = (double)(float)(fsum / NT);
    out[3] = S;
    out[4] = em / 256.0;
    out[5] = wf;
  }
}

inline int sweep_grid(long N) { return (int)std::min<long>(2048, std::max<long>(1, (N + TB - 1) / TB)); }

// ---------------------------------------------------------------- flip-consistency scores
// mine_samples.py:16-51 (eval_sample: three sm_only steps in a row on the same tensors) and
// consistency_filter.py:49-95 (three binary IoUs) of one image in two sweeps and a finishing block.  a is the soft
// mask of the image, b(y, x) = bm[y][W - 1 - x] the soft mask of its mirror read back through the mirror, gt the
// ground truth.  The pairs are (pred, mask) = (a, gt), (b, gt') and (a, b), where gt' is gt as step 1 left it.
//
// accumulator slots of sweep 1 (doubles at the start of the workspace)
enum {
  F_YSUM = 0, F_N1, F_CX, F_CY,                        // gt: raw sum; count and centroid moments of gt >= 0.5
  F_AFG1, F_AFG2, F_ABG1, F_ABG2,                      // object moments of a on / off that foreground
  F_BFG1, F_BFG2, F_BBG1, F_BBG2,                      // the same of b
  F_ASUM, F_BSUM,                                      // raw sums of a and of b (b's is also pair 3's mask sum)
  F_NB1, F_BCX, F_BCY,                                 // count and centroid moments of b >= 0.5
  F_CFG1, F_CFG2, F_CBG1, F_CBG2,                      // object moments of a on / off b >= 0.5
  F_I_AG, F_U_AG, F_I_BG, F_U_BG, F_I_AB, F_U_AB,      // intersection / union counts of the three IoU pairs
  F_NS1
};
// sweep 2: [4][8] = n, g, a, aa, ag, b, bb, bg per quadrant about gt's centroid (g = gt >= 0.5), then
// [4][5] = n, m, a, aa, am per quadrant about b's centroid (m = b >= 0.5)
constexpr int FQ_G = 32;
constexpr int FQ_B = FQ_G + 32;
constexpr int FQ_N = 32 + 20;
constexpr int F_WORDS = 96;

// 4 waves per SIMD: the 2048 blocks of sweep_grid then run as two full rounds of 1024.  At the 6 waves its 80 VGPRs
// would allow, the rounds are 1536 + 512 blocks, the second on a third of the wave slots, and the kernel measured
// 64 us against 58 us at 1536 x 2048 (metrics kernels)
__global__ void __launch_bounds__(TB) __attribute__((amdgpu_waves_per_eu(4, 4)))
flip_stats_kernel(const float* __restrict__ a, const float* __restrict__ bm, const float* __restrict__ gt, long N, int W,
                  float thr, double* __restrict__ acc) {
  double v[F_NS1] = {};
  SWEEP(i, N) {
    const long y = i / W, x = i - y * W;
    const float pa = a[i], pb = bm[i + (W - 1 - 2 * x)], m = gt[i];     // b(y, x) = bm[y][W - 1 - x]
    v[F_YSUM] += (double)m; v[F_ASUM] += (double)pa; v[F_BSUM] += (double)pb;
    if (m >= 0.5f) { v[F_N1] += 1.0; v[F_CX] += (double)x; v[F_CY] += (double)y; }
    OBJ_ADD(v + F_AFG1, m >= 0.5f, pa);
    OBJ_ADD(v + F_BFG1, m >= 0.5f, pb);
    if (pb >= 0.5f) { v[F_NB1] += 1.0; v[F_BCX] += (double)x; v[F_BCY] += (double)y; }
    OBJ_ADD(v + F_CFG1, pb >= 0.5f, pa);
    const bool ta = pa > thr, tb = pb > thr, tg = m > 0.5f;              // calculate_iou's binarisation
    v[F_I_AG] += (ta && tg) ? 1.0 : 0.0; v[F_U_AG] += (ta || tg) ? 1.0 : 0.0;
    v[F_I_BG] += (tb && tg) ? 1.0 : 0.0; v[F_U_BG] += (tb || tg) ? 1.0 : 0.0;
    v[F_I_AB] += (ta && tb) ? 1.0 : 0.0; v[F_U_AB] += (ta || tb) ? 1.0 : 0.0;
  }
  block_add(v, acc);
}

__global__ void __launch_bounds__(TB) flip_region_kernel(const float* __restrict__ a, const float* __restrict__ bm,
                                                         const float* __restrict__ gt, int H, int W, double* __restrict__ acc) {
  long X, Y, XB, YB;       // the centroids of gt >= 0.5 (pairs 1 and 2) and of b >= 0.5 (pair 3)
  centroid(acc[F_N1], acc[F_CX], acc[F_CY], H, W, X, Y);
  centroid(acc[F_NB1], acc[F_BCX], acc[F_BCY], H, W, XB, YB);
  const long N = (long)H * W;
  double v[FQ_N] = {};
  SWEEP(i, N) {
    const long y = i / W, x = i - y * W;
    const float pb = bm[i + (W - 1 - 2 * x)];
    const double ad = a[i], bd = pb;
    const double mg = gt[i] >= 0.5f ? 1.0 : 0.0, mb = pb >= 0.5f ? 1.0 : 0.0;
    const double tg[8] = {1.0, mg, ad, ad * ad, ad * mg, bd, bd * bd, bd * mg};
    const double tb[5] = {1.0, mb, ad, ad * ad, ad * mb};
    QUAD_ADD(v, quadrant(x, y, X, Y), tg);
    QUAD_ADD(v + (FQ_B - FQ_G), quadrant(x, y, XB, YB), tb);
  }
  block_add(v, acc + FQ_G);
}

__global__ void flip_final_kernel(const double* __restrict__ acc, int H, int W, double* __restrict__ out) {
  if (threadIdx.x != 0) return;
  double q1[24], q2[24], q3[24];
  for (int k = 0; k < 4; k++) {
    const double* g = acc + FQ_G + 8 * k;
    const double* b = acc + FQ_B + 5 * k;
    const double r1[6] = {g[0], g[2], g[1], g[3], g[1], g[4]};     // a vs g (g * g = g)
    const double r2[6] = {g[0], g[5], g[1], g[6], g[1], g[7]};     // b vs g
    const double r3[6] = {b[0], b[2], b[1], b[3], b[1], b[4]};     // a vs m
    for (int j = 0; j < 6; j++) { q1[6 * k + j] = r1[j]; q2[6 * k + j] = r2[j]; q3[6 * k + j] = r3[j]; }
  }
  const double ysum = acc[F_YSUM], n1 = acc[F_N1];
  // step 1 binarises gt in place unless its raw mean is 0 or 1 (region_kernel's `special`); step 2 then sees the
  // binarised plane, whose sum is n1
  const bool special = ysum == 0.0 || ysum == (double)H * W;
  const PairSums p1 = {ysum, acc[F_ASUM], n1, acc[F_AFG1], acc[F_AFG2], acc[F_ABG1], acc[F_ABG2], acc[F_CX], acc[F_CY]};
  const PairSums p2 = {special ? ysum : n1, acc[F_BSUM], n1, acc[F_BFG1], acc[F_BFG2], acc[F_BBG1], acc[F_BBG2], acc[F_CX], acc[F_CY]};
  const PairSums p3 = {acc[F_BSUM], acc[F_ASUM], acc[F_NB1], acc[F_CFG1], acc[F_CFG2], acc[F_CBG1], acc[F_CBG2], acc[F_BCX], acc[F_BCY]};
  out[0] = s_measure(p1, q1, H, W);
  out[1] = s_measure(p2, q2, H, W);
  out[2] = s_measure(p3, q3, H, W);
  for (int j = 0; j < 6; j++) out[3 + j] = acc[F_I_AG + j];
}

// s3od_eval_metrics' workspace for an H x W image: the accumulators, four planes and, for rows too wide for
// edt_row_kernel's LDS, two planes of envelope scratch.  ws may be null when only `bytes` is wanted.
struct EvalWs {
  long bytes = 0;
  double* acc;
  int *feat, *idx, *d2;
  float* et;
  int *sx, *sd;
  EvalWs(int H, int W, void* ws) {
    const long plane = (long)H * W * 4, env = W > EDT_LDS_W ? plane : 0;
    auto take = [&](long n) { char* p = ws ? (char*)ws + bytes : nullptr; bytes += n; return p; };
    acc = (double*)take((long)ACC_WORDS * 8);
    feat = (int*)take(plane); idx = (int*)take(plane); d2 = (int*)take(plane);
    et = (float*)take(plane);
    sx = (int*)take(env); sd = (int*)take(env);
  }
};

}  // namespace

extern "C" {

// *bytes (host) = scratch s3od_eval_metrics needs for an H x W image
int s3od_eval_metrics_ws(int H, int W, long* bytes) {
  S3OD_REQUIRE(bytes && H > 0 && W > 0, "eval_metrics_ws: bad arguments");
  *bytes = EvalWs(H, W, nullptr).bytes;
  return 0;
}

// pred: fp32 [H][W] soft mask in [0,1]; gt: fp32 [H][W] in [0,1] (binarised in place at 0.5 when
// `binarize` and the mask is neither all-0 nor all-1, as metrics.py:239-240 does to the caller's
// tensor); thr: host float[255] = torch.linspace(0, 1 - 1e-10, 255); k7: host double[49] =
// matlab_style_gauss2D((7, 7), 5); ws: device scratch of s3od_eval_metrics_ws(H, W) bytes;
// out: device double[6] = MAE, MaxF, AvgF, S-measure, E-measure (mean of the 256-point curve), weighted F
// (sm_only: only out[3] is meaningful).
int s3od_eval_metrics(const float* pred, float* gt, int H, int W, const float* thr, const double* k7, void* ws, long ws_bytes,
                      int sm_only, int binarize, double* out, void* stream) {
  S3OD_REQUIRE(pred && gt && ws && out && thr && k7, "eval_metrics: null pointer");
  S3OD_REQUIRE(H >= 2 && W >= 2 && H <= 32768 && W <= 32768, "eval_metrics: image must be 2..32768 on each side");
  const EvalWs w(H, W, ws);
  S3OD_REQUIRE(ws_bytes >= w.bytes, "eval_metrics: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  const long N = (long)H * W;
  Tables T;
  for (int i = 0; i < NT; i++) T.thr[i] = thr[i];
  for (int i = 0; i < 49; i++) T.k7[i] = k7[i];
  double* acc = w.acc;
  hipError_t e = hipMemsetAsync(acc, 0, (size_t)ACC_WORDS * 8, st);
  if (e != hipSuccess) return (int)e;
  const int g = sweep_grid(N);
  hipLaunchKernelGGL(stats_kernel, dim3(g), dim3(TB), 0, st, pred, (const float*)gt, N, W, T, sm_only, acc);
  if (!sm_only) {
    // the distance transform reads gt before region_kernel may binarise it (same foreground either way)
    hipLaunchKernelGGL(edt_col_kernel, dim3(cdiv(W, 64)), dim3(64), 0, st, (const float*)gt, H, W, w.feat);
    hipLaunchKernelGGL(edt_row_kernel, dim3(H), dim3(64), 0, st, (const int*)w.feat, H, W, w.idx, w.d2, w.sx, w.sd);
    hipLaunchKernelGGL(wf_et_kernel, dim3(g), dim3(TB), 0, st, pred, (const float*)gt, N, (const int*)w.idx, w.et);
    hipLaunchKernelGGL(wf_sum_kernel, dim3(g), dim3(TB), 0, st, pred, (const float*)gt, H, W, (const float*)w.et,
                       (const int*)w.d2, T, acc);
  }
  hipLaunchKernelGGL(region_kernel, dim3(g), dim3(TB), 0, st, pred, gt, H, W, binarize, acc);
  hipLaunchKernelGGL(final_kernel, dim3(1), dim3(256), 0, st, (const double*)acc, H, W, sm_only, out);
  return s3od_check_launch("eval_metrics");
}

// *bytes (host) = scratch s3od_flip_scores needs for an H x W image (the accumulators; it does not grow with the image)
int s3od_flip_scores_ws(int H, int W, long* bytes) {
  S3OD_REQUIRE(bytes && H > 0 && W > 0, "flip_scores_ws: bad arguments");
  *bytes = (long)F_WORDS * 8;
  return 0;
}

// a: fp32 [H][W] soft mask of the image; bm: fp32 [H][W] soft mask of the mirrored image, still mirrored (read as
// b(y, x) = bm[y][W-1-x]); gt: fp32 [H][W] in [0,1]; nothing is modified.  ws: device scratch of s3od_flip_scores_ws
// bytes, 8-byte aligned; out: device double[9] = S(a, gt), S(b, gt'), S(a, b) as three EvaluationMetrics(sm_only)
// steps in that order on the same tensors give them (gt' = gt binarised at 0.5 when step 1 did so, i.e. when gt's
// raw mean is neither 0 nor 1), then intersection and union counts of (a, gt), (b, gt), (a, b) with a > threshold,
// b > threshold, gt > 0.5.
int s3od_flip_scores(const float* a, const float* bm, const float* gt, int H, int W, float threshold, void* ws, long ws_bytes,
                     double* out, void* stream) {
  S3OD_REQUIRE(a && bm && gt && ws && out, "flip_scores: null pointer");
  S3OD_REQUIRE(H >= 2 && W >= 2 && H <= 32768 && W <= 32768, "flip_scores: image must be 2..32768 on each side");
  S3OD_REQUIRE(ws_bytes >= (long)F_WORDS * 8 && (uintptr_t)ws % 8 == 0 && (uintptr_t)out % 8 == 0,
               "flip_scores: workspace too small or workspace / output not 8-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const long N = (long)H * W;
  double* acc = (double*)ws;
  hipError_t e = hipMemsetAsync(acc, 0, (size_t)F_WORDS * 8, st);
  if (e != hipSuccess) return (int)e;
  const int g = sweep_grid(N);
  hipLaunchKernelGGL(flip_stats_kernel, dim3(g), dim3(TB), 0, st, a, bm, gt, N, W, threshold, acc);
  hipLaunchKernelGGL(flip_region_kernel, dim3(g), dim3(TB), 0, st, a, bm, gt, H, W, acc);
  hipLaunchKernelGGL(flip_final_kernel, dim3(1), dim3(64), 0, st, (const double*)acc, H, W, out);
  return s3od_check_launch("flip_scores");
}

}  // extern "C"
