// What the memory-bound kernels share for their column reductions: the reduction of a block's row phases in LDS and
// the fold of the replicated accumulators (common.hpp, S3OD_NREP) those reductions add into.
#pragma once
#include "common.hpp"

// ------------------------------------------------------------------ phase reduction in LDS
// A block is NG column groups x nph phases (rows, pixels): thread t = phase * NG + group holds 8-wide partial sums of
// its group's 8 columns.  phase_put stores them to red[t * 8 + e] (red: 8 floats per thread of the block); it first
// waits for the readers of an earlier reduction through the same `red`, unless this is the kernel's first (`fresh`).
// After it every thread may read.  Both readers add the phases in ascending order, starting from phase 0's value, so
// which of them a kernel uses does not change a bit of its result:
//   phase_sum8  a group's 8 sums, for the group's phase-0 thread (t < NG), whose own v is phase 0's value;
//   phase_col   one column c of the 8 NG, for any thread -- the final adds and the atomics that follow spread over
//               every lane of the block instead of the first NG.
DEV void phase_put(const float* v, float* red, int t, bool fresh = false) {
  if (!fresh) __syncthreads();
#pragma unroll
  for (int e = 0; e < 8; e++) red[t * 8 + e] = v[e];
  __syncthreads();
}
DEV void phase_sum8(float* v, const float* red, int g, int NG, int nph) {
  for (int q = 1; q < nph; q++)
#pragma unroll
    for (int e = 0; e < 8; e++) v[e] += red[(q * NG + g) * 8 + e];
}
template <int NPH> DEV float phase_col(const float* red, int c, int NG) {
  float s = red[c];
#pragma unroll
  for (int q = 1; q < NPH; q++) s += red[q * NG * 8 + c];
  return s;
}
// NV reductions in a row; the phase-0 threads (t < NG) end with the sums in v
template <int NV> DEV void phase_reduce(float (&v)[NV][8], float* red, int t, int NG, int nph) {
#pragma unroll
  for (int j = 0; j < NV; j++) {
    phase_put(v[j], red, t);
    if (t < NG) phase_sum8(v[j], red, t, NG, nph);
  }
}

// ------------------------------------------------------------------ replica fold
// s[k] += words i[k] of replicas first .. S3OD_NREP-1 of a [S3OD_NREP][n][D] accumulator, in ascending order (the K words
// of a replica are loaded together), clearing what is read.  Starting from s = 0 with first = 0, or from replica 0's
// words with first = 1, gives the same bits.
template <typename A, int K> DEV void replica_sum(A* ws, int n, int D, const int (&i)[K], A (&s)[K], int first = 0) {
  for (int r = first; r < S3OD_NREP; r++) {
    A* rep = ws + (long)r * n * D;
#pragma unroll
    for (int k = 0; k < K; k++) s[k] += rep[i[k]];
#pragma unroll
    for (int k = 0; k < K; k++) rep[i[k]] = 0;
  }
}

// a[i] += sum_r ws[r][i], b[i] += sum_r ws[r][D + i]: the fold of replicated [a | b] partials, 2 x D words per
// replica (a / b may be null).  The replicas are cleared: the workspace enters and leaves all zero.
template <typename A> __global__ void replica_fold2_kernel(A* __restrict__ ws, A* __restrict__ a, A* __restrict__ b, int D) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= 2 * D) return;
  A s[1] = {0};
  replica_sum(ws, 2, D, {i}, s);
  if (i < D) { if (a) a[i] += s[0]; }
  else if (b) b[i - D] += s[0];
}
template <typename A> void replica_fold2(A* ws, A* a, A* b, int D, hipStream_t st) {
  hipLaunchKernelGGL(replica_fold2_kernel<A>, dim3(cdiv(2 * D, 256)), dim3(256), 0, st, ws, a, b, D);
}
