// Shared device/host helpers for libs3od_hip (gfx950 / CDNA4 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>

typedef __bf16 bf16;
typedef bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef short s16x4 __attribute__((ext_vector_type(4)));

// dtype enum shared with include/s3od_hip.h
enum { S3OD_F32 = 0, S3OD_BF16 = 1 };

#define DEV __device__ __forceinline__

// q is stored pre-scaled by log2(e)/sqrt(64) so attention scores come out in log2 units
// (attention.hip); the q-gradient path (qkv_unrope) still scales by 1/8 because the attention
// backward returns dS.K with dS in natural units (see attention.hip).
constexpr float S3OD_QSCALE = 0.125f * 1.4426950408889634f;

// ------------------------------------------------------------------ error reporting
void s3od_set_error(const char* fmt, ...);
int s3od_check_launch(const char* what);

#define S3OD_REQUIRE(cond, ...)                     \
  do {                                              \
    if (!(cond)) {                                  \
      s3od_set_error(__VA_ARGS__);                  \
      return 22; /* EINVAL-like, distinct from hipError codes used below */ \
    }                                               \
  } while (0)

// runs the statement block with T = bf16 / float for dtype S3OD_BF16 / S3OD_F32, inside an entry point that returns int
#define DISPATCH_T(dtype, ...)                                                  \
  do {                                                                          \
    if ((dtype) == S3OD_BF16) { typedef bf16 T; __VA_ARGS__ }                   \
    else if ((dtype) == S3OD_F32) { typedef float T; __VA_ARGS__ }              \
    else { s3od_set_error("bad dtype %d", (int)(dtype)); return 22; }           \
  } while (0)

// ------------------------------------------------------------------ conversions
template <typename T> DEV float to_f(T v);
template <> DEV float to_f<float>(float v) { return v; }
template <> DEV float to_f<bf16>(bf16 v) { return (float)v; }
template <typename T> DEV T from_f(float v);
template <> DEV float from_f<float>(float v) { return v; }
template <> DEV bf16 from_f<bf16>(float v) { return (bf16)v; }

// 8 consecutive elements <-> floats (16 B for bf16, 32 B for f32)
template <typename T> DEV void load8(const T* p, float* v);
template <> DEV void load8<float>(const float* p, float* v) {
  float4 a = *(const float4*)p, b = *(const float4*)(p + 4);
  v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}
template <> DEV void load8<bf16>(const bf16* p, float* v) {
  bf16x8 a = *(const bf16x8*)p;
#pragma unroll
  for (int i = 0; i < 8; i++) v[i] = (float)a[i];
}
// 4 consecutive elements <-> floats (8 B for bf16, 16 B for f32)
template <typename T> DEV void load4(const T* p, float* v) {
  if constexpr (sizeof(T) == 4) { const float4 a = *(const float4*)p; v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; }
  else {
    const bf16x4 a = *(const bf16x4*)p;
#pragma unroll
    for (int i = 0; i < 4; i++) v[i] = (float)a[i];
  }
}
template <typename T> DEV void store4(T* p, const float* v) {
  if constexpr (sizeof(T) == 4) *(float4*)p = make_float4(v[0], v[1], v[2], v[3]);
  else *(bf16x4*)p = bf16x4{(bf16)v[0], (bf16)v[1], (bf16)v[2], (bf16)v[3]};
}
template <typename T> DEV void store8(T* p, const float* v);
template <> DEV void store8<float>(float* p, const float* v) {
  *(float4*)p = make_float4(v[0], v[1], v[2], v[3]);
  *(float4*)(p + 4) = make_float4(v[4], v[5], v[6], v[7]);
}
template <> DEV void store8<bf16>(bf16* p, const float* v) {
  bf16x8 a;
#pragma unroll
  for (int i = 0; i < 8; i++) a[i] = (bf16)v[i];
  *(bf16x8*)p = a;
}

// butterfly reductions over the 64 lanes of a wave: every lane gets the result
template <typename T> DEV T warp_sum(T v) {      // float, double
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
DEV int wave_min_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o));
  return v;
}
DEV int wave_max_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o));
  return v;
}

// torchvision / albumentations Normalize with the ImageNet statistics, v in [0, 1]: float32 value - float64 mean,
// / float64 std, rounded once to float32 (numpy's arithmetic on a float32 image)
DEV float imagenet_norm(float v, int c) {
  const double mean[3] = {0.485, 0.456, 0.406}, stdv[3] = {0.229, 0.224, 0.225};
  return (float)(((double)v - mean[c]) / stdv[c]);
}

DEV float gelu_erf(float x) { return 0.5f * x * (1.0f + erff(x * 0.70710678118654752f)); }
DEV float gelu_erf_grad(float x) {
  float cdf = 0.5f * (1.0f + erff(x * 0.70710678118654752f));
  float pdf = 0.39894228040143268f * __expf(-0.5f * x * x);
  return cdf + x * pdf;
}

// Branch-free erf-GELU for the bf16 path (its output is rounded to bf16, 2^-9 relative): erf by
// Abramowitz & Stegun 7.1.26, |error| <= 1.5e-7, one v_rcp + one v_exp + 6 FMA and no |x|-range
// branches (ocml's erff takes several, and they diverge inside a wave).  The f32 strict-parity
// path keeps erff.  e = exp(-x^2/2) is shared with the derivative: gelu'(x) = Phi(x) + x phi(x).
DEV void erf_as(float x, float& erf_x, float& e) {
  const float z = fabsf(x) * 0.70710678118654752f;
  const float t = __builtin_amdgcn_rcpf(fmaf(0.3275911f, z, 1.0f));
  float poly = fmaf(t, 1.061405429f, -1.453152027f);
  poly = fmaf(t, poly, 1.421413741f);
  poly = fmaf(t, poly, -0.284496736f);
  poly = fmaf(t, poly, 0.254829592f);
  poly *= t;
  e = __expf(-z * z);
  erf_x = copysignf(fmaf(-poly, e, 1.0f), x);
}
DEV float gelu_fast(float x) { float f, e; erf_as(x, f, e); return 0.5f * x * (1.0f + f); }
DEV float gelu_fast_grad(float x) {
  float f, e; erf_as(x, f, e);
  return 0.5f * (1.0f + f) + x * (0.39894228040143268f * e);
}

// 8 consecutive elements held raw (16 B for bf16, 32 B for f32) until they are consumed
template <typename T> struct Row8;
template <> struct Row8<float> {
  float4 a, b;
  DEV void load(const float* p) { a = ((const float4*)p)[0]; b = ((const float4*)p)[1]; }
  DEV void get(float* v) const { v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w; }
};
template <> struct Row8<bf16> {
  uint4 u;
  DEV void load(const bf16* p) { u = *(const uint4*)p; }
  DEV void get(float* v) const {
    const bf16x8 x = __builtin_bit_cast(bf16x8, u);
#pragma unroll
    for (int e = 0; e < 8; e++) v[e] = (float)x[e];
  }
};

// Dispatch / dev knobs (A/B switches and micro-benchmark sweeps; the defaults are the product path).
// S3OD_KNOB(name, def) reads the environment ONCE, on the first call through that site, into a function-local
// static; the per-call path never calls getenv.  S3OD_AB=1 (itself read once) re-reads every knob on every call,
// for the tests and tools that toggle a knob between calls inside one process (A/B of two kernels).
#include <stdlib.h>
static inline int dev_knob(const char* name, int def) {
  const char* e = getenv(name);
  return e ? atoi(e) : def;
}
static inline bool s3od_ab_mode() {
  static const bool ab = dev_knob("S3OD_AB", 0) != 0;
  return ab;
}
#define S3OD_KNOB(name, def) \
  (s3od_ab_mode() ? dev_knob(name, def) : [] { static const int v_ = dev_knob(name, def); return v_; }())
// true when the knob is set to 0 (the "off" switch of a specialised path)
#define S3OD_OFF(name) (S3OD_KNOB(name, 1) == 0)

// ------------------------------------------------------------------ wave synchronisation (hand-pipelined kernels)
// counted wait on this wave's vector-memory queue (LDS-DMA pieces, loads and stores count together, in issue order)
template <int N> DEV void wait_vmcnt() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }
DEV void wait_lgkm0() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }
// vmcnt(0) through the builtin (lgkmcnt 15, expcnt 7 = no wait there): the waitcnt pass cannot see the inline-asm waits
// above, so after an LDS-DMA main loop it still counts those DMAs as in flight and puts a vmcnt(0) in front of EVERY
// later LDS read -- in an epilogue, behind the previous segment's global stores (vmcnt counts stores too), which
// serialises the stores.  One of these after the main loop clears its scoreboard.
DEV void vm_drain() { __builtin_amdgcn_s_waitcnt(0x0F70); }
// s_barrier WITHOUT the vmcnt(0) a __syncthreads() emits: LDS-DMA stays in flight across it
DEV void raw_barrier() { __builtin_amdgcn_s_barrier(); asm volatile("" ::: "memory"); }
DEV void lds_barrier() { wait_lgkm0(); __builtin_amdgcn_s_barrier(); asm volatile("" ::: "memory"); }

// Column reductions over many workgroups add into S3OD_NREP replicas of the accumulator
// (workgroup b -> replica b % S3OD_NREP) and a second pass folds the replicas: fp32/fp64 atomics
// from ~1000 workgroups onto the same few KB serialise at the memory side (measured 2-3x slower
// end to end for the BN backward / q,v-bias reductions).
constexpr int S3OD_NREP = 32;
// the replica of a [S3OD_NREP][n][D] accumulator (n vectors of D columns) that workgroup `block` adds into; reduce.hpp
// folds the replicas
template <typename A> DEV A* replica(A* ws, unsigned block, int n, int D) { return ws + (long)(int)(block % S3OD_NREP) * n * D; }

// compute units of the current device (read once per process)
static inline int s3od_cu_count() {
  static const int n = [] {
    int dev = 0, c = 0;
    (void)hipGetDevice(&dev);
    (void)hipDeviceGetAttribute(&c, hipDeviceAttributeMultiprocessorCount, dev);
    return c > 0 ? c : 256;
  }();
  return n;
}

static inline int cdiv(long a, long b) { return (int)((a + b - 1) / b); }
