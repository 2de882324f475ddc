// Launchers and shape predicates of the hand-pipelined bf16 conv kernels (defined in gemm_ops.hip and wgrad_dma.hip;
// the entries of conv_ops.hip check the shapes they take and route to them).
#pragma once
#include "common.hpp"

// 8 x 32-pixel output tiles of the 3x3 halo weight-gradient kernels (gemm_ops.hip, wgrad_dma.hip)
constexpr int HT_TH = 8, HT_TW = 32, HT_HR = HT_TH + 2, HT_HC = HT_TW + 2, HT_PX = HT_HR * HT_HC;
// LDS-DMA 3x3 weight gradient, 64 x 64 channel blocks (wgrad_dma.hip; needs H % 8 == 0, W % 32 == 0)
int wgrad3x3_dma_launch(bool relu_x, const bf16* dy, const bf16* x, float* ws, int B, int H, int W, int CinT, int CoT,
                        hipStream_t st);
// The hand-pipelined bf16 conv kernels of gemm_ops.hip.
// Register-weight 3x3 s1 p1 convs over 64 input channels: forward 64 -> 64 (+ ReLU), the ReLU'-masked data gradient
// (Cout 64 or 96 channels of dy, + column sums) and the three fused mask heads; rw_ok = dtype, size limits, knob
bool rw_ok(int dtype, int B, int H, int W);
int conv3x3_rw_launch(bool relu, const bf16* x, const bf16* w, const float* bias, bf16* out, int B, int H, int W,
                      hipStream_t st);
int conv3x3_rw_dgrad_launch(int Cout, const bf16* dy, const bf16* wT, const bf16* res1, float* colsum, bf16* dx, int B,
                            int H, int W, hipStream_t st);
int mask_heads_rw_launch(const bf16* feat, const bf16* w1p, const float* b1, const float* w2, const float* b2,
                         float* logits, bf16* hsave, int B, int H, int W, hipStream_t st);
// ConvTranspose2d(128, 64, 4, 2, 1) forward and its data gradient, the strided Conv2d(64, 128, 4, 2, 1); H x W = the
// 128-channel grid
bool convt_rw_ok(int dtype, int B, int H, int W);
int convT4s2_rw_launch(const bf16* x, const bf16* wt, const float* bias, bool relu, bf16* out, int B, int H, int W,
                       hipStream_t st);
int conv4s2_rw_launch(const bf16* x, const bf16* w, float* colsum, bf16* out, int B, int H, int W, hipStream_t st);
// weight gradients into the zeroed GEMM-layout workspace ws: register-staged 3x3 halo tiles (CoT % 64 == 0 or 96) and
// the 4x4 s2 conv view by LDS-DMA (CinT, CoT multiples of 64)
int wgrad3x3_halo_launch(bool relu_x, const bf16* dy, const bf16* x, float* ws, int B, int H, int W, int CinT, int CoT,
                         hipStream_t st);
int wgrad4s2_dma_launch(const bf16* dy, const bf16* x, float* ws, int B, int OH, int OW, int CinT, int CoT, hipStream_t st);
