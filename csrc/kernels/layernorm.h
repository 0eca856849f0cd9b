#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
// LayerNorm kernels (layernorm.hip): a dense [rows][C] tensor normalised over C, C % 8 == 0, 8 <= C <= 2048,
// rows >= 1, rows * C < 2^40.  x is 16-bit (the dtype of y) or fp32; y / dy are 16-bit; dx has the dtype of x;
// gamma, beta (may be null), mean[rows], rstd[rows] and the gradient partials are fp32.  fp32 math, one rounding of
// y and of dx.  x, y, dy and dx must be 16-byte aligned.
namespace pdt {
struct LnPlan {
  int L;       // lanes that share a row: a power of two, 1..64
  int NV;      // 8-channel vectors per lane, 1..4 (L * NV >= C / 8; vector q * L + lane belongs to `lane`)
  int blocks;  // persistent 256-thread blocks; each walks groups of 256 / L rows with stride `blocks`
};
// (L, NV) from C alone, the block count from the row groups and `max_blocks` (>= 1)
LnPlan layernorm_plan(int64_t rows, int C, int max_blocks);
// y = (x - mean) * rstd * gamma + beta, mean / rstd per row (two passes over registers)
void layernorm_fwd_launch(int dtype, bool x_f32, const void* x, const float* gamma, const float* beta, uint16_t* y,
                          float* mean, float* rstd, int64_t rows, int C, float eps, const LnPlan& plan, hipStream_t s);
// dx = rstd * (a - mean_C(a) - xhat * mean_C(a * xhat)), a = gamma * dy, xhat = (x - mean) * rstd.  partials (may be
// null: no gamma / beta gradient) receives [plan.blocks][2][C]: each block's sums of dy * xhat and of dy over the rows
// it walked; sum them with wgrad_reduce_launch.
void layernorm_bwd_launch(int dtype, bool x_f32, const uint16_t* dy, const void* x, const float* mean,
                          const float* rstd, const float* gamma, void* dx, float* partials, int64_t rows, int C,
                          const LnPlan& plan, hipStream_t s);
}  // namespace pdt
