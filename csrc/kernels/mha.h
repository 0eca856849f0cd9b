#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "winattn.h"
// Global attention kernels (mha.hip): y = softmax(scale * q k^T) v per (batch, head) over 1 <= N <= 4096 tokens, heads of
// dimension 64, no bias, no mask, no dropout (ViT's nn.MultiheadAttention).  q / k / v / dy and the gradients are
// 16-bit and are addressed as a WaOperand: a base pointer and element strides (sw: batch, st: token, sh: head) with the
// 64 channels dense, every stride a multiple of 8 and every base 16-byte aligned.  y is token-major
// [B][N][heads * 64].  fp32 math, one rounding of y, dq, dk, dv.
// lse is fp32 [B][heads][N], the log-sum-exp of a row's scaled scores in the BASE-2 domain:
//   lse = log2(sum_j exp2(scale * log2(e) * s_ij)),  natural log-sum-exp = lse * ln 2.
// delta is the backward's fp32 workspace [B][heads][N]: delta_i = sum_d dO_id * y_id, written by the first pass.
namespace pdt {
struct MhaArgs {
  WaOperand q, k, v, dy, dq, dk, dv;  // the forward reads q, k, v only
  uint16_t* y;                        // forward: written; backward: read
  float* lse;
  float* delta;  // backward only, every element written
  int B, heads, N;
  float scale;
};
// head_dim == 64, 1 <= N <= 4096, the grid below 2^31 blocks and every element offset below 2^40
bool mha_fits(int64_t B, int64_t heads, int64_t N, int64_t head_dim);
void mha_fwd_launch(int dtype, const MhaArgs& a, hipStream_t s);
// two kernels (dQ and delta, then dK and dV), counted once
void mha_bwd_launch(int dtype, const MhaArgs& a, hipStream_t s);
}  // namespace pdt
