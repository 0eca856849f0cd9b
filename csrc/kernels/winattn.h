#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
// Window attention kernels (winattn.hip): softmax(scale * q k^T + bias [+ -100 where region labels differ]) v over
// Bw windows of N <= 64 tokens and `heads` heads of dimension 32.  q / k / v / dy and the gradients are 16-bit and are
// addressed by a base pointer and element strides (window, token, head) with the 32 channels dense; every stride is a
// multiple of 8 and every base 16-byte aligned.  y is token-major [Bw][N][heads * 32].  bias is fp32 [heads][N][N],
// region (may be null) uint8 [nwin][N] with window w reading row w % nwin, stat fp32 [Bw][heads][N][2] (row max and
// row sum of the forward).  fp32 math, one rounding of y, dq, dk, dv.
namespace pdt {
struct WaOperand {
  uint16_t* p;
  int64_t sw, st, sh;  // element strides: window, token, head
};
struct WaPlan {
  int blocks;  // persistent 256-thread blocks: blocks * 4 waves = slabs * heads
  int slabs;   // window slots: wave (slot, head) walks windows slot, slot + slabs, ...; one dbias slab per slot
};
struct WaArgs {
  WaOperand q, k, v, dy, dq, dk, dv;  // the forward reads q, k, v only
  uint16_t* y;                        // forward only
  const float* bias;
  const uint8_t* region;
  float* stat;
  float* partial;  // backward: [slabs][heads][N][N], every element written
  int nwin, Bw, heads, N;
  float scale;
};
bool winattn_fits(int64_t Bw, int64_t heads, int64_t N, int64_t head_dim);
// blocks <= max_blocks where heads allows: blocks is a multiple of heads / gcd(heads, 4)
WaPlan winattn_plan(int64_t Bw, int heads, int max_blocks);
void winattn_fwd_launch(int dtype, const WaArgs& a, const WaPlan& plan, hipStream_t s);
void winattn_bwd_launch(int dtype, const WaArgs& a, const WaPlan& plan, hipStream_t s);
}  // namespace pdt
