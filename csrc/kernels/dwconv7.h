#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
// 7x7 depthwise convolution kernels (dwconv7.hip): groups == Cin == Cout == C, kernel 7x7, stride 1, padding 3,
// dilation 1, C % 8 == 0, optional per-channel bias.  NHWC 16-bit activations, taps-major [7][7][C] 16-bit weight
// (the layout of dwconv.hip), fp32 math, one rounding of the output.  N <= 65535, H * W * C < 2^31.
namespace pdt {
// y[N][H][W][C] = depthwise 7x7 conv of x[N][H][W][C] with w[7][7][C], + bias[C] (16-bit, may be null)
void dwconv7_fwd_launch(int dtype, const uint16_t* x, const uint16_t* w, const uint16_t* bias, uint16_t* y, int64_t N,
                        int H, int W, int C, hipStream_t s);
// dx[N][H][W][C] from dy[N][H][W][C]: the same conv with the taps flipped and no bias
void dwconv7_dgrad_launch(int dtype, const uint16_t* dy, const uint16_t* w, uint16_t* dx, int64_t N, int H, int W,
                          int C, hipStream_t s);

struct Dw7WgradPlan {
  int splits;         // partial slabs (grid.y)
  int pix_per_split;  // output pixels (n, p, q) per slab
  int groups;         // channel groups of 8 channel vectors = 64 channels (grid.x)
};
// split count from the pixel count N * H * W, the channel count and a target number of blocks
Dw7WgradPlan dwconv7_wgrad_plan(int64_t npix, int C, int target_blocks);
// ws[splits][50][C] fp32 partial slabs: rows 0..48 the taps r * 7 + s, row 49 the sum of dy (the bias gradient);
// sum them with wgrad_reduce_launch (rows = 50, cols = C)
void dwconv7_wgrad_launch(int dtype, const uint16_t* x, const uint16_t* dy, float* ws, int64_t N, int H, int W, int C,
                          const Dw7WgradPlan& plan, hipStream_t s);
}  // namespace pdt
