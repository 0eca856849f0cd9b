#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
// Depthwise convolution kernels (dwconv.hip): groups == Cin == Cout == C, square kernel R in {3, 5}, stride in
// {1, 2}, dilation 1, pad R / 2, C % 8 == 0.  NHWC 16-bit activations, taps-major [R][S][C] 16-bit weight, fp32 math.
namespace pdt {
// y[N][P][Q][C] = depthwise conv of x[N][H][W][C] with w[R][R][C]   (P = (H - 1) / stride + 1, Q likewise)
void dwconv_fwd_launch(int dtype, const uint16_t* x, const uint16_t* w, uint16_t* y, int64_t N, int H, int W, int C,
                       int R, int stride, hipStream_t s);
// dx[N][H][W][C] from dy[N][P][Q][C]: gather form, every dx element written exactly once
void dwconv_dgrad_launch(int dtype, const uint16_t* dy, const uint16_t* w, uint16_t* dx, int64_t N, int H, int W,
                         int C, int R, int stride, hipStream_t s);

struct DwWgradPlan {
  int splits;         // partial slabs (grid.y)
  int pix_per_split;  // output pixels (n, p, q) per slab
  int groups;         // channel groups of `cvb` 8-channel vectors (grid.x)
  int cvb;            // 8-channel vectors per block
  int pl;             // pixel lanes per block: cvb * pl * R <= 256 threads are active
};
// split count from the pixel count N * P * Q, the channel count and a target number of blocks
DwWgradPlan dwconv_wgrad_plan(int64_t npix, int C, int R, int target_blocks);
// ws[splits][R * R][C] fp32 partial slabs (sum them with wgrad_reduce_launch: rows = R * R, cols = C)
void dwconv_wgrad_launch(int dtype, const uint16_t* x, const uint16_t* dy, float* ws, int64_t N, int H, int W, int C,
                         int R, int stride, const DwWgradPlan& plan, hipStream_t s);
}  // namespace pdt
