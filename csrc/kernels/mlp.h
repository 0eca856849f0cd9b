#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pwconv.h"
// The second half of a channel MLP, Linear(C, Hd) -> GELU -> Linear(Hd, Co), with the bias of the first Linear, the exact
// (erf) GELU, its derivative and the bias of the second folded into the GEMMs next to them (mlp.hip).  The first
// Linear's three passes run on pwconv.hip.  All operands 16-bit [rows][channels], biases and weight gradients fp32:
//   z0[M][Hd] = round16(x * w1^T) (pwconv_gemm_launch), v = z0 + b1 (fp32), h = round16(gelu(v)) (never in memory)
//   y[M][Co]  = round16(h * w2^T + b2)
//   dz[M][Hd] = round16((dy * w2) .* gelu'(v)), db1 = colsum(dz), dw2[Co][Hd] = dy^T * h
// Hd % 8 == Co % 8 == 0, 8 <= Co <= 512, 8 <= Hd <= 2048, 1 <= M <= kPwMaxRows.
namespace pdt {
constexpr int kMlpMaxOut = 512, kMlpMaxHidden = 2048;
// (M, C, Hd, Co) of the whole MLP: C is the first Linear's input width (pwconv's kernels take it)
inline bool mlp_fits(int64_t M, int64_t C, int64_t Hd, int64_t Co) {
  return pwconv_fits(M, C, Hd) && pwconv_fits(M, Hd, Co) && C <= kMlpMaxOut && Co <= kMlpMaxOut &&
         Hd <= kMlpMaxHidden;
}

// y[M][Co] = round16(gelu(z0[M][Hd] + b1) * w2[Co][Hd]^T + b2)
void mlp_fc2_fwd_launch(int dtype, const uint16_t* z0, const float* b1, const uint16_t* w2, const float* b2,
                        uint16_t* y, int64_t M, int Hd, int Co, hipStream_t s);

// dz[M][Hd] = round16((dy[M][Co] * w2t[Hd][Co]^T) .* gelu'(z0 + b1)) and db1[Hd] = the column sums of the rounded dz:
// every block keeps fp32 sums over the tiles it walks and writes one partial row (col_reduce.h's [blocks][C][1]
// layout, stream-ordered scratch) that wgrad_reduce_launch folds in a fixed order.  max_blocks: the persistent blocks
// aimed for (0 = the default); fewer make a block walk more tiles.  chain: the longest run of fp32 additions a sum
// passes through.
struct MlpDgradPlan {
  int row_blocks;  // partial rows = persistent blocks per 128-channel slice of Hd
  int chain;
};
MlpDgradPlan mlp_fc2_dgrad_launch(int dtype, const uint16_t* dy, const uint16_t* w2t, const uint16_t* z0,
                                  const float* b1, uint16_t* dz, float* db1, int64_t M, int Hd, int Co, int max_blocks,
                                  hipStream_t s);

struct MlpWgradPlan {
  int splits;          // partial slabs
  int rows_per_split;  // a multiple of the 128-row reduction step
  int h_tiles;         // 64-wide tiles over Hd
  int o_tiles;         // 64-wide tiles over Co
  int chain;           // roundings of 2^-24 an element may pass through: 2 (one fp32 ulp) per product of a split's
                       // rows, per wave of the block's fold and per slab
};
MlpWgradPlan mlp_fc2_wgrad_plan(int64_t M, int Hd, int Co, int target_blocks);
// ws[splits][Co][Hd] fp32 partial slabs of dw2 = dy^T * round16(gelu(z0 + b1)) (sum them with wgrad_reduce_launch:
// rows = Co, cols = Hd)
void mlp_fc2_wgrad_launch(int dtype, const uint16_t* z0, const float* b1, const uint16_t* dy, float* ws, int64_t M,
                          int Hd, int Co, const MlpWgradPlan& plan, hipStream_t s);
}  // namespace pdt
