#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
// Pointwise (1x1, stride 1, pad 0, groups 1, no bias) convolution kernels (pwconv.hip) for the widths the
// implicit-GEMM kernels do not take: NHWC 16-bit activations seen as [M][C] (M = N * H * W), 16-bit weight [K][C],
// C % 8 == 0, K % 8 == 0, 8 <= C, K <= 2048, any M in [1, kPwMaxRows].  fp32 accumulation on v_mfma_f32_16x16x32.
namespace pdt {
constexpr int kPwMinCh = 8, kPwMaxCh = 2048;
// rows (pixels) one launch addresses: tile and pixel indices are 32-bit, operands are addressed through per-tile
// buffer resources (64-bit base, 32-bit offsets inside a tile), so the byte size of an operand is not limited
constexpr int64_t kPwMaxRows = int64_t(1) << 30;
inline bool pwconv_fits(int64_t M, int64_t C, int64_t K) {
  return M >= 1 && M <= kPwMaxRows && C >= kPwMinCh && C <= kPwMaxCh && C % 8 == 0 && K >= kPwMinCh &&
         K <= kPwMaxCh && K % 8 == 0;
}

// out[M][N] = in[M][R] * B[N][R]^T, rounded once to the dtype.  Forward: in = x, B = w, (R, N) = (C, K);
// backward data: in = dy, B = w^T as a [C][K] tensor, (R, N) = (K, C).  `dgrad` only selects the dispatch counter.
void pwconv_gemm_launch(int dtype, const uint16_t* in, const uint16_t* B, uint16_t* out, int64_t M, int R, int N,
                        bool dgrad, hipStream_t s);

// The forward with the BatchNorm statistics of its own (rounded) output: y as pwconv_gemm_launch writes it, bit for bit,
// and slots[kStatSlots][K][2] fp64 (sum y, sum y^2 per channel), the layout bn_finalize_slots reads.  The GEMM blocks
// emit fp32 partial rows [row_blocks][K][2] (stream-ordered scratch) that stat_rows_reduce folds; no atomics.
// max_blocks: the persistent blocks the launch aims for (0 = the forward's own 1536); fewer make a block walk more
// tiles.  chain: the longest run of fp32 additions a statistic passes through before the fp64 sums.
struct PwStatsPlan {
  int row_blocks;  // partial rows = persistent blocks per output slice
  int chain;
};
PwStatsPlan pwconv_fwd_stats_launch(int dtype, const uint16_t* x, const uint16_t* w, uint16_t* y, double* slots,
                                    int64_t M, int C, int K, int max_blocks, hipStream_t s);

struct PwWgradPlan {
  int splits;         // partial slabs
  int pix_per_split;  // pixels per slab: a multiple of the 128-pixel reduction step
  int c_tiles;        // 64-wide tiles over C
  int k_tiles;        // 64-wide tiles over K
};
PwWgradPlan pwconv_wgrad_plan(int64_t M, int C, int K, int target_blocks);
// ws[splits][K][C] fp32 partial slabs of dw[K][C] = dy[M][K]^T * x[M][C] (sum them with wgrad_reduce_launch:
// rows = K, cols = C)
void pwconv_wgrad_launch(int dtype, const uint16_t* x, const uint16_t* dy, float* ws, int64_t M, int C, int K,
                         const PwWgradPlan& plan, hipStream_t s);
}  // namespace pdt
