#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
// First conv of the depthwise-separable family (stem3x3.hip): 3x3, stride 2, padding 1, 3 input channels, groups 1, no
// bias.  The image x[N][H][W][3] is fp32 NHWC (the storage of a dense channels_last [N, 3, H, W] tensor, 4-byte
// aligned) and is rounded to the 16-bit compute dtype in registers; weight w[K][3][3][3] (KRSC) and y / dy
// [N][P][Q][K] are 16-bit, P = (H - 1) / 2 + 1, Q = (W - 1) / 2 + 1, K % 8 == 0, 8 <= K <= 64.  The reduction index
// j = (r * 3 + s) * 3 + c has 27 terms, padded with zeros to one 32-element K-step of v_mfma_f32_16x16x32.
namespace pdt {
constexpr int kStemMinK = 8, kStemMaxK = 64;
constexpr int kStemRed = 27, kStemRedPad = 32;
// output pixels one launch addresses: pixel and tile indices are 32-bit; image bases are 64-bit and offsets inside
// one image are 32-bit, so one image stays below 2^31 bytes while the whole input may be of any size
constexpr int64_t kStemMaxPix = int64_t(1) << 30;
inline int64_t stem3x3_out(int64_t v) { return (v - 1) / 2 + 1; }
inline bool stem3x3_fits(int64_t N, int64_t H, int64_t W, int64_t K) {
  if (N < 1 || H < 1 || W < 1 || N > kStemMaxPix || H > kStemMaxPix || W > kStemMaxPix) return false;
  if (K < kStemMinK || K > kStemMaxK || K % 8 != 0) return false;
  if (H * W * 12 >= (int64_t(1) << 31)) return false;
  const int64_t PQ = stem3x3_out(H) * stem3x3_out(W);  // < 2^60
  return PQ <= kStemMaxPix && N * PQ <= kStemMaxPix;
}

// y[N][P][Q][K] = conv(x, w), fp32 accumulation, rounded once to the dtype
void stem3x3_fwd_launch(int dtype, const float* x, const uint16_t* w, uint16_t* y, int64_t N, int H, int W, int K,
                        hipStream_t s);

struct StemWgradPlan {
  int splits;         // partial slabs
  int pix_per_split;  // output pixels per slab: a multiple of the 128-pixel reduction step
};
StemWgradPlan stem3x3_wgrad_plan(int64_t M, int K, int target_blocks);
// ws[splits][K][32] fp32 partial slabs of dw[K][27] = dy[M][K]^T * patch[M][27] (columns 27..31 are written as
// zeros); sum them with wgrad_reduce_launch (rows = K, cols = 27, ldw = 32)
void stem3x3_wgrad_launch(int dtype, const float* x, const uint16_t* dy, float* ws, int64_t N, int H, int W, int K,
                          const StemWgradPlan& plan, hipStream_t s);
}  // namespace pdt
