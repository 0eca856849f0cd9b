// Pointwise (1x1, stride 1, pad 0, groups 1, no bias) convolutions of the depthwise-separable family (MobileNetV2/V3,
// MNASNet, EfficientNet, ShuffleNetV2, DenseNet): thin GEMMs whose widths (16, 24, 96, 144, 960, ...) are multiples
// of 8 but mostly not of 32, so the implicit-GEMM kernels (C % 32 == 0, 64 / 128 / 256-wide output tiles) and the
// fixed-width conv1x1 kernels do not take them.  v_mfma_f32_16x16x32_{bf16,f16}, fp32 accumulation, wave64.
//
//   * pwconv_gemm_kernel: out[M][N] = in[M][R] * B[N][R]^T (forward: in = x, B = w; backward data: in = dy,
//     B = w^T).  Both operands have the reduction index contiguous, which is the MFMA operand layout itself: a
//     lane's fragment (row lane & 15, reduction chunk lane >> 4) is ONE 16-byte buffer load, no LDS.  The weights
//     are the MFMA A operand with the conv1x1.hip fragment-row permutation, so a lane ends with 8 consecutive
//     output channels of one pixel: one 16-byte store.  A block (4 waves) owns a slice of NG * 32 output channels
//     and walks pixel tiles (4 * PT * 16 rows) persistently.  KS > 0 (R <= 32 * KS): the slice's weight fragments
//     stay in registers for the block's life and only pixels stream; KS == 0: loop over the reduction in steps of
//     32, the next step's weight (L2) and activation fragments loaded behind this step's MFMAs.
//     Tails are masked at the load: a 16-byte chunk past R, a row past M or a weight row past N goes to the
//     zero-filling offset kOOB (C % 8 == 0: a chunk is wholly in or out), so no stale or neighbouring value ever
//     meets a zero weight; stores past M or N go to kOOB too (dropped).  Operands are addressed through per-tile
//     buffer resources (64-bit tile base, offsets < 1 MiB), so an operand's byte size is not limited.
//   * pwconv_wgrad_kernel: dw[K][C] = dy[M][K]^T * x[M][C], both operands reduced over their ROW index: 128-pixel
//     steps of a [pixel][64 ch] tile pair go through registers into a double-buffered LDS image and are read back
//     with ds_read_b64_tr_b16 (the conv_wgrad.hip image and swizzle).  64 (c) x 64 (k) accumulator per wave, each
//     wave taking 32 pixels of a step; the waves are summed through LDS in a fixed order and the block writes one
//     fp32 partial tile of its split's slab [split][K][C] for wgrad_reduce (no atomics: bit-identical runs).
#include "../common.h"
#include "conv_fwd.h"
#include "pwconv.h"

namespace pdt {

namespace {

typedef unsigned int pw_v4u __attribute__((vector_size(16)));
typedef __attribute__((address_space(3))) s16x4_t pw_lds_s16x4;

PDT_DEVICE uint4 pw_load16(__amdgpu_buffer_rsrc_t r, uint32_t off) {
  return __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(r, (int)off, 0, 0));
}
PDT_DEVICE void pw_store16(__amdgpu_buffer_rsrc_t r, uint32_t off, uint4 v) {
  __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(pw_v4u, v), r, (int)off, 0, 0);
}
// a + b, or kOOB when either part is kOOB (kOOB + kOOB would wrap to a valid offset)
PDT_DEVICE uint32_t pw_off(uint32_t a, uint32_t b) { return ((a | b) & kOOB) ? kOOB : a + b; }

// output channel (within a 32-channel group pair) of row `row` of weight fragment i: fragments 2p and 2p + 1 give a
// lane (rows 4 * fq + r) the 8 consecutive channels p * 32 + 8 * fq + [0, 8)
PDT_DEVICE int pw_frag_ch(int i, int row) { return (i >> 1) * 32 + (row >> 2) * 8 + (i & 1) * 4 + (row & 3); }

// Sum over the 16 lanes of a DPP row in a fixed butterfly (lane ^ 1, lane ^ 2, the half's mirror, the row's mirror):
// every lane of the row ends with the same total.  Pure VALU.
template <int CTRL>
PDT_DEVICE float pw_dpp(float x) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), CTRL, 0xf, 0xf, false));
}
PDT_DEVICE float pw_row16_fold(float v) {
  v += pw_dpp<0xB1>(v);   // quad_perm [1, 0, 3, 2]
  v += pw_dpp<0x4E>(v);   // quad_perm [2, 3, 0, 1]
  v += pw_dpp<0x141>(v);  // row_half_mirror
  v += pw_dpp<0x140>(v);  // row_mirror
  return v;
}

// STATS: the block also emits the BatchNorm statistics (sum y, sum y^2 per channel, of the ROUNDED outputs) of the
// rows it wrote, as its slice of one fp32 partial row srows[blockIdx.x / nslices][N][2] (col_reduce.h's [C][K = 2]
// layout) for stat_rows_reduce.  A lane keeps the sums of its 8 * NG channels across every tile the block walks
// (rows past M and channels past N come from zero-filled operands: their outputs are exactly 0 and add nothing),
// the 16 lanes that share the channels are folded by DPP, the 4 waves through LDS in wave order.  No atomics.
template <int DT, int NG, int PT, int KS, bool STATS>
__global__ __launch_bounds__(256) void pwconv_gemm_kernel(const uint16_t* __restrict__ in,
                                                          const uint16_t* __restrict__ B,
                                                          uint16_t* __restrict__ out, int64_t M, int R, int N,
                                                          int nslices, int mtiles, float* __restrict__ srows) {
  using E = E16<DT>;
  typedef typename E::vec8 vec8;
  constexpr int NF = NG * 2;   // 16-channel weight fragments of the slice
  constexpr int WR = PT * 16;  // rows per wave
  constexpr int BR = 4 * WR;   // rows per block tile
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int fr = lane & 15, fq = lane >> 4;
  const int slice = blockIdx.x % nslices;
  const int n0 = slice * (NG * 32);
  const int tstride = gridDim.x / nslices;  // the launcher's grid is a multiple of nslices
  const __amdgpu_buffer_rsrc_t rb = make_rsrc(B, (uint32_t)N * (uint32_t)R * 2u);  // <= 8 MiB

  // a 32-channel group wholly past N is skipped (wave-uniform): no loads, no MFMAs, no stores
  bool gok[NG];
#pragma unroll
  for (int p = 0; p < NG; ++p) gok[p] = n0 + p * 32 < N;

  uint32_t wrow[NF];  // byte offset of this lane's weight row per fragment, kOOB past N
#pragma unroll
  for (int i = 0; i < NF; ++i) {
    const int ch = n0 + pw_frag_ch(i, fr);
    wrow[i] = ch < N ? (uint32_t)ch * (uint32_t)R * 2u : kOOB;
  }
  // byte offset of this lane's reduction chunk of step kk, kOOB past R
  auto kpart = [&](int kk) {
    const int k = kk * 32 + fq * 8;
    return k < R ? (uint32_t)k * 2u : kOOB;
  };

  vec8 ares[NF][KS > 0 ? KS : 1];
  if constexpr (KS > 0) {
#pragma unroll
    for (int i = 0; i < NF; ++i)
#pragma unroll
      for (int kk = 0; kk < KS; ++kk)
        ares[i][kk] = __builtin_bit_cast(vec8, pw_load16(rb, gok[i >> 1] ? pw_off(wrow[i], kpart(kk)) : kOOB));
  }

  float st[STATS ? NG : 1][2][8];  // [group][sum, sum of squares][channel of the lane's 8]
  if constexpr (STATS) {
#pragma unroll
    for (int p = 0; p < NG; ++p)
#pragma unroll
      for (int e = 0; e < 8; ++e) st[p][0][e] = st[p][1][e] = 0.f;
  }

  for (int t = blockIdx.x / nslices; t < mtiles; t += tstride) {
    const int64_t m0 = (int64_t)t * BR;
    const int64_t left = M - m0;
    const int rows = left < BR ? (int)left : BR;
    const __amdgpu_buffer_rsrc_t ri = make_rsrc(in + m0 * R, (uint32_t)rows * (uint32_t)R * 2u);
    const __amdgpu_buffer_rsrc_t ro = make_rsrc(out + m0 * N, (uint32_t)rows * (uint32_t)N * 2u);
    uint32_t xrow[PT];
#pragma unroll
    for (int j = 0; j < PT; ++j) {
      const int row = wave * WR + j * 16 + fr;
      xrow[j] = row < rows ? (uint32_t)row * (uint32_t)R * 2u : kOOB;
    }

    f32x4_t acc[NF][PT];
#pragma unroll
    for (int i = 0; i < NF; ++i)
#pragma unroll
      for (int j = 0; j < PT; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};

    if constexpr (KS > 0) {
#pragma unroll
      for (int kk = 0; kk < KS; ++kk) {
        const uint32_t kb = kpart(kk);
        vec8 bf[PT];
#pragma unroll
        for (int j = 0; j < PT; ++j) bf[j] = __builtin_bit_cast(vec8, pw_load16(ri, pw_off(xrow[j], kb)));
#pragma unroll
        for (int i = 0; i < NF; ++i) {
          if (!gok[i >> 1]) continue;
#pragma unroll
          for (int j = 0; j < PT; ++j) acc[i][j] = E::mfma16x16x32(ares[i][kk], bf[j], acc[i][j]);
        }
      }
    } else {
      const int ksteps = (R + 31) >> 5;
      vec8 a0[NF], b0[PT];
      auto load_step = [&](int kk, vec8(&a)[NF], vec8(&b)[PT]) {
        const uint32_t kb = kpart(kk);  // past the reduction: every chunk is kOOB (zeros, no memory traffic)
#pragma unroll
        for (int i = 0; i < NF; ++i)
          a[i] = __builtin_bit_cast(vec8, pw_load16(rb, gok[i >> 1] ? pw_off(wrow[i], kb) : kOOB));
#pragma unroll
        for (int j = 0; j < PT; ++j) b[j] = __builtin_bit_cast(vec8, pw_load16(ri, pw_off(xrow[j], kb)));
      };
      load_step(0, a0, b0);
      for (int kk = 0; kk < ksteps; ++kk) {
        vec8 a1[NF], b1[PT];
        load_step(kk + 1, a1, b1);
#pragma unroll
        for (int i = 0; i < NF; ++i) {
          if (!gok[i >> 1]) continue;
#pragma unroll
          for (int j = 0; j < PT; ++j) acc[i][j] = E::mfma16x16x32(a0[i], b0[j], acc[i][j]);
        }
#pragma unroll
        for (int i = 0; i < NF; ++i) a0[i] = a1[i];
#pragma unroll
        for (int j = 0; j < PT; ++j) b0[j] = b1[j];
      }
    }

    // fragment pair p gives the lane channels n0 + p * 32 + 8 * fq + [0, 8) of row wave * WR + j * 16 + fr
#pragma unroll
    for (int j = 0; j < PT; ++j) {
      const int row = wave * WR + j * 16 + fr;
#pragma unroll
      for (int p = 0; p < NG; ++p) {
        if (!gok[p]) continue;
        const int ch = n0 + p * 32 + 8 * fq;
        uint4 pk;
        pk.x = E::pack2(acc[2 * p][j][0], acc[2 * p][j][1]);
        pk.y = E::pack2(acc[2 * p][j][2], acc[2 * p][j][3]);
        pk.z = E::pack2(acc[2 * p + 1][j][0], acc[2 * p + 1][j][1]);
        pk.w = E::pack2(acc[2 * p + 1][j][2], acc[2 * p + 1][j][3]);
        const uint32_t off = (row < rows && ch < N) ? ((uint32_t)row * (uint32_t)N + (uint32_t)ch) * 2u : kOOB;
        pw_store16(ro, off, pk);
        if constexpr (STATS) {
          uint16_t h[8];
          unpack8(pk, h);
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const float f = E::to_f(h[e]);
            st[p][0][e] += f;
            st[p][1][e] = fmaf(f, f, st[p][1][e]);  // the square of a 16-bit value is exact in fp32
          }
        }
      }
    }
  }

  if constexpr (STATS) {
    __shared__ float red[4][NG * 32][2];
#pragma unroll
    for (int p = 0; p < NG; ++p)
#pragma unroll
      for (int k = 0; k < 2; ++k)
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float t = pw_row16_fold(st[p][k][e]);
          if (fr == 0) red[wave][p * 32 + 8 * fq + e][k] = t;
        }
    __syncthreads();
    const int idx = threadIdx.x;  // (channel of the slice, quantity)
    if (idx < NG * 64 && n0 + (idx >> 1) < N) {
      const float* r0 = &red[0][0][0];
      float t = r0[idx];
#pragma unroll
      for (int w = 1; w < 4; ++w) t += r0[w * NG * 64 + idx];
      srows[((int64_t)(blockIdx.x / nslices) * N + n0) * 2 + idx] = t;
    }
  }
}

// chunk swizzle of a [pixel][64 ch] (128-byte row) LDS image read by ds_read_b64_tr_b16 (conv_wgrad.hip's)
PDT_DEVICE int pw_tr_swz(int row) { return (((row >> 1) & 1) << 1) | (((row >> 3) & 1) << 2); }

template <int DT>
__global__ __launch_bounds__(256) void pwconv_wgrad_kernel(const uint16_t* __restrict__ x,
                                                           const uint16_t* __restrict__ dy, float* __restrict__ ws,
                                                           int M, int C, int K, int pps, int c_tiles, int k_tiles) {
  using E = E16<DT>;
  typedef typename E::vec8 vec8;
  constexpr int BKP = 128;        // pixels per reduction step
  constexpr int ROWB = 128;       // 64 channels * 2 B
  constexpr int XB = BKP * ROWB;  // bytes of one operand's tile
  constexpr int STAGE = 2 * XB;
  __shared__ __attribute__((aligned(1024))) char smem[2 * STAGE];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  // consecutive blocks = the tiles of ONE pixel range: its rows come from HBM once and from L2 after that
  const int ntile = c_tiles * k_tiles;
  const int tile = blockIdx.x % ntile, split = blockIdx.x / ntile;
  const int kt = tile % k_tiles, ct = tile / k_tiles;
  const int c0 = ct * 64, k0 = kt * 64;
  const int pix_begin = split * pps;
  const int pix_end = min(M, pix_begin + pps);
  const int nsteps = (pix_end - pix_begin + BKP - 1) / BKP;

  // staging geometry: piece (wave * 4 + j) is 8 rows x 8 chunks = 1 KiB, LDS chunk pch of a row holds the source
  // chunk pch ^ swz(row); a row past the split's range or a chunk past C / K loads zeros (kOOB)
  const int lrow = lane >> 3, pch = lane & 7;
  uint4 rx[4], ry[4];
  auto gload = [&](int step) {
    const int pb = pix_begin + step * BKP;
    const int rows = min(BKP, pix_end - pb);
    const __amdgpu_buffer_rsrc_t rsx = make_rsrc(x + (int64_t)pb * C, (uint32_t)(rows * C * 2));
    const __amdgpu_buffer_rsrc_t rsy = make_rsrc(dy + (int64_t)pb * K, (uint32_t)(rows * K * 2));
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int row = (wave * 4 + j) * 8 + lrow;
      const int lch = pch ^ pw_tr_swz(row);
      const int c = c0 + lch * 8, k = k0 + lch * 8;
      rx[j] = pw_load16(rsx, (row < rows && c < C) ? (uint32_t)((row * C + c) * 2) : kOOB);
      ry[j] = pw_load16(rsy, (row < rows && k < K) ? (uint32_t)((row * K + k) * 2) : kOOB);
    }
  };
  auto lstore = [&](int buf) {
    char* sb = smem + buf * STAGE + (wave * 4) * 1024 + lane * 16;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      *(uint4*)(sb + j * 1024) = rx[j];
      *(uint4*)(sb + XB + j * 1024) = ry[j];
    }
  };

  f32x4_t acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  // transposed-read lane geometry: group g = lane >> 4 holds pixels 8g .. 8g + 7 of the wave's 32-pixel slice
  const int g = lane >> 4, li = lane & 15, q = li >> 2, p4 = li & 3;

  if (nsteps > 0) {  // block-uniform
    gload(0);
    lstore(0);
    __syncthreads();
    for (int s = 0; s < nsteps; ++s) {
      const int cur = s & 1;
      if (s + 1 < nsteps) gload(s + 1);  // in flight behind this step's MFMAs
      const char* sb = smem + cur * STAGE;
      vec8 af[4], bfr[4];
#pragma unroll
      for (int f = 0; f < 4; ++f) {
        const int r0 = wave * 32 + 8 * g + q, r1 = r0 + 4;
        const int col = f * 16 + 4 * p4;  // element within the 64-wide row
        const int ch = col >> 3, off = (col & 7) * 2;
        const int o0 = r0 * ROWB + ((ch ^ pw_tr_swz(r0)) << 4) + off;
        const int o1 = r1 * ROWB + ((ch ^ pw_tr_swz(r1)) << 4) + off;
        s16x4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((pw_lds_s16x4*)(sb + o0));
        s16x4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((pw_lds_s16x4*)(sb + o1));
        af[f] = __builtin_bit_cast(vec8, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
        lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((pw_lds_s16x4*)(sb + XB + o0));
        hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((pw_lds_s16x4*)(sb + XB + o1));
        bfr[f] = __builtin_bit_cast(vec8, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
      }
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = E::mfma16x16x32(af[i], bfr[j], acc[i][j]);
      if (s + 1 < nsteps) lstore(cur ^ 1);  // the other buffer: last read before the previous barrier
      __syncthreads();
    }
  }

  // sum the 4 waves' tiles through LDS in wave order; acc[i][j]: rows c = 16i + 4 * (lane >> 4) + r, col k = 16j + (lane & 15)
  float* red = (float*)smem;  // [4 waves][64 k][64 c]
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int k = 16 * j + (lane & 15);
      const int c = 16 * i + 4 * (lane >> 4);
      *(f32x4_t*)(red + (wave * 64 + k) * 64 + c) = acc[i][j];
    }
  __syncthreads();
  float* slab = ws + (int64_t)split * K * C;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int idx = (e * 256 + tid) * 4;  // 0 .. 4095
    const int k = idx >> 6, c = idx & 63;
    f32x4_t v = *(f32x4_t*)(red + k * 64 + c);
#pragma unroll
    for (int w = 1; w < 4; ++w) v += *(f32x4_t*)(red + (w * 64 + k) * 64 + c);
    // C % 8 == 0: a group of 4 channels is wholly in or out
    if (k0 + k < K && c0 + c < C) *(f32x4_t*)(slab + (int64_t)(k0 + k) * C + c0 + c) = v;
  }
}

// persistent blocks the GEMM aims for: a few per CU (256 CUs)
constexpr int kPwGemmBlocks = 1536;

// STATS: the statistics kernels; their partial rows live in stream-ordered scratch and are folded into the fp64
// `slots` right behind the GEMM.  Returns (row blocks per slice, longest fp32 chain of a statistic).
template <int DT, int NG, int PT, bool STATS>
PwStatsPlan pw_gemm_go(const uint16_t* in, const uint16_t* B, uint16_t* out, int64_t M, int R, int N, double* slots,
                       int max_blocks, hipStream_t s) {
  const int nslices = (N + NG * 32 - 1) / (NG * 32);
  const int64_t BR = 4 * PT * 16;
  const int mtiles = (int)((M + BR - 1) / BR);
  int per = max_blocks / nslices;
  if (per < 1) per = 1;
  if (per > mtiles) per = mtiles;
  const dim3 g((unsigned)(per * nslices));
  // every block owns at least one tile (per <= mtiles) and writes its slice of its partial row exactly once
  Scratch part(STATS ? (size_t)per * N * 2 * sizeof(float) : 0, s);
  float* srows = part.as<float>();
#define PDT_PW_G(KS)                                                                                                 \
  hipLaunchKernelGGL((pwconv_gemm_kernel<DT, NG, PT, KS, STATS>), g, dim3(256), 0, s, in, B, out, M, R, N, nslices, \
                     mtiles, srows)
  if (R <= 32) PDT_PW_G(1);
  else if (R <= 64) PDT_PW_G(2);
  else PDT_PW_G(0);
#undef PDT_PW_G
  if constexpr (STATS) stat_rows_reduce_launch(srows, per, N * 2, slots, s);
  // the lane's chain over its tiles (PT rows each), the 16-lane fold, the 4-wave fold
  return PwStatsPlan{per, (mtiles + per - 1) / per * PT + 16 + 4};
}

template <int DT, bool STATS>
PwStatsPlan pw_gemm_dt(const uint16_t* in, const uint16_t* B, uint16_t* out, int64_t M, int R, int N, double* slots,
                       int max_blocks, hipStream_t s) {
  // the slice width follows the output width alone: no per-shape table
  if (N <= 32) return pw_gemm_go<DT, 1, 4, STATS>(in, B, out, M, R, N, slots, max_blocks, s);
  if (N <= 64) return pw_gemm_go<DT, 2, 4, STATS>(in, B, out, M, R, N, slots, max_blocks, s);
  return pw_gemm_go<DT, 4, 2, STATS>(in, B, out, M, R, N, slots, max_blocks, s);
}

}  // namespace

void pwconv_gemm_launch(int dtype, const uint16_t* in, const uint16_t* B, uint16_t* out, int64_t M, int R, int N,
                        bool dgrad, hipStream_t s) {
  if (!pwconv_fits(M, R, N)) pdt_hip_fail("pwconv_gemm_launch: operand outside the kernels' addressing", hipErrorInvalidValue, __FILE__, __LINE__);
  if (dgrad) PDT_COUNT("pwconv_dgrad");
  else PDT_COUNT("pwconv_fwd");
  if (dtype == kBF16) pw_gemm_dt<kBF16, false>(in, B, out, M, R, N, nullptr, kPwGemmBlocks, s);
  else pw_gemm_dt<kF16, false>(in, B, out, M, R, N, nullptr, kPwGemmBlocks, s);
}

PwStatsPlan pwconv_fwd_stats_launch(int dtype, const uint16_t* x, const uint16_t* w, uint16_t* y, double* slots,
                                    int64_t M, int C, int K, int max_blocks, hipStream_t s) {
  if (!pwconv_fits(M, C, K) || max_blocks < 0)
    pdt_hip_fail("pwconv_fwd_stats_launch: operand outside the kernels' addressing", hipErrorInvalidValue, __FILE__, __LINE__);
  PDT_COUNT("pwconv_fwd_stats");
  if (max_blocks == 0) max_blocks = kPwGemmBlocks;
  if (dtype == kBF16) return pw_gemm_dt<kBF16, true>(x, w, y, M, C, K, slots, max_blocks, s);
  return pw_gemm_dt<kF16, true>(x, w, y, M, C, K, slots, max_blocks, s);
}

PwWgradPlan pwconv_wgrad_plan(int64_t M, int C, int K, int target_blocks) {
  PwWgradPlan pl{};
  pl.c_tiles = (C + 63) / 64;
  pl.k_tiles = (K + 63) / 64;
  const int64_t tiles = (int64_t)pl.c_tiles * pl.k_tiles;
  int64_t splits = ((int64_t)target_blocks + tiles - 1) / tiles;
  const int64_t most = (M + 127) / 128;  // at least one reduction step per split
  if (splits > most) splits = most;
  if (splits > 4096) splits = 4096;  // bounds the slab workspace
  if (splits < 1) splits = 1;
  int64_t pps = M > 0 ? (M + splits - 1) / splits : 128;
  pps = (pps + 127) / 128 * 128;
  pl.pix_per_split = (int)pps;
  pl.splits = M > 0 ? (int)((M + pps - 1) / pps) : 1;
  return pl;
}

void pwconv_wgrad_launch(int dtype, const uint16_t* x, const uint16_t* dy, float* ws, int64_t M, int C, int K,
                         const PwWgradPlan& plan, hipStream_t s) {
  if (!pwconv_fits(M, C, K)) pdt_hip_fail("pwconv_wgrad_launch: operand outside the kernels' addressing", hipErrorInvalidValue, __FILE__, __LINE__);
  PDT_COUNT("pwconv_wgrad");
  const dim3 g((unsigned)(plan.c_tiles * plan.k_tiles * plan.splits));
  if (dtype == kBF16)
    hipLaunchKernelGGL((pwconv_wgrad_kernel<kBF16>), g, dim3(256), 0, s, x, dy, ws, (int)M, C, K,
                       plan.pix_per_split, plan.c_tiles, plan.k_tiles);
  else
    hipLaunchKernelGGL((pwconv_wgrad_kernel<kF16>), g, dim3(256), 0, s, x, dy, ws, (int)M, C, K, plan.pix_per_split,
                       plan.c_tiles, plan.k_tiles);
}

}  // namespace pdt
